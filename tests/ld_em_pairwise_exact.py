"""The integers and the panels of pairwise-complete EM (ops.ld_em(missing="pairwise"), ops.ld_em_counts(missing="pairwise");
include/ldx.h, "pairwise-complete EM") -- TEST INFRASTRUCTURE ONLY, a plain module like tests/ld_pairwise_exact.py, for
tests/test_ld_em_pairwise_host.py and tests/test_gpu_ld_em_pairwise.py.

Written from the definitions in include/ldx.h alone; numpy and the standard library only.  Individual k owns haplotypes 2k and
2k + 1 and is called at a SNP when BOTH codes are 0 or 1; g is the ALT dosage of a called individual.  For row x of side I and
row y of side J, over the individuals called at both:

    N    A = sum g_x    B = sum g_y    S = sum g_x g_y    H = #{g_x = 1 and g_y = 1}

as integer matrix products over per-individual indicator planes: ld_pairwise_exact.ind_planes' (called, g) and the het plane
g == 1 (0 where the individual is not called, as g is).  The exact r and D' of a tuple are ld_em_exact.solve(N, A, B, S, H):
that oracle takes any genotype table, whatever its N.
"""
from __future__ import annotations

import numpy as np

import ld_dosage_exact as dx
import ld_em_exact as emx
import ld_pairwise_exact as px
import ld_rect_cases as rc

SETS = ("N", "A", "B", "S", "H")          # the order of include/ldx.h and ops.EM_PAIRWISE_COUNTS

# the kernel's workgroup tile is 128 x 128: (129, 257) and (257, 129) are one row and one column past both a 128- and a 256-row tile
TILE = 128
COUNT_CASES = tuple(c for c in rc.EDGE_CASES if c[1] % 2 == 0) + (((257, 129), 256),)
BIG_CASE = px.BIG_CASE                    # N = 5120, S = 20 480 (all-ALT x all-ALT), H = 5120 (all-het x all-het)
TILES_CASE = px.TILES_CASE                # holes in rows [128, 256) of each side only: four tile kinds in one launch
WALK_CASE = ((4097, 130), 254)            # the walk's bands are 32 I blocks of 128 rows: one row into the second band, two J slabs
HOLED_CASE = ((300, 130), 1008)           # ld_em_exact.panel with holes added
DENSE_CASES = (("mixed", (129, 257), 2), ("mixed", (129, 257), 254), ("mixed", (257, 129), 256), ("mixed", (300, 130), 258),
               ("holed",) + HOLED_CASE, ("big",) + BIG_CASE)
ROW_HET, ROW_ALT = 2, 3                   # big(): the all-het and the complete all-ALT row of each side


def pair_counts(codes_i, codes_j) -> np.ndarray:
    """int64 [5, n_i, n_j]: N A B S H of every pair, from integer matrix products of the indicator planes."""
    (qi, gi, _), (qj, gj, _) = px.ind_planes(codes_i), px.ind_planes(codes_j)
    ti, tj = (gi == 1).astype(np.int64), (gj == 1).astype(np.int64)
    N, A, B, S, H = px._gemm(qi, qj), px._gemm(gi, qj), px._gemm(qi, gj), px._gemm(gi, gj), px._gemm(ti, tj)
    assert (A <= 2 * N).all() and (B <= 2 * N).all() and (H <= N).all() and (S <= 4 * N).all() and ((S - H) % 2 == 0).all()
    return np.stack((N, A, B, S, H))


def loop_counts(codes_i, codes_j) -> np.ndarray:
    """The same integers by a plain loop over the individuals of every pair (small panels only)."""
    ci, cj = np.asarray(codes_i), np.asarray(codes_j)
    out = np.zeros((5, ci.shape[0], cj.shape[0]), dtype=np.int64)
    for i in range(ci.shape[0]):
        for j in range(cj.shape[0]):
            for k in range(ci.shape[1] // 2):
                x, y = ci[i, 2 * k:2 * k + 2].tolist(), cj[j, 2 * k:2 * k + 2].tolist()
                if all(c in (0, 1) for c in x + y):
                    gx, gy = sum(x), sum(y)
                    out[:, i, j] += (1, gx, gy, gx * gy, int(gx == 1 and gy == 1))
    return out


def degenerate(counts) -> np.ndarray:
    """bool [n_i, n_j]: N = 0, or A or B is 0 or 2 N within the joint set (both cells -0.0f)."""
    N, A, B = counts[0], counts[1], counts[2]
    return (N == 0) | (A == 0) | (A == 2 * N) | (B == 0) | (B == 2 * N)


def sample_live(counts, count: int, seed: int):
    """Up to ``count`` seeded (i, j) of the pairs that are not degenerate -- all of them where there are fewer."""
    ii, jj = np.nonzero(~degenerate(counts))
    if ii.size > count:
        pick = np.sort(np.random.default_rng(seed).choice(ii.size, size=count, replace=False))
        ii, jj = ii[pick], jj[pick]
    return ii, jj


# ---- panels: (codes_i, codes_j, {kind: what was planted}), read-only, built once per process ------------------------------------
_PANELS = {}


def _keep(key, ci, cj, planted):
    ci.setflags(write=False)
    cj.setflags(write=False)
    _PANELS[key] = (ci, cj, planted)
    return _PANELS[key]


def mixed(shape, n_hap: int, family: int = 0):
    """ld_pairwise_exact.mixed_pair: holes at rate MISS in the rows with index % 3 != 0, its structured rows (a whole individual
    missing, side I's row 4 half-missing, rows 7 with disjoint called sets, row 10 of side I polymorphic overall but
    monomorphic where row 10 of side J is called) and ld_rect_cases.special_rows (monomorphic, all-ALT, all-missing)."""
    ci, cj, planted = px.mixed_pair(shape, n_hap, family=family)
    planted = dict(planted)
    if min(shape) >= 5:
        planted["all_missing"] = (shape[0] - 1, shape[1] - 1)
    return ci, cj, planted


def holed(shape=HOLED_CASE[0], n_hap: int = HOLED_CASE[1]):
    """ld_em_exact.panel (duplicate, complement and all-het rows on side J, side I's row 0 their source) with holes added by
    ld_pairwise_exact.add_holes; the planted rows and side I's row 0 keep every call."""
    key = ("holed", shape, n_hap)
    if key not in _PANELS:
        src_i, src_j, where = emx.panel(shape, n_hap)
        ci, cj = np.array(src_i), np.array(src_j)
        rng = np.random.default_rng(11 * rc.pair_seed(shape, n_hap) + 3)
        px.add_holes(ci, rng)
        px.add_holes(cj, rng)
        ci[0] = src_i[0]
        for rows in where.values():
            cj[rows] = src_j[rows]
        _keep(key, ci, cj, {k: list(v) for k, v in where.items()})
    return _PANELS[key]


def big():
    """BIG_CASE: mixed()'s panel with an all-het row 2 and a complete all-ALT row 3 on both sides: N = 5120, all-ALT x all-ALT
    gives S = 20 480, all-het x all-het H = 5120."""
    key = ("big",)
    if key not in _PANELS:
        shape, n_hap = BIG_CASE
        src_i, src_j, planted = mixed(shape, n_hap)
        ci, cj = np.array(src_i), np.array(src_j)
        ci[ROW_HET], cj[ROW_HET] = dx.all_het_row(n_hap, seed=n_hap + 7), dx.all_het_row(n_hap, seed=n_hap + 8)
        ci[ROW_ALT], cj[ROW_ALT] = 1, 1
        _keep(key, ci, cj, dict(planted))
    return _PANELS[key]


def tiles():
    """TILES_CASE: ld_pairwise_exact.tiles_pair -- clean x clean, holes x clean, clean x holes and holes x holes tiles."""
    ci, cj = px.tiles_pair()
    return ci, cj, {}


def panel(kind: str, shape, n_hap: int):
    """The panel of a DENSE_CASES entry."""
    if kind == "mixed":
        return mixed(shape, n_hap)
    if kind == "holed":
        return holed(shape, n_hap)
    assert kind == "big" and (shape, n_hap) == BIG_CASE
    return big()


def walk():
    """WALK_CASE: a panel without holes except in side I's LAST row (the one row of the second band) and in column 77 of side
    J: the tiles of the walk are clean but for the last I block and the first J slab."""
    key = ("walk",)
    if key not in _PANELS:
        shape, n_hap = WALK_CASE
        ci, cj = (np.array(c) for c in px.complete_pair(shape, n_hap))
        rng = np.random.default_rng(99)
        ci[-1, rng.random(n_hap) < 0.1] = 2
        cj[77, rng.random(n_hap) < 0.1] = 2
        _keep(key, ci, cj, {"rows": [shape[0] - 1], "cols": [77]})
    return _PANELS[key]

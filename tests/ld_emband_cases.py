"""Panels, windows and host mirrors for the EM band tests (tests/test_ld_emband_host.py, tests/test_gpu_ld_emband.py) -- TEST
INFRASTRUCTURE ONLY, a plain module (imported like tests/ld_pwband_cases.py).  numpy only; everything is seeded; the mirrors
import ld_tools_amd.ops when they are called.

The sizes sit on the band kernel's loops (ldx_emband.hip): a tile is 128 rows x one 128-column slab, a K-block 256 haplotypes,
I block ti meets the slabs lo[128 ti] / 128 .. (r1 - 1) / 128, and a fixed grid of workgroups strides over the tile numbers.
The panels are those of ld_pwband_cases with an all-heterozygous row planted: a SNP without dosage variance that the EM counts
as live.  Expected cells never come from the band operators: they are the rectangle's (ops.ld_em), the list epilogue's
(ops.ld_em_from_counts on ld_em_pairwise_exact.pair_counts) or the 60-digit oracle's (ld_em_exact.solve).
"""
from __future__ import annotations

import numpy as np

import ld_band_cases as bc
import ld_em_exact as emx
import ld_em_pairwise_exact as epx
import ld_pairwise_exact as px
import ld_pwband_cases as pb

PW = pb.PW
N_MAIN = pb.N_MAIN                # six slabs (the last with 60 columns): six I blocks, the last ragged
MAIN_HAPS = (254, 1008)           # under one K-block; four K-blocks with a ragged last chunk
MAIN_WINDOW = pb.MAIN_WINDOW      # about 205 SNPs each side: an I block meets two to four slabs, mostly partly inside
TILES_WINDOW_SNPS = pb.TILES_WINDOW_SNPS
ROW_HET = 50                      # the planted all-heterozygous row (no copy of ld_codes reads it)
NBR_R2 = pb.NBR_R2
SAMPLED_CELLS = 400
GRID_CASE = (4100, 62)            # the everything window: 33 I blocks, 561 tiles -- more than a grid of two workgroups per CU
GRID_TILES = 561
GRID_HOLE_ROWS = (4099, 77)       # one hole-carrying row past row 4096, one inside column slab 0
SMALL_SIZES = (1, 129)
# past the first trip of the plan (ldx_band_plan.h: plan_kernel prefix-sums 256 I blocks per trip and carries the total on):
# 258 I blocks of 128 rows, blocks 256 (full) and 257 (77 rows) in the second trip; pb.ragged_positions, pb.PLAN_WINDOW
PLAN_TRIP = pb.PLAN_TRIP
PLAN_CASE = (128 * 257 + 77, 62)  # 32 973 SNPs
PLAN_WINDOW = pb.PLAN_WINDOW
PLAN_CELLS, PLAN_REACH, PLAN_TILES, PLAN_TILES_PAST = 836_438, 38, 515, 4   # pinned by tests/test_ld_emband_host.py
PLAN_HOLE_ROWS = slice(128 * 256, 128 * 257)   # plan_panel's only rows with holes: I block 256 = slab 256
PLAN_SAMPLED_FROM = 128 * 255     # the oracle's sample: rows of I blocks 255 and above
PLAN_SAMPLED_CELLS = 200

_CACHE = {}


def plant_het(codes) -> np.ndarray:
    """A writable copy with row ROW_HET all-heterozygous: every individual 0 | 1."""
    out = np.array(codes)
    if out.shape[0] > ROW_HET:
        out[ROW_HET, 0::2] = 0
        out[ROW_HET, 1::2] = 1
    return out


def _keep(key, build):
    if key not in _CACHE:
        codes = build()
        codes.setflags(write=False)
        _CACHE[key] = codes
    return _CACHE[key]


def mixed_panel(n: int, n_hap: int) -> np.ndarray:
    """pb.mixed_panel (holes, the structured and the special rows) with the all-heterozygous row."""
    return _keep(("mixed", n, n_hap), lambda: plant_het(pb.mixed_panel(n, n_hap)[0]))


def complete_panel(n: int, n_hap: int) -> np.ndarray:
    """pb.complete_panel (no holes; monomorphic and all-ALT rows) with the all-heterozygous row."""
    return _keep(("complete", n, n_hap), lambda: plant_het(pb.complete_panel(n, n_hap)))


def tiles_panel(n: int = N_MAIN, n_hap: int = 1008) -> np.ndarray:
    """pb.tiles_panel: holes in the rows pb.HOLE_ROWS only (slab 2), with the all-heterozygous row."""
    return _keep(("tiles", n, n_hap), lambda: plant_het(pb.tiles_panel(n, n_hap)))


def grid_panel() -> np.ndarray:
    """complete_panel at GRID_CASE with two hole-carrying rows: GRID_HOLE_ROWS."""
    def build():
        n, n_hap = GRID_CASE
        codes = plant_het(pb.complete_panel(n, n_hap))
        rng = np.random.default_rng(77)
        for row in GRID_HOLE_ROWS:
            codes[row] = (rng.random(n_hap) < 0.4).astype(np.int8)
            codes[row, rng.choice(n_hap, size=9, replace=False)] = 2
        return codes
    return _keep(("grid",), build)


def plan_panel() -> np.ndarray:
    """complete_panel at PLAN_CASE with holes (MISS) in the rows PLAN_HOLE_ROWS only: with PLAN_WINDOW the I blocks of
    plan_kernel's second trip hold clean x clean, holes x clean, clean x holes and holes x holes tiles."""
    def build():
        codes = plant_het(pb.complete_panel(*PLAN_CASE))
        px.add_holes(codes, np.random.default_rng(4245), rows=PLAN_HOLE_ROWS)
        return codes
    return _keep(("plan",), build)


def tile_kinds(codes, lo, first_block: int = 0) -> set:
    """{(holes in the I block, holes in the slab)} over the 128 x 128 tiles the band kernel walks for this layout, from I
    block ``first_block`` on."""
    holes = ~px.complete_rows(codes)
    n = codes.shape[0]
    kinds = set()
    for ti in range(first_block, (n + 127) // 128):
        r0, r1 = 128 * ti, min(128 * (ti + 1), n)
        for tj in range(int(lo[r0]) // 128, (r1 - 1) // 128 + 1):
            kinds.add((bool(holes[r0:r1].any()), bool(holes[128 * tj: 128 * (tj + 1)].any())))
    return kinds


def tiles_walked(lo, n: int, first_block: int = 0) -> int:
    """Tiles of the band kernel's walk: the sum over I blocks of 128 rows (from ``first_block`` on) of the slabs lo[128 ti] / 128
    .. (r1 - 1) / 128."""
    return sum((min(128 * (ti + 1), n) - 1) // 128 - int(lo[128 * ti]) // 128 + 1 for ti in range(first_block, (n + 127) // 128))


def own_counts(codes, pairwise: bool):
    """(N, A) int64 [n] over each SNP's own called individuals -- the diagonal of the oracle's pair counts; plain form: every
    individual, a missing code as REF."""
    codes = np.asarray(codes)
    if not pairwise:
        codes = np.where(codes == 1, 1, 0)
    q, g, _ = px.ind_planes(codes)
    return q.sum(axis=1).astype(np.int64), g.sum(axis=1).astype(np.int64)


def own_live(codes, pairwise: bool) -> np.ndarray:
    """bool [n]: 0 < A < 2 N over the SNP's own called individuals."""
    N, A = own_counts(codes, pairwise)
    return (A > 0) & (A < 2 * N)


def pair_counts(codes, rows, cols, pairwise: bool) -> np.ndarray:
    """int64 [5, m]: N A B S H of the pairs (rows[k], cols[k]) from epx.pair_counts over the rows involved."""
    codes = np.asarray(codes)
    if not pairwise:
        codes = np.where(codes == 1, 1, 0).astype(np.int8)
    out = np.zeros((5, len(rows)), dtype=np.int64)
    for k, (i, j) in enumerate(zip(rows, cols)):
        out[:, k] = epx.pair_counts(codes[i:i + 1], codes[j:j + 1])[:, 0, 0]
    return out


def sample_cells(rows, cols, live, count: int, seed: int) -> np.ndarray:
    """Up to ``count`` seeded cell numbers among the band's cells whose two SNPs are live."""
    cand = np.flatnonzero(live[rows] & live[cols])
    if cand.size > count:
        cand = np.sort(np.random.default_rng(seed).choice(cand, size=count, replace=False))
    return cand


def cells_pass_the_oracle(counts, r_cells, d_cells) -> list:
    """The sampled cells that miss emx.cells_ok against emx.solve on their own five integers (degenerate-within-the-pair tuples
    must be -0.0f in both)."""
    bad = []
    deg = epx.degenerate(counts)
    for k in range(counts.shape[1]):
        N, A, B, S, H = (int(x) for x in counts[:, k])
        r, d = np.float32(r_cells[k]), np.float32(d_cells[k])
        if deg[k]:
            if r.view(np.uint32) != 0x80000000 or d.view(np.uint32) != 0x80000000:
                bad.append((k, "degenerate", float(r), float(d)))
            continue
        if not emx.cells_ok(emx.solve(N, A, B, S, H), float(r), float(d)):
            bad.append((k, (N, A, B, S, H), float(r), float(d)))
    return bad


def expected_neighbors(n: int, rows, cols, r_values, d_values, bound):
    """(offsets int64 [n + 1], i, j, r float32, D' float32) of ldx_ld_em_neighbors_dev + the finishing step:
    pb.expected_neighbors' rule with D' in the fourth column -- the cells with r *f32 r >= bound and r not -0.0f, in both
    orientations, sorted by (i, j)."""
    r = np.asarray(r_values, dtype=np.float32)
    d = np.asarray(d_values, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.multiply(r, r, dtype=np.float32)
        keep = (s >= np.float32(bound)) & (r.view(np.uint32) != np.uint32(0x80000000))
    i = np.concatenate([rows[keep], cols[keep]])
    j = np.concatenate([cols[keep], rows[keep]])
    rr, dd = np.concatenate([r[keep], r[keep]]), np.concatenate([d[keep], d[keep]])
    order = np.lexsort((j, i))
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=offsets[1:])
    return offsets, i[order], j[order], rr[order], dd[order]


def band_cells(positions, window: int):
    """(lo, offsets, rows, cols) of the band layout of these positions: ops.band_layout_host and bc.cell_rows_cols."""
    from ld_tools_amd import ops
    lo, off = ops.band_layout_host(positions, window)
    rows, cols = bc.cell_rows_cols(lo, off)
    return lo, off, rows, cols

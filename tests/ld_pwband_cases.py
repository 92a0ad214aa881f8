"""Panels, windows and host mirrors for the pairwise-complete band tests (tests/test_ld_pwband_host.py,
tests/test_gpu_ld_pwband.py) -- TEST INFRASTRUCTURE ONLY, a plain module (imported like tests/ld_band_cases.py).  numpy only;
everything is seeded; the mirrors import ld_tools_amd.ops when they are called.

The sizes sit on the band kernel's loops (ldx_pwband.hip): a tile is 256 rows x one 128-column slab, a K-block 256 haplotypes,
I block ti meets the slabs lo[256 ti] / 128 .. (r1 - 1) / 128, and a fixed grid of workgroups strides over the tile numbers.
"""
from __future__ import annotations

import numpy as np

import ld_band_cases as bc
import ld_pairwise_exact as px
import ld_rect_cases as rc

PW = "pairwise"
N_MAIN = 700                      # three I blocks (the last with 188 rows), six slabs (the last with 60 columns)
MAIN_HAPS = (254, 1008, 1009)     # under one K-block; four K-blocks with a ragged last chunk; odd: the haplotype form only
SHIFT = 16                        # structured_rows' "side J" is the panel from row SHIFT on: its pairs are SHIFT rows apart
STEP_MAX = 40                     # ragged positions: steps of 0 .. 39, duplicates included
MAIN_WINDOW = 4000                # about 205 SNPs each side: every I block meets three or four slabs, most of them partly
TILES_WINDOW_SNPS = 300
HOLE_ROWS = slice(256, 384)       # the four-tile-kinds panel: holes in slab 2 = the first half of I block 1
NBR_R2 = 0.2
MIN_DECIDED_IN = px.MIN_DECIDED_IN
AMBIGUOUS_SHARE_MAX = px.AMBIGUOUS_SHARE_MAX
BIG_CASE = (130, 10240)           # an all-ALT row: the largest counts
GRID_CASE = (8269, 62)            # the everything window: 33 I blocks, 1 105 tiles -- more than a grid of two workgroups per CU
WALK_SIZES = (1, 257, 4096 + 130)
N_ANNOT = 3
# past the first trip of the plan (ldx_band_plan.h: plan_kernel prefix-sums 256 I blocks per trip and carries the total on):
# 258 I blocks, blocks 256 (full) and 257 (77 rows) in the second trip; ragged positions, about 25 SNPs each side
PLAN_TRIP = 256                   # I blocks per trip of plan_kernel
PLAN_CASE = (256 * 257 + 77, 62)  # 65 869 SNPs
PLAN_WINDOW = 500
PLAN_CELLS, PLAN_REACH, PLAN_TILES, PLAN_TILES_PAST = 1_669_273, 41, 772, 5   # pinned by tests/test_ld_pwband_host.py
# plan_panel's only rows with holes: the second slab of I block 256.  I block 257 starts at row 65 792, whose window reaches
# back to slab 513 and no further, so slab 513 is the one slab a hole-free I block of the second trip meets with holes in it
# (the block's first slab, 512, is met by block 256 alone: no clean x holes tile)
PLAN_HOLE_ROWS = slice(256 * 256 + 128, 256 * 256 + 256)

_CACHE = {}


def ragged_positions(n: int, seed: int = 5) -> np.ndarray:
    """Non-decreasing int64 positions with steps of 0 .. STEP_MAX - 1 (about one step in forty is a duplicate)."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(1000 + np.cumsum(rng.integers(0, STEP_MAX, size=n)).astype(np.int64))


def ld_codes(n: int, n_hap: int, rng) -> np.ndarray:
    """rc.random_codes with LD inside any window of a few SNPs: every fifth row is a 5 %-noisy copy of the row before it,
    every 35th an exact copy of the row three back, every 49th its complement."""
    codes = rc.random_codes(n, n_hap, rng)
    for k in range(10, n, 5):
        src = codes[k - 1].copy()
        flip = rng.random(n_hap) < 0.05
        src[flip & (src != 2)] ^= 1
        codes[k] = src
    for k in range(12, n, 35):
        codes[k] = codes[k - 3]
    for k in range(20, n, 49):
        src = codes[k - 3]
        codes[k] = np.where(src == 2, 2, 1 - src).astype(np.int8)
    return codes


def mixed_panel(n: int, n_hap: int):
    """(codes, {kind: planted}) -- ld_pairwise_exact's mixed panel as ONE panel: ld_codes, MISS of the codes missing in the rows
    with index % 3 != 0, structured_rows with the panel from row SHIFT on as its side J (so the disjoint pair is rows
    (7 + SHIFT, 7), the monomorphic-within-the-partner pair (10 + SHIFT, 10), the whole-individual rows SHIFT + r), and
    rc.special_rows on top.  Built once per process, read-only."""
    key = ("mixed", n, n_hap)
    if key not in _CACHE:
        rng = np.random.default_rng(31 * n + n_hap)
        codes = ld_codes(n, n_hap, rng)
        px.add_holes(codes, rng)
        done = px.structured_rows(codes, codes[SHIFT:]) if n > SHIFT + px.ROW_MONO else {}
        rc.special_rows(codes)
        codes.setflags(write=False)
        _CACHE[key] = (codes, done)
    return _CACHE[key]


def complete_panel(n: int, n_hap: int) -> np.ndarray:
    """ld_codes with every missing code made REF: a panel without holes (with monomorphic and all-ALT rows)."""
    key = ("complete", n, n_hap)
    if key not in _CACHE:
        codes = ld_codes(n, n_hap, np.random.default_rng(17 * n + n_hap))
        rc.special_rows(codes)
        codes[codes == 2] = 0
        codes.setflags(write=False)
        _CACHE[key] = codes
    return _CACHE[key]


def tiles_panel(n: int = N_MAIN, n_hap: int = 1008) -> np.ndarray:
    """complete_panel with holes (MISS) in the rows HOLE_ROWS only: with TILES_WINDOW_SNPS the launch holds clean x clean,
    holes x clean, clean x holes and holes x holes tiles."""
    key = ("tiles", n, n_hap)
    if key not in _CACHE:
        codes = np.array(complete_panel(n, n_hap))
        px.add_holes(codes, np.random.default_rng(4243), rows=HOLE_ROWS)
        codes.setflags(write=False)
        _CACHE[key] = codes
    return _CACHE[key]


def plan_panel() -> np.ndarray:
    """complete_panel at PLAN_CASE with holes (MISS) in the rows PLAN_HOLE_ROWS only: with PLAN_WINDOW the I blocks of
    plan_kernel's second trip hold clean x clean, holes x clean, clean x holes and holes x holes tiles."""
    key = ("plan",)
    if key not in _CACHE:
        codes = np.array(complete_panel(*PLAN_CASE))
        px.add_holes(codes, np.random.default_rng(4244), rows=PLAN_HOLE_ROWS)
        codes.setflags(write=False)
        _CACHE[key] = codes
    return _CACHE[key]


def tile_kinds(codes, lo, first_block: int = 0) -> set:
    """{(holes in the I block, holes in the slab)} over the tiles the band kernel walks for this layout, from I block
    ``first_block`` on."""
    holes = ~px.complete_rows(codes)
    n = codes.shape[0]
    kinds = set()
    for ti in range(first_block, (n + 255) // 256):
        r0, r1 = 256 * ti, min(256 * (ti + 1), n)
        for tj in range(int(lo[r0]) // 128, (r1 - 1) // 128 + 1):
            kinds.add((bool(holes[r0:r1].any()), bool(holes[128 * tj: 128 * (tj + 1)].any())))
    return kinds


def tiles_walked(lo, n: int, first_block: int = 0) -> int:
    """Tiles of the band kernel's walk: the sum over I blocks (from ``first_block`` on) of the slabs lo[256 ti] / 128 ..
    (r1 - 1) / 128."""
    return sum((min(256 * (ti + 1), n) - 1) // 128 - int(lo[256 * ti]) // 128 + 1 for ti in range(first_block, (n + 255) // 256))


def annot_matrix(n: int) -> np.ndarray:
    """bool [n, N_ANNOT]: three overlapping categories, one of them rare."""
    rng = np.random.default_rng(99 + n)
    return np.stack([rng.random(n) < 0.5, rng.random(n) < 0.3, rng.random(n) < 0.02], axis=1)


# ---- host mirrors: the band the operators must produce, from the numpy mirrors of ops alone ---------------------------------
def own_live(counts, dosage: bool) -> np.ndarray:
    """bool [n]: the SNP is polymorphic over its own called set, from the diagonal of the pairwise counts [sets, n, n]."""
    k = np.asarray(counts)
    d = [np.diagonal(k[s]).astype(np.int64) for s in range(k.shape[0])]
    if dosage:
        N, A, _, HA = d[0], d[1], d[2], d[3]
        return N * (A + 2 * HA) - A * A > 0
    n, a = d[0], d[1]
    return a * (n - a) > 0


def expected_band(codes, positions, window: int, dosage: bool) -> dict:
    """The band of ld_band(missing="pairwise"): lo, offsets, the cells' (rows, cols), values float32 [n_cells], diag, live."""
    from ld_tools_amd import ops
    counts = ops.pairwise_counts_host(codes, codes, dosage=dosage)
    cell = ops.pairwise_cell_host(counts, dosage)
    lo, off = ops.band_layout_host(positions, window)
    rows, cols = bc.cell_rows_cols(lo, off)
    lo_w, _ = ops.window_bounds(positions, min(int(window), ops.BAND_WINDOW_MAX))
    assert np.array_equal(lo_w, lo.astype(np.int64))
    live = own_live(counts, dosage)
    diag = np.where(live, np.float32(1.0), np.float32(-0.0)).astype(np.float32)
    return dict(lo=lo, offsets=off, rows=rows, cols=cols, values=np.ascontiguousarray(cell[rows, cols]), diag=diag, live=live,
                counts=counts)


def expected_sums(n: int, rows, cols, values, live, annot_bits=None, n_annot: int = 0) -> np.ndarray:
    """uint64 [n, 1 + n_annot]: ldx_ld_pw_score_dev's sums from a band's cells -- every cell's score_terms to both of its SNPs
    (word 1 + k where the OTHER SNP carries category k), every live SNP's own 2^32 (word 1 + k where it carries k itself)."""
    from ld_tools_amd import ops
    terms = ops.score_terms(values).astype(np.int64)
    own = np.where(live, np.int64(1) << 32, np.int64(0))
    out = np.zeros((n, 1 + n_annot), dtype=np.int64)
    out[:, 0] = bc.pair_sums(n, rows, cols, terms, own)
    for k in range(n_annot):
        has = ((np.asarray(annot_bits) >> k) & 1).astype(bool)
        s = np.where(has, own, 0)
        np.add.at(s, rows[has[cols]], terms[has[cols]])
        np.add.at(s, cols[has[rows]], terms[has[rows]])
        out[:, 1 + k] = s
    return out.view(np.uint64)


def expected_neighbors(n: int, rows, cols, values, bound):
    """(offsets int64 [n + 1], i, j, r float32, s float32) of ldx_ld_pw_neighbors_dev + the finishing step: the cells with
    r *f32 r >= bound and r not -0.0f, in both orientations, sorted by (i, j)."""
    r = np.asarray(values, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.multiply(r, r, dtype=np.float32)
        keep = (s >= np.float32(bound)) & (r.view(np.uint32) != np.uint32(0x80000000))
    i = np.concatenate([rows[keep], cols[keep]])
    j = np.concatenate([cols[keep], rows[keep]])
    rr, ss = np.concatenate([r[keep], r[keep]]), np.concatenate([s[keep], s[keep]])
    order = np.lexsort((j, i))
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=offsets[1:])
    return offsets, i[order], j[order], rr[order], ss[order]

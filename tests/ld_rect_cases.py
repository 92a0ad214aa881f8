"""Panels for the rectangular-LD tests (tests/test_ld_rect_host.py, tests/test_gpu_ld_rect.py) -- TEST INFRASTRUCTURE ONLY, a
plain module (imported like tests/ld_exact.py).  numpy only; everything is seeded.

The shapes sit on the rectangle kernel's edges, not on a workload's: a J slab is 128 SNPs, a workgroup's I block 256 rows (a
wave's 64), a K-block 256 haplotypes, and the last output tile is partial in both directions.
"""
from __future__ import annotations

import numpy as np

# (n_i, n_j) x n_hap of the oracle test: every n_hap with two shapes, every shape with at least two n_hap
SHAPES = ((1, 1), (5, 700), (700, 5), (129, 257), (300, 130))
EDGE_CASES = (
    ((1, 1), 2), ((129, 257), 2),
    ((5, 700), 254), ((300, 130), 254),
    ((700, 5), 256), ((129, 257), 256),
    ((1, 1), 258), ((300, 130), 258),
    ((5, 700), 1008), ((700, 5), 1008),
    ((129, 257), 5008), ((300, 130), 5008),
)
HITS_CASE = ((300, 130), 1008)      # two I blocks, two J slabs, both last tiles partial
FAMILY = 100                        # rows [0, FAMILY) of the hits panel's side I are noisy copies of FAMILY / 20 base rows
# the walk (tile_of, ldx_rect.hip): workgroups are numbered inside bands of 16 I blocks of 256 rows.  One full band; 16 + 1
# with one row in the last block; 16 + 2; the long side on J (35 slabs under one band); 16 + 16 + 1
I_BLOCK, BAND_BLOCKS = 256, 16
WALK_CASES = (
    ((4096, 130), 64),
    ((4097, 130), 254),
    ((4353, 257), 254),
    ((130, 4353), 254),
    ((8200, 130), 64),
)
WALK_HITS_CASE = ((4353, 257), 254)
WALK_SWAPPED = ((130, 4353), 254)   # WALK_HITS_CASE's two panels swapped, side I cut to 130 rows: see walk_codes


def random_codes(n_snps: int, n_hap: int, rng, miss: float = 0.005) -> np.ndarray:
    """int8 [n_snps, n_hap]: ALT with a per-SNP frequency from (0.05, 0.95), `miss` of the codes missing (2); rows with
    index % 3 == 0 carry no missing code (their exact copies and complements then give r = +-1 exactly)."""
    f = rng.uniform(0.05, 0.95, size=(n_snps, 1))
    codes = (rng.random((n_snps, n_hap)) < f).astype(np.int8)
    holes = rng.random((n_snps, n_hap)) < miss
    holes[0::3] = False
    codes[holes] = 2
    return codes


def special_rows(codes: np.ndarray) -> None:
    """Degenerate rows in place, where the panel has room: monomorphic REF, all ALT, all missing."""
    n = codes.shape[0]
    if n >= 5:
        codes[1] = 0
        codes[n // 2] = 1
        codes[n - 1] = 2


def pair_codes(n_i: int, n_j: int, n_hap: int, seed: int, family: int = 0):
    """Two independent code matrices over the same haplotypes with copies planted across them: of side J's rows about 1/4
    are exact copies of a side-I row (|r| = 1 where the source has no missing code and is not degenerate), 1/8 complements
    (r = -1) and 1/8 copies with a tenth of the codes flipped.  ``family``: side I's first rows are 2 %-noisy copies of
    family / 20 base rows, and half of the planted rows take their source there (many hits per planted column)."""
    rng = np.random.default_rng(seed)
    ci = random_codes(n_i, n_hap, rng)
    cj = random_codes(n_j, n_hap, rng)
    if family:
        assert n_i > family + 3 * (family // 20) + 3 and family % 20 == 0
        for k in range(family):
            base = ci[(family + 2) // 3 * 3 + 3 * (k // 20)].copy()   # a row beyond the family without missing codes (index % 3 == 0)
            flip = rng.random(n_hap) < 0.02
            base[flip & (base != 2)] ^= 1
            ci[k] = base
    special_rows(ci)
    special_rows(cj)
    for b in range(n_j):
        u = rng.random()
        if u >= 0.5:
            continue
        lo, hi = (0, family) if family and rng.random() < 0.5 else (0, n_i)
        src = ci[int(rng.integers(lo, hi))].copy()
        if u < 0.25:
            cj[b] = src
        elif u < 0.375:
            cj[b] = np.where(src == 2, 2, 1 - src).astype(np.int8)
        else:
            flip = rng.random(n_hap) < 0.1
            src[flip & (src != 2)] ^= 1
            cj[b] = src
    return ci, cj


def pair_seed(shape, n_hap: int) -> int:
    return 1000 * shape[0] + shape[1] + n_hap


def walk_codes(shape, n_hap: int):
    """The two code matrices of a WALK_CASES entry: pair_codes, so copies and complements are planted across the sides.
    (130, 4353) takes the panels of (4353, 257) swapped -- side I is the first 130 rows of that case's side J, side J its
    side I -- so that its cells are the transpose of that case's first 130 columns."""
    if (shape, n_hap) == WALK_SWAPPED:
        ci, cj = walk_codes(*WALK_HITS_CASE)
        assert ci.shape[0] == shape[1] and cj.shape[0] >= shape[0]
        return np.ascontiguousarray(cj[:shape[0]]), ci
    return pair_codes(shape[0], shape[1], n_hap, seed=pair_seed(shape, n_hap))


def walk_bands(n_i: int):
    """I blocks per band of the walk, in order: [16, 16, ..., the rest]."""
    blocks = (n_i + I_BLOCK - 1) // I_BLOCK
    return [min(BAND_BLOCKS, blocks - b) for b in range(0, blocks, BAND_BLOCKS)]


def triangle_panel():
    """The panel of the bit-for-bit test against the r32 triangle: 400 x 1008 with missing codes, monomorphic, all-ALT and
    all-missing rows; ``rows`` in arbitrary order with a repeat, ``cols`` another list that shares SNPs with it."""
    rng = np.random.default_rng(20261)
    codes = random_codes(400, 1008, rng, miss=0.01)
    codes[[3, 77, 256]] = 0
    codes[[4, 130, 399]] = 1
    codes[[5, 255]] = 2
    for k in range(10, 60, 5):                 # some real LD: near copies of a neighbour
        src = codes[k - 1].copy()
        flip = rng.random(1008) < 0.05
        src[flip & (src != 2)] ^= 1
        codes[k] = src
    rows = rng.permutation(400)[:150].astype(np.int64)
    rows[:6] = [3, 4, 5, 256, 130, 255]        # the degenerate rows take part
    rows[17], rows[20] = rows[3], rows[10]     # repeats: of a degenerate row and of an ordinary one
    cols = np.concatenate([rng.permutation(400)[:200], rows[:40]]).astype(np.int64)
    cols = cols[rng.permutation(cols.size)]
    return codes, rows, cols

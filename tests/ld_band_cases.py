"""Positions, windows and synthetic cells for the stored-band tests past the kernels' strides (tests/test_ld_band_host.py,
tests/test_gpu_ld_band.py) -- TEST INFRASTRUCTURE ONLY, a plain module (imported like tests/ld_rect_cases.py).  numpy only;
everything is seeded.

The sizes sit on the kernels' loops, not on a workload's: the layout kernel's one workgroup walks the SNPs in tiles of 4096
and carries offsets[base] between them; the sweep's workgroup of 16 rows walks its columns in spans of 2048; the store's band
passes walk 128-column tiles.
"""
from __future__ import annotations

import numpy as np

import ld_exact as lx

LAYOUT_TILE = 4096                # SNPs per tile of band_layout_kernel
SWEEP_SPAN = 2048                 # columns per span of band_sweep_kernel
SWEEP_ROWS = 16                   # rows per workgroup of band_sweep_kernel

# either side of one tile, two tiles, three tiles and a ragged fourth
layout_sizes = (4095, 4096, 4097, 8192, 8193, 3 * 4096 + 77)
# everything in one window: offsets[n] = n (n - 1) / 2 > 2^32, the carry between tiles crosses 32 bits
layout_size_64 = 92_700
assert layout_size_64 * (layout_size_64 - 1) // 2 > 1 << 32

CLUSTER_RUNS = (2500, 1, 15, 1984)   # SNPs per run; all SNPs of a run share one position
CLUSTER_STEP = 7                     # distance of consecutive runs


def grid(n: int) -> np.ndarray:
    """SNPs 100 apart."""
    return 1 + 100 * np.arange(n, dtype=np.int64)


def clustered(n: int) -> np.ndarray:
    """Runs of 2500, 1, 15 and 1984 SNPs, repeated until n SNPs are placed; the SNPs of a run share one position and
    consecutive runs are 7 apart.  With window 0 each run is one window: a reach of 2499, and lo jumps at rows (2500, 2501,
    2516, ...) that are no multiple of 16."""
    runs = []
    placed = 0
    while placed < n:
        for length in CLUSTER_RUNS:
            runs.append(length)
            placed += length
            if placed >= n:
                break
    pos = np.repeat(1 + CLUSTER_STEP * np.arange(len(runs), dtype=np.int64), runs)[:n]
    return np.ascontiguousarray(pos)


def ragged(n: int) -> np.ndarray:
    """The ragged spacing of ld_exact.score_windows (steps of 0 .. 39, duplicates included)."""
    pos, w = lx.score_windows(n, n)[6]
    assert w == 150
    return pos


def position_cases(n: int):
    """(positions, window) pairs of the layout tests."""
    g, c, r = grid(n), clustered(n), ragged(n)
    return [
        (g, 0), (g, 300), (g, 100 * 2100), (g, int(g[-1])),
        (c, 0), (c, CLUSTER_STEP),
        (r, 150),
        (r + (np.int64(1) << 50), 150),      # differences in doubles stay exact
        (g, 1 << 62),                        # acts as 2^52: everything
    ]


def position_cases_64(n: int = layout_size_64):
    """The two cases of the large layout: the everything window (offsets beyond 2^32) and clustered runs with window 0."""
    g = grid(n)
    return [(g, int(g[-1])), (clustered(n), 0)]


def sweep_cases(n: int = 4500):
    """(positions, window) of the consumer and store tests: the everything window (a reach of n - 1: three spans), the grid
    with 2100 SNPs each side (two spans; jmin is no multiple of 2048 after the first rows) and clustered runs with window 0
    (lo jumps inside a 16-row group whose first rows reach back 2499 columns)."""
    g = grid(n)
    return [(g, int(g[-1])), (g, 100 * 2100), (clustered(n), 0)]


CELL_SEEDS = (11, 12, 13)            # synthetic_cells' seed per sweep case (values; values2 takes seed + 100)
BIG_SHARE = 1.0 / 4096.0             # of the cells, with big=True
BIG_VALUES = (2.0 ** 22, -2.0 ** 22, 2.0 ** 23, -2.0 ** 23, 2.0 ** 30, -2.0 ** 30)
SPECIAL_SHARE = 1.0 / 64.0


def synthetic_cells(n_cells: int, seed: int, big: bool = False) -> np.ndarray:
    """float32 [n_cells]: uniform in (-1, 1), sprinkled with +0.0, -0.0, exact +-1 and values near 2^-20; with ``big`` about
    one cell in 4096 is +-2^22, +-2^23 or +-2^30 (the matvec clamp is reached, and a SNP that collects several such cells
    wraps its 64-bit sum).  No NaN, no infinity."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, size=n_cells).astype(np.float32)
    v[np.abs(v) >= 1.0] = np.float32(0.5)                              # (the float32 rounding of a double just below 1)
    special = np.flatnonzero(rng.random(n_cells) < SPECIAL_SHARE)
    kind = rng.integers(0, 6, size=special.size)
    tiny = (np.ldexp(1.0 + rng.random(special.size), -20) * np.where(rng.random(special.size) < 0.5, -1.0, 1.0))
    table = np.stack([np.zeros(special.size), -np.zeros(special.size), np.ones(special.size), -np.ones(special.size), tiny,
                      -tiny])
    v[special] = table[kind, np.arange(special.size)].astype(np.float32)
    if big:
        where = np.flatnonzero(rng.random(n_cells) < BIG_SHARE)
        v[where] = np.asarray(BIG_VALUES, dtype=np.float32)[rng.integers(0, len(BIG_VALUES), size=where.size)]
    assert np.isfinite(v).all()
    return v


def cell_rows_cols(lo, offsets):
    """(rows, cols) int64 of every stored cell in layout order, the way LDBand.to_csr derives them."""
    lo = np.asarray(lo).astype(np.int64)
    off = np.asarray(offsets).astype(np.int64)
    n = lo.size
    length = np.arange(n, dtype=np.int64) - lo
    rows = np.repeat(np.arange(n, dtype=np.int64), length)
    cols = np.arange(off[n], dtype=np.int64) - np.repeat(off[:-1] - lo, length)
    return rows, cols


CHUNK_ROWS = 4096                    # band_chunks' default height


def band_chunks(lo, offsets, height: int = CHUNK_ROWS):
    """The band in chunks of ``height`` rows, for a reference that is computed on sub-rectangles: yields
    ((a, b), (c0, b), cells, li, lj) -- the rows [a, b), the columns [c0, b) with c0 = lo[a] (lo is non-decreasing and a cell's
    column is below its row, so they hold every cell of those rows), the cell numbers of those rows in layout order (int64,
    consecutive) and the cells' (row - a, column - c0).  Nothing of size n x n is built."""
    lo = np.asarray(lo).astype(np.int64)
    off = np.asarray(offsets).astype(np.int64)
    n = lo.size
    for a in range(0, n, height):
        b = min(a + height, n)
        c0 = int(lo[a])
        length = np.arange(a, b, dtype=np.int64) - lo[a:b]
        cells = np.arange(off[a], off[b], dtype=np.int64)
        li = np.repeat(np.arange(b - a, dtype=np.int64), length)
        lj = cells - np.repeat(off[a:b] - lo[a:b], length) - c0
        yield (a, b), (c0, b), cells, li, lj


def pair_sums(n: int, rows, cols, terms, own=None) -> np.ndarray:
    """int64 [n]: every cell's term added to both of its SNPs, plus the SNPs' own terms; int64 addition wraps, as the
    kernels' 64-bit words do."""
    sums = np.zeros(n, dtype=np.int64) if own is None else np.array(own, dtype=np.int64)
    with np.errstate(over="ignore"):
        np.add.at(sums, rows, terms)
        np.add.at(sums, cols, terms)
    return sums

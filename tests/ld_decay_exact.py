"""Exact LD decay histograms from tests/ld_exact.py's integers, and the case list of the LD-decay tests.

Numpy only; nothing of ld_tools_amd except synth (through ld_exact) for the panels.  A pair is i > j with
d = pos_i - pos_j <= window, both SNPs live (a r > 0) and kept; its bin is d // bin_width in int64; the reference sum of a bin
is the float64 sum of the exact r^2 = num^2 / den2 of its pairs (each within 2^-53 relative, nothing beside the bound below).

Bound of the sums (the LD-score test's, per bin): the kernel's cell is within 4 float32 ulps of r, its float32 square within
(1 + 4 2^-23)^2 (1 + 2^-24) - 1 < 2^-19 of r^2 (tests/ld_exact.py), and each term rint(2^32 s) adds at most 2^-33:
    |sum_r2[b] - exact[b]| <= 2^-19 exact[b] + counts[b] 2^-33.
"""
import numpy as np

import ld_exact as lx

MAX_BINS = 1024                   # LDX_DECAY_MAX_BINS
SMALL_SNPS = (1, 2, 127, 128, 129, 300)
SMALL_HAPS = (64, 333)
PANELS = list(lx.LONG_RANGE)[:2] + [(n, h) for h in SMALL_HAPS for n in SMALL_SNPS]   # lr1000, lr700, edge panels
assert PANELS[:2] == ["lr1000", "lr700"]

_SMALL = {}


def panel(key):
    """(codes, Exact) of a case panel: a long-range panel by name or edge_panel(n, h); built once, never modified."""
    if isinstance(key, str):
        codes, _, ex = lx.long_range_panel(key)
        return codes, ex
    if key not in _SMALL:
        codes = lx.edge_panel(*key)
        codes.setflags(write=False)
        _SMALL[key] = (codes, lx.Exact(codes))
    return _SMALL[key]


def n_bins(window: int, width: int) -> int:
    return int(window) // int(width) + 1


def bin_widths(window: int):
    """1, 7, 100, the window itself (two bins, the last holding only d == window) and window + 1 (one bin) -- each only
    where it is a width (>= 1: a window of 0 keeps its single-bin cases) and gives at most MAX_BINS bins (the operator
    refuses more)."""
    out = []
    for w in (1, 7, 100, int(window), int(window) + 1):
        if w >= 1 and n_bins(window, w) <= MAX_BINS and w not in out:
            out.append(w)
    return out


def cases(key):
    """[(positions, window, width)] of a panel: the seven windows of ld_exact.score_windows times bin_widths."""
    n = panel(key)[1].n_snps
    return [(pos, w, bw) for pos, w in lx.score_windows(n, n) for bw in bin_widths(w)]


def pairs(ex, positions, window: int, keep=None):
    """(rows, cols, d) of the counted pairs."""
    pos = np.asarray(positions, dtype=np.int64)
    ok = ex.live.copy()
    if keep is not None:
        ok &= np.asarray(keep, dtype=bool)
    rows, cols = np.tril_indices(ex.n_snps, -1)
    d = pos[rows] - pos[cols]
    assert (d >= 0).all()
    sel = (d <= int(window)) & ok[rows] & ok[cols]
    return rows[sel], cols[sel], d[sel]


def exact_decay(ex, positions, window: int, width: int, keep=None):
    """(counts int64 [n_bins], float64 sums of exact r^2 [n_bins])."""
    rows, cols, d = pairs(ex, positions, window, keep)
    b = d // int(width)
    nb = n_bins(window, width)
    counts = np.bincount(b, minlength=nb).astype(np.int64)
    sums = np.bincount(b, weights=ex.r2_64[rows, cols], minlength=nb)
    return counts, sums


def bound(exact, counts):
    return 2.0 ** -19 * exact + counts * 2.0 ** -33


def keep_mask(n: int) -> np.ndarray:
    """About 70 % of the SNPs."""
    return np.random.default_rng(1000 + n).random(n) < 0.7

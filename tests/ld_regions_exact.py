"""Exact cross-LD profiles from tests/ld_exact.py's integers, brute-force optimal cuts, and the case list of the LD-region
tests.

Numpy only; nothing of ld_tools_amd except synth (through ld_exact) for the panels.  cross[k] is the float64 sum of the exact
r^2 = num^2 / den2 over the pairs j < k <= i with pos_i - pos_j <= window and both SNPs live (a r > 0); pairs[k] counts them.

Bound (the LD-decay test's, derived in tests/ld_decay_exact.py, applied per cut): the kernel's cell is within 4 float32 ulps
of r, its float32 square within 2^-19 of r^2, and each term rint(2^32 s) adds at most 2^-33:
    |cross_r2[k] - exact[k]| <= 2^-19 exact[k] + pairs[k] 2^-33.
The profile is a prefix sum of integer differences of one-sided sums, exact modulo 2^64, so it is the plain sum of the terms
of the straddling pairs and the per-term bound carries over unchanged.
"""
from itertools import combinations

import numpy as np

import ld_decay_exact as dx
import ld_exact as lx

PANELS = dx.PANELS                # lr1000, lr700 and the edge panels (n, h), n in {1, 2, 127, 128, 129, 300}, h in {64, 333}
panel = dx.panel


def cases(key):
    """[(positions, window)]: the seven windows of ld_exact.score_windows."""
    n = panel(key)[1].n_snps
    return lx.score_windows(n, n)


def exact_cross(ex, positions, window: int):
    """(float64 [n + 1] sums of exact r^2, int64 [n + 1] pair counts) per cut k = 0 .. n."""
    rows, cols, _ = dx.pairs(ex, positions, window)
    n = ex.n_snps
    # counts: the pair (i, j), i > j, straddles the cuts j + 1 .. i -- a difference array, summed once (integers)
    cnt = np.zeros(n + 2, dtype=np.int64)
    np.add.at(cnt, cols + 1, 1)
    np.add.at(cnt, rows + 1, -1)
    # sums: only additions of non-negative numbers (no cancelling differences).  M holds the counted pairs' r^2 below the
    # diagonal; C[i][k - 1] = sum over j < k of M[i][j]; cross[k] = sum over i >= k of C[i][k - 1].  Relative error below
    # 2 n 2^-53, nothing beside the bound.
    M = np.zeros((n, n), dtype=np.float64)
    M[rows, cols] = ex.r2_64[rows, cols]
    exact = np.zeros(n + 1, dtype=np.float64)
    exact[1:] = np.tril(np.cumsum(M, axis=1), -1).sum(axis=0)
    return exact, np.cumsum(cnt)[:n + 1]


def bound(exact, pairs):
    return dx.bound(exact, pairs)


def cross_loops(r32, positions, window, live=None):
    """The definition as a double loop over an r32 square: uint64 [n + 1] of Python-integer sums of the terms."""
    from ld_tools_amd import ops
    n = r32.shape[0]
    pos = np.asarray(positions, dtype=np.int64)
    t = ops.score_terms(r32).astype(object)
    out = [0] * (n + 1)
    for i in range(n):
        for j in range(i):
            if pos[i] - pos[j] <= window and (live is None or (live[i] and live[j])):
                for k in range(j + 1, i + 1):
                    out[k] += int(t[i, j])
    return np.asarray(out, dtype=np.uint64)


# ---- optimal cuts by enumeration ---------------------------------------------------------------------------------------
def admissible(n, cuts, mn, mx):
    edges = [0, *cuts, n]
    return all(mn <= b - a <= mx for a, b in zip(edges, edges[1:]))


def brute_split(cost, mn, mx):
    """Every admissible cut set of n = len(cost) - 1 SNPs (n <= 14): (minimum total, the cut set the recurrence's tie rule
    picks) or None.  cost[k]: the cost of a cut before SNP k.  Every prefix of an optimal set is optimal for its end point
    (a cheaper prefix would give a cheaper set), so "prev[k] is the LARGEST p at the minimum", followed back from n, picks
    among the optimal sets the one with the largest last cut, then the largest cut before it, and so on, "no further cut"
    (p = 0) ranking lowest: the maximum of the reversed cut tuples in Python's tuple order."""
    n = len(cost) - 1
    best, sets = None, []
    for m in range(n):
        for cuts in combinations(range(1, n), m):
            if not admissible(n, cuts, mn, mx):
                continue
            total = sum(int(cost[c]) for c in cuts)
            if best is None or total < best:
                best, sets = total, [cuts]
            elif total == best:
                sets.append(cuts)
    if best is None:
        return None
    return best, max(sets, key=lambda c: tuple(reversed(c)))


def split_cases():
    """[(cost uint64 [n + 1] already shifted left by 16, min, max)] for n <= 14: random small integers with many ties, all
    zeros, min == max, min = 1, max >= n."""
    rng = np.random.default_rng(11)
    out = []
    for n in (1, 2, 3, 5, 8, 11, 14):
        for mn, mx in ((1, 1), (1, n), (1, n + 5), (2, 3), (3, 3), (2, 5), (3, 7), (4, 14), (n, n)):
            if not 1 <= mn <= mx:
                continue
            for kind in ("ties", "zero", "wide"):
                c = {"ties": rng.integers(0, 3, size=n + 1), "zero": np.zeros(n + 1, dtype=np.int64),
                     "wide": rng.integers(0, 1 << 40, size=n + 1)}[kind]
                # low bits below the shift must not matter: fill them with noise
                cross = (c.astype(np.uint64) << np.uint64(16)) | rng.integers(0, 1 << 16, size=n + 1).astype(np.uint64)
                out.append((cross, mn, mx))
    return out

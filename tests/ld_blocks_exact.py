"""An exact oracle for the four-gamete test and its haplotype blocks, and the panels of the block tests -- TEST
INFRASTRUCTURE ONLY, a plain module (imported like tests/ld_exact.py).

Written from the definitions in include/ldx.h (ldx_ld_fgt_dev, ldx_ld_blocks_dev) alone; numpy and the standard library only,
nothing of ld_tools_amd except synth (through ld_exact) for the random panels.  With A = (codes == 1), a = row sums of A,
n = n_hap and n11 = A A^T (integers):

    g11 = n11,  g10 = a_i - n11,  g01 = a_j - n11,  g00 = n - a_i - a_j + n11        ("not ALT" is the other allele)
    (i, j), i > j, is RECOMBINANT at m  iff  min(g11, g10, g01, g00) >= m,
    evaluated iff keep_i, keep_j and pos_i - pos_j <= window
    left[i] = 1 + max{ j < i : (i, j) recombinant }, 0 if none

and the partition walks the kept SNPs left to right: with s the current block's first SNP, i starts a block iff there is none,
or (i, j) is recombinant for some s <= j < i, or pos_i - pos_s > window.  Everything is integers: equality, no tolerance.

Random panels are useless for blocks (96-97 % of the pairs of lr1000 / lr700 are recombinant), so the panels here are
PERFECT PHYLOGENIES per block: a random laminar family of haplotype subsets (the ranges of a random recursive split of a
random haplotype order), every SNP a clade or its complement -- two such SNPs show at most three gametes.  About 10 % of the
rows then get 1-3 flipped haplotypes (so min_count 1, 2 and 4 disagree), 0.2 % of the codes go missing, and pairs built from
counts (conftest.realise) whose smallest gamete count is exactly c are planted for every c in {m - 1, m} at row distances
128 k + {0, 1, 127}.
"""
from collections import Counter

import numpy as np

import ld_exact as lx

NOT_KEPT = 0xFFFFFFFF
BASE_COUNTS = (1, 2, 4)                # min_count of every panel, and ceil(0.01 n_hap) beside them

# lengths: the perfect-phylogeny blocks in order (1, 2, ~130 and >= 300 SNPs among them); `long`: the index of the block that the
# plants keep out of (it crosses two 128-column tile boundaries); plants: (first source row, k list) -- distances 128 k + delta
PHYLO = {
    "ph700": dict(n_snps=700, n_hap=333, seed=17, lengths=(1, 2, 37, 310, 1, 2, 32, 130, 60, 125), long=3,
                  plants=((0, (3,)), (352, (1,)))),
    "ph1000": dict(n_snps=1000, n_hap=1008, seed=12, lengths=(1, 2, 57, 320, 2, 1, 130, 140, 47, 300), long=3,
                   plants=((0, (3, 4)), (384, (1, 2)))),
    "ph300": dict(n_snps=300, n_hap=64, seed=13, lengths=(1, 2, 130, 1, 2, 164), long=None, plants=((0, (1,)),)),
}
assert all(sum(p["lengths"]) == p["n_snps"] for p in PHYLO.values())


def min_counts(n_hap: int):
    """The min_count values of a panel's tests: 1, 2, 4 and Haploview's ceil(0.01 n_hap)."""
    return sorted(set(BASE_COUNTS) | {max(1, -(-n_hap // 100))})


class Gametes:
    """Exact gamete counts of one int8 code matrix [n_snps, n_hap] (1 = ALT, anything else: not ALT)."""

    def __init__(self, codes, n11=None):
        codes = np.asarray(codes)
        assert codes.ndim == 2 and codes.dtype == np.int8
        self.n_snps, self.n_hap = codes.shape
        n = np.int64(self.n_hap)
        self.a = (codes == 1).sum(axis=1).astype(np.int64)
        if n11 is None:
            n11 = lx.alt_counts_gemm(codes)              # int64 A A^T (an exact float32 GEMM, checked there)
        g10 = self.a[:, None] - n11
        g01 = self.a[None, :] - n11
        g00 = n - self.a[:, None] - self.a[None, :] + n11
        self.min_gamete = np.minimum(np.minimum(n11, g10), np.minimum(g01, g00))   # int64 [n, n], symmetric
        assert int(self.min_gamete.min(initial=0)) >= 0 and np.array_equal(self.min_gamete, self.min_gamete.T)


def min_gamete_by_tuples(codes, i: int, j: int) -> int:
    """The same count, in pure Python, from the multiset of observed (x, y) haplotypes."""
    seen = Counter((int(x) == 1, int(y) == 1) for x, y in zip(codes[i], codes[j]))
    return min(seen.get((p, q), 0) for p in (True, False) for q in (True, False))


def tested(positions, window: int, keep=None) -> np.ndarray:
    """bool [n, n]: the pairs (i, j), i > j, that the test evaluates."""
    pos = np.asarray(positions, dtype=np.int64)
    n = pos.shape[0]
    d = pos[:, None] - pos[None, :]
    t = np.tril(np.ones((n, n), dtype=bool), -1) & (d <= int(window))
    assert (d[np.tril_indices(n, -1)] >= 0).all()
    if keep is not None:
        k = np.asarray(keep, dtype=bool)
        t &= k[:, None] & k[None, :]
    return t


def recombinant(g: Gametes, positions, window: int, min_count: int, keep=None) -> np.ndarray:
    """bool [n, n] (lower triangle): evaluated and recombinant."""
    return tested(positions, window, keep) & (g.min_gamete >= int(min_count))


def exact_left(rec) -> np.ndarray:
    """uint32 [n]: 1 + the highest recombinant column of every row, 0 if none."""
    n = rec.shape[0]
    return np.where(rec, np.arange(1, n + 1, dtype=np.int64)[None, :], 0).max(axis=1, initial=0).astype(np.uint32)


def exact_partition(rec, positions, window: int, keep=None):
    """(block_of uint32 [n], n_blocks, rm, causes) straight from the recombinant matrix (not through `left`): causes[b] is
    'first', 'left' or 'window' for block b ('left' outranks 'window')."""
    pos = np.asarray(positions, dtype=np.int64)
    n = pos.shape[0]
    kept = np.ones(n, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    block_of = np.full(n, NOT_KEPT, dtype=np.uint32)
    causes = []
    s = None
    for i in range(n):
        if not kept[i]:
            continue
        if s is None:
            causes.append("first")
            s = i
        elif rec[i, s:i].any():
            causes.append("left")
            s = i
        elif pos[i] - pos[s] > window:
            causes.append("window")
            s = i
        block_of[i] = len(causes) - 1
    return block_of, len(causes), causes.count("left"), causes


def blocks_of(block_of):
    """[(first, last)] of the blocks of a block_of array (kept SNPs only)."""
    kept = np.flatnonzero(np.asarray(block_of) != NOT_KEPT)
    b = np.asarray(block_of)[kept].astype(np.int64)
    assert (np.diff(b) >= 0).all() and (np.diff(b) <= 1).all() and (b.size == 0 or b[0] == 0)
    cuts = np.flatnonzero(np.diff(b) != 0) + 1
    return [(int(m[0]), int(m[-1])) for m in np.split(kept, cuts) if m.size]


def check_invariants(block_of, g: Gametes, positions, window: int, min_count: int, keep=None):
    """On the exact matrix: no recombinant pair inside a block, every span <= window, every non-first start justified."""
    pos = np.asarray(positions, dtype=np.int64)
    kept = np.ones(g.n_snps, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    rec = g.min_gamete >= int(min_count)
    prev = None
    for first, last in blocks_of(block_of):
        idx = np.arange(first, last + 1)[kept[first:last + 1]]
        sub = rec[np.ix_(idx, idx)]
        assert not np.tril(sub, -1).any(), ("a recombinant pair inside a block", first, last)
        assert pos[last] - pos[first] <= window, ("a block wider than the window", first, last)
        if prev is not None:        # the start: a recombinant partner inside the previous block, or beyond the window of its first SNP
            pidx = np.arange(prev[0], first)[kept[prev[0]:first]]
            by_left = bool((rec[first, pidx] & (pos[first] - pos[pidx] <= window)).any())
            assert by_left or pos[first] - pos[prev[0]] > window, ("an unjustified block start", first)
        prev = (first, last)


# ---- panels ------------------------------------------------------------------------------------------------------------
def laminar_family(rng, n_hap: int):
    """The ranges [lo, hi) of a random recursive split of 0 .. n_hap (every proper non-empty node), over a random order of
    the haplotypes: any two of the sets are nested or disjoint."""
    order = rng.permutation(n_hap)
    ranges, stack = [], [(0, n_hap)]
    while stack:
        lo, hi = stack.pop()
        if hi - lo < n_hap:
            ranges.append((lo, hi))
        if hi - lo >= 2:
            cut = int(rng.integers(lo + 1, hi))
            stack += [(lo, cut), (cut, hi)]
    return order, ranges


def planted_pair(n: int, c: int, variant: int):
    """Two complete rows whose smallest gamete count is exactly c, the smallest being g11 / g10 / g01 / g00 by `variant`;
    built from counts as the fixtures are (conftest.realise)."""
    from conftest import realise
    rest = n - c
    big = [rest // 3, rest // 3, rest - 2 * (rest // 3)]
    assert min(big) > c
    g = big[:variant] + [c] + big[variant:]                    # g11, g10, g01, g00
    a1, a2 = g[0] + g[1], g[0] + g[2]
    r1, r2 = realise(n, g[0], a1, n - a1, a2, n - a2)
    return np.asarray(r1, dtype=np.int8), np.asarray(r2, dtype=np.int8)


def thresholds(n_hap: int):
    """The smallest gamete counts to plant: m - 1 and m for every m the tests use."""
    return sorted({c for m in min_counts(n_hap) for c in (m - 1, m)})


def phylo_codes(name: str):
    """(codes int8 [n, h], plants [(source row, planted row, c)], (first, last + 1) of the long block or None)."""
    spec = PHYLO[name]
    n, h = spec["n_snps"], spec["n_hap"]
    rng = np.random.default_rng(spec["seed"])
    codes = np.zeros((n, h), dtype=np.int8)
    row, long_range = 0, None
    for b, length in enumerate(spec["lengths"]):
        order, ranges = laminar_family(rng, h)
        if b == spec["long"]:
            long_range = (row, row + length)
        for _ in range(length):
            lo, hi = ranges[int(rng.integers(len(ranges)))]
            allele = np.zeros(h, dtype=np.int8)
            allele[order[lo:hi]] = 1
            codes[row] = 1 - allele if rng.random() < 0.5 else allele
            row += 1
    flip = np.flatnonzero(rng.random(n) < 0.10)
    for i in flip:                                             # 1-3 flipped haplotypes: a fourth gamete of 1-3 copies
        at = rng.choice(h, size=int(rng.integers(1, 4)), replace=False)
        codes[i, at] = 1 - codes[i, at]
    codes[rng.random((n, h)) < 0.002] = 2                      # missing: counts with REF
    used = set(range(*long_range)) if long_range else set()
    plants, idx = [], 0
    cs = thresholds(h)
    for start, ks in spec["plants"]:
        src = start
        for c in cs:
            for delta in lx.PLANT_DELTAS:
                dist = 128 * ks[idx % len(ks)] + delta
                while src in used or src + dist in used:
                    src += 1
                assert src + dist < n, (name, c, dist)
                codes[src], codes[src + dist] = planted_pair(h, c, idx % 4)
                used |= {src, src + dist}
                plants.append((src, src + dist, c))
                idx += 1
    return codes, plants, long_range


_PANELS = {}
SMALL_SNPS = (1, 2, 127, 128, 129, 300)
SMALL_HAPS = (64, 333)
EDGE_PANELS = [(n, h) for h in SMALL_HAPS for n in SMALL_SNPS]


def panel(key):
    """(codes, Gametes) of a case panel: a phylogeny panel or a long-range panel by name, or edge_panel(n, h); built once
    per process, never modified."""
    if key not in _PANELS:
        n11 = None
        if isinstance(key, str) and key in PHYLO:
            codes = phylo_codes(key)[0]
        elif isinstance(key, str):
            codes, _, ex = lx.long_range_panel(key)
            n11 = ex.n11                                 # (the same GEMM, already done for the other oracles)
        else:
            codes = lx.edge_panel(*key)
        codes = np.array(codes)
        codes.setflags(write=False)
        _PANELS[key] = (codes, Gametes(codes, n11))
    return _PANELS[key]


def windows(key):
    """[(positions, window)]: the seven cases of ld_exact.score_windows."""
    n = panel(key)[0].shape[0]
    return lx.score_windows(n, n)


def keep_mask(n: int) -> np.ndarray:
    """About 70 % of the SNPs."""
    return np.random.default_rng(2000 + n).random(n) < 0.7

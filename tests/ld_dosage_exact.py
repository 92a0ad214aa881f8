"""An exact oracle for genotype-dosage LD (the dosage r32 cells, LD scores and neighbour lists), computed from the allele
codes with integers -- TEST INFRASTRUCTURE ONLY, a plain module like tests/ld_exact.py, whose decision classes it reuses.

Written from the definitions in include/ldx.h ("genotype-dosage LD") alone; numpy and the standard library only.  With N =
n_hap / 2 individuals (individual k owns haplotypes 2k and 2k + 1) and g = the number of code-1 alleles of an individual
(REF, missing and any other code count 0):

    a = sum g      hom = #{g == 2}      Q = sum g^2 = a + 2 hom      v = N Q - a^2        0 <= v <= N^2 < 2^25
    S_ij = sum_k g_ik g_jk              <= 4 N = 20 480 < 2^24: a float32 GEMM of g is exact in any summation order
    num  = N S_ij - a_i a_j             int64, |num| < 2^27 at n_hap <= 10 240
    den2 = v_i v_j                      int64, <= N^4 < 2^50 (so its float64 conversion is exact; asserted on the values)
    r    = num / sqrt(den2)             r^2 = num^2 / den2  (num^2 < 2^54: an exact int64)

A SNP with v == 0 is degenerate (its cells are -0.0f, its diagonal too); a pair with num == 0 has the cell +0.0f; the
diagonal of a SNP with v > 0 is exactly 1.

Threshold decisions: the contract puts a cell within 4 float32 ulps of exact r, as for the haplotype cells, and the kept test
is the same float32 comparison, so ld_exact's derivation of the 2^-19 relative margin holds unchanged; Exact.classes /
Exact._at_least are inherited (they read num2, den2, r2_64 and degenerate only, and decide near an edge with Python ints).
"""
from __future__ import annotations

import numpy as np

import ld_exact as lx
from ld_exact import AMBIGUOUS, IN, MARGIN, OUT, pair_classes, tile_crossing, ulp32_err, window_mask  # noqa: F401

MAX_HAPS = lx.MAX_HAPS


def dosages(codes) -> np.ndarray:
    """int64 [n_snps, N]: code-1 alleles per individual."""
    alt = np.asarray(codes) == 1
    return alt[:, 0::2].astype(np.int64) + alt[:, 1::2].astype(np.int64)


def dosage_gemm(g, block: int = 512) -> np.ndarray:
    """S int64 [n, n] from a blocked float32 GEMM of the dosages (exact: every partial sum <= 4 N < 2^24)."""
    G = g.astype(np.float32)
    n = G.shape[0]
    assert 4 * G.shape[1] < (1 << 24)
    out = np.empty((n, n), dtype=np.int64)
    for r0 in range(0, n, block):
        blk = G[r0:r0 + block] @ G.T
        out[r0:r0 + block] = blk.astype(np.int64)
        assert np.array_equal(out[r0:r0 + block].astype(np.float32), blk)   # integers, nothing lost
    return out


class DosageExact(lx.Exact):
    """Exact dosage pair statistics of one int8 code matrix [n_snps, n_hap], n_hap even."""

    def __init__(self, codes):   # (not Exact.__init__: other counts, the same attribute names)
        codes = np.asarray(codes)
        assert codes.ndim == 2 and codes.dtype == np.int8
        self.n_snps, self.n_hap = codes.shape
        assert 2 <= self.n_hap <= MAX_HAPS and self.n_hap % 2 == 0
        self.n_ind = self.n_hap // 2
        N = np.int64(self.n_ind)
        self.g = dosages(codes)
        self.a = self.g.sum(axis=1)
        self.hom = (self.g == 2).sum(axis=1)
        self.q = (self.g * self.g).sum(axis=1)
        assert np.array_equal(self.q, self.a + 2 * self.hom)
        self.v = N * self.q - self.a * self.a
        assert int(self.v.min(initial=0)) >= 0 and int(self.v.max(initial=0)) <= int(N) ** 2 < (1 << 25)
        self.S = dosage_gemm(self.g)
        assert np.array_equal(np.diagonal(self.S), self.q) and np.array_equal(self.S, self.S.T)
        assert int(self.S.max(initial=0)) <= 4 * self.n_ind
        self.num = N * self.S - np.multiply.outer(self.a, self.a)
        assert np.array_equal(np.diagonal(self.num), self.v)
        self.den2 = np.multiply.outer(self.v, self.v)
        # nothing overflows and every conversion to float64 below is exact: the bounds of the module docstring on the values
        assert int(np.abs(self.num).max(initial=0)) < (1 << 27)
        assert int(self.den2.max(initial=0)) < (1 << 50) and int(self.den2.min(initial=0)) >= 0
        self.num2 = self.num * self.num
        assert int(self.num2.max(initial=0)) < (1 << 54)
        self.live = self.v > 0
        self.degenerate = self.den2 == 0
        self.zero_num = (self.num == 0) & ~self.degenerate
        den = np.where(self.degenerate, 1, self.den2).astype(np.float64)
        self.r64 = np.where(self.degenerate, 0.0, self.num.astype(np.float64) / np.sqrt(den))
        self.r2_64 = np.where(self.degenerate, 0.0, self.num2.astype(np.float64) / den)
        self._classes = {}

    def diagonal(self) -> np.ndarray:
        """float64 [n]: 1 for a SNP whose dosage varies, 0 for a degenerate one (whose cell is -0.0f)."""
        return self.live.astype(np.float64)


class DosageExactBlock(lx.ExactBlock):
    """ExactBlock's dosage counterpart: the rows of one code matrix against the rows of another over the same individuals
    (n_hap even) -- the off-diagonal block of DosageExact(stacked), each attribute [n_i, n_j]."""

    def __init__(self, codes_i, codes_j):   # (not ExactBlock.__init__: other counts, the same attribute names)
        codes_i, codes_j = np.asarray(codes_i), np.asarray(codes_j)
        assert codes_i.ndim == codes_j.ndim == 2 and codes_i.dtype == codes_j.dtype == np.int8
        assert codes_i.shape[1] == codes_j.shape[1]
        self.n_i, self.n_j, self.n_hap = codes_i.shape[0], codes_j.shape[0], codes_i.shape[1]
        assert 2 <= self.n_hap <= MAX_HAPS and self.n_hap % 2 == 0
        self.n_ind = self.n_hap // 2
        N = np.int64(self.n_ind)
        g_i, g_j = dosages(codes_i), dosages(codes_j)
        self.a_i, self.a_j = g_i.sum(axis=1), g_j.sum(axis=1)
        self.v_i = N * (g_i * g_i).sum(axis=1) - self.a_i * self.a_i
        self.v_j = N * (g_j * g_j).sum(axis=1) - self.a_j * self.a_j
        for v in (self.v_i, self.v_j):
            assert int(v.min(initial=0)) >= 0 and int(v.max(initial=0)) <= int(N) ** 2 < (1 << 25)
        assert 4 * self.n_ind < (1 << 24)
        G, H = g_i.astype(np.float32), g_j.astype(np.float32)
        self.S = np.empty((self.n_i, self.n_j), dtype=np.int64)
        for r0 in range(0, self.n_i, 512):
            blk = G[r0:r0 + 512] @ H.T
            self.S[r0:r0 + 512] = blk.astype(np.int64)
            assert np.array_equal(self.S[r0:r0 + 512].astype(np.float32), blk)   # integers, nothing lost
        assert int(self.S.max(initial=0)) <= 4 * self.n_ind
        self._finish(N * self.S - np.multiply.outer(self.a_i, self.a_j), np.multiply.outer(self.v_i, self.v_j))


# ---- the panels of tests/test_gpu_ld_dosage.py, pinned on the CPU by tests/test_ld_dosage_host.py -----------------------
# n_snps x n_hap: everything degenerate; the tiny case (n_hap % 4 == 2: the last individual sits in the upper half of the
# last nibble group); the chunk tail; the K-block boundary (256 haplotypes) from both sides; three tiles (diagonal,
# off-diagonal and edge units); LDX_MAX_HAPS, where an all-ALT row against itself gives S = 4 N = 20 480.
SHAPES = [(1, 2), (5, 6), (130, 130), (129, 254), (129, 256), (129, 258), (300, 1008), (130, 10240)]
NEIGHBOUR_R2 = 0.2
AMBIGUOUS_SHARE_MAX = 0.01        # of the in-window ordered pairs, per panel and window
MIN_DECIDED_IN = 50               # ordered pairs, on every panel of more than 128 SNPs (a smaller one has no second tile)


def all_het_row(n_hap: int, seed: int) -> np.ndarray:
    """Every individual heterozygous, the ALT allele on a random side: a r > 0 but v == 0."""
    first = np.random.default_rng(seed).integers(0, 2, size=n_hap // 2).astype(np.int8)
    row = np.empty(n_hap, dtype=np.int8)
    row[0::2], row[1::2] = first, 1 - first
    return row


def _source_row(codes, k: int) -> np.ndarray:
    """Row k made complete (missing -> REF) and, if its dosage then has no variance, given three genotype classes."""
    h = codes.shape[1]
    row = np.where(codes[k] == 1, 1, 0).astype(np.int8)
    g = row[0::2] + row[1::2]
    if h >= 4 and g.min() == g.max():
        row[:] = 0
        row[: 2 * ((h // 2 + 2) // 3)] = 1        # a third of the individuals 1|1
        row[h - 1] = 1                            # ... and one 0|1
    return row


def special_rows(codes):
    """Plant the special SNPs in place, as far as the rows last.  From 8 SNPs on: a monomorphic SNP, an all-ALT SNP, an
    all-heterozygous SNP, a SNP with second-ALT codes (2), a duplicate pair (r = 1) and a complementary pair (r = -1); the
    pairs sit next to each other and, from 300 SNPs on, also 128 + 1 and 128 + 127 rows apart (the next two tiles).  Fewer rows
    keep the head of the list [source, duplicate, complement, all-het, code 2]; one row is the all-het SNP.  Returns
    {kind: [rows]}."""
    n, h = codes.shape
    where = {}
    if n == 1:
        codes[0] = all_het_row(h, 1)
        return {"all_het": [0]}
    src = _source_row(codes, 0)
    plan = [("source", src), ("duplicate", src), ("complement", (1 - src).astype(np.int8)), ("all_het", all_het_row(h, n + h))]
    two = codes[4 % n].copy()
    two[::3] = 2                                   # every third allele a second ALT: g counts code 1 only
    two[1] = 1
    plan += [("code2", two), ("mono", np.zeros(h, dtype=np.int8)), ("all_alt", np.ones(h, dtype=np.int8))]
    for k, (kind, row) in enumerate(plan):
        if k < n:
            codes[k] = row
            where.setdefault(kind, []).append(k)
    if n >= 300:
        far = _source_row(codes, 20)
        codes[20] = far
        codes[20 + 128 + 1] = far
        codes[20 + 128 + 127] = 1 - far
        where["source"].append(20)
        where["duplicate"].append(20 + 128 + 1)
        where["complement"].append(20 + 128 + 127)
    return where


_PANELS = {}


def panel(shape):
    """(codes, {kind: rows}, DosageExact) of one shape of SHAPES: LD blocks 200 SNPs long (LD that crosses 128-column
    tiles), missing codes in half of the rows, the special rows on top.  Built once per process, never modified."""
    if shape not in _PANELS:
        from ld_tools_amd import synth
        n, h = shape
        codes = synth.synth_codes_host(n, h, seed=3 * n + h, block_len=200, rho=0.97, miss=0.01, miss_rows=0.5)
        where = special_rows(codes)
        codes.setflags(write=False)
        _PANELS[shape] = (codes, where, DosageExact(codes))
    return _PANELS[shape]


def positions(n: int) -> np.ndarray:
    """SNPs 100 apart."""
    return 1 + 100 * np.arange(n, dtype=np.int64)


def neighbour_windows(n: int):
    """(positions, window): everything, and 129 SNPs each side (cuts tiles)."""
    pos = positions(n)
    return [(pos, int(pos[-1])), (pos, 100 * 129)]


def score_windows(n: int, seed: int):
    """(positions, window_bp) in base pairs: self only, everything, 129 SNPs each side, ragged spacing with duplicates."""
    pos = positions(n)
    ragged = np.cumsum(np.random.default_rng(seed).integers(0, 40, size=n)).astype(np.int64) + 7
    return [(pos, 0), (pos, int(pos[-1])), (pos, 100 * 129), (ragged, 1500)]


def rephase(codes, seed: int) -> np.ndarray:
    """The same genotypes written another way: per SNP the two alleles of random individuals swapped (the order inside an
    unphased call is arbitrary), then the individuals permuted.  Dosages, a, hom and S are unchanged up to that permutation
    of the individuals (S, a, hom: unchanged); the haplotype columns are not a permutation of the old ones."""
    rng = np.random.default_rng(seed)
    n, h = codes.shape
    pairs = np.array(codes).reshape(n, h // 2, 2)
    swap = rng.random((n, h // 2)) < 0.5
    pairs[swap] = pairs[swap][:, ::-1]
    return np.ascontiguousarray(pairs[:, rng.permutation(h // 2)].reshape(n, h))


def rephased(shape) -> np.ndarray:
    """panel(shape)'s codes in another phase and order of individuals (rephase), read-only, built once per process."""
    key = ("rephased", shape)
    if key not in _PANELS:
        out = rephase(panel(shape)[0], seed=shape[0] + shape[1] + 1)
        out.setflags(write=False)
        _PANELS[key] = out
    return _PANELS[key]

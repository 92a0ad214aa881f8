"""An exact oracle for pairwise-complete LD (ops.ld_rect(missing="pairwise"), ops.ld_rect_counts), computed from the allele
codes with integers -- TEST INFRASTRUCTURE ONLY, a plain module like tests/ld_dosage_exact.py -- and the panels of
tests/test_ld_pairwise_host.py and tests/test_gpu_ld_pairwise.py.

Written from the definitions in include/ldx.h ("pairwise-complete LD") alone; numpy and the standard library only.  For row x
of side I and row y of side J over the same n_hap haplotypes (code 1 = ALT, 0 = REF, anything else missing):

  haplotype form   over the haplotypes called in both rows:
      n    a = #{x = 1}    b = #{y = 1}    c = #{x = 1 and y = 1}
      num = c n - a b                  v_x = a (n - a)              v_y = b (n - b)
  dosage form      individual k owns haplotypes 2k and 2k + 1 and is called at a SNP when BOTH codes are 0 or 1; g = its ALT
                   dosage; over the individuals called at both SNPs:
      N    A = sum g_x    B = sum g_y    HA = #{g_x = 2}    HB = #{g_y = 2}    S = sum g_x g_y
      num = S N - A B                  v_x = N (A + 2 HA) - A^2     v_y = N (B + 2 HB) - B^2
  den2 = v_x v_y       r = num / sqrt(den2)       r^2 = num^2 / den2

Bounds (asserted on the values): every count <= 10 240 (S <= 20 480), so |num| < 2^27; 0 <= v <= n^2 / 4 (haplotype form) and
0 <= v <= N^2 (dosage form: N times the sum of g^2 minus the squared sum is N^2 times a variance of values in [0, 2], largest
with half the individuals at 0 and half at 2), both <= 5120^2, so den2 < 2^50.  den2 = 0 is the degenerate pair (cell -0.0f;
n = 0 and N = 0 included), num = 0 the cell +0.0f.  The counts come from float32 GEMMs of 0/1/2 matrices: every partial sum is an
integer <= 20 480 < 2^24, exact in any order (checked on the values).

Threshold decisions: the cell is within 4 float32 ulps of exact r and the kept test is the same float32 comparison as for the
plain rectangle, so ld_exact's 2^-19 relative margin holds unchanged; Exact.classes / Exact._at_least are reused as they are
(they read num2, den2, r2_64 and degenerate only).
"""
from __future__ import annotations

import numpy as np

import ld_exact as lx
import ld_rect_cases as rc
from ld_exact import AMBIGUOUS, IN, OUT, ulp32_err  # noqa: F401

MAX_HAPS = lx.MAX_HAPS
HAP_SETS = ("n", "a", "b", "c")
DOSAGE_SETS = ("N", "A", "B", "HA", "HB", "S")


def _gemm(x, y) -> np.ndarray:
    """int64 x @ y.T through float32, exact (asserted)."""
    X, Y = x.astype(np.float32), y.astype(np.float32)
    out = np.empty((X.shape[0], Y.shape[0]), dtype=np.int64)
    for r0 in range(0, X.shape[0], 512):
        blk = X[r0:r0 + 512] @ Y.T
        out[r0:r0 + 512] = blk.astype(np.int64)
        assert np.array_equal(out[r0:r0 + 512].astype(np.float32), blk) and float(blk.max(initial=0.0)) < (1 << 24)
    return out


def hap_planes(codes):
    """(called, alt) int64 [n_snps, n_hap] of one side."""
    codes = np.asarray(codes)
    return ((codes == 0) | (codes == 1)).astype(np.int64), (codes == 1).astype(np.int64)


def ind_planes(codes):
    """(called, g, hom) int64 [n_snps, N] of one side: an individual is called when both of its codes are 0 or 1; g and hom
    are 0 where it is not."""
    called, alt = hap_planes(codes)
    q = called[:, 0::2] * called[:, 1::2]
    g = (alt[:, 0::2] + alt[:, 1::2]) * q
    return q, g, (g == 2).astype(np.int64)


def complete_rows(codes) -> np.ndarray:
    """bool [n_snps]: the row has no missing code."""
    codes = np.asarray(codes)
    return ((codes == 0) | (codes == 1)).all(axis=1)


class PairwiseExactBlock(lx.ExactBlock):
    """Exact pairwise-complete statistics of the rows of one code matrix against the rows of another: ExactBlock's attributes
    (num, den2, num2, degenerate, zero_num, r64, r2_64), each [n_i, n_j], plus ``counts`` int64 [4 or 6, n_i, n_j] in the
    order of include/ldx.h, ``names`` and one attribute per count."""

    classes = lx.Exact.classes          # the decision classes of ld_exact, on this block's num2 / den2
    _at_least = lx.Exact._at_least

    def __init__(self, codes_i, codes_j, dosage: bool = False):   # (not ExactBlock.__init__: other counts, the same attribute names)
        codes_i, codes_j = np.asarray(codes_i), np.asarray(codes_j)
        assert codes_i.ndim == codes_j.ndim == 2 and codes_i.dtype == codes_j.dtype == np.int8
        assert codes_i.shape[1] == codes_j.shape[1]
        self.n_i, self.n_j, self.n_hap = codes_i.shape[0], codes_j.shape[0], codes_i.shape[1]
        assert 1 <= self.n_hap <= MAX_HAPS
        self.dosage = bool(dosage)
        if dosage:
            assert self.n_hap % 2 == 0
            (qi, gi, hi), (qj, gj, hj) = ind_planes(codes_i), ind_planes(codes_j)
            N, A, B = _gemm(qi, qj), _gemm(gi, qj), _gemm(qi, gj)
            HA, HB, S = _gemm(hi, qj), _gemm(qi, hj), _gemm(gi, gj)
            self.names, sets = DOSAGE_SETS, (N, A, B, HA, HB, S)
            assert int(N.max(initial=0)) <= self.n_hap // 2 and int(S.max(initial=0)) <= 2 * self.n_hap
            assert (A <= 2 * N).all() and (B <= 2 * N).all() and (2 * HA <= A).all() and (2 * HB <= B).all()
            num = S * N - A * B
            v_x, v_y = N * (A + 2 * HA) - A * A, N * (B + 2 * HB) - B * B
            assert int(max(v_x.max(initial=0), v_y.max(initial=0))) <= (self.n_hap // 2) ** 2
        else:
            (ci, ai), (cj, aj) = hap_planes(codes_i), hap_planes(codes_j)
            n, a, b, c = _gemm(ci, cj), _gemm(ai, cj), _gemm(ci, aj), _gemm(ai, aj)
            self.names, sets = HAP_SETS, (n, a, b, c)
            assert int(n.max(initial=0)) <= self.n_hap and (a <= n).all() and (b <= n).all() and (c <= a).all() and (c <= b).all()
            num = c * n - a * b
            v_x, v_y = a * (n - a), b * (n - b)
            assert 4 * int(max(v_x.max(initial=0), v_y.max(initial=0))) <= self.n_hap ** 2
        assert int(v_x.min(initial=0)) >= 0 and int(v_y.min(initial=0)) >= 0
        self.counts = np.stack(sets)
        for name, k in zip(self.names, sets):
            setattr(self, name, k)
        self.v_x, self.v_y = v_x, v_y
        den2 = v_x * v_y
        assert int(np.abs(num).max(initial=0)) < (1 << 27) and int(den2.max(initial=0)) < (1 << 50)   # this oracle's own bounds
        self._finish(num, den2)
        self._classes = {}


# ---- panels ---------------------------------------------------------------------------------------------------------------
MISS = 0.05                       # the missing rate of the rows that carry holes (index % 3 != 0)
HITS_R2 = 0.2
AMBIGUOUS_SHARE_MAX = 0.01        # of the pairs of the hits panel
MIN_DECIDED_IN = 50
BIG_CASE = ((130, 130), 10240)    # an all-ALT complete row against itself reaches the largest counts
TILES_CASE = ((300, 257), 1008)   # holes confined to rows [128, 256) of each side: four tile kinds in one launch
WALK_CASE = ((4097, 130), 254)    # one I block more than a band of 4096 rows (either form), one row in it; two J slabs
ROW_HALF, ROW_DISJOINT, ROW_MONO = 4, 7, 10   # the structured rows (index % 3 == 1: rows that may hold holes)


def add_holes(codes, rng, miss: float = MISS, rows=None) -> None:
    """Missing codes (2) at rate ``miss`` in place, in the rows of the slice ``rows`` whose index % 3 != 0."""
    holes = rng.random(codes.shape) < miss
    holes[0::3] = False
    if rows is not None:
        keep = np.zeros(codes.shape[0], dtype=bool)
        keep[rows] = True
        holes[~keep] = False
    codes[holes] = 2


def structured_rows(ci, cj) -> dict:
    """Plant the structured cases in place where the panels have room (n_hap >= 8); returns {kind: what was planted}.
      individual   a whole individual (haplotypes 2, 3) missing in every row of side J's first slab with index % 3 != 0
      half         side I's row 4: every fourth individual half-missing, its other allele ALT
      disjoint     row 7 of side I is called on the first half of the individuals only, row 7 of side J on the second: n = 0
      mono         row 10 of side J misses the first third of the individuals; row 10 of side I has its only ALT alleles there:
                   polymorphic, but monomorphic within that partner's called set"""
    h = ci.shape[1]
    done = {}
    if h < 8:
        return done
    rows = [r for r in range(min(128, cj.shape[0])) if r % 3]
    if rows:
        cj[rows, 2:4] = 2
        done["individual"] = rows
    if ci.shape[0] > ROW_HALF:
        ci[ROW_HALF, 0::8] = 2
        ci[ROW_HALF, 1::8] = 1
        done["half"] = ROW_HALF
    cut = (h // 4) * 2
    if ci.shape[0] > ROW_DISJOINT and cj.shape[0] > ROW_DISJOINT:
        ci[ROW_DISJOINT, cut:] = 2
        cj[ROW_DISJOINT, :cut] = 2
        done["disjoint"] = ROW_DISJOINT
    third = max(2, (h // 6) * 2)
    if ci.shape[0] > ROW_MONO and cj.shape[0] > ROW_MONO:
        cj[ROW_MONO, :third] = 2
        cj[ROW_MONO, third:] = np.where(np.arange(h - third) % 3 == 0, 1, 0)
        ci[ROW_MONO] = 0
        ci[ROW_MONO, 0:third:2] = 1
        done["mono"] = ROW_MONO
    return done


_PANELS = {}


def mixed_pair(shape, n_hap: int, family: int = 0):
    """(codes_i, codes_j, {kind: planted}) of one case: rc.pair_codes with the missing rate of the rows that carry holes raised
    to MISS, the structured rows, and rc.special_rows again on top (the monomorphic, all-ALT and all-missing rows stay what
    they are).  Built once per process, read-only."""
    key = ("mixed", shape, n_hap, family)
    if key not in _PANELS:
        ci, cj = rc.pair_codes(shape[0], shape[1], n_hap, seed=rc.pair_seed(shape, n_hap), family=family)
        rng = np.random.default_rng(7 * rc.pair_seed(shape, n_hap) + 1)
        add_holes(ci, rng)
        add_holes(cj, rng)
        done = structured_rows(ci, cj)
        rc.special_rows(ci)
        rc.special_rows(cj)
        ci.setflags(write=False)
        cj.setflags(write=False)
        _PANELS[key] = (ci, cj, done)
    return _PANELS[key]


def complete_pair(shape, n_hap: int):
    """(codes_i, codes_j) of rc.pair_codes with every missing code made REF: a panel without holes."""
    key = ("complete", shape, n_hap)
    if key not in _PANELS:
        ci, cj = rc.pair_codes(shape[0], shape[1], n_hap, seed=rc.pair_seed(shape, n_hap))
        ci[ci == 2] = 0
        cj[cj == 2] = 0
        ci.setflags(write=False)
        cj.setflags(write=False)
        _PANELS[key] = (ci, cj)
    return _PANELS[key]


def tiles_pair():
    """TILES_CASE: complete_pair's codes with holes (MISS) only in rows [128, 256) of each side -- the tiles of the launch are
    clean x clean, holes x clean, clean x holes and holes x holes."""
    key = ("tiles",)
    if key not in _PANELS:
        shape, n_hap = TILES_CASE
        ci, cj = (np.array(c) for c in complete_pair(shape, n_hap))
        rng = np.random.default_rng(4242)
        add_holes(ci, rng, rows=slice(128, 256))
        add_holes(cj, rng, rows=slice(128, 256))
        ci.setflags(write=False)
        cj.setflags(write=False)
        _PANELS[key] = (ci, cj)
    return _PANELS[key]


def permute_individuals(codes, seed: int) -> np.ndarray:
    """The same panel with its individuals (pairs of haplotype columns; an odd last haplotype stays) in another order."""
    n, h = codes.shape
    perm = np.random.default_rng(seed).permutation(h // 2)
    out = np.array(codes)
    out[:, : 2 * (h // 2)] = np.array(codes)[:, : 2 * (h // 2)].reshape(n, h // 2, 2)[:, perm].reshape(n, 2 * (h // 2))
    return out


def rephase(codes, seed: int) -> np.ndarray:
    """The same genotypes written another way: per SNP the two alleles of random individuals swapped (a half-missing call
    stays half-missing)."""
    n, h = codes.shape
    pairs = np.array(codes).reshape(n, h // 2, 2)
    swap = np.random.default_rng(seed).random((n, h // 2)) < 0.5
    pairs[swap] = pairs[swap][:, ::-1]
    return np.ascontiguousarray(pairs.reshape(n, h))

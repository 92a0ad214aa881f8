"""An exact oracle for unphased LD by EM (include/ldx.h, "unphased LD by EM"): the maximum-likelihood double-heterozygote
split x*, and from it r and D', to 60 decimal digits and more -- TEST INFRASTRUCTURE ONLY, a plain module like tests/ld_exact.py.
Written from the definitions in include/ldx.h alone; numpy and the standard library only (`decimal`, no mpmath).

    counts   a_i, a_j, S = sum g_i g_j, H = #{g_i = g_j = 1}: integer GEMMs of the dosages g and of (g == 1)
    table    n1 = (S - H) / 2, n2 = a_i - n1 - H, n3 = a_j - n1 - H, n4 = T - a_i - a_j + n1        (T = 2 N)
    g(x)     = 2 x^3 + c2 x^2 + c1 x + c0 with integer coefficients; its critical points come from the quadratic g', and on
             each monotone piece of [0, H] a root is bracketed by the signs at the ends and refined inside the bracket (Newton
             steps that stay inside it, bisection otherwise) until the step is below 10^-52
    l(x)     = n1 ln h1 + n2 ln h2 + n3 ln h3 + n4 ln h4 + H ln(h1 h4 + h2 h3) with Decimal.ln (0 ln 0 = 0); only computed
             where [0, H] holds more than one root
    x*       the root with the largest l; near_best = the roots whose l is within 1e-9 (1 + |l_best|) of it

A pair is AMBIGUOUS if near_best holds two distinct x (more than 10^-20 apart): an exact or near tie of two local maxima,
which the kernel may resolve either way (its rule decides exact ties of ITS fp64 l, not of the real one).  A cell passes if it
is within tolerance of the exact value at ANY near-best x: ties are accepted this way, not excluded.

Tolerance of a float32 cell against the exact v: |cell - v| <= 2 ulp32(v) + 2^-40.  The fp64 evaluation of the algorithm is
measured on the CPU to stay within 2.5e-14 < 2^-45 of the exact value (tests/test_ld_em_host.py prints the maximum), so 2^-40
leaves a 32-fold margin; half an ulp is the float32 rounding, the second ulp covers the final division.
"""
from __future__ import annotations

import math
from decimal import Decimal, localcontext
from functools import lru_cache

import numpy as np

import ld_dosage_exact as dx
import ld_rect_cases as rc

PREC = 80          # the results are asked to 60 digits; the rest keeps the root search's last steps above its own rounding
ABS_TOL = 2.0 ** -40
ULPS = 2.0
DISTINCT = Decimal(10) ** -20
STEP = Decimal(10) ** -52

# the kernel's workgroup tile is 128 x 128 (one slab of I x one slab of J), not the rectangle's 256 x 128: (129, 257) is one
# row past one tile and one column past two, (257, 129) the same the other way round
TILE = 128
TILE_CASES = (((257, 129), 256),)
# the kernel's walk: bands of 32 I blocks of 128 rows; one row into the second band, two J slabs
WALK_CASE = ((4097, 130), 254)
COUNT_CASES = tuple(c for c in rc.EDGE_CASES if c[1] % 2 == 0) + TILE_CASES
BIG_CASE = ((5, 130), 10240)          # all-ALT x all-ALT gives S = 20 480, all-het x all-het H = 5 120
DENSE_CASES = (((129, 257), 2), ((129, 257), 254), ((129, 257), 256), ((129, 257), 258), ((300, 130), 1008), BIG_CASE)


# ---- counts ------------------------------------------------------------------------------------------------------------------
def pair_counts(codes_i, codes_j):
    """(N, a_i [n_i], a_j [n_j], S [n_i, n_j], H [n_i, n_j]) as int64, from integer GEMMs of g and of (g == 1)."""
    gi, gj = dx.dosages(codes_i), dx.dosages(codes_j)
    assert gi.shape[1] == gj.shape[1]
    n_ind = gi.shape[1]
    S = gi @ gj.T
    H = (gi == 1).astype(np.int64) @ (gj == 1).astype(np.int64).T
    assert S.dtype == np.int64 and H.dtype == np.int64
    return n_ind, gi.sum(axis=1), gj.sum(axis=1), S, H


def table(n_ind, a_i, a_j, S, H):
    """(n1, n2, n3, n4) as Python ints, or None for a tuple that is no genotype table."""
    N, a_i, a_j, S, H = int(n_ind), int(a_i), int(a_j), int(S), int(H)
    T = 2 * N
    if min(a_i, a_j, S, H) < 0 or a_i > T or a_j > T or H > N or S < H or (S - H) % 2:
        return None
    n1 = (S - H) // 2
    n2, n3, n4 = a_i - n1 - H, a_j - n1 - H, T - a_i - a_j + n1
    if min(n2, n3, n4) < 0:
        return None
    assert n1 + n2 + n3 + n4 + 2 * H == T
    return n1, n2, n3, n4


def live_tables(n_ind):
    """(a_i, a_j, S, H) of every 3 x 3 genotype table of n_ind individuals with 0 < a_i, a_j < T, one entry per table (tables
    that share a tuple repeat it)."""
    out = []

    def rec(cells, left):
        if len(cells) == 8:
            t = cells + [left]
            a_i = sum((k // 3) * t[k] for k in range(9))
            a_j = sum((k % 3) * t[k] for k in range(9))
            if 0 < a_i < 2 * n_ind and 0 < a_j < 2 * n_ind:
                out.append((a_i, a_j, sum((k // 3) * (k % 3) * t[k] for k in range(9)), t[4]))
            return
        for c in range(left + 1):
            rec(cells + [c], left - c)

    rec([], n_ind)
    return out


# ---- the solution of one tuple ---------------------------------------------------------------------------------------------
class Solution:
    """roots: the roots of g in [0, H], ascending (Decimal); ell: their l (None where there is one root only); best: x*;
    near_best: the roots accepted for a cell; three_real: the cubic has three distinct real roots (anywhere on the line)."""

    def __init__(self, key, n, roots, ell, three_real):
        self.key, self.n, self.roots, self.ell, self.three_real = key, n, roots, ell, three_real
        if len(roots) == 1:
            self.best, self.near_best = roots[0], [roots[0]]
        else:
            top = max(ell)
            slack = Decimal("1e-9") * (1 + abs(top))
            self.best = roots[ell.index(top)]
            self.near_best = [x for x, l in zip(roots, ell) if top - l <= slack]
        self.ambiguous = self.near_best[-1] - self.near_best[0] > DISTINCT

    def values(self, x):
        """(r, D') at x as Decimals."""
        n_ind, a_i, a_j, _, _ = self.key
        with localcontext() as ctx:
            ctx.prec = PREC
            T = 2 * n_ind
            dn = T * (self.n[0] + x) - a_i * a_j
            r = dn / Decimal(a_i * (T - a_i) * a_j * (T - a_j)).sqrt()
            dmax = min(a_i * (T - a_j), (T - a_i) * a_j) if dn >= 0 else min(a_i * a_j, (T - a_i) * (T - a_j))
            return r, abs(dn) / dmax


def _refine(g, dg, lo, hi, glo):
    """The root of g in (lo, hi), g(lo) and g(hi) of opposite signs: every iterate stays inside the bracket."""
    x = (lo + hi) / 2
    for _ in range(600):
        gx = g(x)
        if gx == 0:
            return x
        if (gx < 0) == (glo < 0):
            lo = x
        else:
            hi = x
        d = dg(x)
        xn = x - gx / d if d != 0 else lo
        if not lo < xn < hi:
            xn = (lo + hi) / 2
        if abs(xn - x) <= STEP:
            return xn
        x = xn
    raise AssertionError("the bracketed root search did not settle")


@lru_cache(maxsize=None)
def solve(n_ind, a_i, a_j, S, H):
    """Solution of a live tuple (a table with 0 < a_i, a_j < T)."""
    key = tuple(int(v) for v in (n_ind, a_i, a_j, S, H))
    n = table(*key)
    assert n is not None and 0 < key[1] < 2 * key[0] and 0 < key[2] < 2 * key[0], key
    n1, n2, n3, n4 = n
    H = key[4]
    with localcontext() as ctx:
        ctx.prec = PREC
        if H == 0:
            return Solution(key, n, [Decimal(0)], None, False)
        c3, c2 = 2, n1 + n4 - n2 - n3 - 3 * H
        c1 = (n2 + H) * (n3 + H) - H * (n1 + n4) + n1 * n4
        c0 = -H * n1 * n4
        cubic_disc = 18 * c3 * c2 * c1 * c0 - 4 * c2 ** 3 * c0 + c2 * c2 * c1 * c1 - 4 * c3 * c1 ** 3 - 27 * c3 * c3 * c0 * c0

        def g(x):
            return ((c3 * x + c2) * x + c1) * x + c0

        def dg(x):
            return (3 * c3 * x + 2 * c2) * x + c1

        assert g(Decimal(0)) == c0 <= 0 and g(Decimal(H)) == H * n2 * n3 >= 0     # the product form at the ends
        cuts = [Decimal(0)]
        disc = c2 * c2 - 3 * c3 * c1
        if disc > 0:
            sq = Decimal(disc).sqrt()
            cuts += [c for c in ((-c2 - sq) / (3 * c3), (-c2 + sq) / (3 * c3)) if 0 < c < H]
        cuts.append(Decimal(H))
        roots = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            glo, ghi = g(lo), g(hi)
            found = [lo] if glo == 0 else []
            if ghi == 0:
                found.append(hi)
            if glo != 0 and ghi != 0 and (glo < 0) != (ghi < 0):
                found.append(_refine(g, dg, lo, hi, glo))
            for x in found:
                if not roots or x - roots[-1] > DISTINCT:
                    roots.append(x)
        assert roots, key
        ell = None
        if len(roots) > 1:
            def term(cnt, h):
                return cnt * h.ln() if cnt else Decimal(0)

            ell = []
            for x in roots:
                h1, h4, h2, h3 = n1 + x, n4 + x, n2 + H - x, n3 + H - x
                ell.append(term(n1, h1) + term(n2, h2) + term(n3, h3) + term(n4, h4) + H * (h1 * h4 + h2 * h3).ln())
        return Solution(key, n, roots, ell, cubic_disc > 0)


def self_check(sol):
    """The oracle against its own definitions: g(x*) = 0 to 50 digits or x* on the boundary, and x* a fixed point that 200
    plain EM iterations do not leave."""
    n1, n2, n3, n4 = sol.n
    H = sol.key[4]
    assert min(sol.n) >= 0 and sum(sol.n) + 2 * H == 2 * sol.key[0]
    with localcontext() as ctx:
        ctx.prec = PREC
        x = sol.best
        assert 0 <= x <= H
        a, b = x * (n2 + H - x) * (n3 + H - x), (H - x) * (n1 + x) * (n4 + x)
        assert x in (0, H) and a == b or abs(a - b) <= Decimal(10) ** -50 * max(a, b, 1), (sol.key, x, a - b)
        for _ in range(200):
            coupling, repulsion = (n1 + x) * (n4 + x), (n2 + H - x) * (n3 + H - x)
            if coupling + repulsion == 0:
                break
            x = H * coupling / (coupling + repulsion)
        assert abs(x - sol.best) <= Decimal(10) ** -40, (sol.key, sol.best, x)


# ---- cells -----------------------------------------------------------------------------------------------------------------
def ulp32(v: float) -> float:
    """The spacing of float32 at |v| (normal range)."""
    a = abs(float(v))
    return 2.0 ** (math.frexp(a)[1] - 24) if a >= 2.0 ** -126 else 2.0 ** -149


def cell_error(cell, v) -> float:
    """|cell - v| - (2 ulp32(v) + 2^-40): <= 0 passes.  cell a float (a float32 cell, or a float64 of em_host), v a Decimal."""
    with localcontext() as ctx:
        ctx.prec = PREC
        return float(abs(Decimal(float(cell)) - v)) - (ULPS * ulp32(float(v)) + ABS_TOL)


def cells_ok(sol, r_cell, d_cell) -> bool:
    """Both cells within tolerance of the exact values at ONE near-best x."""
    for x in sol.near_best:
        r, d = sol.values(x)
        if cell_error(r_cell, r) <= 0.0 and cell_error(d_cell, d) <= 0.0:
            return True
    return False


def host_error(sol, r64, d64) -> float:
    """max(|r64 - r|, |d64 - D'|) at the near-best x that suits best: the fp64 restatement's distance from the oracle."""
    best = math.inf
    with localcontext() as ctx:
        ctx.prec = PREC
        for x in sol.near_best:
            r, d = sol.values(x)
            best = min(best, max(float(abs(Decimal(float(r64)) - r)), float(abs(Decimal(float(d64)) - d))))
    return best


# ---- panels ------------------------------------------------------------------------------------------------------------------
_PANELS = {}


def panel(shape, n_hap, extremes=False):
    """(codes_i, codes_j, {kind: side-J rows}) of one case, read-only, built once per process: ld_rect_cases.pair_codes with
    ld_dosage_exact.special_rows planted on side J (source, duplicate, complement, all-het, code 2, mono, all-ALT, as far as
    its rows last) and side I's row 0 = side J's source row, so that (0, duplicate) is a duplicate pair and (0, complement) a
    complementary one.  ``extremes`` (the counts test's largest case): side I also gets an all-het row 2 and an all-ALT row 3,
    so that all-ALT x all-ALT reaches S = 4 N and all-het x all-het H = N.  (Not on the other panels: an all-het SNP has a
    table that is symmetric under x -> H - x, so it ties with every partner, and side J's one such column is already close to
    the 1 % of ties the host test allows.)"""
    key = (tuple(shape), n_hap, bool(extremes))
    if key not in _PANELS:
        ci, cj = rc.pair_codes(shape[0], shape[1], n_hap, seed=rc.pair_seed(shape, n_hap))
        where = dx.special_rows(cj)
        if "source" in where:
            ci[0] = cj[where["source"][0]]
        if extremes:
            ci[2] = dx.all_het_row(n_hap, seed=n_hap + 7)
            ci[3] = 1
        ci.setflags(write=False)
        cj.setflags(write=False)
        _PANELS[key] = (ci, cj, where)
    return _PANELS[key]


def rephased(shape, n_hap):
    """panel(shape, n_hap)'s two sides in another phase and ONE other order of the individuals (ld_dosage_exact.rephase with
    one seed for both sides: the swaps differ per SNP, the permutation of the individuals is shared)."""
    ci, cj, _ = panel(shape, n_hap)
    both = dx.rephase(np.concatenate([ci, cj]), seed=shape[0] + shape[1] + n_hap + 1)
    return np.ascontiguousarray(both[:shape[0]]), np.ascontiguousarray(both[shape[0]:])


def homozygous_codes(n_snps, n_ind, seed):
    """int8 [n_snps, 2 n_ind] without missing codes where haplotype 2k + 1 is a copy of haplotype 2k: H = 0 everywhere."""
    half = rc.random_codes(n_snps, n_ind, np.random.default_rng(seed), miss=0.0)
    return np.ascontiguousarray(np.repeat(half, 2, axis=1))


def sample_live(n_ind, a_i, a_j, S, H, count, seed):
    """Up to `count` seeded (i, j) of the live pairs (0 < a_i, a_j < T) -- all of them where there are fewer."""
    T = 2 * n_ind
    live = ((a_i > 0) & (a_i < T))[:, None] & ((a_j > 0) & (a_j < T))[None, :]
    ii, jj = np.nonzero(live)
    if ii.size > count:
        pick = np.sort(np.random.default_rng(seed).choice(ii.size, size=count, replace=False))
        ii, jj = ii[pick], jj[pick]
    return ii, jj

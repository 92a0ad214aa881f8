"""An exact oracle for the D' confidence bounds of a pair (include/ldx.h, "Gabriel blocks") -- TEST INFRASTRUCTURE ONLY, a plain
module like tests/ld_em_exact.py, on whose solve() it stands.  Written from the definition in include/ldx.h alone; `decimal`
at 60 digits and `fractions`, no numpy in the arithmetic.

    sign     s = -1 iff Dn* = T (n1 + x*) - a_i a_j < 0 at the exact maximum-likelihood x* (ld_em_exact.solve().best)
    grid     h1 = (a_i a_j + s k Dm / 100) / T for k = 0 .. 100 as exact rationals, h2 = a_i - h1, h3 = a_j - h1,
             h4 = T - a_i - a_j + h1, each clamped below at 2^-20
    L_k      n1 ln h1 + n2 ln h2 + n3 ln h3 + n4 ln h4 + H ln(h1 h4 + h2 h3); a term with count 0 skipped.  Every argument is a
             rational: ln(p / q) = ln p - ln q with the logarithms of integers cached
    bounds   w_k = exp(L_k - max L), W = sum w_k; lo = (smallest k with sum_{m <= k} w_m > W / 20) - 1 floored at 0,
             hi = (largest k with sum_{m >= k} w_m > W / 20) + 1 capped at 100

A tuple is FRAGILE -- an fp64 evaluation may legitimately land on the neighbouring integer, or on the other sign -- iff
    * some cumulative sum, from either end, lies within 2^-30 W of W / 20: T <= 10 240 gives |L| < T ln T < 2^17, one ulp of
      which is 2^-36; a dozen roundings per L_k make about 2^-32 of relative error in w_k, and 2^-30 leaves a 4-fold margin;
    * |Dn*| < 10^-6: the sign of the r cell is decided by rounding;
    * two local maxima of l lie within 10^-9 of each other: the EM estimate, and with it the sign, may be either.

Two arithmetics run the same code.  bounds() is the reference: Decimal at 60 digits (about 500 Decimal.ln per tuple: 50 ms).
bounds_fast() is for the GPU tests, which look at hundreds of cells in seconds: the same sums in fixed point, integers in units of
2^-240 (72 digits), with ln and exp of its own (a table of ln(1 + j / 256) from Decimal, then the atanh series; halving and
Taylor).  tests/test_ld_gabriel_host.py checks the two functions of FixedMath against Decimal and bounds_fast() against bounds() on
every tuple it tests.
"""
from __future__ import annotations

from decimal import Decimal, localcontext
from fractions import Fraction
from functools import lru_cache

import ld_em_exact as emx

PREC = 60
NO_CI = 0xFF
EPS = Fraction(1, 1 << 20)
NEAR_LINE_BITS = 30
NEAR_ZERO = Decimal(10) ** -6
NEAR_TIE = Decimal(10) ** -9


class DecimalMath:
    """Logarithms of integers and exponentials of non-positive numbers as Decimals (inside a context of PREC digits)."""

    zero = Decimal(0)

    @staticmethod
    @lru_cache(maxsize=None)
    def ln_int(v: int) -> Decimal:
        with localcontext() as ctx:
            ctx.prec = PREC
            return Decimal(v).ln()

    @staticmethod
    def exp(d: Decimal) -> Decimal:
        return d.exp()


class FixedMath:
    """The same in fixed point: a value v stands for v / 2^BITS.  Every step truncates by less than 2^-BITS and there are a
    few dozen of them, so a logarithm is good to about 2^-230 and a weight to 2^-220 relative."""

    BITS = 240
    ONE = 1 << BITS
    zero = 0
    _table = None

    @classmethod
    def _const(cls):
        if cls._table is None:
            with localcontext() as ctx:
                ctx.prec = 90
                scale = Decimal(cls.ONE)
                cls._table = [int((Decimal(256 + j) / 256).ln() * scale) for j in range(256)]
                cls._ln2 = int(Decimal(2).ln() * scale)
        return cls._table, cls._ln2

    @classmethod
    @lru_cache(maxsize=None)
    def ln_int(cls, v: int) -> int:
        table, ln2 = cls._const()
        e = v.bit_length() - 1
        m = (v << cls.BITS) >> e                       # v / 2^e in [1, 2)
        j = (m >> (cls.BITS - 8)) - 256                # its first eight fraction bits
        m = (m << 8) // (256 + j)                      # / (1 + j / 256): in [1, 1 + 2^-8)
        z = ((m - cls.ONE) << cls.BITS) // (m + cls.ONE)   # ln m = 2 atanh z, z < 2^-9
        z2 = (z * z) >> cls.BITS
        total, term, k = 0, z, 1
        while term:
            total += term // k
            term = (term * z2) >> cls.BITS
            k += 2
        return e * ln2 + table[j] + 2 * total

    @classmethod
    def exp(cls, d: int) -> int:
        """exp of d <= 0."""
        _, ln2 = cls._const()
        x = -d
        n, r = divmod(x, ln2)
        if n > cls.BITS:
            return 0
        r >>= 16                                        # exp(-r / 2^16) by Taylor, then sixteen squarings
        total, term, k = cls.ONE, cls.ONE, 1
        while term:
            term = (term * r) >> cls.BITS
            term //= k
            total += -term if k & 1 else term
            k += 1
        for _ in range(16):
            total = (total * total) >> cls.BITS
        return total >> n


def usable(n_ind, a_i, a_j, S, H) -> bool:
    """A genotype table with 0 < a_i, a_j < T."""
    T = 2 * int(n_ind)
    return emx.table(n_ind, a_i, a_j, S, H) is not None and 0 < int(a_i) < T and 0 < int(a_j) < T


def _bounds(key, mt):
    N, ai, aj, S, H = key
    if not usable(N, ai, aj, S, H):
        return NO_CI, NO_CI, False
    sol = emx.solve(N, ai, aj, S, H)
    n1, n2, n3, n4 = sol.n
    T = 2 * N
    with localcontext() as ctx:
        ctx.prec = PREC
        dn = T * (n1 + sol.best) - ai * aj
        fragile = abs(dn) < NEAR_ZERO
        if sol.ell is not None:
            best = max(sol.ell)
            fragile = fragile or sum(1 for l in sol.ell if best - l <= NEAR_TIE) > 1
        s = -1 if dn < 0 else 1
        dm = min(ai * aj, (T - ai) * (T - aj)) if s < 0 else min(ai * (T - aj), (T - ai) * aj)
        den = 100 * T
        ln_den = mt.ln_int(den)
        ell = []
        for k in range(101):
            # every h is an integer over 100 T; the clamp bites iff numerator * 2^20 < 100 T (k = 100, or T > 10 485)
            a1 = 100 * ai * aj + s * k * dm
            nums = (a1, den * ai - a1, den * aj - a1, den * (T - ai - aj) + a1)
            l = mt.zero
            if min(nums) << 20 >= den:
                for cnt, a in zip((n1, n2, n3, n4), nums):
                    if cnt:
                        l += cnt * (mt.ln_int(a) - ln_den)
                if H:
                    l += H * (mt.ln_int(nums[0] * nums[3] + nums[1] * nums[2]) - 2 * ln_den)
            else:
                h1, h2, h3, h4 = (max(Fraction(a, den), EPS) for a in nums)
                for cnt, h in ((n1, h1), (n2, h2), (n3, h3), (n4, h4), (H, h1 * h4 + h2 * h3)):
                    if cnt:
                        l += cnt * (mt.ln_int(h.numerator) - mt.ln_int(h.denominator))
            ell.append(l)
        top = max(ell)
        w = [mt.exp(l - top) for l in ell]
        W = sum(w)
        ends = []
        for order in (range(101), range(100, -1, -1)):
            cum, hit = mt.zero, None
            for k in order:
                cum += w[k]
                # cum against W / 20, and within 2^-30 W of it
                fragile = fragile or abs(20 * cum - W) * (1 << NEAR_LINE_BITS) <= 20 * W
                if hit is None and 20 * cum > W:
                    hit = k
            ends.append(hit)
    return max(ends[0] - 1, 0), min(ends[1] + 1, 100), bool(fragile)


@lru_cache(maxsize=None)
def bounds(n_ind, a_i, a_j, S, H):
    """(lo, hi, fragile) of one count tuple in Decimal; (NO_CI, NO_CI, False) for a tuple without an interval."""
    return _bounds(tuple(int(v) for v in (n_ind, a_i, a_j, S, H)), DecimalMath)


@lru_cache(maxsize=None)
def bounds_fast(n_ind, a_i, a_j, S, H):
    """bounds() in fixed point."""
    return _bounds(tuple(int(v) for v in (n_ind, a_i, a_j, S, H)), FixedMath)

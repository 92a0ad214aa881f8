"""Helper (not a test): brute-force genotype tables and exact oracles for the epistasis scan (include/ldx.h, "epistasis scan").

  * tables_brute: the 18 integers of every pair straight from the int8 codes, one individual at a time.
  * allelic_exact: rationals up to the two logarithms, then Decimal at 60 digits.
  * boost_exact: the same iterative proportional fitting in Decimal at 60 digits, iterated until a cycle changes nothing above
    1e-45, and G2 from it.  The exact statistic does not depend on the orientation of the table, so none is chosen here.
  * tuples(): the tables every accuracy, flag and cycle-cap statement of the header is made on.
"""
from decimal import Context, Decimal, localcontext
from fractions import Fraction
from functools import lru_cache

import numpy as np

from ld_logistic_exact import ln_p_exact as ln_normal_tail

PREC = 60
CTX = Context(prec=PREC, Emax=999999999, Emin=-999999999)
STOP = Decimal("1e-45")
MAX_GROUP = 5120   # LDX_MAX_HAPS / 2


# ---- brute force ---------------------------------------------------------------------------------------------------------------
def genotypes(codes) -> np.ndarray:
    """int8 [n_snps, n_ind]: 0 / 1 / 2, or -1 where either code of the individual is not 0 or 1."""
    c = np.asarray(codes)
    ok = (c >= 0) & (c <= 1)
    g = (c[:, 0::2] == 1).astype(np.int8) + (c[:, 1::2] == 1).astype(np.int8)
    return np.where(ok[:, 0::2] & ok[:, 1::2], g, -1).astype(np.int8)


def tables_brute(codes_i, codes_j, case) -> np.ndarray:
    """int64 [18, n_i, n_j]: index 9 c + 3 a + b, c = 0 the cases (case == 1), 1 the controls (case == 0)."""
    gi, gj = genotypes(codes_i), genotypes(codes_j)
    case = np.asarray(case, dtype=np.float64)
    out = np.zeros((18, gi.shape[0], gj.shape[0]), dtype=np.int64)
    for k in range(gi.shape[1]):
        if np.isnan(case[k]):
            continue
        c = 0 if case[k] == 1.0 else 1
        a, b = gi[:, k].astype(np.int64), gj[:, k].astype(np.int64)
        ii, jj = np.nonzero((a >= 0)[:, None] & (b >= 0)[None, :])
        np.add.at(out, (9 * c + 3 * a[ii] + b[jj], ii, jj), 1)
    return out


# ---- exact oracles -------------------------------------------------------------------------------------------------------------
def _ln(fr: Fraction) -> Decimal:
    with localcontext(CTX):
        return (Decimal(fr.numerator) / Decimal(fr.denominator)).ln()


def _allele(n9):
    N = sum(n9)
    A = sum((k // 3) * n9[k] for k in range(9))
    B = sum((k % 3) * n9[k] for k in range(9))
    S = sum((k // 3) * (k % 3) * n9[k] for k in range(9))
    return S, 2 * A - S, 2 * B - S, 4 * N - 2 * A - 2 * B + S


def allelic_exact(t):
    """(chisq Decimal or None, dir Decimal or None, flags) of one tuple of 18 integers."""
    cells = [_allele([int(x) for x in t[9 * c:9 * c + 9]]) for c in range(2)]
    if any(x == 0 for cell in cells for x in cell):
        return None, None, 2
    with localcontext(CTX):
        L = [_ln(Fraction(a * d, b * c)) for a, b, c, d in cells]
        V = sum(Fraction(1, x) for cell in cells for x in cell)
        d = L[0] - L[1]
        return d * d * Decimal(V.denominator) / Decimal(V.numerator), d, 0


def boost_exact(t, max_cycles: int = 2000):
    """(G2 Decimal or None, flags without the cap bit and bit 2, cycles the Decimal fit took) of one tuple of 18 integers.  G2 is
    None for an empty group, and for a table whose fit has not come to rest after ``max_cycles`` cycles: with a zero in a two-way
    margin the fit can crawl towards a boundary at the rate 1 / cycles, and no cap of the scan's is meant to wait for that."""
    n = [int(x) for x in t]
    if sum(n[:9]) == 0 or sum(n[9:]) == 0:
        return None, 1, 0
    ab = [n[k] + n[9 + k] for k in range(9)]
    ac = [[sum(n[9 * c + 3 * a:9 * c + 3 * a + 3]) for a in range(3)] for c in range(2)]
    bc = [[n[9 * c + b] + n[9 * c + 3 + b] + n[9 * c + 6 + b] for b in range(3)] for c in range(2)]
    flags = 8 if (0 in ab or any(0 in r for r in ac) or any(0 in r for r in bc)) else 0
    with localcontext(CTX):
        mu = [Decimal(1)] * 18
        for cyc in range(1, max_cycles + 1):
            old = list(mu)
            for k in range(9):
                s = mu[k] + mu[9 + k]
                f = Decimal(ab[k]) / s if s else Decimal(0)
                mu[k], mu[9 + k] = mu[k] * f, mu[9 + k] * f
            for c in range(2):
                for a in range(3):
                    at = 9 * c + 3 * a
                    s = mu[at] + mu[at + 1] + mu[at + 2]
                    f = Decimal(ac[c][a]) / s if s else Decimal(0)
                    for x in (at, at + 1, at + 2):
                        mu[x] = mu[x] * f
            for c in range(2):
                for b in range(3):
                    at = 9 * c + b
                    s = mu[at] + mu[at + 3] + mu[at + 6]
                    f = Decimal(bc[c][b]) / s if s else Decimal(0)
                    for x in (at, at + 3, at + 6):
                        mu[x] = mu[x] * f
            if max(abs(x - y) for x, y in zip(mu, old)) <= STOP:
                break
        else:
            return None, flags, max_cycles
        g2 = 2 * sum((Decimal(n[k]) * (Decimal(n[k]) / mu[k]).ln() for k in range(18) if n[k] > 0), Decimal(0))
        return g2, flags, cyc


def ln_tail_exact(chisq: Decimal, test: str) -> Decimal:
    """ln p of an exact chi-square: the two-sided normal tail of its root (1 df) or -x + ln(1 + x), x = chisq / 2 (4 df)."""
    if test == "allelic":
        with localcontext(CTX):
            root = chisq.sqrt()
        return ln_normal_tail(root)
    with localcontext(CTX):
        x = chisq / 2
        return -x + (1 + x).ln()


def rel_error(got: float, want: Decimal) -> float:
    """|got - want| / max(want, 1): the header's measure (absolute below 1, where the statistic is what is left of a sum that
    cancels)."""
    with localcontext(CTX):
        return float(abs(Decimal(float(got)) - want) / max(want, Decimal(1)))


# ---- tuples --------------------------------------------------------------------------------------------------------------------
def _multinomial(rng, n, p):
    return rng.multinomial(n, p / p.sum()).astype(np.int64)


def _xor_table(rng, n_case, n_ctrl, leak):
    """XOR penetrance: a case where exactly one of the two genotypes is heterozygous; ``leak`` of each group on the other cells."""
    fa, fb = rng.uniform(0.3, 0.5, 2)
    ga = np.array([(1 - fa) ** 2, 2 * fa * (1 - fa), fa * fa])
    gb = np.array([(1 - fb) ** 2, 2 * fb * (1 - fb), fb * fb])
    joint = np.outer(ga, gb).reshape(-1)
    xor = np.array([((k // 3) == 1) != ((k % 3) == 1) for k in range(9)])
    return np.concatenate([_multinomial(rng, n_case, joint * np.where(xor, 1.0, leak)),
                           _multinomial(rng, n_ctrl, joint * np.where(xor, leak, 1.0))])


@lru_cache(maxsize=None)
def tuples() -> np.ndarray:
    """int64 [m, 18]: random tables over four decades of group size, tables with sampling zeros, a zero in each of the three
    two-way margins, an empty group, single-individual groups, XOR penetrance (perfect and leaky) and totals at the
    5120-per-group limit.  Fixed seed: the header's cycle cap and accuracy bound are measured on exactly these."""
    rng = np.random.default_rng(20101)
    out = []
    for n_case, n_ctrl in ((40, 60), (150, 37), (500, 500), (2000, 1300), (5120, 5120), (5120, 77)):
        for _ in range(6):   # random
            out.append(np.concatenate([_multinomial(rng, n_case, rng.uniform(0.2, 1.0, 9)),
                                       _multinomial(rng, n_ctrl, rng.uniform(0.2, 1.0, 9))]))
        for _ in range(3):   # no interaction: both groups from one product table
            p = np.outer(rng.dirichlet(np.ones(3) * 4), rng.dirichlet(np.ones(3) * 4)).reshape(-1)
            out.append(np.concatenate([_multinomial(rng, n_case, p), _multinomial(rng, n_ctrl, p)]))
    for _ in range(24):      # sampling zeros
        n_case, n_ctrl = rng.integers(4, 40, 2)
        p = rng.dirichlet(np.ones(9) * 0.6)
        out.append(np.concatenate([_multinomial(rng, n_case, p), _multinomial(rng, n_ctrl, rng.dirichlet(np.ones(9) * 0.6))]))
    base = np.concatenate([_multinomial(rng, 300, rng.uniform(0.3, 1.0, 9)), _multinomial(rng, 200, rng.uniform(0.3, 1.0, 9))])
    for cell in (0, 4, 8):   # SNP i x SNP j
        t = base.copy()
        t[cell] = t[9 + cell] = 0
        out.append(t)
    for c, a in ((0, 2), (1, 0), (0, 1)):   # SNP i x group
        t = base.copy()
        t[9 * c + 3 * a:9 * c + 3 * a + 3] = 0
        out.append(t)
    for c, b in ((1, 2), (0, 0), (1, 1)):   # SNP j x group
        t = base.copy()
        t[[9 * c + b, 9 * c + 3 + b, 9 * c + 6 + b]] = 0
        out.append(t)
    for c in range(2):       # an empty group
        t = base.copy()
        t[9 * c:9 * c + 9] = 0
        out.append(t)
    for a, b in ((0, 0), (1, 1), (2, 1), (1, 2)):   # single-individual groups
        t = np.zeros(18, dtype=np.int64)
        t[3 * a + b] = 1
        t[9 + 3 * b + a] = 1
        out.append(t)
        t = base.copy()
        t[:9] = 0
        t[3 * a + b] = 1
        out.append(t)
    for n_case, n_ctrl, leak in ((150, 150, 0.0), (1000, 1000, 0.0), (5120, 5120, 0.0), (150, 150, 0.05), (1000, 1000, 0.05),
                                 (5120, 5120, 0.3)):
        out.append(_xor_table(rng, n_case, n_ctrl, leak))
    t = np.zeros(18, dtype=np.int64)   # the limit in one cell per group
    t[4] = t[9 + 4] = MAX_GROUP
    out.append(t)
    t = np.zeros(18, dtype=np.int64)
    t[0], t[8], t[9 + 2], t[9 + 6] = MAX_GROUP // 2, MAX_GROUP // 2, MAX_GROUP // 2, MAX_GROUP // 2
    out.append(t)
    return np.stack(out).astype(np.int64)


@lru_cache(maxsize=None)
def oracle():
    """The exact results of every tuple, computed once: a list of (allelic (chisq, dir, flags), boost (g2, flags, cycles))."""
    return [(allelic_exact(t), boost_exact(t)) for t in tuples()]


# ---- panels --------------------------------------------------------------------------------------------------------------------
def epi_codes(n_snps: int, n_ind: int, seed: int, miss: float = 0.0, miss_ind=None) -> np.ndarray:
    """int8 [n_snps, 2 n_ind]: independent SNPs with ALT frequencies in [0.2, 0.5]; ``miss`` of the haplotype codes missing (2),
    among the individuals ``miss_ind`` (a bool mask) where given."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.2, 0.5, n_snps)
    codes = (rng.random((n_snps, 2 * n_ind)) < f[:, None]).astype(np.int8)
    if miss:
        hole = rng.random(codes.shape) < miss
        if miss_ind is not None:
            hole &= np.repeat(np.asarray(miss_ind, dtype=bool), 2)[None, :]
        codes[hole] = 2
    return codes


def case_vector(n_ind: int, n_case: int, n_ctrl: int, seed: int) -> np.ndarray:
    """float64 [n_ind]: n_case ones, n_ctrl zeros and NaN for the rest, shuffled."""
    v = np.full(n_ind, np.nan)
    v[:n_case] = 1.0
    v[n_case:n_case + n_ctrl] = 0.0
    np.random.default_rng(seed).shuffle(v)
    return v

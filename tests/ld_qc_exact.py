"""Exact oracle of the genotype QC and table tests (include/ldx.h, "genotype QC and table tests"); no device, no float.

The HWE and Fisher distributions are exact integer weights (every step of the term ratio is checked to divide exactly), the
two-sided tail rule is decided on integers, p and mid-p are ``fractions.Fraction`` and ln p is taken by ``decimal`` at 60 digits.
``admissible`` is the condition under which the device can decide the tail rule: no exact ratio P(k) / P(obs) in
[1 + 2^-31, 1 + 2^-29].  The oracle ASSERTS it for every tuple it is asked about -- a condition on the inputs, not a skip.
The chi-square statistics of --model are exact rationals; their 1-df tail is ld_logistic_exact's erfc, the 2-df tail exp(-x / 2).
"""
from decimal import Context, Decimal, localcontext
from fractions import Fraction
from math import comb, factorial

import numpy as np

from ld_glm_exact import glm_codes
from ld_logistic_exact import ln_p_exact as ln_normal_tail

PREC = 60
CTX = Context(prec=PREC, Emax=999999999, Emin=-999999999)
TIE = Fraction(1) + Fraction(1, 1 << 30)
TIE_LO, TIE_HI = Fraction(1) + Fraction(1, 1 << 31), Fraction(1) + Fraction(1, 1 << 29)
LN_P_BOUND = 2.0 ** -30          # |ln p - exact| <= LN_P_BOUND max(1, |exact|)
LN10 = Decimal("2.302585092994045684017991454684364207601101488628772976033327900967572609677")


def ln_fraction(fr: Fraction) -> Decimal:
    with localcontext(CTX):
        return Decimal(fr.numerator).ln() - Decimal(fr.denominator).ln()


def hwe_weights(n: int, het: int, hom: int):
    """(integer weights of k = k0, k0 + 2, ..., index of the observed term): w_k = 2^k n! / (hA! k! hB!), built from the first
    term by the ratio 4 hA hB / ((k + 2)(k + 1)), each step an exact division."""
    nA = het + 2 * hom
    nB = 2 * n - nA
    assert 0 <= het and 0 <= hom and het + hom <= n and 0 < nA and 0 < nB
    k0, kmax = nA & 1, min(nA, nB)
    w = [(factorial(n) // (factorial((nA - k0) // 2) * factorial(k0) * factorial((nB - k0) // 2))) << k0]
    for k in range(k0, kmax, 2):
        num = w[-1] * 4 * ((nA - k) // 2) * ((nB - k) // 2)
        q, r = divmod(num, (k + 2) * (k + 1))
        assert r == 0
        w.append(q)
    return w, (het - k0) // 2


def fisher_weights(a: int, b: int, c: int, d: int):
    """(integer weights of the first cell x = lo .. hi, index of the observed one): w_x = C(r1, x) C(r2, c1 - x), by the ratio
    (r1 - x)(c1 - x) / ((x + 1)(r2 - c1 + x + 1))."""
    r1, r2, c1 = a + b, c + d, a + c
    assert min(a, b, c, d) >= 0 and r1 > 0 and r2 > 0 and c1 > 0 and b + d > 0
    lo, hi = max(0, c1 - r2), min(r1, c1)
    w = [comb(r1, lo) * comb(r2, c1 - lo)]
    for x in range(lo, hi):
        q, r = divmod(w[-1] * (r1 - x) * (c1 - x), (x + 1) * (r2 - c1 + x + 1))
        assert r == 0
        w.append(q)
    return w, a - lo


def admissible(w, io) -> bool:
    """No exact ratio w_k / w_obs in [1 + 2^-31, 1 + 2^-29]: the device's recurrences (relative error below 2^-35) decide the
    tail rule as the integers do."""
    wo = w[io]
    return not any(x * TIE_LO.denominator >= wo * TIE_LO.numerator and x * TIE_HI.denominator <= wo * TIE_HI.numerator for x in w)


def closest_non_tie(w, io) -> Fraction:
    """min |w_k / w_obs - 1| over the terms that are not exact ties (1 when there is none)."""
    wo = w[io]
    return min((abs(Fraction(x, wo) - 1) for x in w if x != wo), default=Fraction(1))


def tail_exact(w, io, midp=False) -> Fraction:
    """p (or mid-p) by the two-sided tail rule: the terms with w_k / w_obs <= 1 + 2^-30; asserts admissibility."""
    assert admissible(w, io), "a term ratio lies in [1 + 2^-31, 1 + 2^-29]: the tuple is outside the rule's decidable inputs"
    wo = w[io]
    tail = sum(x for x in w if x * TIE.denominator <= wo * TIE.numerator)
    return Fraction(2 * tail - wo, 2 * sum(w)) if midp else Fraction(tail, sum(w))


def hwe_exact(n, het, hom, midp=False):
    """(p Fraction or None, flag) of the exact HWE test."""
    if n == 0:
        return None, 1
    nA = het + 2 * hom
    if nA == 0 or nA == 2 * n:
        return Fraction(1), 2
    return tail_exact(*hwe_weights(n, het, hom), midp), 0


def fisher_exact(a, b, c, d, midp=False):
    """(p Fraction or None, flag) of Fisher's exact test on [[a, b], [c, d]]."""
    if a + b + c + d == 0:
        return None, 1
    if 0 in (a + b, c + d, a + c, b + d):
        return Fraction(1), 2
    return tail_exact(*fisher_weights(a, b, c, d), midp), 0


def hwe_brute(n, nA):
    """{het count: number of pairings} over ALL pairings of 2n labelled alleles, nA of them ALT, into n unordered genotypes --
    the definition the exact test's distribution comes from (n <= 5)."""
    alleles = [1] * nA + [0] * (2 * n - nA)
    out = {}

    def rec(rest, het):
        if not rest:
            out[het] = out.get(het, 0) + 1
            return
        first = rest[0]
        for j in range(1, len(rest)):
            rec(rest[1:j] + rest[j + 1:], het + (alleles[first] != alleles[rest[j]]))

    rec(list(range(2 * n)), 0)
    return out


def ln_check(ln_got, p: Fraction) -> float:
    """|ln_got - ln p| in units of the bound 2^-30 max(1, |ln p|)."""
    want = ln_fraction(p)
    with localcontext(CTX):
        err = abs(Decimal(float(ln_got)) - want)
        return float(err / (Decimal(LN_P_BOUND) * max(Decimal(1), abs(want))))


def check_exact(kind, tuples, midp, p, nlp, flags):
    """Compare device or mirror outputs with the oracle on every tuple: equal flags, NaN where the oracle has no p, and
    ln p = -neglog10_p ln 10 within the contract; p itself within 2^-28 relatively where it is a normal double.  Returns the
    largest ln error in units of the bound."""
    exact = hwe_exact if kind == "hwe" else fisher_exact
    worst = 0.0
    for i, t in enumerate(tuples):
        want, flag = exact(*(int(v) for v in t), midp)
        assert int(flags[i]) == flag, (kind, t, int(flags[i]), flag)
        if want is None:
            assert np.isnan(p[i]) and np.isnan(nlp[i]), (kind, t)
            continue
        assert np.isfinite(nlp[i]) and nlp[i] >= 0.0, (kind, t, nlp[i])
        units = ln_check(-float(nlp[i]) * float(LN10), want)
        assert units <= 1.0, (kind, t, midp, float(nlp[i]), units)
        worst = max(worst, units)
        if want == 1 and not midp:
            assert p[i] == 1.0 and nlp[i] == 0.0, (kind, t, p[i], nlp[i])
        if float(want) > 1e-300:
            assert abs(p[i] / float(want) - 1.0) <= 2.0 ** -28, (kind, t, p[i], float(want))
        else:
            assert 0.0 <= p[i] <= 1e-299, (kind, t, p[i])
    return worst


# ---- the chi-square tests of --model ------------------------------------------------------------------------------------------
def _table(T, a, b, c, d):
    den = (a + b) * (c + d) * (a + c) * (b + d)
    return (None, 2) if den == 0 else (Fraction(T * (a * d - b * c) ** 2, den), 0)


def model_exact(R, r1, r2, S, s1, s2, min_cell=5):
    """([(chisq Fraction or None, flag)] x 5 in the order allelic, trend, genotypic, dominant, recessive, odds Fraction / inf /
    None)."""
    if R == 0 or S == 0:
        return [(None, 1)] * 5, None
    N, r0, s0 = R + S, R - r1 - r2, S - s1 - s2
    n0, n1, n2 = r0 + s0, r1 + s1, r2 + s2
    a, c = r1 + 2 * r2, s1 + 2 * s2
    b, d = 2 * R - a, 2 * S - c
    out = [_table(2 * N, a, b, c, d)]
    odds = None if out[0][1] else (float("inf") if b * c == 0 else Fraction(a * d, b * c))
    U = N * (r1 + 2 * r2) - R * (n1 + 2 * n2)
    D = N * (n1 + 4 * n2) - (n1 + 2 * n2) ** 2
    out.append((None, 2) if R * S * D == 0 else (Fraction(N * U * U, R * S * D), 0))
    if 0 in (n0, n1, n2):
        out.append((None, 2))
    elif min(r0, r1, r2, s0, s1, s2) < min_cell:
        out.append((None, 3))
    else:
        x2 = Fraction(0)
        for row, cells in ((R, (r0, r1, r2)), (S, (s0, s1, s2))):
            for col, o in zip((n0, n1, n2), cells):
                e = Fraction(row * col, N)
                x2 += (o - e) ** 2 / e
        out.append((x2, 0))
    out.append(_table(N, r1 + r2, r0, s1 + s2, s0))
    out.append(_table(N, r2, r0 + r1, s2, s0 + s1))
    return out, odds


def ln_chisq_tail(x2: Fraction, df: int) -> Decimal:
    """ln of the upper tail of a chi-square statistic with 1 or 2 degrees of freedom."""
    with localcontext(CTX):
        x = Decimal(x2.numerator) / Decimal(x2.denominator)
        if df == 2:
            return -x / 2
    from ld_logistic_exact import WIDE

    with localcontext(WIDE):
        return ln_normal_tail((Decimal(x2.numerator) / Decimal(x2.denominator)).sqrt())


def model_tail_units(x2: Fraction, df: int, nlp: float) -> float:
    want = ln_chisq_tail(x2, df)
    with localcontext(CTX):
        err = abs(Decimal(-float(nlp)) * LN10 - want)
        return float(err / (Decimal(LN_P_BOUND) * max(Decimal(1), abs(want))))


# ---- tuple sets and the comparison the host and the device tests share --------------------------------------------
def small_hwe_tuples(n_max):
    return [(n, het, (nA - het) // 2) for n in range(1, n_max + 1) for nA in range(0, 2 * n + 1)
            for het in range(nA & 1, min(nA, 2 * n - nA) + 1, 2)]


def balanced_tables(m_max):
    return [(a, m - a, c, m - c) for m in range(1, m_max + 1, 3) for a in range(0, m + 1, max(1, m // 6)) for c in range(0, m + 1, max(1, m // 5))]


def model_tuples():
    rng = np.random.default_rng(3)
    out = [(0, 0, 0, 10, 3, 1), (10, 3, 1, 0, 0, 0), (10, 0, 0, 12, 0, 0), (10, 10, 0, 12, 12, 0), (10, 0, 10, 12, 0, 12),
           (40, 20, 5, 50, 25, 6), (40, 20, 5, 50, 25, 5), (40, 20, 5, 50, 25, 4), (40, 20, 0, 50, 25, 0), (2560, 1200, 400, 2560, 1000, 300),
           (2560, 0, 2560, 2560, 0, 0), (30, 12, 3, 30, 12, 3)]
    for _ in range(60):
        R, S = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        r2, s2 = int(rng.integers(0, R + 1)), int(rng.integers(0, S + 1))
        out.append((R, int(rng.integers(0, R - r2 + 1)), r2, S, int(rng.integers(0, S - s2 + 1)), s2))
    return out


def check_model(tuples, min_cell, chisq, p, nlp, odds, flags, rel):
    """The statistics against the exact rationals within ``rel``, equal flags, NaN under a flag, the tails within the contract."""
    seen, worst = set(), 0.0
    for i, t in enumerate(tuples):
        want, want_odds = model_exact(*t, min_cell)
        for k, (x2, flag) in enumerate(want):
            assert int(flags[i, k]) == flag, (t, k, int(flags[i, k]), flag)
            seen.add(flag)
            if flag:
                assert np.isnan(chisq[i, k]) and np.isnan(p[i, k]) and np.isnan(nlp[i, k]), (t, k)
                continue
            assert abs(Fraction(float(chisq[i, k])) - x2) <= Fraction(rel) * x2, (t, k, chisq[i, k], float(x2))
            worst = max(worst, model_tail_units(Fraction(float(chisq[i, k])), 2 if k == 2 else 1, nlp[i, k]))
            if chisq[i, k] < 1400.0:
                assert abs(p[i, k] / 10.0 ** -nlp[i, k] - 1.0) <= 1e-9, (t, k)
        if want_odds is None:
            assert np.isnan(odds[i])
        elif want_odds == float("inf"):
            assert odds[i] == np.inf
        else:
            assert abs(Fraction(float(odds[i])) - want_odds) <= Fraction(2.0 ** -52) * want_odds
    assert worst <= 1.0, worst
    return seen, worst


# ---- panels ---------------------------------------------------------------------------------------------------------------------
def qc_codes(n_ind, n_snps, seed, miss=0.0):
    """glm_codes with a few special rows where the panel is long enough: SNP 3 monomorphic REF, SNP 5 all heterozygous, SNP 7
    without a call."""
    codes = glm_codes(n_ind, n_snps, seed, miss)
    if n_snps > 3:
        codes[3] = 0
    if n_snps > 5:
        codes[5, 0::2], codes[5, 1::2] = 1, 0
    if n_snps > 7:
        codes[7] = 2
    return codes


def case_vector(n_ind, seed):
    """0 / 1 / NaN per individual: about 45 % cases, 45 % controls, the rest left out; the last individual is a case."""
    rng = np.random.default_rng(seed)
    u = rng.random(n_ind)
    v = np.where(u < 0.45, 1.0, np.where(u < 0.9, 0.0, np.nan))
    v[-1] = 1.0
    return v


def group_sets(n_ind, seed):
    """{name: bool [n_groups, n_ind]}: one group of everybody; all / cases / controls; 32 groups with an empty one, overlapping
    ones and one whose only member is the last individual."""
    rng = np.random.default_rng(seed)
    case = case_vector(n_ind, seed)
    g32 = rng.random((32, n_ind)) < rng.uniform(0.05, 0.9, size=(32, 1))
    g32[0] = True
    g32[5] = False
    g32[6] = g32[4]
    g32[31] = False
    g32[31, n_ind - 1] = True
    return {"all": np.ones((1, n_ind), dtype=bool), "cc": np.stack([np.ones(n_ind, dtype=bool), case == 1.0, case == 0.0]),
            "g32": g32}

"""An exact oracle for the association scan (include/ldx.h, "association scan") -- TEST INFRASTRUCTURE ONLY, a plain module like
tests/ld_geno_exact.py.  No tests here.

Written from the definition alone; numpy integers, ``fractions`` and ``decimal`` only.  From the allele codes and the integers q, e
of the design it computes z, zc and the counts, then mu, gg, h, b, d, beta, sigma^2 and t^2 as exact Fractions (yy is the exact
integer sum, NOT rounded to fp64: the definition's one rounding is part of what the bound of the host test covers); se, t and the
tail come from Decimal at 80 digits.

The tail takes a route that is not the kernel's (a continued fraction with lgamma): the hypergeometric series
    I_x(a, b) = x^a (1 - x)^b / (a B(a, b)) sum_n (a + b)_n / (a + 1)_n x^n
in x = df / (df + t^2) when 1 - x >= 1/32 (at most some 6 000 terms), else 1 - I_y(1/2, df/2) by the same series in
y = t^2 / (df + t^2); every term is positive.  The complement subtracts: with y < 1/32, p >= exp(-df / 62), more than 1e-36 for every
df a panel can have (df < 5120), so at least 40 of the 80 digits are left.
B(df/2, 1/2) comes from factorials: (m - 1)! 4^m m! / (2 m)! for df = 2 m, (2 m)! pi / (4^m m!^2) for df = 2 m + 1, pi to 100 digits.
"""
from decimal import Context, Decimal, localcontext
from fractions import Fraction
from math import factorial

import numpy as np

PREC = 80
CTX = Context(prec=PREC, Emax=999999999, Emin=-999999999)
PI = Decimal("3.1415926535897932384626433832795028841971693993751058209749445923078164062862089986280348253421170679")
SCALE_BITS = 30


def dec(fr: Fraction) -> Decimal:
    with localcontext(CTX):
        return Decimal(fr.numerator) / Decimal(fr.denominator)


def beta_half(df: int) -> Decimal:
    """B(df / 2, 1 / 2)."""
    with localcontext(CTX):
        if df % 2 == 0:
            m = df // 2
            return dec(Fraction(factorial(m - 1) * 4 ** m * factorial(m), factorial(2 * m)))
        m = (df - 1) // 2
        return dec(Fraction(factorial(2 * m), 4 ** m * factorial(m) ** 2)) * PI


def _series(a: Fraction, b: Fraction, x: Decimal) -> Decimal:
    """sum_n (a + b)_n / (a + 1)_n x^n."""
    with localcontext(CTX):
        total = term = Decimal(1)
        n = 0
        stop = Decimal(10) ** -(PREC - 5)
        while True:
            term = term * dec((a + b + n) / (a + 1 + n)) * x
            total += term
            n += 1
            r = max(dec((a + b + n) / (a + 1 + n)) * x, x)   # the term ratio is monotone in n and tends to x: its bound from here on
            if r < 1 and term * r / (1 - r) < stop * total:     # the rest is below a geometric series
                return total
            if n > 200000:
                raise RuntimeError("the oracle's series did not converge")


def ln_p_exact(t2: Fraction, df: int) -> Decimal:
    """ln of p = I_x(df / 2, 1 / 2), x = df / (df + t^2), for an exact t^2 >= 0."""
    with localcontext(CTX):
        if t2 == 0:
            return Decimal(0)
        x, y = Fraction(df) / (df + t2), t2 / (df + t2)
        a, b = Fraction(df, 2), Fraction(1, 2)
        B = beta_half(df)
        xa = (dec(x) ** df).sqrt()          # x^(df / 2)
        yb = dec(y).sqrt()                  # (1 - x)^(1 / 2)
        if y >= Fraction(1, 32):
            return (xa * yb / (dec(a) * B) * _series(a, b, dec(x))).ln()
        comp = yb * xa / (dec(b) * B) * _series(b, a, dec(y))
        return (Decimal(1) - comp).ln()


def planes(codes, keep=None):
    """(g, c) int64 [n_snps, n_ind]: the ALT dosage of the called genotypes (0 where missing) and the called flag."""
    x = np.asarray(codes)
    h0, h1 = x[:, 0::2].astype(np.int64), x[:, 1::2].astype(np.int64)
    c = np.isin(h0, (0, 1)) & np.isin(h1, (0, 1))
    if keep is not None:
        c = c & np.asarray(keep, dtype=bool)[:, None]
    return (h0 + h1) * c, c.astype(np.int64)


def counts_exact(codes, keep=None) -> np.ndarray:
    """int64 [n_snps, 4]: called, het, hom ALT, 0."""
    g, c = planes(codes, keep)
    return np.stack([c.sum(1), ((g == 1) & (c == 1)).sum(1), ((g == 2) & (c == 1)).sum(1), np.zeros(len(g), dtype=np.int64)], axis=1)


class Cell:
    """One (SNP, phenotype) cell: ``flag`` and, for flags 0 and 5, the exact ``beta``, ``s2`` (sigma^2), ``t2``, ``d``."""

    __slots__ = ("flag", "beta", "s2", "t2", "d")

    def __init__(self, flag, beta=None, s2=None, t2=None, d=None):
        self.flag, self.beta, self.s2, self.t2, self.d = flag, beta, s2, t2, d

    @property
    def se(self) -> Decimal:
        with localcontext(CTX):
            return Decimal(0) if self.s2 <= 0 else dec(self.s2 / self.d).sqrt()

    @property
    def t(self) -> Decimal:
        with localcontext(CTX):
            r = dec(self.t2).sqrt()
            return -r if self.beta < 0 else r


def scan_exact(codes, q, e, n_cov: int, keep=None, max_vif=50, snps=None):
    """{(i, j): Cell} for the SNPs ``snps`` (default: all) of the panel ``codes`` [n_snps, 2 N] and the design integers ``q``
    int [N, k], ``e`` [k]: every quantity an exact Fraction."""
    g, c = planes(codes, keep)
    qi = np.asarray(q).astype(np.int64)
    n_ind, k = qi.shape
    df = n_ind - n_cov - 1
    z, zc = g @ qi, c @ qi                                   # |sum| <= 2 N 2^30 < 2^63: exact in int64
    cnt = counts_exact(codes, keep)
    scale = [Fraction(2) ** (int(v) - SCALE_BITS) for v in e]
    yy = [sum(int(v) ** 2 for v in qi[:, col]) * scale[col] ** 2 for col in range(n_cov, k)]
    out = {}
    for i in (range(len(g)) if snps is None else snps):
        n, het, hom = (int(v) for v in cnt[i, :3])
        s, e2 = het + 2 * hom, het + 4 * hom
        flag = 1 if n == 0 else (2 if n * e2 == s * s else 0)
        if flag == 0:
            mu, gg = Fraction(s, n), Fraction(n * e2 - s * s, n)
            d = gg - sum(((int(z[i, a]) - mu * int(zc[i, a])) * scale[a]) ** 2 for a in range(n_cov))
            if d * Fraction(max_vif) < gg:
                flag = 3
        for j in range(k - n_cov):
            col = n_cov + j
            if flag:
                out[i, j] = Cell(flag)
            elif yy[j] == 0:
                out[i, j] = Cell(4)
            else:
                b = (int(z[i, col]) - mu * int(zc[i, col])) * scale[col]
                beta, s2 = b / d, (yy[j] - b * b / d) / df
                out[i, j] = Cell(5, beta, s2, None, d) if s2 <= 0 else Cell(0, beta, s2, beta * beta * d / s2, d)
    return out


# ---- panels and cases that the host and the GPU tests share -----------------------------------------------------------------------
LN10 = 2.302585092994046
LN_P_BOUND = 2.0 ** -30          # |ln p - exact| <= LN_P_BOUND max(1, |exact|): the quantisation step of the inputs


def glm_codes(n_ind, n_snps, seed, miss=0.0):
    """int8 [n_snps, 2 n_ind]: ALT frequencies uniform in [0.1, 0.5]; ``miss`` of the genotypes missing on both haplotypes and a
    further miss / 5 half-missing."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.1, 0.5, size=n_snps)
    codes = (rng.random((n_snps, 2 * n_ind)) < f[:, None]).astype(np.int8)
    if miss:
        u = rng.random((n_snps, n_ind))
        codes[np.repeat(u < miss, 2, axis=1)] = 2
        codes[:, 1::2][(u >= miss) & (u < 1.2 * miss)] = 2
    return codes


def glm_traits(codes, p, n_cov, seed, effect=0.5):
    """(Y [N, p], covar [N, n_cov - 1] or None): standard normal covariates and phenotypes; phenotype j adds ``effect`` times the
    dosage of SNP j (missing as 0) where the panel has such a SNP, so that some cells carry a signal."""
    g, _ = planes(codes)
    rng = np.random.default_rng(seed)
    n = g.shape[1]
    Y = rng.standard_normal((n, p))
    for j in range(min(p, g.shape[0])):
        Y[:, j] += effect * g[j]
    return Y, (rng.standard_normal((n, n_cov - 1)) if n_cov > 1 else None)


def ln_p_check(result, codes, n_cov, cells=None, limit=300, keep=None):
    """Compare ln p of ``result`` (a GlmResult) with the oracle on ``cells`` (default: at most ``limit`` of the cells with flag
    0, evenly spread, the smallest and the largest p among them).  Returns (cells compared, largest error / allowed error)."""
    flags = result.flags.cpu().numpy()
    nlp = result.neglog10_p.cpu().numpy()
    if cells is None:
        live = np.argwhere(flags == 0)
        if len(live) > limit:
            order = np.argsort(nlp[flags == 0], kind="stable")
            pick = np.unique(np.concatenate([[order[0], order[-1]], np.arange(0, len(live), -(-len(live) // (limit - 2)))]))
            live = live[pick]
        cells = [(int(i), int(j)) for i, j in live]
    exact = scan_exact(codes, result.design.q, result.design.exps, n_cov, keep=keep, snps=sorted({i for i, _ in cells}))
    worst = 0.0
    for i, j in cells:
        assert exact[i, j].flag == 0 == flags[i, j], (i, j, exact[i, j].flag, flags[i, j])
        want = float(ln_p_exact(exact[i, j].t2, result.df))
        worst = max(worst, abs(-nlp[i, j] * LN10 - want) / (LN_P_BOUND * max(1.0, abs(want))))
    return len(cells), worst


N_FLAG = 64


def flag_panel():
    """The flag cases, on 64 individuals without covariates.  Returns (codes [7, 128], keep, Y [64, 4], want uint8 [7, 4]).
    SNPs: 0 no call; 1 monomorphic; 2 every genotype het; 3 and 5 random; 4: 16 hom ALT, 32 het, 16 hom REF (mean dosage 1, so
    that every quantity of its cells is a dyadic number); 6 random but dropped by ``keep``.  Phenotypes: 0 standard normal;
    1 the constant 2 (flag 4); 2 = 3 g_4 + 2, an exact line in SNP 4 (flag 5 there); 3 = +-1, balanced inside every genotype
    class of SNP 4 (t = 0 there)."""
    rng = np.random.default_rng(11)
    codes = glm_codes(N_FLAG, 7, seed=12)
    codes[0] = 2
    codes[1] = 0
    codes[2, 0::2], codes[2, 1::2] = 1, 0
    g4 = np.repeat([2, 1, 0], [16, 32, 16])
    codes[4, 0::2], codes[4, 1::2] = (g4 >= 1), (g4 == 2)
    keep = np.ones(7, dtype=bool)
    keep[6] = False
    sign = np.tile([1.0, -1.0], N_FLAG // 2)          # the classes of SNP 4 start at even individuals and have even sizes
    Y = np.stack([rng.standard_normal(N_FLAG), np.full(N_FLAG, 2.0), 3.0 * g4 + 2.0, sign], axis=1)
    want = np.zeros((7, 4), dtype=np.uint8)
    want[:, 1] = 4
    want[4, 2] = 5
    want[[0, 6]] = 1
    want[[1, 2]] = 2
    return codes, keep, Y, want


def check_flag_panel(res, dosage_res):
    """The assertions on the flag panel: ``res`` = scan of flag_panel(), ``dosage_res`` = scan of phenotype 0 with the dosage of
    SNP 3 as the covariate (flag 3 at SNP 3)."""
    _, _, _, want = flag_panel()
    flags = res.flags.cpu().numpy()
    assert np.array_equal(flags, want), flags
    outs = [x.cpu().numpy() for x in (res.beta, res.se, res.t, res.p, res.neglog10_p)]
    dead = (want != 0) & (want != 5)
    for x in outs:
        assert np.isnan(x[dead]).all() and np.isfinite(x[want == 0]).all()
    beta, se, t, p, nlp = (x[4, 2] for x in outs)                                    # the perfect fit
    assert (beta, se, t, p, nlp) == (3.0, 0.0, np.inf, 0.0, np.inf)
    beta, se, t, p, nlp = (x[4, 3] for x in outs)                                    # t = 0
    assert beta == 0.0 and se > 0.0 and t == 0.0 and p == 1.0 and nlp == 0.0
    f3 = dosage_res.flags.cpu().numpy()[:, 0]
    assert f3[3] == 3 and np.array_equal(f3[[0, 1, 2, 6]], [1, 2, 2, 1]) and (f3[[4, 5]] == 0).all(), f3
    assert np.isnan(dosage_res.beta.cpu().numpy()[3, 0])

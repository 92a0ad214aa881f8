"""An exact oracle for the logistic association scan (include/ldx.h, "logistic association scan") -- TEST INFRASTRUCTURE ONLY, a
plain module like tests/ld_glm_exact.py.  No tests here.

Written from the definition alone; numpy integers, ``fractions`` and ``decimal`` only (no mpmath).  A cell is fitted on the RAW
design [1 | X | x] -- not on the orthonormal basis the scan iterates on: beta^ and se do not depend on the parametrisation -- by a
damped Newton iteration from 0 at 60 digits: the step is halved while it lowers the log-likelihood, and the iteration ends when the
Newton decrement U^T I^-1 U is below 1e-80 (that last step is applied).  se comes from the information matrix at the optimum.

ln erfc(t) is a Taylor series of erf below t = 6 (at 140 digits: the terms reach e^(t^2) and the difference 1 - erf loses as much
again) and the continued fraction  erfc(t) = e^(-t^2) / sqrt(pi) / (t + (1/2) / (t + 1 / (t + (3/2) / (t + ...))))  from there on,
400 terms from the bottom (the two agree to 50 digits at t = 6: tests/test_logistic_host.py).
"""
from decimal import Context, Decimal, localcontext
from fractions import Fraction

import numpy as np

PREC = 60
CTX = Context(prec=PREC, Emax=999999999, Emin=-999999999)
WIDE = Context(prec=140, Emax=999999999, Emin=-999999999)
PI = Decimal("3.1415926535897932384626433832795028841971693993751058209749445923078164062862089986280348253421170679"
             "8214808651328230664709384460955058223172535940812848111745")
DECREMENT = Decimal("1e-80")
MAX_NEWTON = 200


def planes(codes, keep=None):
    """(g, c) int64 [n_snps, n_ind]: the ALT dosage of the called genotypes (0 where missing) and the called flag."""
    x = np.asarray(codes)
    h0, h1 = x[:, 0::2].astype(np.int64), x[:, 1::2].astype(np.int64)
    c = np.isin(h0, (0, 1)) & np.isin(h1, (0, 1))
    if keep is not None:
        c = c & np.asarray(keep, dtype=bool)[:, None]
    return (h0 + h1) * c, c.astype(np.int64)


def _solve(info, grad):
    """(delta, [I^-1]_last,last) of the symmetric positive definite ``info`` by Cholesky, or None where a pivot is not > 0."""
    m = len(grad)
    L = [[Decimal(0)] * m for _ in range(m)]
    for i in range(m):
        for j in range(i + 1):
            s = info[i][j] - sum((L[i][k] * L[j][k] for k in range(j)), Decimal(0))
            if i == j:
                if s <= 0:
                    return None
                L[i][i] = s.sqrt()
            else:
                L[i][j] = s / L[j][j]
    zf = [Decimal(0)] * m
    for i in range(m):
        zf[i] = (grad[i] - sum((L[i][k] * zf[k] for k in range(i)), Decimal(0))) / L[i][i]
    d = [Decimal(0)] * m
    for i in range(m - 1, -1, -1):
        d[i] = (zf[i] - sum((L[k][i] * d[k] for k in range(i + 1, m)), Decimal(0))) / L[i][i]
    return d, 1 / (L[m - 1][m - 1] * L[m - 1][m - 1]), sum((t * t for t in zf), Decimal(0))


class Fit:
    """One cell's exact fit: ``ok`` (a finite maximiser was found), ``theta`` (the genotype's coefficient last), ``beta``, ``se``,
    ``z`` as Decimals, ``max_eta`` = max |eta^| and the Newton steps taken."""

    __slots__ = ("ok", "theta", "beta", "se", "z", "max_eta", "steps")

    def __init__(self, ok, theta=None, se=None, max_eta=None, steps=0):
        self.ok, self.theta, self.se, self.max_eta, self.steps = ok, theta, se, max_eta, steps
        self.beta = theta[-1] if ok else None
        with localcontext(CTX):
            self.z = self.beta / se if ok else None


def fit_exact(rows, y, max_eta=Decimal(40)) -> Fit:
    """The maximum-likelihood logistic fit of ``y`` (0/1) on the design whose columns are ``rows`` (a list of m sequences of N
    Decimals; the standard error is that of the LAST one).  Not ok: the information loses positive definiteness, |eta| passes
    ``max_eta`` (separation: the likelihood has no finite maximiser) or MAX_NEWTON steps do not converge."""
    with localcontext(CTX):
        m, n = len(rows), len(y)
        cols = [[rows[i][a] for i in range(m)] for a in range(n)]
        one = Decimal(1)

        def state(theta):
            eta = [sum((t * v for t, v in zip(theta, va)), Decimal(0)) for va in cols]
            big = max(abs(e) for e in eta)
            if big > max_eta:
                return None
            ex = [(-abs(e)).exp() for e in eta]
            # ln(1 + e^eta) = max(eta, 0) + ln(1 + e^-|eta|)
            ll = sum((e * yy - (max(e, Decimal(0)) + (one + x).ln()) for e, yy, x in zip(eta, y, ex)), Decimal(0))
            mu = [one / (one + x) if e >= 0 else x / (one + x) for e, x in zip(eta, ex)]
            return ll, mu, big

        theta = [Decimal(0)] * m
        cur = state(theta)
        for step in range(1, MAX_NEWTON + 1):
            ll, mu, big = cur
            info = [[Decimal(0)] * m for _ in range(m)]
            grad = [Decimal(0)] * m
            for va, mm, yy in zip(cols, mu, y):
                w, r = mm * (one - mm), yy - mm
                for i in range(m):
                    vi = va[i]
                    if vi == 0:
                        continue
                    grad[i] += vi * r
                    wv = w * vi
                    ri = info[i]
                    for j in range(i + 1):
                        ri[j] += wv * va[j]
            sol = _solve(info, grad)
            if sol is None:
                return Fit(False, steps=step)
            delta, var, dec = sol
            if dec < DECREMENT:
                theta = [t + d for t, d in zip(theta, delta)]
                fin = state(theta)
                if fin is None:
                    return Fit(False, steps=step)
                # the information once more, at the optimum
                info = [[Decimal(0)] * m for _ in range(m)]
                for va, mm in zip(cols, fin[1]):
                    w = mm * (one - mm)
                    for i in range(m):
                        wv = w * va[i]
                        for j in range(i + 1):
                            info[i][j] += wv * va[j]
                sol = _solve(info, [Decimal(0)] * m)
                if sol is None:
                    return Fit(False, steps=step)
                return Fit(True, theta, sol[1].sqrt(), fin[2], step)
            t = one
            # a full step gains about dec / 2: below 1e-45 |l| that is under the rounding of l at 60 digits, and the test is moot
            moot = dec < Decimal("1e-45") * max(one, abs(ll))
            while True:
                trial = [a + t * d for a, d in zip(theta, delta)]
                nxt = state(trial)
                if nxt is not None and (moot or nxt[0] >= ll):
                    break
                t = t / 2
                if t < Decimal("1e-12"):
                    return Fit(False, steps=step)
            theta, cur = trial, nxt
        return Fit(False, steps=MAX_NEWTON)


def cell_rows(codes, covar, i, keep=None):
    """The raw design of SNP ``i``: [1 | X | x] as rows of Decimals, x = g - mu over the called, 0 where missing; None for a SNP
    without a call or with a constant genotype."""
    g, c = planes(codes, keep)
    n_ind = g.shape[1]
    n = int(c[i].sum())
    if n == 0:
        return None
    s = int(g[i].sum())
    if n * int((g[i] * g[i]).sum()) == s * s:
        return None
    with localcontext(CTX):
        mu = Decimal(s) / Decimal(n)
        x = [Decimal(int(g[i, a])) - mu if c[i, a] else Decimal(0) for a in range(n_ind)]
    rows = [[Decimal(1)] * n_ind]
    if covar is not None:
        X = np.asarray(covar, dtype=np.float64).reshape(n_ind, -1)
        rows += [[Decimal(float(v)) for v in X[:, k]] for k in range(X.shape[1])]
    return rows + [x]


def cell_exact(codes, Y, covar, i, j, keep=None) -> Fit:
    """The exact fit of cell (SNP i, phenotype j); not ok where the SNP has no fit (flags 1, 2) too."""
    rows = cell_rows(codes, covar, i, keep)
    if rows is None:
        return Fit(False)
    y = np.asarray(Y).reshape(len(rows[0]), -1)[:, j]
    return fit_exact(rows, [Decimal(int(v)) for v in y])


def table_exact(a: int, b: int, c: int, d: int):
    """(beta, se) of the 2 x 2 table {cases, controls} x {genotype value high, low} = a, b (cases) and c, d (controls):
    beta = ln(a d / (b c)) per unit of the genotype difference, se = sqrt(1/a + 1/b + 1/c + 1/d), as Decimals."""
    with localcontext(CTX):
        return (Decimal(a * d) / Decimal(b * c)).ln(), (Decimal(1) / a + Decimal(1) / b + Decimal(1) / c + Decimal(1) / d).sqrt()


def ln_erfc_series(t: Decimal) -> Decimal:
    with localcontext(WIDE):
        t = +t
        term, total, n, t2 = t, t, 0, t * t
        while abs(term) > Decimal(10) ** -135 * max(abs(total), Decimal("1e-30")) or n < 4:
            n += 1
            term = -term * t2 / n
            total += term / (2 * n + 1)
            if n > 4000:
                raise RuntimeError("the oracle's erf series did not converge")
        return (1 - 2 * total / PI.sqrt()).ln()


def ln_erfc_cf(t: Decimal) -> Decimal:
    with localcontext(WIDE):
        t = +t
        f = Decimal(0)
        for k in range(400, 0, -1):
            f = (Decimal(k) / 2) / (t + f)
        return -t * t - PI.sqrt().ln() - (t + f).ln()


def ln_erfc(t) -> Decimal:
    """ln erfc(t), t >= 0 (a float is taken exactly)."""
    t = t if isinstance(t, Decimal) else Decimal(float(t))
    return ln_erfc_series(t) if t < 6 else ln_erfc_cf(t)


def ln_p_exact(z) -> Decimal:
    """ln of p = erfc(|z| / sqrt 2) for the fp64 (or Decimal) ``z`` taken exactly."""
    with localcontext(WIDE):
        zz = z if isinstance(z, Decimal) else Decimal(float(z))
        return ln_erfc(abs(zz) / Decimal(2).sqrt())


# ---- generators ----------------------------------------------------------------------------------------------------------------
def logit_codes(n_ind: int, n_snps: int, seed: int, miss: float = 0.0) -> np.ndarray:
    """int8 [n_snps, 2 n_ind]: independent SNPs with ALT frequencies in [0.15, 0.5], ``miss`` of the haplotype codes missing (2)."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.15, 0.5, n_snps)
    codes = (rng.random((n_snps, 2 * n_ind)) < f[:, None]).astype(np.int8)
    if miss:
        codes[rng.random(codes.shape) < miss] = 2
    return codes


def logit_traits(codes, n_pheno: int, n_cov: int, seed: int, effect: float = 0.9, cov_effect: float = 0.4):
    """(Y uint8 [N, n_pheno], C float64 [N, n_cov] or None): standard normal covariates; phenotype j is Bernoulli with log odds
    -0.2 + cov_effect (first covariate) + effect (dosage of SNP j mod n_snps, centred): one planted SNP per phenotype."""
    rng = np.random.default_rng(seed)
    g, _ = planes(codes)
    n_ind = g.shape[1]
    C = rng.standard_normal((n_ind, n_cov)) if n_cov else None
    Y = np.zeros((n_ind, n_pheno), dtype=np.uint8)
    for j in range(n_pheno):
        x = g[j % g.shape[0]].astype(np.float64)
        eta = -0.2 + effect * (x - x.mean()) + (cov_effect * C[:, 0] if n_cov else 0.0)
        Y[:, j] = rng.random(n_ind) < 1.0 / (1.0 + np.exp(-eta))
    return Y, C


def table_panel(a: int, b: int, c: int, d: int):
    """(codes int8 [1, 2 N], y uint8 [N]) of the 2 x 2 table of table_exact with genotype values 1 (high) and 0 (low), no missing
    call: the a + c heterozygotes first."""
    n = a + b + c + d
    g = np.array([1] * a + [0] * b + [1] * c + [0] * d)
    y = np.array([1] * a + [1] * b + [0] * c + [0] * d, dtype=np.uint8)
    order = np.random.default_rng(a + 7 * d).permutation(n)
    g, y = g[order], y[order]
    codes = np.zeros((1, 2 * n), dtype=np.int8)
    codes[0, 0::2] = g
    return codes, y


def flag_panel():
    """(codes [6, 2 x 40], keep, Y [40, 2], covar [40, 1]) on which every flag occurs on purpose:
    SNP 0 ordinary (flag 0 under phenotype 0), SNP 1 not kept (1), SNP 2 monomorphic among the called (2), SNP 3 whose dosages ARE
    the covariate column (3), SNP 4 with g > 0 <=> case of phenotype 0 (5: complete separation), SNP 5 without a call (1);
    phenotype 1 is all cases (4 wherever flags 1 - 3 do not apply)."""
    n = 40
    rng = np.random.default_rng(12)
    codes = (rng.random((6, 2 * n)) < 0.35).astype(np.int8)
    codes[2] = 1
    codes[2, :6] = 2                                    # three individuals missing, the others homozygous ALT
    codes[5] = 2
    y0 = (rng.random(n) < 0.5).astype(np.uint8)
    y0[:4] = (0, 1, 0, 1)
    codes[4] = 0
    codes[4, 0::2] = y0                                  # heterozygous exactly in the cases
    g3 = (codes[3, 0::2] == 1).astype(np.float64) + (codes[3, 1::2] == 1)
    keep = np.array([1, 0, 1, 1, 1, 1], dtype=bool)
    Y = np.stack([y0, np.ones(n, dtype=np.uint8)], axis=1)
    return codes, keep, Y, g3[:, None]


FLAG_PANEL_WANT = np.array([[0, 4], [1, 1], [2, 2], [3, 3], [5, 4], [1, 1]], dtype=np.uint8)


def check_flag_panel(res) -> None:
    """``res``: the scan of flag_panel() with its covariate and keep."""
    to_np = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)  # noqa: E731
    flags = to_np(res.flags)
    assert flags.dtype == np.uint8 and np.array_equal(flags, FLAG_PANEL_WANT), flags
    dead = flags != 0
    for name in ("beta", "se", "z", "p", "neglog10_p"):
        v = to_np(getattr(res, name))
        assert np.isnan(v[dead]).all() and np.isfinite(v[~dead]).all(), name
    it = to_np(res.n_iter)
    assert (it[flags < 5] <= 12).all() and (it[(flags >= 1) & (flags <= 4)] == 0).all() and it[0, 0] >= 2


def compare(res, codes, Y, covar, cells, keep=None):
    """The largest errors of ``res`` over ``cells`` [(i, j)] in units of the bounds of include/ldx.h: (beta error / (2^-40 se),
    se relative error / 2^-40, ln p error / (2^-30 max(1, |ln p|)), the largest max |eta^| of the oracle).  Every cell must carry
    flag 0 and have an exact fit."""
    to_np = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)  # noqa: E731
    beta, se, z, nlp, flags = (to_np(getattr(res, k)) for k in ("beta", "se", "z", "neglog10_p", "flags"))
    worst_b = worst_s = worst_p = worst_eta = 0.0
    with localcontext(CTX):
        tol = Decimal(2) ** -40
        for i, j in cells:
            assert flags[i, j] == 0, (i, j, flags[i, j])
            fit = cell_exact(codes, Y, covar, i, j, keep)
            assert fit.ok, (i, j)
            worst_eta = max(worst_eta, float(fit.max_eta))
            worst_b = max(worst_b, float(abs(Decimal(float(beta[i, j])) - fit.beta) / (tol * fit.se)))
            worst_s = max(worst_s, float(abs(Decimal(float(se[i, j])) / fit.se - 1) / tol))
            assert float(z[i, j]) == float(beta[i, j]) / float(se[i, j])
            lnp = ln_p_exact(float(z[i, j]))
            got = Decimal(float(nlp[i, j])) * -Decimal(10).ln()
            worst_p = max(worst_p, float(abs(got - lnp) / (Decimal(2) ** -30 * max(Decimal(1), abs(lnp)))))
    return worst_b, worst_s, worst_p, worst_eta


def pick_cells(res, limit: int = 8):
    """At most ``limit`` flag-0 cells of ``res``, the smallest and the largest |z| among them, the others spread evenly."""
    to_np = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)  # noqa: E731
    flags, z = to_np(res.flags), np.abs(to_np(res.z))
    live = np.argwhere(flags == 0)
    if len(live) == 0:
        return []
    order = live[np.argsort(z[live[:, 0], live[:, 1]], kind="stable")]
    if len(order) <= limit:
        return [tuple(int(v) for v in c) for c in order]
    idx = np.unique(np.round(np.linspace(0, len(order) - 1, limit)).astype(int))
    return [tuple(int(v) for v in order[k]) for k in idx]


# ---- the shared cases: (n_ind, n_snps, missing rate, phenotypes, n_cov) ----------------------------------------------------------
# 37 and 203 individuals leave a partial 64-individual step and a partial K-group of 4, 64 is exactly one step, 203 more than three;
# 1, 130 and 300 SNPs are a slab tail and more than two slabs; n_cov 0 and 13 are the empty and the full parameter tile.  (37
# individuals are never paired with 13 covariates: that separates.)
CASES = ((37, 300, 0.05, 1, 0), (37, 130, 0.0, 3, 1), (64, 130, 0.0, 1, 3), (64, 1, 0.05, 3, 13),
         (203, 1, 0.05, 1, 1), (203, 300, 0.05, 3, 3), (203, 130, 0.05, 2, 13))
# per case the generator's seed: chosen on the CPU so that the mirror flags at most 2 % of the cells with 5 and the oracle has
# max |eta^| <= 15 on every compared cell (tests/test_logistic_host.py asserts both)
CASE_SEEDS = {c: 1 for c in CASES}
MAX_ETA = 15.0
_CASE_CACHE = {}


def case_data(case):
    """(codes, Y, C) of a case, made once."""
    if case not in _CASE_CACHE:
        n_ind, n_snps, miss, p, n_cov = case
        seed = 1000 * CASE_SEEDS[case] + n_ind + n_snps + p + n_cov
        codes = logit_codes(n_ind, n_snps, seed, miss)
        # 64 individuals under 15 parameters: weak covariate and SNP effects keep the fit away from separation
        small = n_ind <= 5 * (n_cov + 2)
        Y, C = logit_traits(codes, p, n_cov, seed + 1, effect=0.5 if small else 0.9, cov_effect=0.2 if small else 0.4)
        _CASE_CACHE[case] = (codes, Y, C)
    return _CASE_CACHE[case]

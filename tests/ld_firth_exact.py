"""An exact oracle for the Firth logistic association scan (include/ldx.h, "Firth logistic association scan") -- TEST
INFRASTRUCTURE ONLY, a plain module like tests/ld_logistic_exact.py, whose generators, cases and tail oracle it shares.  No tests here.

Written from the definition alone, ``decimal`` at 60 digits.  A cell is fitted on the RAW design [1 | X | x] (beta^ and se do not
depend on the parametrisation: ln det I changes by a constant) by Fisher scoring on the modified score
U* = sum_a v_a [y_a - mu_a + h_a (1/2 - mu_a)] from 0, the step halved while it lowers l* = l + 1/2 ln det I.  A point is returned
only when the modified score evaluated AT it has lambda*^2 = U*^T I^-1 U* < 1e-44: the scoring step left is under 1e-22 se, nine
decades under the 2^-40 of the accuracy contract.  se comes from the unpenalised information at that point.
"""
from decimal import Decimal, localcontext

import numpy as np

from ld_logistic_exact import (CASES, CTX, Fit, case_data, cell_rows, flag_panel, ln_p_exact, logit_codes, logit_traits,  # noqa: F401
                               pick_cells, planes, table_panel)

STOP = Decimal("1e-44")
MAX_SCORING = 400


def _cholesky(info):
    """(L, L^-1) of the symmetric positive definite ``info`` (its lower triangle), or None where a pivot is not > 0."""
    m = len(info)
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
    M = [[Decimal(0)] * m for _ in range(m)]
    for i in range(m):
        M[i][i] = 1 / L[i][i]
        for j in range(i):
            M[i][j] = -sum((L[i][k] * M[k][j] for k in range(j, i)), Decimal(0)) / L[i][i]
    return L, M


def fit_firth_exact(rows, y, max_eta=Decimal(60)) -> Fit:
    """The Firth fit of ``y`` (0/1) on the design whose columns are ``rows`` (a list of m sequences of N Decimals; the standard
    error is that of the LAST one).  Not ok: the information loses positive definiteness, |eta| passes ``max_eta`` or MAX_SCORING
    steps do not converge."""
    with localcontext(CTX):
        m, n = len(rows), len(y)
        cols = [[rows[i][a] for i in range(m)] for a in range(n)]
        one, half = Decimal(1), Decimal("0.5")

        def state(theta):
            """(l*, modified score as zf = L^-1 U*, lambda*^2, M, max |eta|) at theta, or None."""
            eta = [sum((t * v for t, v in zip(theta, va)), Decimal(0)) for va in cols]
            big = max(abs(e) for e in eta)
            if big > max_eta:
                return None
            ex = [(-abs(e)).exp() for e in eta]
            ll = sum((e * yy - (max(e, Decimal(0)) + (one + x).ln()) for e, yy, x in zip(eta, y, ex)), Decimal(0))
            mu = [one / (one + x) if e >= 0 else x / (one + x) for e, x in zip(eta, ex)]
            info = [[Decimal(0)] * m for _ in range(m)]
            for va, mm in zip(cols, mu):
                w = mm * (one - mm)
                for i in range(m):
                    wv = w * va[i]
                    if wv == 0:
                        continue
                    ri = info[i]
                    for j in range(i + 1):
                        ri[j] += wv * va[j]
            fac = _cholesky(info)
            if fac is None:
                return None
            L, M = fac
            score = [Decimal(0)] * m
            for va, mm, yy in zip(cols, mu, y):
                t2 = Decimal(0)
                for i in range(m):
                    t = sum((M[i][k] * va[k] for k in range(i + 1)), Decimal(0))
                    t2 += t * t
                adj = yy - mm + mm * (one - mm) * t2 * (half - mm)
                for i in range(m):
                    score[i] += va[i] * adj
            zf = [sum((M[i][k] * score[k] for k in range(i + 1)), Decimal(0)) for i in range(m)]
            lstar = ll + sum((L[i][i].ln() for i in range(m)), Decimal(0))
            return lstar, zf, sum((t * t for t in zf), Decimal(0)), M, big

        theta = [Decimal(0)] * m
        cur = state(theta)
        if cur is None:
            return Fit(False)
        for step in range(1, MAX_SCORING + 1):
            lstar, zf, dec, M, big = cur
            if dec < STOP:
                return Fit(True, theta, M[m - 1][m - 1], big, step)     # [I^-1]_last,last = M_last,last^2
            delta = [sum((M[k][i] * zf[k] for k in range(i, m)), Decimal(0)) for i in range(m)]
            t = one
            # the gain of a step is of the order of dec: below 1e-45 |l*| it is under the rounding of l* at 60 digits
            moot = dec < Decimal("1e-45") * max(one, abs(lstar))
            while True:
                trial = [a + t * d for a, d in zip(theta, delta)]
                nxt = state(trial)
                if nxt is not None and (moot or nxt[0] >= lstar):
                    break
                t = t / 2
                if t < Decimal("1e-12"):
                    return Fit(False, steps=step)
            theta, cur = trial, nxt
        return Fit(False, steps=MAX_SCORING)


def cell_firth_exact(codes, Y, covar, i, j, keep=None) -> Fit:
    """The exact Firth fit of cell (SNP i, phenotype j); not ok where the SNP has no fit (flags 1, 2) too."""
    rows = cell_rows(codes, covar, i, keep)
    if rows is None:
        return Fit(False)
    y = np.asarray(Y).reshape(len(rows[0]), -1)[:, j]
    return fit_firth_exact(rows, [Decimal(int(v)) for v in y])


def table_firth_exact(a: int, b: int, c: int, d: int):
    """(beta, se) of the 2 x 2 table {cases, controls} x {genotype value high, low} = a, b (cases) and c, d (controls) under Firth's
    penalty, the Haldane-Anscombe estimate: beta = ln[(a + 1/2)(d + 1/2) / ((b + 1/2)(c + 1/2))] and
    se^2 = 1 / (n_h mu_h (1 - mu_h)) + 1 / (n_l mu_l (1 - mu_l)) with mu_h = (a + 1/2) / (a + c + 1), mu_l = (b + 1/2) / (b + d + 1),
    n_h = a + c, n_l = b + d -- as Decimals.  Zero cells are fine."""
    with localcontext(CTX):
        h = Decimal("0.5")
        beta = ((a + h) * (d + h) / ((b + h) * (c + h))).ln()
        mu_h, mu_l = (a + h) / (a + c + 1), (b + h) / (b + d + 1)
        var = 1 / ((a + c) * mu_h * (1 - mu_h)) + 1 / ((b + d) * mu_l * (1 - mu_l))
        return beta, var.sqrt()


RARE_SEED = 3


def rare_panel(n_ind: int = 203, n_snps: int = 40, n_cov: int = 3, seed: int = RARE_SEED):
    """(codes int8 [n_snps, 2 n_ind], Y uint8 [n_ind, 2], C [n_ind, n_cov]): the even SNPs are ordinary (logit_codes, 3 % of the
    codes missing), the odd ones have 3 - 8 heterozygous carriers and no other ALT allele, every carrier a case of phenotype 0:
    quasi-complete separation, the maximum-likelihood scan's flag 5.  RARE_SEED is chosen on the CPU so that the ML mirror flags
    at least 10 cells with 5 and the Firth mirror none (tests/test_firth_host.py asserts both)."""
    codes = logit_codes(n_ind, n_snps, 7000 + seed, miss=0.03)
    Y, C = logit_traits(codes, 2, n_cov, 7001 + seed)
    rng = np.random.default_rng(7002 + seed)
    cases = np.flatnonzero(Y[:, 0] != 0)
    for i in range(1, n_snps, 2):
        carriers = rng.choice(cases, size=int(rng.integers(3, 9)), replace=False)
        codes[i] = 0
        codes[i, 2 * carriers] = 1
    return codes, Y, C


def singleton_panel(n_ind: int = 203, n_snps: int = 8, n_cov: int = 3):
    """(codes int8 [n_snps, 2 n_ind], Y uint8 [n_ind, 1], C): SNP k has ONE heterozygous carrier, individual k, and no missing call.
    Such a carrier has a hat value near 1, the penalty's curvature is then about that of the likelihood itself, and the plain
    scoring step goes about twice as far as it should: every one of these cells triggers the step-length safeguard of the
    iteration (include/ldx.h)."""
    codes = logit_codes(n_ind, n_snps, 900 + n_ind, 0.0)
    Y, C = logit_traits(codes, 1, n_cov, 901)
    codes[:] = 0
    codes[np.arange(n_snps), 2 * np.arange(n_snps)] = 1
    return codes, Y, C


def pick_firth_cells(res):
    """At most 3 flag-0 cells of ``res``: the smallest |z|, the largest |z| and the most information evaluations."""
    to_np = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)  # noqa: E731
    flags, z, it = to_np(res.flags), np.abs(to_np(res.z)), to_np(res.n_iter)
    live = np.argwhere(flags == 0)
    if len(live) == 0:
        return []
    zz, ii = z[live[:, 0], live[:, 1]], it[live[:, 0], live[:, 1]]
    picks = []
    for k in (int(np.argmin(zz)), int(np.argmax(zz)), int(np.argmax(ii))):
        cell = (int(live[k, 0]), int(live[k, 1]))
        if cell not in picks:
            picks.append(cell)
    return picks


def compare_firth(res, codes, Y, covar, cells, keep=None):
    """The largest errors of ``res`` over ``cells`` [(i, j)] in units of the bounds of include/ldx.h: (beta error / (2^-40 se),
    se relative error / 2^-40, ln p error / (2^-30 max(1, |ln p|))).  Every cell must carry flag 0 and have an exact fit."""
    to_np = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)  # noqa: E731
    beta, se, z, nlp, flags = (to_np(getattr(res, k)) for k in ("beta", "se", "z", "neglog10_p", "flags"))
    worst_b = worst_s = worst_p = 0.0
    with localcontext(CTX):
        tol = Decimal(2) ** -40
        for i, j in cells:
            assert flags[i, j] == 0, (i, j, flags[i, j])
            fit = cell_firth_exact(codes, Y, covar, i, j, keep)
            assert fit.ok, (i, j)
            worst_b = max(worst_b, float(abs(Decimal(float(beta[i, j])) - fit.beta) / (tol * fit.se)))
            worst_s = max(worst_s, float(abs(Decimal(float(se[i, j])) / fit.se - 1) / tol))
            assert float(z[i, j]) == float(beta[i, j]) / float(se[i, j])
            lnp = ln_p_exact(float(z[i, j]))
            got = Decimal(float(nlp[i, j])) * -Decimal(10).ln()
            worst_p = max(worst_p, float(abs(got - lnp) / (Decimal(2) ** -30 * max(Decimal(1), abs(lnp)))))
    return worst_b, worst_s, worst_p

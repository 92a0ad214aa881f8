"""CPU: the association scan (include/ldx.h, "association scan") on the host mirrors -- the numpy mirror against the exact oracle
(tests/ld_glm_exact.py), the definition against an explicit least-squares fit of the unquantised phenotypes, the flags, the
refusals, the phenotype / covariate parsers and the .glm.linear writer.

The three measured bounds (each: the largest deviation seen over this file's panels, times four, rounded up to a power of two):
  REL_BOUND  beta, se, t of the mirror against the oracle, relative.  Largest seen: 5.44e-14 = 245 x 2^-52 (panel "wide"; "one"
             1.4, "few" 7.6, "full" 32 x 2^-52).  se alone stays at the expected max_vif x n_cov x 2^-52 -- d = gg - sum h^2 is its
             one cancellation and flag 3 bounds it -- but the bound is RELATIVE, and the largest errors belong to the cells of the
             null phenotypes, where b = zy - mu cy cancels to a beta (and t) near 0.
  DEF_BOUND  beta, se, t of ld_glm_host against numpy.linalg.lstsq of the unquantised Y on [1, X, g].
             Largest seen: 1.18e-6 = 1270 x 2^-30 (panel "wide"; "one" 24, "few" 251, "full" 348 x 2^-30): the inputs are quantised
             to 2^-30 of their column's largest entry, a cell sums N of them, and again the largest RELATIVE deviations are those
             of the t nearest 0.
  P_BOUND    p of ld_glm_host against 2 scipy.stats.t.sf(|t|, df) at the t of that least-squares fit, relative.  Largest seen:
             1.71e-8 ("wide"; "one" 4.6e-9, "few" 5.2e-9, "full" 1.25e-8): p is smooth where t passes 0, so it does not share
             the large relative deviations of the t nearest 0.
ln p is held to the fixed 2^-30 max(1, |ln p|) of the definition."""
import math

import numpy as np
import pytest

import ld_glm_exact as X

REL_BOUND = 2.0 ** -42      # 4 x 5.44e-14 = 2.18e-13 <= 2^-42 = 2.27e-13
DEF_BOUND = 2.0 ** -17      # 4 x 1.18e-6 = 4.7e-6 <= 2^-17 = 7.6e-6
P_BOUND = 2.0 ** -23        # 4 x 1.71e-8 = 6.84e-8 <= 2^-23 = 1.19e-7

# name: (n_ind, n_snps, missing rate, phenotypes, n_cov)
PANELS = {"one": (37, 60, 0.0, 1, 1), "few": (64, 40, 0.05, 3, 3), "wide": (200, 30, 0.05, 25, 11), "full": (70, 6, 0.05, 40, 24)}


@pytest.fixture(scope="module")
def scans():
    from ld_tools_amd import ld_glm_host

    out = {}
    for name, (n_ind, n_snps, miss, p, n_cov) in PANELS.items():
        codes = X.glm_codes(n_ind, n_snps, seed=len(name) + n_ind, miss=miss)
        Y, C = X.glm_traits(codes, p, n_cov, seed=n_snps)
        out[name] = (codes, Y, C, n_cov, ld_glm_host(codes, Y, C))
    return out


@pytest.mark.parametrize("name", list(PANELS))
def test_mirror_against_the_oracle(scans, name):
    codes, _, _, n_cov, res = scans[name]
    exact = X.scan_exact(codes, res.design.q, res.design.exps, n_cov)
    flags = res.flags.numpy()
    assert (flags != 6).all()
    worst = 0.0
    for (i, j), cell in exact.items():
        assert cell.flag == flags[i, j], (i, j)
        if cell.flag == 0:
            for got, want in ((res.beta, X.dec(cell.beta)), (res.se, cell.se), (res.t, cell.t)):
                worst = max(worst, abs(float((X.Decimal(got[i, j].item()) - want) / want)))
    n, worst_ln = X.ln_p_check(res, codes, n_cov)
    print(f"{name}: largest relative error of beta, se, t = {worst:.3g} = {worst * 2.0 ** 52:.3g} x 2^-52; "
          f"ln p: {n} cells, largest error / bound = {worst_ln:.3g}")
    assert worst <= REL_BOUND and worst_ln <= 1.0
    p, nlp = res.p.numpy()[flags == 0], res.neglog10_p.numpy()[flags == 0]
    assert np.allclose(-np.log10(p), nlp, rtol=1e-12, atol=1e-15)
    cnt = X.counts_exact(codes)
    assert np.array_equal(res.n_obs, cnt[:, 0])
    assert np.array_equal(res.a1_freq, (cnt[:, 1] + 2 * cnt[:, 2]) / (2.0 * cnt[:, 0]))


def lstsq_cells(codes, Y, C):
    """(beta, se, t) [n_snps, p] of the fit of Y on [1, C, g], g the dosage with the SNP's mean where a call is missing."""
    g, c = X.planes(codes)
    n = g.shape[1]
    D = np.ones((n, 1)) if C is None else np.concatenate([np.ones((n, 1)), C], axis=1)
    out = np.empty((3, len(g), Y.shape[1]))
    for i in range(len(g)):
        gi = np.where(c[i] == 1, g[i], g[i].sum() / c[i].sum())
        A = np.concatenate([D, gi[:, None]], axis=1)
        coef, _, _, _ = np.linalg.lstsq(A, Y, rcond=None)
        rss = ((Y - A @ coef) ** 2).sum(axis=0)
        se = np.sqrt(rss / (n - A.shape[1]) * np.linalg.inv(A.T @ A)[-1, -1])
        out[:, i] = coef[-1], se, coef[-1] / se
    return out


@pytest.fixture(scope="module")
def fits(scans):
    return {name: lstsq_cells(codes, Y, C) for name, (codes, Y, C, _, _) in scans.items()}


@pytest.mark.parametrize("name", list(PANELS))
def test_definition_against_least_squares(scans, fits, name):
    res = scans[name][4]
    assert (res.flags.numpy() == 0).all()
    worst = max(np.abs(got.numpy() / want - 1.0).max() for got, want in zip((res.beta, res.se, res.t), fits[name]))
    print(f"{name}: largest relative deviation from lstsq = {worst:.3g} = {worst * 2.0 ** 30:.3g} x 2^-30")
    assert worst <= DEF_BOUND


@pytest.mark.parametrize("name", list(PANELS))
def test_p_against_scipy(scans, fits, name):
    stats = pytest.importorskip("scipy.stats")
    res = scans[name][4]
    want = 2.0 * stats.t.sf(np.abs(fits[name][2]), res.df)
    worst = np.abs(res.p.numpy() / want - 1.0).max()
    print(f"{name}: largest relative deviation of p from scipy = {worst:.3g}")
    assert worst <= P_BOUND


def test_tail_against_mpmath():
    mp = pytest.importorskip("mpmath")
    from ld_tools_amd import glm_tail_host

    mp.mp.dps = 60
    steps = 0.0
    for df in (1, 2, 3, 4, 5, 6, 7, 30, 200, 1000, 2490, 5118):
        for t in (1e-8, 1e-3, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 37.0, 100.0, 1e3, 1e4, 1e6):
            want = mp.log(mp.betainc(mp.mpf(df) / 2, mp.mpf(1) / 2, 0, mp.mpf(df) / (df + mp.mpf(t) ** 2), regularized=True))
            oracle = mp.mpf(str(X.ln_p_exact(X.Fraction(t) ** 2, df)))
            assert abs(oracle - want) <= mp.mpf(10) ** -35 * max(1, abs(want)), (df, t)
            p, nlp, ok = glm_tail_host(np.array([t, -t]), df)
            assert ok.all() and nlp[0] == nlp[1] and p[0] == p[1]
            steps = max(steps, abs(-nlp[0] * X.LN10 - float(want)) / (X.LN_P_BOUND * max(1.0, abs(float(want)))))
    print("mirror tail against mpmath: largest error / bound =", steps)
    assert steps <= 1.0


def test_flags_each_on_purpose():
    from ld_tools_amd import ld_glm_host

    codes, keep, Y, _ = X.flag_panel()
    g, _ = X.planes(codes)
    X.check_flag_panel(ld_glm_host(codes, Y, keep=keep), ld_glm_host(codes, Y[:, 0], covar=g[3].astype(np.float64), keep=keep))


def test_planted_effect_below_the_float_range():
    from ld_tools_amd import ld_glm_host

    codes = X.glm_codes(200, 5, seed=5)
    g, _ = X.planes(codes)
    Y = g[2] + 0.01 * np.random.default_rng(1).standard_normal(200)
    res = ld_glm_host(codes, Y)
    p, nlp = res.p.numpy()[2, 0], res.neglog10_p.numpy()[2, 0]
    assert p < 2.3e-308 and 300.0 < nlp < 1000.0 and res.flags.numpy()[2, 0] == 0
    assert X.ln_p_check(res, codes, 1, cells=[(2, 0)])[1] <= 1.0


def test_individuals_subset_and_keep():
    from ld_tools_amd import ld_glm_host

    codes = X.glm_codes(50, 20, seed=8, miss=0.05)
    rows = np.random.default_rng(2).permutation(50)[:31]
    Y, C = X.glm_traits(codes[:, np.stack([2 * rows, 2 * rows + 1], 1).reshape(-1)], 2, 3, seed=4)
    keep = np.arange(20) % 3 != 0
    a = ld_glm_host(codes, Y, C, individuals=rows, keep=keep)
    b = ld_glm_host(np.ascontiguousarray(codes[:, np.stack([2 * rows, 2 * rows + 1], 1).reshape(-1)]), Y, C, keep=keep)
    for f in ("beta", "se", "t", "p", "neglog10_p", "flags"):
        assert np.array_equal(getattr(a, f).numpy(), getattr(b, f).numpy(), equal_nan=True)
    assert (a.flags.numpy()[~keep] == 1).all() and (a.flags.numpy()[keep] == 0).all() and a.df == 31 - 3 - 1


def test_refusals():
    from ld_tools_amd import LdxError, glm_design, glm_linear_host, ld_glm_host

    rng = np.random.default_rng(0)
    Y, C = rng.standard_normal((20, 2)), rng.standard_normal((20, 3))
    with pytest.raises(LdxError, match="rank-deficient"):
        glm_design(Y, np.concatenate([C, C[:, :1] + C[:, 1:2]], axis=1))
    with pytest.raises(LdxError, match="rank-deficient"):
        glm_design(Y, np.concatenate([C, np.full((20, 1), 3.0)], axis=1))           # a second intercept
    with pytest.raises(LdxError, match="df"):
        glm_design(Y[:5], C[:5])                                                    # df = 5 - 4 - 1 = 0
    assert glm_design(Y[:6], C[:6]).df == 1
    with pytest.raises(LdxError, match="64"):
        glm_design(rng.standard_normal((100, 61)), rng.standard_normal((100, 3)))    # k = 65
    assert glm_design(rng.standard_normal((100, 60)), rng.standard_normal((100, 3))).q.shape == (100, 64)
    bad = Y.copy()
    bad[3, 1] = np.nan
    with pytest.raises(LdxError, match="not finite"):
        glm_design(bad, C)
    with pytest.raises(LdxError, match="not finite"):
        glm_design(Y, np.where(np.arange(60).reshape(20, 3) == 7, np.inf, C))
    codes = X.glm_codes(20, 4, seed=1)
    with pytest.raises(LdxError, match="20"):
        ld_glm_host(codes, Y[:19])
    with pytest.raises(LdxError, match="max_vif"):
        ld_glm_host(codes, Y, max_vif=1.0)
    with pytest.raises(LdxError):
        glm_linear_host(np.zeros((4, 3), dtype=np.int64), np.zeros((4, 3), dtype=np.int64), np.zeros((4, 4)), np.zeros(3), np.ones(1),
                        3, 2, 50.0)                                                 # df = 0


def test_missing_pairwise_is_refused():
    from ld_tools_amd import LdxError, ops

    with pytest.raises(LdxError, match="complete-case"):
        ops._glm_missing("ld_glm", "pairwise")
    with pytest.raises(LdxError):
        ops._glm_missing("ld_glm", "ref")
    ops._glm_missing("ld_glm", None)


def test_design_integers():
    from ld_tools_amd import glm_design

    rng = np.random.default_rng(3)
    Y, C = rng.standard_normal((30, 2)) * [1.0, 1e6], rng.standard_normal((30, 4))
    des = glm_design(Y, C)
    assert (des.n_ind, des.n_cov, des.n_pheno, des.df) == (30, 5, 2, 24) and des.q.dtype == np.int32 and des.q.shape == (30, 7)
    u = des.q * np.ldexp(1.0, des.exps - 30)[None, :]
    assert np.abs(u[:, :5].T @ u[:, :5] - np.eye(5)).max() < 1e-8 and np.abs(u[:, :5].T @ u[:, 5:]).max() < 1e-8 * 1e6
    assert np.abs(des.q).max(axis=0).min() > 2 ** 29                                # every column uses its 30 bits
    for j in range(2):
        exact = sum(int(v) ** 2 for v in des.q[:, 5 + j])
        assert des.yy[j] == math.ldexp(float(exact), 2 * (int(des.exps[5 + j]) - 30))
    A = np.c_[np.ones(30), C]
    rss = ((Y - A @ np.linalg.lstsq(A, Y, rcond=None)[0]) ** 2).sum(axis=0)
    assert np.allclose(des.yy, rss, rtol=1e-7, atol=0.0)
    # a phenotype inside the span of the design leaves a zero column, whatever its size
    des = glm_design(np.stack([7.0 + 2.0 * C[:, 1], Y[:, 0]], axis=1), C)
    assert not des.q[:, 5].any() and des.yy[0] == 0.0 and des.yy[1] > 0.0


# ---- parsers and the writer ---------------------------------------------------------------------------------------------------------
def test_pheno_and_covar_parsers(tmp_path):
    from ld_tools_amd import LdxError, plink

    a = tmp_path / "a.txt"
    a.write_text("#FID IID height bmi\nF1 I1 1.5 NA\nF1 I2 -9 22\n\nF2 I3 nan 3e1\n")
    fid, iid, names, v = plink.read_pheno(a)
    assert (fid, iid, names) == (["F1", "F1", "F2"], ["I1", "I2", "I3"], ["height", "bmi"])
    assert np.array_equal(v, [[1.5, np.nan], [np.nan, 22.0], [np.nan, 30.0]], equal_nan=True)
    a.write_text("FID\tIID\tx\nF1\tI1\t-9\n")
    assert np.array_equal(plink.read_covar(a)[3], [[-9.0]])                         # -9 is a covariate value
    assert np.isnan(plink.read_pheno(a)[3]).all()
    a.write_text("#IID x y\nI1 1 2\nI2 3 4\n")
    fid, iid, names, v = plink.read_pheno(a)
    assert fid is None and iid == ["I1", "I2"] and names == ["x", "y"] and np.array_equal(v, [[1, 2], [3, 4]])   # no FID column
    for text, what in (("ID x\nI1 1\n", "header"), ("#IID x\nI1 1 2\n", "fields"), ("#IID x\nI1 abc\n", "no number"),
                       ("#IID\nI1\n", "column"), ("#IID x x\nI1 1 2\n", "repeated"), ("#IID x\nI1 1\nI1 2\n", "a line already"),
                       ("#FID IID x\nF I1 1\nG I1 2\nF I1 3\n", "a line already")):
        a.write_text(text)
        with pytest.raises(LdxError, match=what):
            plink.read_pheno(a)
    with pytest.raises(LdxError, match="cannot read"):
        plink.read_covar(tmp_path / "absent")


def test_eigenvec_round_trip_as_covariates(tmp_path):
    from ld_tools_amd import plink
    from ld_tools_amd.drivers.pca import PcaTable, write_eigenvec

    coords = np.random.default_rng(4).standard_normal((5, 3))
    for fid in (["A", "A", "B", "B", "C"], [f"I{k}" for k in range(5)]):           # '#FID IID' and '#IID'
        table = PcaTable(fid, [f"I{k}" for k in range(5)], None, coords, np.ones(5, dtype=bool))
        write_eigenvec(str(tmp_path / "x.eigenvec"), table)
        got = plink.read_covar(tmp_path / "x.eigenvec")
        assert got[0] == (fid if fid != table.iid else None) and got[1] == table.iid and got[2] == ["PC1", "PC2", "PC3"]
        assert np.array_equal(got[3].view(np.uint64), coords.view(np.uint64))


def test_glm_linear_writer(tmp_path):
    from ld_tools_amd import ld_glm_host
    from ld_tools_amd.drivers.glm import GLM_COLUMNS, GlmTable, p_text, write_glm_linear

    codes = X.glm_codes(200, 5, seed=5)
    codes[4] = 0                                                                    # monomorphic: NA
    g, _ = X.planes(codes)
    Y = np.stack([g[2] + 0.01 * np.random.default_rng(1).standard_normal(200), np.random.default_rng(2).standard_normal(200)], 1)
    res = ld_glm_host(codes, Y)
    table = GlmTable(["3"] * 5, [100, 200, 300, 400, 500], [f"rs{k}" for k in range(5)], ["A"] * 5, ["G"] * 5, ["strong", "null"], res)
    path = tmp_path / "x.strong.glm.linear"
    assert write_glm_linear(str(path), table, "strong") == 5
    lines = [ln.split("\t") for ln in path.read_text().splitlines()]
    assert tuple(lines[0]) == GLM_COLUMNS and all(len(ln) == 12 for ln in lines)
    assert lines[5][:8] == ["3", "500", "rs4", "A", "G", "G", "ADD", "200"] and lines[5][8:] == ["NA"] * 4
    row = lines[3]
    assert [float(v) for v in row[8:11]] == [res.beta[2, 0].item(), res.se[2, 0].item(), res.t[2, 0].item()]
    mant, ex = row[11].split("e")
    assert int(ex) < -308 and float(row[11]) == 0.0                                 # below the float64 range, exponent kept
    assert abs(math.log10(float(mant)) + int(ex) + res.neglog10_p[2, 0].item()) < 1e-5
    assert float(lines[1][11]) == res.p[0, 0].item()                                # an ordinary p reads back to its bits
    write_glm_linear(str(path), table, 1)
    assert [float(ln.split("\t")[11]) for ln in path.read_text().splitlines()[1:5]] == res.p[:4, 1].tolist()
    assert p_text(0.0, math.inf) == "0" and p_text(0.0, 400.0) == "1e-400" and p_text(0.0, 399.9999999999) == "1e-400"
    assert p_text(0.25, -math.log10(0.25)) == "0.25"


# ---- the C entries' argument rules, all checked before any HIP call -------------------------------------------------------------------
def test_symbols_and_argument_rules():
    from ld_tools_amd import _lib

    lib, P = _lib.lib, 1 << 20      # P: a non-null, 16-byte aligned address that is never used: every call below is refused first
    for name in ("ldx_geno_snp_counts_dev", "ldx_glm_linear_dev"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)

    def lin(z=P, zc=P, ld_z=8, counts=P, n_snps=10, n_ind=20, n_cov=3, n_pheno=2, exps=P, yy=P, vif=50.0, outs=(P,) * 5, flags=P,
            ld_out=2):
        return lib.ldx_glm_linear_dev(z, zc, ld_z, counts, n_snps, n_ind, n_cov, n_pheno, exps, yy, vif, *outs, flags, ld_out, None)

    refused = [dict(z=None), dict(zc=None), dict(counts=None), dict(exps=None), dict(yy=None), dict(flags=None),
               *(dict(outs=tuple(None if a == b else P for a in range(5))) for b in range(5)),
               dict(n_snps=0), dict(n_cov=0), dict(n_pheno=0), dict(n_cov=40, n_pheno=25, ld_z=65, ld_out=25, n_ind=100),
               dict(ld_z=4), dict(ld_out=1), dict(n_ind=4), dict(n_ind=3), dict(vif=1.0), dict(vif=0.5), dict(vif=float("nan"))]
    for kw in refused:
        assert lin(**kw) == -1, kw
        assert b"ldx_glm_linear_dev" in lib.ldx_last_error()

    def cnt(alt=P, ref=P, n_snps=10, n_hap=20, keep=None, counts=P):
        return lib.ldx_geno_snp_counts_dev(alt, ref, n_snps, n_hap, keep, counts, None)

    for kw in (dict(alt=None), dict(ref=None), dict(counts=None), dict(counts=P + 4), dict(n_hap=0), dict(n_hap=21), dict(n_snps=0)):
        assert cnt(**kw) == -1, kw
    assert cnt(n_hap=_lib.MAX_HAPS + 2) == -3

"""CPU: the Firth logistic association scan (include/ldx.h, "Firth logistic association scan") on the host -- the exact oracle
(tests/ld_firth_exact.py) pinned by the Haldane-Anscombe closed form, zero cells included; the numpy mirror
ld_glm_logistic_host(firth=) against the oracle on the cases the GPU tests run; the fallback on the flag panel and on a panel of
rare all-case variants; the entry's declaration and refusals; the .glm.logistic.hybrid and .glm.firth writers.

Bounds (include/ldx.h): |beta - beta_exact| <= 2^-40 se_exact, |se / se_exact - 1| <= 2^-40; the mirror itself stays 2^6 inside.
Measured here for the mirror over the whole case list (3 cells a case): at most 0.0050 of the bound (2^-47.6 se) in beta and 0.0011
(2^-49.9) in se; 0.0135 and 0.0091 on the separated cells of the flag panel and the rare panel; at most 37 information evaluations
(the case of 64 individuals under 15 parameters, and the flag panel's separated cell); a largest step contraction
lambda*_(k+1) / lambda*_k of 0.447 (64 individuals under 15 parameters).
"""
import math
import re
from decimal import Decimal, localcontext
from pathlib import Path

import numpy as np
import pytest

import ld_firth_exact as F
import ld_logistic_exact as X
from ld_tools_amd import FIRTH_STOP, LdxError, _lib, ld_glm_logistic_host, logit_tail_host, ops

ROOT = Path(__file__).resolve().parents[1]
OUTS = ("beta", "se", "z", "p", "neglog10_p")
TABLES = ((30, 11, 8, 25), (7, 5, 0, 9), (12, 0, 0, 9))


def same(a, b, where):
    """The seven arrays of two host results are equal (NaNs equal) on the cells ``where``."""
    for k in OUTS + ("flags", "n_iter"):
        if not np.array_equal(getattr(a, k).numpy()[where], getattr(b, k).numpy()[where], equal_nan=True):
            return False
    return True


@pytest.fixture(scope="module")
def rare():
    codes, Y, C = F.rare_panel()
    return codes, Y, C, {mode: ld_glm_logistic_host(codes, Y, C, firth=mode) for mode in (None, "fallback", "always")}


def test_oracle_pinned_by_the_closed_form():
    for tab in TABLES:
        codes, y = X.table_panel(*tab)
        fit = F.cell_firth_exact(codes, y, None, 0, 0)
        beta, se = F.table_firth_exact(*tab)
        assert fit.ok
        with localcontext(X.CTX):
            assert abs(fit.beta - beta) <= Decimal("1e-20") * abs(beta) and abs(fit.se - se) <= Decimal("1e-20") * se, tab
    # the zero cells have no maximum-likelihood fit
    assert not X.cell_exact(*X.table_panel(7, 5, 0, 9), None, 0, 0).ok


def test_closed_form_tables_on_the_mirror():
    for tab in TABLES:
        codes, y = X.table_panel(*tab)
        res = ld_glm_logistic_host(codes, y, firth="always")
        beta, se = F.table_firth_exact(*tab)
        assert res.flags.numpy()[0, 0] == 0 and res.firth.numpy()[0, 0] == 1
        assert abs(res.beta.numpy()[0, 0] - float(beta)) <= 2.0 ** -40 * float(se), tab
        assert abs(res.se.numpy()[0, 0] / float(se) - 1.0) <= 2.0 ** -40, tab


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_mirror_against_the_oracle(case):
    n_ind, n_snps, miss, p, n_cov = case
    codes, Y, C = X.case_data(case)
    res = ld_glm_logistic_host(codes, Y, C, firth="always")
    flags, it, mark = res.flags.numpy(), res.n_iter.numpy(), res.firth.numpy()
    assert flags.shape == (n_snps, p) and mark.dtype == np.uint8
    assert (flags <= 4).all() and np.array_equal(mark == 1, flags == 0)          # every cell that is fitted has a finite fit
    assert (it <= _lib.FIRTH_MAX_ITER // 2).all() and (it[flags == 0] >= 2).all() and (it[flags != 0] == 0).all()
    cells = F.pick_firth_cells(res)
    assert 1 <= len(cells) <= 3
    b, s, lp = F.compare_firth(res, codes, Y, C, cells)
    print(f"{case}: {len(cells)} cells, beta error / bound = {b:.3g}, se = {s:.3g}, ln p = {lp:.3g}, most evaluations = {it.max()}")
    assert b <= 1.0 and s <= 1.0 and lp <= 1.0
    assert b <= 2.0 ** -6 and s <= 2.0 ** -6                       # the bound stays 2^6 above the mirror's own error


def test_largest_step_contraction():
    """The scoring steps shrink linearly: the ratio of successive lambda* over the first 60 SNPs of every case and the separated SNP
    of the flag panel (DESIGN.md 3.18 cites the number printed here).  With a contraction below 1/2 the steps not taken sum to less
    than the last one taken, 2^-44 se at the stop constant."""
    worst, where = 0.0, None

    def cell(V, y, start, tag):
        nonlocal worst, where
        decs = []
        _th, _se, _it, ok = ops._firth_scoring(V, y, start, V.shape[0] - 1, decs)
        assert ok, tag
        lam = np.sqrt(np.asarray(decs))
        lam = lam[lam > 2.0 ** -46]                                # below that the ratio is rounding noise of U*
        if len(lam) > 1 and (lam[1:] / lam[:-1]).max() > worst:
            worst, where = float((lam[1:] / lam[:-1]).max()), tag

    for case in X.CASES:
        codes, Y, C = X.case_data(case)
        des = ops.logit_design(Y, C)
        g, called = ops.geno_planes_host(codes[:60], None)
        for i in range(g.shape[0]):
            n = called[i].sum()
            x = np.where(called[i] != 0, g[i] - g[i][called[i] != 0].sum() / max(n, 1), 0.0)
            if n == 0 or not x.any():
                continue
            V = np.concatenate([des.basis, x[None]])
            for j in range(des.n_pheno):
                cell(V, des.y[j], np.concatenate([des.theta0[j], [0.0]]), (case, i, j))
    codes, keep, Y, covar = X.flag_panel()
    des = ops.logit_design(Y[:, 0], covar)
    g, _ = ops.geno_planes_host(codes, None)
    cell(np.concatenate([des.basis, (g[4] - g[4].mean())[None]]), des.y[0], np.concatenate([des.theta0[0], [0.0]]), "flag panel")
    print(f"largest step contraction {worst:.3f} at {where}")
    assert worst < 0.5
    assert FIRTH_STOP == 2.0 ** -88


def test_fallback_on_the_flag_panel():
    codes, keep, Y, covar = X.flag_panel()
    ml = ld_glm_logistic_host(codes, Y, covar, keep=keep)
    fb = ld_glm_logistic_host(codes, Y, covar, keep=keep, firth="fallback")
    assert ml.firth is None and ml.flags.numpy()[4, 0] == 5
    want = X.FLAG_PANEL_WANT.copy()
    want[4, 0] = 0
    mark = np.zeros_like(want)
    mark[4, 0] = 1
    assert np.array_equal(fb.flags.numpy(), want) and np.array_equal(fb.firth.numpy(), mark)
    assert same(fb, ml, mark == 0)
    assert all(np.isfinite(getattr(fb, k).numpy()[4, 0]) for k in OUTS) and fb.n_iter.numpy()[4, 0] <= _lib.FIRTH_MAX_ITER // 2
    b, s, lp = F.compare_firth(fb, codes, Y, covar, [(4, 0)], keep)
    print(f"flag panel, cell (4, 0): beta error / bound = {b:.3g}, se = {s:.3g}, {fb.n_iter.numpy()[4, 0]} evaluations")
    assert b <= 1.0 and s <= 1.0 and lp <= 1.0


def test_fallback_on_rare_all_case_variants(rare):
    codes, Y, C, res = rare
    ml, fb, al = res[None], res["fallback"], res["always"]
    lost = ml.flags.numpy() == 5
    assert lost.sum() >= 10 and lost[1::2, 0].all()                # every planted variant separates under phenotype 0
    assert not (fb.flags.numpy() == 5).any() and not (al.flags.numpy() == 5).any()
    mark = fb.firth.numpy() == 1
    assert np.array_equal(mark, lost)
    assert same(fb, ml, ~mark) and same(fb, al, mark)              # the refit does not depend on how the cell was reached
    assert (fb.n_iter.numpy()[mark] <= _lib.FIRTH_MAX_ITER // 2).all()
    cells = [tuple(int(v) for v in c) for c in np.argwhere(mark)[:2]]
    b, s, lp = F.compare_firth(fb, codes, Y, C, cells)
    print(f"rare panel: {lost.sum()} cells refitted, beta error / bound = {b:.3g}, se = {s:.3g}")
    assert b <= 1.0 and s <= 1.0 and lp <= 1.0


def test_singletons_trigger_the_step_length_safeguard():
    """A variant with one carrier: the plain scoring step overshoots about twofold, lambda*^2 does not fall, the point is given up
    and the step length halved -- once per cell here.  Without the safeguard these cells end in a 2-cycle at the cap."""
    codes, Y, C = F.singleton_panel()
    des = ops.logit_design(Y, C)
    g, _ = ops.geno_planes_host(codes, None)
    for i in range(codes.shape[0]):
        decs = []
        V = np.concatenate([des.basis, (g[i] - g[i].mean())[None]])
        _th, _se, it, ok = ops._firth_scoring(V, des.y[0], np.concatenate([des.theta0[0], [0.0]]), des.n_cov + 1, decs)
        assert ok and (np.diff(decs) >= 0).sum() >= 1, (i, it, decs[:4])
    ml = ld_glm_logistic_host(codes, Y, C)
    fb = ld_glm_logistic_host(codes, Y, C, firth="fallback")
    assert (ml.flags.numpy() == 5).all() and (fb.flags.numpy() == 0).all() and (fb.firth.numpy() == 1).all()
    it = fb.n_iter.numpy()
    cells = F.pick_firth_cells(fb)
    b, s, lp = F.compare_firth(fb, codes, Y, C, cells)
    print(f"singletons: beta error / bound = {b:.3g}, se = {s:.3g}, evaluations {it.min()} - {it.max()}")
    assert (it <= _lib.FIRTH_MAX_ITER // 2).all() and b <= 1.0 and s <= 1.0 and lp <= 1.0


def test_entry_is_declared_bound_and_refuses_before_any_hip_call():
    raw = (ROOT / "include" / "ldx.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int\s+ldx_glm_firth_dev\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 24 == len(_lib.SIGNATURES["ldx_glm_firth_dev"][1])
    assert "Firth logistic association scan" in raw and "NOT validated against" in raw
    assert f"#define LDX_FIRTH_MAX_ITER {_lib.FIRTH_MAX_ITER}u" in raw and 72 <= _lib.FIRTH_MAX_ITER <= 255
    from ld_tools_amd import build
    assert "ldx_firth.hip" in build.SOURCES and "ldx_logit.hip" in build.SOURCES
    # every call below breaks one rule; the pointers are never followed (16 is no address)
    fn, q = _lib.lib.ldx_glm_firth_dev, 16
    good = dict(alt=q, ref=q, n_snps=4, n_hap=40, keep=None, counts=q, design=q, ld_design=20, n_cov=2, y=q, theta0=q, n_pheno=1,
                max_vif=50.0, beta=q, se=q, z=q, p=q, nlp=q, flags=q, n_iter=q, ld_out=1, mode=0, firth=q, stream=None)
    bad = [("mode", 2), ("mode", 7), ("firth", None), ("alt", None), ("counts", None), ("design", None), ("y", None),
           ("theta0", None), ("beta", None), ("flags", None), ("n_iter", None), ("n_hap", 41), ("n_hap", 0), ("n_snps", 0),
           ("n_pheno", 0), ("n_cov", 14), ("ld_design", 19), ("ld_out", 0), ("n_hap", 8), ("max_vif", 1.0),
           ("max_vif", float("nan"))]
    for key, value in bad:
        args = dict(good, **{key: value})
        assert fn(*args.values()) == -1, (key, value)                      # LDX_E_ARG
        assert b"ldx_glm_firth_dev" in _lib.lib.ldx_last_error()
    with pytest.raises(LdxError, match="firth must be"):
        ld_glm_logistic_host(np.zeros((2, 40), dtype=np.int8), np.arange(20) % 2, firth="yes")


def test_hybrid_and_firth_writers(tmp_path):
    from ld_tools_amd.drivers.glm import (HYBRID_COLUMNS, LOGISTIC_COLUMNS, LogisticTable, write_glm_firth, write_glm_hybrid,
                                          write_glm_logistic)

    codes, keep, Y, covar = X.flag_panel()
    n = codes.shape[0]

    def table(res):
        return LogisticTable(["1"] * n, list(range(100, 100 + n)), [f"rs{k}" for k in range(n)], ["A"] * n, ["G"] * n, ["cc", "all"], res)

    fb = ld_glm_logistic_host(codes, Y, covar, keep=keep, firth="fallback")
    fb.z[0, 0], fb.p[0, 0], fb.neglog10_p[0, 0] = 41.0, 0.0, float(logit_tail_host(np.array([41.0]))[1][0])
    path = str(tmp_path / "x.glm.logistic.hybrid")
    assert write_glm_hybrid(path, table(fb), "cc") == n
    lines = [ln.split("\t") for ln in open(path).read().splitlines()]
    assert tuple(lines[0]) == HYBRID_COLUMNS == ("#CHROM", "POS", "ID", "REF", "ALT", "A1", "FIRTH?", "TEST", "OBS_CT", "OR",
                                                 "LOG(OR)_SE", "Z_STAT", "P", "ERRCODE")
    assert all(len(ln) == 14 and ln[7] == "ADD" and ln[5] == "G" for ln in lines[1:])
    assert [ln[6] for ln in lines[1:]] == ["N", "N", "N", "N", "Y", "N"]
    assert [ln[13] for ln in lines[1:]] == [".", "NO_CALL", "CONSTANT_GENOTYPE", "VIF", ".", "NO_CALL"]
    assert all(ln[9:13] == ["NA"] * 4 for k, ln in enumerate(lines[1:]) if k not in (0, 4))
    assert float(lines[5][9]) == math.exp(float(fb.beta[4, 0])) and float(lines[5][10]) == float(fb.se[4, 0])
    assert float(lines[5][11]) == float(fb.z[4, 0]) and float(lines[5][12]) == float(fb.p[4, 0])
    assert re.fullmatch(r"\d(\.\d+)?e-3\d\d", lines[1][12])                   # a P below the float64 range keeps its exponent
    assert [int(ln[8]) for ln in lines[1:]] == fb.n_obs.tolist()
    write_glm_hybrid(path, table(fb), 1)
    assert [ln.split("\t")[13] for ln in open(path).read().splitlines()[1:]][0] == "UNUSABLE_PHENOTYPE"
    al = ld_glm_logistic_host(codes, Y, covar, keep=keep, firth="always")
    path = str(tmp_path / "x.glm.firth")
    assert write_glm_firth(path, table(al), "cc") == n
    lines = [ln.split("\t") for ln in open(path).read().splitlines()]
    assert tuple(lines[0]) == LOGISTIC_COLUMNS and all(len(ln) == 13 and ln[6] == "ADD" for ln in lines[1:])
    assert [ln[12] for ln in lines[1:]] == [".", "NO_CALL", "CONSTANT_GENOTYPE", "VIF", ".", "NO_CALL"]
    assert float(lines[5][8]) == math.exp(float(al.beta[4, 0])) and float(lines[1][9]) == float(al.se[0, 0])
    # a scan without firth= has no FIRTH? column to fill; its own writer is as it was
    ml = ld_glm_logistic_host(codes, Y, covar, keep=keep)
    with pytest.raises(LdxError, match="without firth"):
        write_glm_hybrid(path, table(ml), "cc")
    write_glm_logistic(path, table(ml), "cc")
    assert open(path).readline().rstrip("\n").split("\t") == list(LOGISTIC_COLUMNS)

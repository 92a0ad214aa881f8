"""CPU: the logistic association scan (include/ldx.h, "logistic association scan") on the host -- the exact oracle
(tests/ld_logistic_exact.py) pinned by a closed form, the numpy mirror ld_glm_logistic_host against the oracle on the cases the GPU
tests run, the five flags each on purpose, the refusals, the writer's columns and bfile_logistic's codings.

Bounds (include/ldx.h): |beta - beta_exact| <= 2^-40 se_exact, |se / se_exact - 1| <= 2^-40, ln p within 2^-30 max(1, |ln p|) of the
exact ln erfc at the result's own z.  Measured here for the mirror over the whole case list: 2^-50.6 se in beta, 2^-52.1 relative
in se, 2e-7 of the ln p bound, at most 7 information evaluations -- the 2^-40 stands more than 2^10 above the mirror's error.
"""
import ctypes
import math
import re
from decimal import Decimal, localcontext
from pathlib import Path

import numpy as np
import pytest

import ld_logistic_exact as X
from ld_tools_amd import (LOGIT_FLAGS, LdxError, _lib, ld_glm_logistic, ld_glm_logistic_host, logit_design,  # noqa: F401
                          logit_tail_host)

ROOT = Path(__file__).resolve().parents[1]


def test_oracle_pinned_by_the_closed_form():
    """n_cov = 0, no missing call, a SNP with two genotype values: beta^ = ln(a d / (b c)), se = sqrt(1/a + 1/b + 1/c + 1/d)."""
    for tab in ((7, 5, 4, 9), (30, 11, 8, 25), (3, 40, 20, 6)):
        codes, y = X.table_panel(*tab)
        fit = X.cell_exact(codes, y, None, 0, 0)
        beta, se = X.table_exact(*tab)
        assert fit.ok
        with localcontext(X.CTX):
            assert abs(fit.beta - beta) <= Decimal("1e-50") * abs(beta) and abs(fit.se - se) <= Decimal("1e-50") * se, tab


def test_oracle_ln_erfc_branches_agree():
    with localcontext(X.WIDE):
        for t in (Decimal(6), Decimal("7.5")):
            a, b = X.ln_erfc_series(t), X.ln_erfc_cf(t)
            assert abs(a - b) <= Decimal("1e-50") * abs(a)
        assert abs(X.ln_erfc(Decimal(0))) <= Decimal("1e-100")
        # erfc(1) to 30 digits
        assert abs(X.ln_erfc(Decimal(1)).exp() - Decimal("0.157299207050285130658779364917")) <= Decimal("1e-29")


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_mirror_against_the_oracle(case):
    n_ind, n_snps, miss, p, n_cov = case
    codes, Y, C = X.case_data(case)
    res = ld_glm_logistic_host(codes, Y, C)
    flags, it = res.flags.numpy(), res.n_iter.numpy()
    assert flags.shape == (n_snps, p) and res.design.n_cov == n_cov
    assert (flags == 5).sum() <= 0.02 * flags.size                 # the seeds keep separation rare
    assert (it[flags == 0] <= 12).all() and (it[flags == 0] >= 2).all() and (it[(flags > 0) & (flags < 5)] == 0).all()
    cells = X.pick_cells(res, 8)
    assert 1 <= len(cells) <= 8
    b, s, lp, eta = X.compare(res, codes, Y, C, cells)
    print(f"{case}: {len(cells)} cells, beta error / bound = {b:.3g}, se = {s:.3g}, ln p = {lp:.3g}, max |eta| = {eta:.3g}")
    assert eta <= X.MAX_ETA and b <= 1.0 and s <= 1.0 and lp <= 1.0
    assert b <= 2.0 ** -6 and s <= 2.0 ** -6                       # the bound stays 2^6 above the mirror's own error


def test_closed_form_table_on_the_mirror():
    tab = (30, 11, 8, 25)
    codes, y = X.table_panel(*tab)
    res = ld_glm_logistic_host(codes, y)
    beta, se = X.table_exact(*tab)
    assert res.flags.numpy()[0, 0] == 0
    assert abs(res.beta.numpy()[0, 0] - float(beta)) <= 2.0 ** -40 * float(se)
    assert abs(res.se.numpy()[0, 0] / float(se) - 1.0) <= 2.0 ** -40


def test_flags_each_on_purpose():
    codes, keep, Y, covar = X.flag_panel()
    res = ld_glm_logistic_host(codes, Y, covar, keep=keep)
    X.check_flag_panel(res)
    assert np.isnan(res.design.theta0[1]).all() and np.isfinite(res.design.theta0[0]).all()
    assert sorted(LOGIT_FLAGS) == [0, 1, 2, 3, 4, 5]
    # separation is what the oracle sees too
    assert not X.cell_exact(codes, Y, covar, 4, 0, keep).ok and X.cell_exact(codes, Y, covar, 0, 0, keep).ok


def test_tail_mirror_against_the_oracle():
    z = np.array([0.0, 1e-9, 0.3, -1.0, 3.0, 7.0, 7.0711, 7.08, -12.5, 38.0, 41.0, -60.0])
    p, nlp = logit_tail_host(z)
    assert p[0] == 1.0 and nlp[0] == 0.0 and p[-1] == 0.0 and p[-2] == 0.0 and np.isfinite(nlp).all() and nlp[-2] > 300
    with localcontext(X.WIDE):
        for zz, pp, nn in zip(z, p, nlp):
            lnp = X.ln_p_exact(float(zz))
            got = Decimal(float(nn)) * -Decimal(10).ln()
            assert abs(got - lnp) <= Decimal(2) ** -30 * max(Decimal(1), abs(lnp)), zz
            if pp > 1e-300:
                assert abs(Decimal(float(pp)).ln() - lnp) <= Decimal("1e-12") * max(Decimal(1), abs(lnp))


def test_design_step_and_refusals():
    rng = np.random.default_rng(3)
    n = 50
    y = (rng.random(n) < 0.4).astype(np.uint8)
    C = rng.standard_normal((n, 3))
    des = logit_design(y, C)
    assert des.basis.shape == (4, n) and des.y.shape == (1, n) and des.theta0.shape == (1, 4) and des.n_cov == 3
    assert np.allclose(des.basis @ des.basis.T, n * np.eye(4), atol=1e-9)          # B = sqrt(N) Q
    # the null fit is a stationary point of the likelihood on B
    mu = 1.0 / (1.0 + np.exp(-(des.theta0[0] @ des.basis)))
    assert np.abs(des.basis @ (y - mu)).max() <= 1e-9
    with pytest.raises(LdxError, match="0 .control. and 1"):
        logit_design(y + 1, C)
    with pytest.raises(LdxError, match="0 .control. and 1"):
        ld_glm_logistic_host(np.zeros((2, 2 * n), dtype=np.int8), y * 0.5, C)
    with pytest.raises(LdxError, match="LDX_LOGIT_MAX_COV"):
        logit_design(y, rng.standard_normal((n, 14)))
    with pytest.raises(LdxError, match="rank-deficient"):
        logit_design(y, np.stack([C[:, 0], 2.0 * C[:, 0]], axis=1))
    with pytest.raises(LdxError, match="degree of freedom"):
        logit_design(y[:5], C[:5])
    with pytest.raises(LdxError, match="not finite"):
        logit_design(y, np.where(np.arange(n)[:, None] == 3, np.nan, C))
    with pytest.raises(LdxError, match="max_vif"):
        ld_glm_logistic_host(np.zeros((2, 2 * n), dtype=np.int8), y, C, max_vif=1.0)
    with pytest.raises(LdxError, match="even n_hap"):
        ld_glm_logistic_host(np.zeros((2, 7), dtype=np.int8), y[:3])


def test_entry_is_declared_bound_and_refuses_before_any_hip_call():
    raw = (ROOT / "include" / "ldx.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int\s+ldx_glm_logistic_dev\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 22 == len(_lib.SIGNATURES["ldx_glm_logistic_dev"][1])
    assert "#define LDX_VERSION 102" in raw.replace("  ", " ") and _lib.version() == 102
    assert "#define LDX_LOGIT_MAX_COV 13u" in raw and "#define LDX_LOGIT_MAX_ITER 30u" in raw
    assert _lib.LOGIT_MAX_COV == 13 and _lib.LOGIT_MAX_ITER == 30
    from ld_tools_amd import build
    assert "ldx_logit.hip" in build.SOURCES
    # every call below breaks one rule; the pointers are never followed (16 is no address)
    fn, q = _lib.lib.ldx_glm_logistic_dev, 16
    good = dict(alt=q, ref=q, n_snps=4, n_hap=40, keep=None, counts=q, design=q, ld_design=20, n_cov=2, y=q, theta0=q, n_pheno=1,
                max_vif=50.0, beta=q, se=q, z=q, p=q, nlp=q, flags=q, n_iter=q, ld_out=1, stream=None)
    bad = [("alt", None), ("counts", None), ("design", None), ("y", None), ("theta0", None), ("beta", None), ("flags", None),
           ("n_iter", None), ("n_hap", 41), ("n_hap", 0), ("n_snps", 0), ("n_pheno", 0), ("n_cov", 14), ("ld_design", 19),
           ("ld_out", 0), ("n_hap", 8), ("max_vif", 1.0), ("max_vif", float("nan"))]
    for key, value in bad:
        args = dict(good, **{key: value})
        assert fn(*args.values()) == -1, (key, value)                      # LDX_E_ARG
        assert b"ldx_glm_logistic_dev" in _lib.lib.ldx_last_error()
    assert isinstance(fn, ctypes._CFuncPtr)


def test_writer_columns(tmp_path):
    import torch

    from ld_tools_amd.drivers.glm import LOGISTIC_COLUMNS, LOGISTIC_ERRCODES, LogisticTable, write_glm_logistic

    codes, keep, Y, covar = X.flag_panel()
    res = ld_glm_logistic_host(codes, Y, covar, keep=keep)
    res.z[0, 0], res.p[0, 0], res.neglog10_p[0, 0] = 41.0, 0.0, float(logit_tail_host(np.array([41.0]))[1][0])
    n = codes.shape[0]
    table = LogisticTable(["1"] * n, list(range(100, 100 + n)), [f"rs{k}" for k in range(n)], ["A"] * n, ["G"] * n, ["cc", "all"], res)
    path = str(tmp_path / "x.glm.logistic")
    assert write_glm_logistic(path, table, "cc") == n
    lines = [ln.split("\t") for ln in open(path).read().splitlines()]
    assert tuple(lines[0]) == LOGISTIC_COLUMNS == ("#CHROM", "POS", "ID", "REF", "ALT", "A1", "TEST", "OBS_CT", "OR", "LOG(OR)_SE",
                                                   "Z_STAT", "P", "ERRCODE")
    assert all(len(ln) == 13 and ln[6] == "ADD" and ln[5] == "G" for ln in lines[1:])
    assert float(lines[1][8]) == math.exp(float(res.beta[0, 0])) and float(lines[1][9]) == float(res.se[0, 0]) and lines[1][12] == "."
    assert re.fullmatch(r"\d(\.\d+)?e-3\d\d", lines[1][11])                   # a P below the float64 range keeps its exponent
    assert [ln[12] for ln in lines[1:]] == [".", "NO_CALL", "CONSTANT_GENOTYPE", "VIF", "NO_FINITE_MAXIMISER", "NO_CALL"]
    assert all(ln[8:12] == ["NA"] * 4 for ln in lines[2:]) and [int(ln[7]) for ln in lines[1:]] == res.n_obs.tolist()
    write_glm_logistic(path, table, 1)
    assert [ln.split("\t")[12] for ln in open(path).read().splitlines()[1:]][0] == LOGISTIC_ERRCODES[4] == "UNUSABLE_PHENOTYPE"
    assert isinstance(res.flags, torch.Tensor)


def test_case_control_codings():
    from ld_tools_amd.drivers.plink import case_control

    nan = float("nan")
    assert np.array_equal(case_control("a", [1, 2, 2, nan, 1]), [0, 1, 1, nan, 0], equal_nan=True)
    assert np.array_equal(case_control("a", [0, 1, 1, nan, 0]), [0, 1, 1, nan, 0], equal_nan=True)
    assert np.array_equal(case_control("a", [1, 1]), [0, 0]) and np.array_equal(case_control("a", [2, 2]), [1, 1])
    for values in ([0, 1, 2], [1.5, 2.0], [-9, 1, 2], [0.1, 0.7]):
        with pytest.raises(LdxError, match="case/control"):
            case_control("a", values)
    with pytest.raises(LdxError, match="no value"):
        case_control("a", [nan, nan])

"""GPU: the Firth logistic association scan (include/ldx.h, "Firth logistic association scan").  ld_glm_logistic(firth="always")
against the numpy mirror (same flags; beta, se within the bounds of each other's oracle) and against the exact oracle
(tests/ld_firth_exact.py) on at most 3 cells a case: the smallest and the largest |z| and the most evaluations; the closed-form
2 x 2 tables, zero cells included; firth="fallback" bit for bit the ML scan where it did not refit and the "always" scan where it
did; bit-identical cells under keep, a SNP subset, one phenotype at a time, an unordered subset of individuals; ldx_glm_firth_dev
driven directly on padded buffers and on a flags array without a 5; the refusals.

Bounds (include/ldx.h): |beta - beta_exact| <= 2^-40 se_exact, |se / se_exact - 1| <= 2^-40, ln p within 2^-30 max(1, |ln p|) of the
exact ln erfc at the device's own z.  Device and mirror each stop within 2^-44 se of the fixed point and then differ by rounding:
the comparison with the mirror allows 2^-39, as the ML scan's does.

Shapes (tests/ld_logistic_exact.py, CASES): 37, 64 and 203 individuals are a partial 64-individual step, exactly one and more than
three, with a partial K-group of 4 in pass A and a partial 16-individual column block in pass B at 37 and 203; 1, 130 and 300 SNPs
are a tail of the four-cell workgroup, a slab tail and more than two slabs; n_cov 0 and 13 are the empty and the full parameter
tile.  5120 individuals (the widest panel) is where the rounding of U* comes closest to the stop constant.
"""
from decimal import Decimal, localcontext

import numpy as np
import pytest

import ld_firth_exact as F
import ld_logistic_exact as X
from ld_tools_amd import FIRTH_STOP, ld_glm_logistic  # noqa: F401  (the feature under test: absent, nothing here can pass)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OUTS = ("beta", "se", "z", "p", "neglog10_p")
ALL = OUTS + ("flags", "n_iter")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


def arrays(res):
    out = {k: getattr(res, k).cpu().numpy() for k in ALL}
    out["firth"] = None if res.firth is None else res.firth.cpu().numpy()
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def same_where(a, b, where):
    """Every word of the seven arrays of two device results is the same on the cells ``where`` (a boolean mask)."""
    a, b = arrays(a), arrays(b)
    for k in OUTS:
        assert same_bits(a[k][where], b[k][where]), k
    for k in ("flags", "n_iter"):
        assert np.array_equal(a[k][where], b[k][where]), k


def same_cells(a, b, rows_a=slice(None), rows_b=slice(None), cols_a=slice(None), cols_b=slice(None)):
    """Every output word of the cells a[rows_a, cols_a] equals that of b[rows_b, cols_b], the firth mark included."""
    a, b = arrays(a), arrays(b)
    for k in OUTS:
        assert same_bits(a[k][rows_a][:, cols_a], b[k][rows_b][:, cols_b]), k
    for k in ("flags", "n_iter", "firth"):
        assert np.array_equal(a[k][rows_a][:, cols_a], b[k][rows_b][:, cols_b]), k


def agree(dev, ref):
    """The device result against the host mirror: the flags and marks, NaN exactly where flagged, beta and se within 2^-39 (se),
    z = beta / se and the tail from it, the evaluations within the cap's half."""
    from ld_tools_amd import _lib, logit_tail_host

    d, r = arrays(dev), arrays(ref)
    assert d["flags"].dtype == np.uint8 and np.array_equal(d["flags"], r["flags"])
    assert d["firth"].dtype == np.uint8 and np.array_equal(d["firth"], r["firth"])
    live = d["flags"] == 0
    for k in OUTS:
        assert np.isnan(d[k][~live]).all() and np.isfinite(d[k][live]).all(), k
    assert (np.abs(d["beta"][live] - r["beta"][live]) <= 2.0 ** -39 * r["se"][live]).all()
    assert (np.abs(d["se"][live] / r["se"][live] - 1.0) <= 2.0 ** -39).all()
    assert same_bits(d["z"][live], d["beta"][live] / d["se"][live])
    p, nlp = logit_tail_host(d["z"][live])
    assert np.allclose(d["p"][live], p, rtol=1e-12, atol=0.0) and np.allclose(d["neglog10_p"][live], nlp, rtol=1e-12, atol=1e-15)
    assert (d["n_iter"][live] <= _lib.FIRTH_MAX_ITER // 2).all() and (d["n_iter"][live] >= 2).all()
    assert (d["n_iter"][(d["flags"] > 0) & (d["flags"] < 5)] == 0).all()
    assert np.array_equal(dev.n_obs, ref.n_obs) and same_bits(dev.a1_freq, ref.a1_freq)


@pytest.fixture(scope="module")
def rare(gpu):
    from ld_tools_amd import PackedPanel

    codes, Y, C = F.rare_panel()
    panel = PackedPanel.from_codes(codes, gpu)
    return codes, Y, C, {mode: ld_glm_logistic(panel, Y, C, firth=mode) for mode in (None, "fallback", "always")}


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_always_against_the_mirror_and_the_oracle(gpu, case):
    from ld_tools_amd import PackedPanel, ld_glm_logistic_host

    n_ind, n_snps, miss, p, n_cov = case
    codes, Y, C = X.case_data(case)
    dev = ld_glm_logistic(PackedPanel.from_codes(codes, gpu), Y, C, firth="always")
    assert dev.beta.is_cuda and tuple(dev.beta.shape) == (n_snps, p) and dev.firth.is_cuda and dev.firth.dtype == torch.uint8
    ref = ld_glm_logistic_host(codes, Y, C, firth="always")
    agree(dev, ref)
    assert (dev.flags <= 4).all()
    cells = F.pick_firth_cells(dev)
    b, s, lp = F.compare_firth(dev, codes, Y, C, cells)
    print(f"{case}: {len(cells)} cells, beta error / bound = {b:.3g}, se = {s:.3g}, ln p = {lp:.3g}, "
          f"mean n_iter = {dev.n_iter.float().mean().item():.2f}, most = {int(dev.n_iter.max())}")
    assert 1 <= len(cells) <= 3
    assert b <= 1.0 and s <= 1.0 and lp <= 1.0


def test_closed_form_tables(gpu):
    """2 x 2 SNPs, n_cov = 0: the Haldane-Anscombe estimate, the zero-cell tables (no maximum-likelihood fit) included; the last
    has 5120 individuals (80 steps of 64), the widest panel there is."""
    from ld_tools_amd import PackedPanel

    for tab in ((30, 11, 8, 25), (7, 5, 0, 9), (12, 0, 0, 9), (2300, 260, 260, 2300)):
        codes, y = X.table_panel(*tab)
        panel = PackedPanel.from_codes(codes, gpu)
        res = arrays(ld_glm_logistic(panel, y, firth="always"))
        beta, se = F.table_firth_exact(*tab)
        assert res["flags"][0, 0] == 0 and res["firth"][0, 0] == 1, tab
        with localcontext(X.CTX):
            eb = abs(Decimal(float(res["beta"][0, 0])) - beta) / (Decimal(2) ** -40 * se)
            es = abs(Decimal(float(res["se"][0, 0])) / se - 1) / Decimal(2) ** -40
        print(f"{tab}: beta error / bound = {float(eb):.3g}, se = {float(es):.3g}, {res['n_iter'][0, 0]} evaluations")
        assert eb <= 1 and es <= 1, tab
        if 0 in tab:
            ml = arrays(ld_glm_logistic(panel, y))
            fb = arrays(ld_glm_logistic(panel, y, firth="fallback"))
            assert ml["flags"][0, 0] == 5 and fb["flags"][0, 0] == 0 and fb["firth"][0, 0] == 1
            assert all(same_bits(fb[k], res[k]) for k in OUTS) and fb["n_iter"][0, 0] == res["n_iter"][0, 0]


def test_fallback_is_the_ml_scan_or_the_always_scan_bit_for_bit(gpu, rare):
    from ld_tools_amd import PackedPanel, ld_glm_logistic_host

    codes, Y, C, res = rare
    ml, fb, al = res[None], res["fallback"], res["always"]
    mark = fb.firth.cpu().numpy() == 1
    lost = ml.flags.cpu().numpy() == 5
    assert ml.firth is None and np.array_equal(mark, lost) and lost.sum() >= 10 and lost[1::2, 0].all()
    same_where(fb, ml, ~mark)
    same_where(fb, al, mark)
    assert not (fb.flags == 5).any() and not (al.flags == 5).any()
    agree(fb, ld_glm_logistic_host(codes, Y, C, firth="fallback"))
    cells = [tuple(int(v) for v in c) for c in np.argwhere(mark)[:2]]
    b, s, lp = F.compare_firth(fb, codes, Y, C, cells)
    print(f"rare panel: {lost.sum()} cells refitted, beta error / bound = {b:.3g}, se = {s:.3g}")
    assert b <= 1.0 and s <= 1.0 and lp <= 1.0
    # the flag panel: the separated cell is refitted, every other cell keeps the ML scan's bits
    codes, keep, Y, covar = X.flag_panel()
    panel = PackedPanel.from_codes(codes, gpu)
    ml, fb, al = (ld_glm_logistic(panel, Y, covar, keep=keep, firth=mode) for mode in (None, "fallback", "always"))
    mark = np.zeros((6, 2), dtype=bool)
    mark[4, 0] = True
    want = X.FLAG_PANEL_WANT.copy()
    want[4, 0] = 0
    assert np.array_equal(fb.firth.cpu().numpy() == 1, mark) and np.array_equal(fb.flags.cpu().numpy(), want)
    assert np.array_equal(al.flags.cpu().numpy(), want) and np.array_equal(al.firth.cpu().numpy() == 1, want == 0)
    same_where(fb, ml, ~mark)
    same_where(fb, al, mark)
    agree(fb, ld_glm_logistic_host(codes, Y, covar, keep=keep, firth="fallback"))
    b, s, lp = F.compare_firth(fb, codes, Y, covar, [(4, 0)], keep)
    assert b <= 1.0 and s <= 1.0 and lp <= 1.0


def test_singletons_take_the_step_length_safeguard(gpu):
    """One carrier per variant: the cells whose plain scoring step overshoots and is halved (tests/ld_firth_exact.py,
    singleton_panel).  The maximum-likelihood scan loses every one of them; both Firth modes fit them, with the mirror's flags."""
    from ld_tools_amd import PackedPanel, ld_glm_logistic_host

    codes, Y, C = F.singleton_panel()
    panel = PackedPanel.from_codes(codes, gpu)
    ml, fb, al = (ld_glm_logistic(panel, Y, C, firth=mode) for mode in (None, "fallback", "always"))
    assert (ml.flags == 5).all() and (fb.flags == 0).all() and (fb.firth == 1).all()
    same_cells(fb, al)
    agree(fb, ld_glm_logistic_host(codes, Y, C, firth="fallback"))
    b, s, lp = F.compare_firth(fb, codes, Y, C, F.pick_firth_cells(fb))
    print(f"singletons: beta error / bound = {b:.3g}, se = {s:.3g}, evaluations {int(fb.n_iter.min())} - {int(fb.n_iter.max())}")
    assert b <= 1.0 and s <= 1.0 and lp <= 1.0


def test_cells_do_not_depend_on_the_call(gpu, rare):
    """The same bits for a cell whatever else the call holds: a keep mask, a SNP subset of the panel, the phenotypes one at a
    time, a second run -- under "always" and, on the rare panel, under "fallback"."""
    from ld_tools_amd import PackedPanel

    case = (203, 300, 0.05, 3, 3)
    codes, Y, C = X.case_data(case)
    panel = PackedPanel.from_codes(codes, gpu)
    full = ld_glm_logistic(panel, Y, C, firth="always")
    same_cells(full, ld_glm_logistic(panel, Y, C, firth="always"))
    keep = np.arange(300) % 3 != 1
    masked = ld_glm_logistic(panel, Y, C, keep=keep, firth="always")
    same_cells(full, masked, keep, keep)
    assert (masked.flags.cpu().numpy()[~keep] == 1).all() and (masked.firth.cpu().numpy()[~keep] == 0).all()
    snps = np.array([299, 0, 130, 5, 127, 128, 64])
    same_cells(full, ld_glm_logistic(panel.select(snps=snps), Y, C, firth="always"), snps)
    for j in range(3):
        same_cells(full, ld_glm_logistic(panel, Y[:, j], C, firth="always"), cols_a=[j])
    codes, Y, C, res = rare
    panel = PackedPanel.from_codes(codes, gpu)
    snps = np.array([39, 1, 0, 17, 22])
    same_cells(res["fallback"], ld_glm_logistic(panel.select(snps=snps), Y, C, firth="fallback"), snps)
    same_cells(res["fallback"], ld_glm_logistic(panel, Y[:, 0], C, firth="fallback"), cols_a=[0])
    keep = np.arange(40) % 4 != 2
    same_cells(res["fallback"], ld_glm_logistic(panel, Y, C, keep=keep, firth="fallback"), keep, keep)


def test_individuals_unordered_subset(gpu):
    from ld_tools_amd import PackedPanel, ld_glm_logistic_host

    codes = X.logit_codes(64, 130, seed=21, miss=0.05)
    rows = np.random.default_rng(5).permutation(64)[:41]
    cols = np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1)
    sub = np.ascontiguousarray(codes[:, cols])
    Y, C = X.logit_traits(sub, 2, 2, seed=6)
    keep = np.arange(130) % 4 != 1
    for mode in ("always", "fallback"):
        dev = ld_glm_logistic(PackedPanel.from_codes(codes, gpu), Y, C, individuals=rows, keep=keep, firth=mode)
        agree(dev, ld_glm_logistic_host(codes, Y, C, individuals=rows, keep=keep, firth=mode))
        same_cells(dev, ld_glm_logistic(PackedPanel.from_codes(sub, gpu), Y, C, keep=keep, firth=mode))


def _entry_buffers(gpu, case=(203, 130, 0.05, 2, 13)):
    from ld_tools_amd import PackedPanel, geno_snp_counts, logit_design

    codes, Y, C = X.case_data(case)
    n_ind, n_snps, _, p, n_cov = case
    panel = PackedPanel.from_codes(codes, gpu)
    des = logit_design(Y, C)
    ld_design, ld_out = n_ind + 5, p + 3
    basis = np.full((n_cov + 1, ld_design), 1e300)
    basis[:, :n_ind] = des.basis
    y8 = np.full((p, ld_design), 0xCD, dtype=np.uint8)
    y8[:, :n_ind] = des.y
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    bd, yd, td = dev(basis), dev(y8), dev(des.theta0)
    counts = geno_snp_counts(panel)
    head = (panel.alt.data_ptr(), panel.ref.data_ptr(), n_snps, panel.n_hap, None, counts.data_ptr(), bd.data_ptr(), ld_design,
            n_cov, yd.data_ptr(), td.data_ptr(), p, 50.0)
    keepalive = (panel, bd, yd, td, counts)
    return panel, Y, C, head, ld_out, p, n_snps, (basis, y8, bd, yd), keepalive


def test_entry_on_padded_buffers(gpu):
    """ldx_glm_firth_dev itself, mode 0: ld_design > n_ind, ld_out > n_pheno; the padding words of the eight outputs keep their
    marks, the inputs are unchanged, and the cells are those of ld_glm_logistic(firth="always")."""
    from ld_tools_amd import _lib

    panel, Y, C, head, ld_out, p, n_snps, (basis, y8, bd, yd), _alive = _entry_buffers(gpu)
    want = arrays(ld_glm_logistic(panel, Y, C, firth="always"))
    outs = [torch.full((n_snps, ld_out), 7.25, dtype=torch.float64, device=gpu) for _ in range(5)]
    flags, n_iter, mark = (torch.full((n_snps, ld_out), 0xAB, dtype=torch.uint8, device=gpu) for _ in range(3))
    rc = _lib.lib.ldx_glm_firth_dev(*head, *(o.data_ptr() for o in outs), flags.data_ptr(), n_iter.data_ptr(), ld_out, 0,
                                    mark.data_ptr(), None)
    assert rc == 0, _lib.lib.ldx_last_error()
    torch.cuda.synchronize()
    for got, name in zip(outs, OUTS):
        g = got.cpu().numpy()
        assert same_bits(g[:, :p], want[name]), name
        assert (g[:, p:] == 7.25).all(), name
    for got, name in ((flags, "flags"), (n_iter, "n_iter"), (mark, "firth")):
        g = got.cpu().numpy()
        assert np.array_equal(g[:, :p], want[name]) and (g[:, p:] == 0xAB).all(), name
    assert np.array_equal(bd.cpu().numpy(), basis) and np.array_equal(yd.cpu().numpy(), y8)


def test_mode_1_without_a_flag_5_touches_nothing_but_the_marks(gpu):
    """Mode 1 on a flags array that holds no 5 (and values no scan writes): firth = 0 in every cell, the padding of firth and every
    byte of the seven other arrays as they were."""
    from ld_tools_amd import _lib

    _panel, _Y, _C, head, ld_out, p, n_snps, _inputs, _alive = _entry_buffers(gpu)
    outs = [torch.full((n_snps, ld_out), 7.25 + k, dtype=torch.float64, device=gpu) for k in range(5)]
    flags0 = (np.arange(n_snps * ld_out).reshape(n_snps, ld_out) % 5).astype(np.uint8)      # 0 .. 4: never a 5
    flags0[::7] = 6
    flags = torch.from_numpy(flags0).to(gpu)
    n_iter, mark = (torch.full((n_snps, ld_out), 0xAB, dtype=torch.uint8, device=gpu) for _ in range(2))
    rc = _lib.lib.ldx_glm_firth_dev(*head, *(o.data_ptr() for o in outs), flags.data_ptr(), n_iter.data_ptr(), ld_out, 1,
                                    mark.data_ptr(), None)
    assert rc == 0, _lib.lib.ldx_last_error()
    torch.cuda.synchronize()
    for k, got in enumerate(outs):
        assert (got.cpu().numpy() == 7.25 + k).all()
    assert np.array_equal(flags.cpu().numpy(), flags0) and (n_iter.cpu().numpy() == 0xAB).all()
    m = mark.cpu().numpy()
    assert (m[:, :p] == 0).all() and (m[:, p:] == 0xAB).all()


def test_refusals(gpu):
    from ld_tools_amd import LdxError, PackedPanel, _lib

    codes = X.logit_codes(20, 4, seed=1)
    panel = PackedPanel.from_codes(codes, gpu)
    rng = np.random.default_rng(0)
    Y = (rng.random((20, 2)) < 0.5).astype(np.uint8)
    with pytest.raises(LdxError, match="firth must be"):
        ld_glm_logistic(panel, Y, firth="yes")
    with pytest.raises(LdxError, match="firth must be"):
        ld_glm_logistic(panel, Y, firth=True)
    with pytest.raises(LdxError, match="complete-case"):
        ld_glm_logistic(panel, Y, missing="pairwise", firth="fallback")
    with pytest.raises(LdxError, match="max_vif"):
        ld_glm_logistic(panel, Y, max_vif=1.0, firth="always")
    with pytest.raises(LdxError, match="LDX_LOGIT_MAX_COV"):
        ld_glm_logistic(panel, Y, rng.standard_normal((20, 14)), firth="always")
    # the C entry, with device buffers that would serve a good call: each call breaks one rule
    t = torch.zeros(64, dtype=torch.float64, device=gpu)
    q = t.data_ptr()
    good = [panel.alt.data_ptr(), panel.ref.data_ptr(), 4, 40, None, q, q, 20, 1, q, q, 1, 50.0, q, q, q, q, q, q, q, 1, 0, q, None]
    for at, value in ((21, 2), (22, None), (0, None), (5, None), (3, 39), (8, 14), (7, 19), (20, 0), (3, 6), (12, 1.0), (11, 0)):
        args = list(good)
        args[at] = value
        assert _lib.lib.ldx_glm_firth_dev(*args) == -1, (at, value)
        assert b"ldx_glm_firth_dev" in _lib.lib.ldx_last_error()

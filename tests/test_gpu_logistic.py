"""GPU: the logistic association scan (include/ldx.h, "logistic association scan").  ld_glm_logistic against the numpy mirror
ld_glm_logistic_host (same flags; beta, se within the bounds below of each other's oracle) and against the exact oracle
(tests/ld_logistic_exact.py) on at most 8 cells a case, the smallest and largest |z| among them; the closed-form 2 x 2 SNP; the five
flags; bit-identical cells under keep, a SNP subset, one phenotype at a time and a second run; an unordered subset of individuals;
ldx_glm_logistic_dev driven directly on padded buffers; the refusals.

Bounds (include/ldx.h): |beta - beta_exact| <= 2^-40 se_exact, |se / se_exact - 1| <= 2^-40, ln p within 2^-30 max(1, |ln p|) of the
exact ln erfc at the device's own z; at most 12 information evaluations.  The numpy mirror's own error is 2^-50.6 se and 2^-52.1
(tests/test_logistic_host.py), so device and mirror may differ by twice the bound at most -- the comparison with the mirror
allows 2^-39.

Shapes (tests/ld_logistic_exact.py, CASES): 37 and 203 individuals leave a partial 64-individual step and a partial K-group of 4, 64
is exactly one step, 203 more than three; 1, 130 and 300 SNPs are a tail of the four-cell workgroup, a slab tail and more than two
slabs; n_cov 0 and 13 are the empty and the full parameter tile.
"""
import numpy as np
import pytest

import ld_logistic_exact as X
from ld_tools_amd import ld_glm_logistic  # noqa: F401  (the feature under test: absent, nothing here can pass)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OUTS = ("beta", "se", "z", "p", "neglog10_p")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


def arrays(res):
    return {k: getattr(res, k).cpu().numpy() for k in OUTS + ("flags", "n_iter")}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def same_cells(a, b, rows_a=slice(None), rows_b=slice(None), cols_a=slice(None), cols_b=slice(None)):
    """Every output word of the cells a[rows_a, cols_a] equals that of b[rows_b, cols_b]."""
    a, b = arrays(a), arrays(b)
    for k in OUTS:
        assert same_bits(a[k][rows_a][:, cols_a], b[k][rows_b][:, cols_b]), k
    for k in ("flags", "n_iter"):
        assert np.array_equal(a[k][rows_a][:, cols_a], b[k][rows_b][:, cols_b]), k


def agree(dev, ref):
    """The device result against the host mirror: the flags, NaN exactly where flagged, beta and se within 2^-39 (se), z = beta / se
    and the tail from it, n_obs, a1_freq, at most 12 evaluations."""
    d, r = arrays(dev), arrays(ref)
    assert d["flags"].dtype == np.uint8 and np.array_equal(d["flags"], r["flags"])
    live = d["flags"] == 0
    for k in OUTS:
        assert np.isnan(d[k][~live]).all() and np.isfinite(d[k][live]).all(), k
    assert (np.abs(d["beta"][live] - r["beta"][live]) <= 2.0 ** -39 * r["se"][live]).all()
    assert (np.abs(d["se"][live] / r["se"][live] - 1.0) <= 2.0 ** -39).all()
    assert same_bits(d["z"][live], d["beta"][live] / d["se"][live])
    p, nlp = __import__("ld_tools_amd").logit_tail_host(d["z"][live])
    assert np.allclose(d["p"][live], p, rtol=1e-12, atol=0.0) and np.allclose(d["neglog10_p"][live], nlp, rtol=1e-12, atol=1e-15)
    assert (d["n_iter"][live] <= 12).all() and (d["n_iter"][live] >= 2).all() and (d["n_iter"][(d["flags"] > 0) & (d["flags"] < 5)] == 0).all()
    assert np.array_equal(dev.n_obs, ref.n_obs) and same_bits(dev.a1_freq, ref.a1_freq)
    assert np.array_equal(dev.design.theta0, ref.design.theta0, equal_nan=True)


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_scan_against_the_mirror_and_the_oracle(gpu, case):
    from ld_tools_amd import PackedPanel, ld_glm_logistic_host

    n_ind, n_snps, miss, p, n_cov = case
    codes, Y, C = X.case_data(case)
    dev = ld_glm_logistic(PackedPanel.from_codes(codes, gpu), Y, C)
    assert dev.beta.is_cuda and tuple(dev.beta.shape) == (n_snps, p) and dev.flags.dtype == torch.uint8
    ref = ld_glm_logistic_host(codes, Y, C)
    agree(dev, ref)
    assert (ref.flags.numpy() == 5).sum() <= 0.02 * n_snps * p
    cells = X.pick_cells(dev, 8)
    b, s, lp, eta = X.compare(dev, codes, Y, C, cells)
    print(f"{case}: {len(cells)} cells, beta error / bound = {b:.3g}, se = {s:.3g}, ln p = {lp:.3g}, max |eta| = {eta:.3g}, "
          f"mean n_iter = {dev.n_iter.float().mean().item():.2f}")
    assert 1 <= len(cells) <= 8 and eta <= X.MAX_ETA
    assert b <= 1.0 and s <= 1.0 and lp <= 1.0


def test_closed_form_table_and_a_tail_below_the_float_range(gpu):
    """Two 2 x 2 SNPs, n_cov = 0: beta^ = ln(a d / (b c)), se = sqrt(1/a + 1/b + 1/c + 1/d).  The second has 5120 individuals (80
    steps of 64) and |z| > 40: p underflows, neglog10_p stays finite and follows ln erfc."""
    from decimal import Decimal, localcontext

    from ld_tools_amd import PackedPanel

    for tab, big in (((30, 11, 8, 25), False), ((2300, 260, 260, 2300), True)):
        codes, y = X.table_panel(*tab)
        res = arrays(ld_glm_logistic(PackedPanel.from_codes(codes, gpu), y))
        beta, se = X.table_exact(*tab)
        assert res["flags"][0, 0] == 0 and res["n_iter"][0, 0] <= 12
        with localcontext(X.CTX):
            assert abs(Decimal(float(res["beta"][0, 0])) - beta) <= Decimal(2) ** -40 * se
            assert abs(Decimal(float(res["se"][0, 0])) / se - 1) <= Decimal(2) ** -40
        z, nlp, p = float(res["z"][0, 0]), float(res["neglog10_p"][0, 0]), float(res["p"][0, 0])
        with localcontext(X.WIDE):
            lnp = X.ln_p_exact(z)
            assert abs(Decimal(nlp) * -Decimal(10).ln() - lnp) <= Decimal(2) ** -30 * max(Decimal(1), abs(lnp))
        if big:
            assert abs(z) > 40.0 and p == 0.0 and np.isfinite(nlp) and nlp > 300.0
            print("2 x 2 with 5120 individuals: z =", z, " -log10 p =", nlp)


def test_flags_each_on_purpose(gpu):
    from ld_tools_amd import PackedPanel, ld_glm_logistic_host

    codes, keep, Y, covar = X.flag_panel()
    dev = ld_glm_logistic(PackedPanel.from_codes(codes, gpu), Y, covar, keep=keep)
    X.check_flag_panel(dev)
    agree(dev, ld_glm_logistic_host(codes, Y, covar, keep=keep))


def test_cells_do_not_depend_on_the_call(gpu):
    """The same bits for a cell whatever else the call holds: a keep mask, a SNP subset of the panel, the phenotypes one at a
    time, a second run."""
    from ld_tools_amd import PackedPanel

    case = (203, 300, 0.05, 3, 3)
    codes, Y, C = X.case_data(case)
    panel = PackedPanel.from_codes(codes, gpu)
    full = ld_glm_logistic(panel, Y, C)
    same_cells(full, ld_glm_logistic(panel, Y, C))
    keep = np.arange(300) % 3 != 1
    masked = ld_glm_logistic(panel, Y, C, keep=keep)
    same_cells(full, masked, keep, keep)
    assert (masked.flags.cpu().numpy()[~keep] == 1).all() and np.isnan(masked.beta.cpu().numpy()[~keep]).all()
    snps = np.array([299, 0, 130, 5, 127, 128, 64])
    same_cells(full, ld_glm_logistic(panel.select(snps=snps), Y, C), snps)
    for j in range(3):
        same_cells(full, ld_glm_logistic(panel, Y[:, j], C), cols_a=[j])


def test_individuals_unordered_subset(gpu):
    from ld_tools_amd import PackedPanel, ld_glm_logistic_host

    codes = X.logit_codes(64, 130, seed=21, miss=0.05)
    rows = np.random.default_rng(5).permutation(64)[:41]
    cols = np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1)
    sub = np.ascontiguousarray(codes[:, cols])
    Y, C = X.logit_traits(sub, 2, 2, seed=6)
    keep = np.arange(130) % 4 != 1
    dev = ld_glm_logistic(PackedPanel.from_codes(codes, gpu), Y, C, individuals=rows, keep=keep)
    agree(dev, ld_glm_logistic_host(sub, Y, C, keep=keep))
    agree(dev, ld_glm_logistic_host(codes, Y, C, individuals=rows, keep=keep))
    same_cells(dev, ld_glm_logistic(PackedPanel.from_codes(sub, gpu), Y, C, keep=keep))


def test_entry_on_padded_buffers(gpu):
    """ldx_glm_logistic_dev itself: ld_design > n_ind, ld_out > n_pheno; the padding words of the seven outputs keep their marks,
    the inputs are unchanged, and the cells are those of ld_glm_logistic."""
    from ld_tools_amd import PackedPanel, _lib, geno_snp_counts, logit_design

    case = (203, 130, 0.05, 2, 13)
    codes, Y, C = X.case_data(case)
    n_ind, n_snps, _, p, n_cov = case
    panel = PackedPanel.from_codes(codes, gpu)
    want = arrays(ld_glm_logistic(panel, Y, C))
    des = logit_design(Y, C)
    ld_design, ld_out = n_ind + 5, p + 3
    basis = np.full((n_cov + 1, ld_design), 1e300)
    basis[:, :n_ind] = des.basis
    y8 = np.full((p, ld_design), 0xCD, dtype=np.uint8)
    y8[:, :n_ind] = des.y
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    bd, yd, td = dev(basis), dev(y8), dev(des.theta0)
    counts = geno_snp_counts(panel)
    outs = [torch.full((n_snps, ld_out), 7.25, dtype=torch.float64, device=gpu) for _ in range(5)]
    flags, n_iter = (torch.full((n_snps, ld_out), 0xAB, dtype=torch.uint8, device=gpu) for _ in range(2))
    rc = _lib.lib.ldx_glm_logistic_dev(panel.alt.data_ptr(), panel.ref.data_ptr(), n_snps, panel.n_hap, None, counts.data_ptr(),
                                       bd.data_ptr(), ld_design, n_cov, yd.data_ptr(), td.data_ptr(), p, 50.0,
                                       *(o.data_ptr() for o in outs), flags.data_ptr(), n_iter.data_ptr(), ld_out, None)
    assert rc == 0, _lib.lib.ldx_last_error()
    torch.cuda.synchronize()
    for got, name in zip(outs, OUTS):
        g = got.cpu().numpy()
        assert same_bits(g[:, :p], want[name]), name
        assert (g[:, p:] == 7.25).all(), name
    for got, name in ((flags, "flags"), (n_iter, "n_iter")):
        g = got.cpu().numpy()
        assert np.array_equal(g[:, :p], want[name]) and (g[:, p:] == 0xAB).all(), name
    assert np.array_equal(bd.cpu().numpy(), basis) and np.array_equal(yd.cpu().numpy(), y8)


def test_refusals(gpu):
    from ld_tools_amd import LdxError, PackedPanel, _lib

    codes = X.logit_codes(20, 4, seed=1)
    panel = PackedPanel.from_codes(codes, gpu)
    rng = np.random.default_rng(0)
    Y = (rng.random((20, 2)) < 0.5).astype(np.uint8)
    with pytest.raises(LdxError, match="complete-case"):
        ld_glm_logistic(panel, Y, missing="pairwise")
    with pytest.raises(LdxError, match="max_vif"):
        ld_glm_logistic(panel, Y, max_vif=1.0)
    with pytest.raises(LdxError, match="20"):
        ld_glm_logistic(panel, Y[:10])
    with pytest.raises(LdxError, match="0 .control. and 1"):
        ld_glm_logistic(panel, Y + 1)
    with pytest.raises(LdxError, match="LDX_LOGIT_MAX_COV"):
        ld_glm_logistic(panel, Y, rng.standard_normal((20, 14)))
    with pytest.raises(LdxError, match="n_hap must be even"):
        ld_glm_logistic(PackedPanel.from_codes(codes[:, :39], gpu), Y)
    # the C entry, with device buffers that would serve a good call: each call breaks one rule
    t = torch.zeros(64, dtype=torch.float64, device=gpu)
    q = t.data_ptr()
    good = [panel.alt.data_ptr(), panel.ref.data_ptr(), 4, 40, None, q, q, 20, 1, q, q, 1, 50.0, q, q, q, q, q, q, q, 1, None]
    for at, value in ((0, None), (5, None), (3, 39), (8, 14), (7, 19), (20, 0), (3, 6), (12, 1.0), (11, 0)):
        args = list(good)
        args[at] = value
        assert _lib.lib.ldx_glm_logistic_dev(*args) == -1, (at, value)
        assert b"ldx_glm_logistic_dev" in _lib.lib.ldx_last_error()

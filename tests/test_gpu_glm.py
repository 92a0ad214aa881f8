"""GPU: the association scan (include/ldx.h, "association scan").  geno_snp_counts against counts made from the codes; ld_glm
against ld_glm_host bit for bit on beta, se, t, the flags, n_obs and a1_freq, and its ln p against the exact oracle
(tests/ld_glm_exact.py) within 2^-30 max(1, |ln p|); ldx_glm_linear_dev driven directly on padded buffers.  Shapes: 37, 64 and
200 individuals are a partial 64-individual vector, exactly one, and more than a 128-individual K-block; 1, 130 and 300 SNPs a slab
tail and more than two slabs (and more than two 128-SNP workgroups of the statistics kernel); k = 36 crosses the reverse product's
32-column group, k = 64 fills it.  No cell may carry flag 6."""
import numpy as np
import pytest

import ld_glm_exact as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_IND = (37, 64, 200)
N_SNPS = (1, 130, 300)
# (n_ind, n_snps, missing rate, phenotypes, n_cov): every (n_ind, n_snps) pair once
CASES = ((37, 300, 0.05, 1, 1), (64, 130, 0.0, 1, 1), (200, 1, 0.05, 1, 1),
         (37, 130, 0.0, 3, 3), (200, 300, 0.05, 3, 3), (64, 300, 0.05, 3, 3),
         (200, 130, 0.05, 25, 11), (37, 1, 0.0, 25, 11),
         (64, 1, 0.05, 40, 24), (37, 130, 0.05, 40, 24))
ORACLE_CELLS = 120     # ln p is compared on at most this many cells of a case, the smallest and the largest p among them


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def agree(dev, ref):
    """The device result against the host mirror: bits of beta, se, t; the flags; n_obs; a1_freq; no flag 6."""
    for name in ("beta", "se", "t"):
        assert same_bits(getattr(dev, name).cpu().numpy(), getattr(ref, name).numpy()), name
    flags = dev.flags.cpu().numpy()
    assert flags.dtype == np.uint8 and np.array_equal(flags, ref.flags.numpy()) and (flags != 6).all()
    assert np.array_equal(dev.n_obs, ref.n_obs) and same_bits(dev.a1_freq, ref.a1_freq) and dev.df == ref.df
    assert np.array_equal(dev.design.q, ref.design.q) and np.array_equal(dev.design.exps, ref.design.exps)
    live = flags == 0
    assert np.allclose(dev.p.cpu().numpy()[live], ref.p.numpy()[live], rtol=1e-9, atol=0.0)
    assert np.array_equal(np.isnan(dev.p.cpu().numpy()), np.isnan(ref.p.numpy()))


@pytest.mark.parametrize("miss", (0.0, 0.05))
@pytest.mark.parametrize("n_ind", N_IND)
def test_snp_counts_against_the_codes(gpu, n_ind, miss):
    from ld_tools_amd import PackedPanel, geno_counts_host, geno_snp_counts

    for n_snps in N_SNPS:
        codes = X.glm_codes(n_ind, n_snps, seed=100 * n_ind + n_snps, miss=miss)
        panel = PackedPanel.from_codes(codes, gpu)
        keep = np.random.default_rng(n_snps).random(n_snps) < 0.7
        for k in (None, keep):
            got = geno_snp_counts(panel, keep=k).cpu().numpy()
            want = X.counts_exact(codes, k)
            assert got.shape == (n_snps, 4) and np.array_equal(got, want), (n_snps, k is None)
            assert np.array_equal(geno_counts_host(codes, k), want)
        assert not got[~keep].any()


def test_snp_counts_agree_with_the_reverse_product(gpu):
    from ld_tools_amd import GenoOperator, PackedPanel, geno_snp_counts

    codes = X.glm_codes(200, 300, seed=9, miss=0.05)
    panel = PackedPanel.from_codes(codes, gpu)
    n, a = (t.cpu().numpy() for t in GenoOperator(panel).stats())
    c = geno_snp_counts(panel).cpu().numpy().astype(np.int64)
    assert np.array_equal(c[:, 0], n) and np.array_equal(c[:, 1] + 2 * c[:, 2], a) and not c[:, 3].any()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_scan_against_the_mirror_and_the_oracle(gpu, case):
    from ld_tools_amd import PackedPanel, ld_glm, ld_glm_host

    n_ind, n_snps, miss, p, n_cov = case
    codes = X.glm_codes(n_ind, n_snps, seed=n_ind + n_snps + p, miss=miss)
    Y, C = X.glm_traits(codes, p, n_cov, seed=n_snps + n_cov)
    dev = ld_glm(PackedPanel.from_codes(codes, gpu), Y, C)
    assert dev.beta.is_cuda and tuple(dev.beta.shape) == (n_snps, p) and dev.df == n_ind - n_cov - 1
    agree(dev, ld_glm_host(codes, Y, C))
    n, worst = X.ln_p_check(dev, codes, n_cov, limit=ORACLE_CELLS)
    print(f"{case}: ln p on {n} cells, largest error / bound = {worst:.3g}")
    assert n >= 1 and worst <= 1.0


def test_individuals_unordered_subset_and_keep(gpu):
    from ld_tools_amd import PackedPanel, ld_glm, ld_glm_host

    codes = X.glm_codes(64, 130, seed=21, miss=0.05)
    rows = np.random.default_rng(5).permutation(64)[:41]
    cols = np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1)
    sub = np.ascontiguousarray(codes[:, cols])
    Y, C = X.glm_traits(sub, 3, 3, seed=6)
    keep = np.arange(130) % 4 != 1
    dev = ld_glm(PackedPanel.from_codes(codes, gpu), Y, C, individuals=rows, keep=keep)
    agree(dev, ld_glm_host(codes, Y, C, individuals=rows, keep=keep))
    agree(dev, ld_glm_host(sub, Y, C, keep=keep))
    assert (dev.flags.cpu().numpy()[~keep] == 1).all() and dev.df == 41 - 3 - 1
    assert X.ln_p_check(dev, sub, 3, limit=ORACLE_CELLS, keep=keep)[1] <= 1.0


def test_planted_effect_below_the_float_range(gpu):
    from ld_tools_amd import PackedPanel, ld_glm, ld_glm_host

    codes = X.glm_codes(200, 5, seed=5)
    g, _ = X.planes(codes)
    Y = g[2] + 0.01 * np.random.default_rng(1).standard_normal(200)
    dev = ld_glm(PackedPanel.from_codes(codes, gpu), Y)
    agree(dev, ld_glm_host(codes, Y))
    p, nlp = dev.p.cpu().numpy()[2, 0], dev.neglog10_p.cpu().numpy()[2, 0]
    assert 0.0 <= p < 2.2250738585072014e-308 and np.isfinite(nlp) and 300.0 < nlp < 1000.0        # 0 or subnormal
    n, worst = X.ln_p_check(dev, codes, 1, cells=[(i, 0) for i in range(5)])
    print("planted: -log10 p =", nlp, " largest ln p error / bound =", worst)
    assert worst <= 1.0


def test_one_degree_of_freedom(gpu):
    from ld_tools_amd import PackedPanel, ld_glm, ld_glm_host

    codes = X.glm_codes(5, 130, seed=31)
    Y, C = X.glm_traits(codes, 2, 3, seed=32)
    dev = ld_glm(PackedPanel.from_codes(codes, gpu), Y, C)
    assert dev.df == 1
    agree(dev, ld_glm_host(codes, Y, C))
    flags = dev.flags.cpu().numpy()
    assert (flags == 0).sum() >= 20                      # (5 individuals leave many constant genotypes: flags 2 and 3)
    assert X.ln_p_check(dev, codes, 3, limit=ORACLE_CELLS)[1] <= 1.0


def test_flags_each_on_purpose(gpu):
    from ld_tools_amd import PackedPanel, ld_glm, ld_glm_host

    codes, keep, Y, _ = X.flag_panel()
    g, _ = X.planes(codes)
    panel = PackedPanel.from_codes(codes, gpu)
    dev, dev3 = ld_glm(panel, Y, keep=keep), ld_glm(panel, Y[:, 0], covar=g[3].astype(np.float64), keep=keep)
    X.check_flag_panel(dev, dev3)
    agree(dev, ld_glm_host(codes, Y, keep=keep))
    agree(dev3, ld_glm_host(codes, Y[:, 0], covar=g[3].astype(np.float64), keep=keep))


def test_refusals(gpu):
    from ld_tools_amd import LdxError, PackedPanel, ld_glm

    codes = X.glm_codes(20, 4, seed=1)
    panel = PackedPanel.from_codes(codes, gpu)
    Y = np.random.default_rng(0).standard_normal((20, 2))
    with pytest.raises(LdxError, match="complete-case"):
        ld_glm(panel, Y, missing="pairwise")
    with pytest.raises(LdxError, match="max_vif"):
        ld_glm(panel, Y, max_vif=1.0)
    with pytest.raises(LdxError, match="20"):
        ld_glm(panel, Y[:10])


def test_statistics_kernel_on_padded_buffers(gpu):
    """ldx_glm_linear_dev on hand-built z, zc, counts: 300 SNPs (rows in the second and third workgroup), ld_z > k, ld_out > p;
    the padding words of the seven buffers keep their marks."""
    from ld_tools_amd import _lib, geno_counts_host, geno_rmatmul_host, glm_design, glm_linear_host

    n_ind, n_snps, p, n_cov, ld_z, ld_out = 64, 300, 5, 4, 12, 7
    codes = X.glm_codes(n_ind, n_snps, seed=77, miss=0.05)
    codes[150] = 2                                                      # a row without a call in the second workgroup
    Y, C = X.glm_traits(codes, p, n_cov, seed=78)
    des = glm_design(Y, C)
    k = n_cov + p
    z, zc = geno_rmatmul_host(codes, des.q)
    counts = geno_counts_host(codes)
    want = glm_linear_host(z, zc, counts, des.exps, des.yy, n_ind, n_cov, 50.0)
    mark = -(1 << 40)
    zp, zcp = (np.full((n_snps, ld_z), mark, dtype=np.int64) for _ in range(2))
    zp[:, :k], zcp[:, :k] = z, zc
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    zd, zcd, cd, ed, yd = dev(zp), dev(zcp), dev(counts.astype(np.int32)), dev(des.exps), dev(des.yy)
    outs = [torch.full((n_snps, ld_out), 7.25, dtype=torch.float64, device=gpu) for _ in range(5)]
    flags = torch.full((n_snps, ld_out), 0xAB, dtype=torch.uint8, device=gpu)
    rc = _lib.lib.ldx_glm_linear_dev(zd.data_ptr(), zcd.data_ptr(), ld_z, cd.data_ptr(), n_snps, n_ind, n_cov, p, ed.data_ptr(),
                                     yd.data_ptr(), 50.0, *(o.data_ptr() for o in outs), flags.data_ptr(), ld_out, None)
    assert rc == 0, _lib.lib.ldx_last_error()
    torch.cuda.synchronize()
    for got, ref, name in zip(outs, want[:3], ("beta", "se", "t")):
        assert same_bits(got.cpu().numpy()[:, :p], ref), name
    for got, ref in zip(outs[3:], want[3:5]):
        g = got.cpu().numpy()[:, :p]
        assert np.array_equal(np.isnan(g), np.isnan(ref)) and np.allclose(g[~np.isnan(g)], ref[~np.isnan(ref)], rtol=1e-9, atol=0.0)
    f = flags.cpu().numpy()
    assert np.array_equal(f[:, :p], want[5]) and (f[150, :p] == 1).all() and (f[:, :p] != 6).all()
    assert (f[:, p:] == 0xAB).all() and all((o.cpu().numpy()[:, p:] == 7.25).all() for o in outs)
    assert (zd.cpu().numpy()[:, k:] == mark).all() and (zcd.cpu().numpy()[:, k:] == mark).all()

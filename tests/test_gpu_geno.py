"""GPU: the genotype products (include/ldx.h, "genotype products") against the numpy mirrors, array_equal on int64 throughout:
shapes across an accumulator tile, a slab, a K-block and a store; every column-tile count; forced K slices; digit extremes up to
one full slice; masks, accumulation, invariances, adjointness and the per-SNP statistics."""
import numpy as np
import pytest

from ld_geno_exact import Q_MAX, panel_codes, random_weights

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_IND = (1, 3, 64, 129, 257)
N_SNPS = (1, 64, 129, 256, 257, 1000)
HOLES = ("none", "3%", "single")      # 257 individuals with the single hole: slabs with and without a missing call in one launch
COLS = (1, 8, 9, 64)                  # one limb tile partly and wholly used, two tiles, two column groups
N_SLICES = (None, 1, 2, 3, 7)
EXTREMES = (0x3F7F7F7F, -0x3F808080, Q_MAX, -Q_MAX)   # digits 127 127 127 63; -128 -128 -128 -63; 0 0 0 64; 0 0 0 -64


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("holes", HOLES)
@pytest.mark.parametrize("n_ind", N_IND)
def test_products_against_the_mirrors(gpu, n_ind, holes):
    from ld_tools_amd import GenoOperator, PackedPanel, geno_matmul_host, geno_rmatmul_host

    for n_snps in N_SNPS:
        rng = np.random.default_rng(1000 * n_ind + n_snps)
        codes = panel_codes(n_ind, n_snps, seed=7000 * n_ind + n_snps, holes=holes)
        w, wc, u = (random_weights(rng, n, max(COLS)) for n in (n_snps, n_snps, n_ind))
        want_y, want_y0 = geno_matmul_host(codes, w, wc), geno_matmul_host(codes, w)   # once, all 64 columns: a column stands alone
        want_z, want_zc = geno_rmatmul_host(codes, u)
        panel = PackedPanel.from_codes(codes, gpu)
        ops = [GenoOperator(panel)] + ([GenoOperator(panel, store_snps=256)] if n_snps == 1000 else [])   # four stores, accumulated
        for k in COLS:
            wk, wck, uk = (np.ascontiguousarray(x[:, :k]) for x in (w, wc, u))
            for op in ops:
                for n_slices in N_SLICES:
                    assert np.array_equal(host(op.matmul_q(wk, wck, n_slices=n_slices)), want_y[:, :k]), (n_snps, k, n_slices)
                assert np.array_equal(host(op.matmul_q(wk)), want_y0[:, :k]), (n_snps, k)
            z, zc = ops[0].rmatmul_q(uk)
            assert np.array_equal(host(z), want_z[:, :k]) and np.array_equal(host(zc), want_zc[:, :k]), (n_snps, k)


def test_digit_extremes(gpu):
    from ld_tools_amd import GenoOperator, PackedPanel

    n_ind, n_snps = 257, 300
    op = GenoOperator(PackedPanel.from_codes(np.ones((n_snps, 2 * n_ind), dtype=np.int8), gpu))   # every genotype 2 and called
    for x in EXTREMES:
        for k in (1, 9):
            w = np.full((n_snps, k), x, dtype=np.int32)
            assert np.array_equal(host(op.matmul_q(w, w)), np.full((n_ind, k), 3 * x * n_snps, dtype=np.int64))
            assert np.array_equal(host(op.matmul_q(w)), np.full((n_ind, k), 2 * x * n_snps, dtype=np.int64))
            z, zc = op.rmatmul_q(np.full((n_ind, k), x, dtype=np.int32))
            assert np.array_equal(host(z), np.full((n_snps, k), 2 * x * n_ind, dtype=np.int64))
            assert np.array_equal(host(zc), np.full((n_snps, k), x * n_ind, dtype=np.int64))
    w = np.tile(np.array(EXTREMES, dtype=np.int32), (n_snps, 1))                                  # and side by side in one tile
    assert np.array_equal(host(op.matmul_q(w, w)), np.tile(3 * n_snps * np.array(EXTREMES, dtype=np.int64), (n_ind, 1)))


def test_one_full_slice(gpu):
    """LDX_GENO_MAX_SLICE_SNPS SNPs in ONE slice at the digit extremes: the int32 accumulators reach 3 x 128 x 2^22 = 0.75 x 2^31."""
    from ld_tools_amd import GenoOperator, PackedPanel, _lib

    n_snps, n_ind = _lib.GENO_MAX_SLICE_SNPS, 2
    op = GenoOperator(PackedPanel.from_codes(np.ones((n_snps, 2 * n_ind), dtype=np.int8), gpu), store_snps=n_snps)
    w = torch.tensor(EXTREMES, dtype=torch.int32, device=gpu).repeat(n_snps, 1)
    want = np.tile(3 * n_snps * np.array(EXTREMES, dtype=np.int64), (n_ind, 1))
    assert np.array_equal(host(op.matmul_q(w, w, n_slices=1)), want)
    assert np.array_equal(host(op.matmul_q(w, w)), want)
    # one SNP more in one slice is refused, before anything is launched
    _, _, store, tables = op._stores[0]
    y = torch.zeros((n_ind, 4), dtype=torch.int64, device=gpu)
    rc = _lib.lib.ldx_geno_matmul_dev(store.data_ptr(), tables.data_ptr(), n_ind, n_snps + 1, w.data_ptr(), None, 4, 4, y.data_ptr(), 4,
                                      0, 1, None)
    assert rc == -1 and b"LDX_GENO_MAX_SLICE_SNPS" in _lib.lib.ldx_last_error()


def test_masks_and_accumulation(gpu):
    from ld_tools_amd import GenoOperator, LdxError, PackedPanel, geno_matmul_host, geno_rmatmul_host

    n_ind, n_snps, k = 70, 700, 5
    rng = np.random.default_rng(4)
    codes = panel_codes(n_ind, n_snps, seed=8, holes="3%")
    keep = rng.random(n_snps) < 0.7
    w, wc, u = random_weights(rng, n_snps, k), random_weights(rng, n_snps, k), random_weights(rng, n_ind, k)
    panel = PackedPanel.from_codes(codes, gpu)
    op = GenoOperator(panel, keep=keep)
    z, zc = (host(t) for t in op.rmatmul_q(u))
    want_z, want_zc = geno_rmatmul_host(codes, u, keep)
    assert np.array_equal(z, want_z) and np.array_equal(zc, want_zc)
    assert not z[~keep].any() and not zc[~keep].any() and zc[keep].any()          # dropped rows are written, as zeros
    assert np.array_equal(host(op.matmul_q(w, wc)), geno_matmul_host(codes, w, wc, keep))
    # two halves of the SNPs, accumulated, are the whole
    whole = host(GenoOperator(panel).matmul_q(w, wc))
    h = 333
    y = GenoOperator(PackedPanel.from_codes(codes[:h], gpu)).matmul_q(w[:h], wc[:h])
    y = GenoOperator(PackedPanel.from_codes(codes[h:], gpu)).matmul_q(w[h:], wc[h:], out=y)
    assert np.array_equal(host(y), whole)
    with pytest.raises(LdxError):
        op.matmul_q(w[:-1], wc[:-1])
    with pytest.raises(LdxError):
        op.matmul_q(w.astype(np.int64))
    with pytest.raises(LdxError):
        op.rmatmul_q(np.full((n_ind, 1), Q_MAX + 1, dtype=np.int32))


def test_invariances_adjointness_and_stats(gpu):
    from ld_tools_amd import GenoOperator, PackedPanel

    n_ind, n_snps, k = 131, 517, 6
    rng = np.random.default_rng(9)
    codes = panel_codes(n_ind, n_snps, seed=10, holes="3%")
    w, wc, u = random_weights(rng, n_snps, k), random_weights(rng, n_snps, k), random_weights(rng, n_ind, k)
    op = GenoOperator(PackedPanel.from_codes(codes, gpu))
    y = host(op.matmul_q(w, wc))
    z, zc = (host(t) for t in op.rmatmul_q(u))
    ps = rng.permutation(n_snps)                                                   # permuted SNPs, w alike
    assert np.array_equal(host(GenoOperator(PackedPanel.from_codes(codes[ps], gpu)).matmul_q(w[ps], wc[ps])), y)
    swap = np.arange(2 * n_ind).reshape(-1, 2)
    flip = rng.random(n_ind) < 0.5
    swap[flip] = swap[flip][:, ::-1]                                               # rephased genotypes
    rephased = GenoOperator(PackedPanel.from_codes(np.ascontiguousarray(codes[:, swap.reshape(-1)]), gpu))
    assert np.array_equal(host(rephased.matmul_q(w, wc)), y)
    pi = rng.permutation(n_ind)                                                    # permuted individuals, u alike
    cols = np.stack([2 * pi, 2 * pi + 1], axis=1).reshape(-1)
    moved = GenoOperator(PackedPanel.from_codes(np.ascontiguousarray(codes[:, cols]), gpu))
    mz, mzc = (host(t) for t in moved.rmatmul_q(u[pi]))
    assert np.array_equal(mz, z) and np.array_equal(mzc, zc)
    assert np.array_equal(host(moved.matmul_q(w, wc)), y[pi])
    # adjoint, exactly: sum u y == sum (w z + wc zc) on Python ints
    dot = lambda a, b: sum(int(p) * int(q) for p, q in zip(a.reshape(-1).tolist(), b.reshape(-1).tolist()))  # noqa: E731
    assert dot(u, y) == dot(w, z) + dot(wc, zc)
    # the statistics are the panel's own per-SNP counts
    h0, h1 = codes[:, 0::2], codes[:, 1::2]
    called = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1))
    n, a = op.stats()
    assert n.dtype == torch.int64 and np.array_equal(host(n), called.sum(axis=1))
    assert np.array_equal(host(a), (((h0 == 1).astype(np.int64) + (h1 == 1)) * called).sum(axis=1))
    assert np.array_equal(host(op.called_counts()), called.sum(axis=0))


def test_float_products(gpu):
    from ld_tools_amd import PackedPanel, geno_matmul, geno_matmul_host, geno_quantize, geno_rmatmul, geno_rmatmul_host

    rng = np.random.default_rng(12)
    codes = panel_codes(40, 300, seed=13, holes="3%")
    panel = PackedPanel.from_codes(codes, gpu)
    W, Wc, U = rng.standard_normal((300, 3)) * [1.0, 1e-4, 300.0], rng.standard_normal((300, 3)), rng.standard_normal((40, 2))
    prod = geno_matmul(panel, W, Wc)
    (qw, qc), e = geno_quantize(W, Wc)
    assert np.array_equal(host(prod.exps), e.numpy()) and np.array_equal(host(prod.sums), geno_matmul_host(codes, qw, qc))
    assert np.array_equal(host(prod.values()), geno_matmul_host(codes, qw, qc).astype(np.float64) * np.ldexp(1.0, e.numpy() - 30))
    pz, pzc = geno_rmatmul(panel, U)
    (qu,), eu = geno_quantize(U)
    want_z, want_zc = geno_rmatmul_host(codes, qu)
    assert np.array_equal(host(pz.sums), want_z) and np.array_equal(host(pzc.sums), want_zc) and np.array_equal(host(pz.exps), eu.numpy())

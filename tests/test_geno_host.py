"""CPU: the host side of the genotype products (include/ldx.h, "genotype products"): the numpy mirrors against a loop on Python
ints, geno_quantize's rounding and exponents, the library's symbols and argument rules (checked before any HIP call, so they
answer without a device), and the host forms of sample_pca and polygenic_score against dense float64."""
import numpy as np
import pytest

from ld_geno_exact import (Q_MAX, check_full_rank, check_structured, full_rank_codes, loop_matmul, loop_rmatmul, panel_codes,
                           random_weights, structured_panel)
from ld_king_exact import hand_table


def _check_mirrors(codes, keep, k, seed):
    from ld_tools_amd import geno_matmul_host, geno_rmatmul_host

    rng = np.random.default_rng(seed)
    n_snps, n_ind = codes.shape[0], codes.shape[1] // 2
    w, wc, u = random_weights(rng, n_snps, k), random_weights(rng, n_snps, k), random_weights(rng, n_ind, k)
    rows, kp = codes.tolist(), (None if keep is None else keep.tolist())
    assert geno_matmul_host(codes, w, wc, keep).tolist() == loop_matmul(rows, w.tolist(), wc.tolist(), kp)
    assert geno_matmul_host(codes, w, None, keep).tolist() == loop_matmul(rows, w.tolist(), None, kp)
    z, zc = geno_rmatmul_host(codes, u, keep)
    want_z, want_zc = loop_rmatmul(rows, u.tolist(), kp)
    assert z.tolist() == want_z and zc.tolist() == want_zc


def test_mirrors_on_the_hand_table():
    codes, keep, *_ = hand_table()   # a second-ALT code, a half-missing call, a masked SNP
    _check_mirrors(codes, keep, 3, seed=0)
    _check_mirrors(codes, None, 1, seed=1)
    from ld_tools_amd import geno_rmatmul_host

    z, zc = geno_rmatmul_host(codes, np.ones((3, 1), dtype=np.int32), keep)
    assert zc[:, 0].tolist() == [3, 3, 2, 2, 0, 3] and z[:, 0].tolist() == [4, 2, 1, 2, 0, 2]   # by hand from the table


@pytest.mark.parametrize("holes", ["none", "3%", "single"])
def test_mirrors_against_the_loop(holes):
    codes = panel_codes(9, 40, seed=21, holes=holes)
    keep = np.random.default_rng(3).random(40) < 0.8
    _check_mirrors(codes, keep, 5, seed=2)
    _check_mirrors(codes, None, 2, seed=3)


def test_quantize_exponents_and_rounding():
    from ld_tools_amd import LdxError, geno_quantize

    x = np.array([[1.0, 0.0, 3.0, 0.25, -1e-3],
                  [-0.5, 0.0, -4.0, 0.125, 5e-4],
                  [0.25, 0.0, 4.0, -0.25, 0.0]])
    (q,), e = geno_quantize(x)
    q, e = q.numpy(), e.numpy()
    assert q.dtype == np.int32 and e.tolist() == [0, 0, 2, -2, -9]   # exact powers of two keep their own exponent; 1e-3 <= 2^-9
    assert q[:, 0].tolist() == [Q_MAX, -Q_MAX // 2, Q_MAX // 4]
    assert q[:, 1].tolist() == [0, 0, 0]
    assert q[:, 2].tolist() == [3 * Q_MAX // 4, -Q_MAX, Q_MAX]   # +-max maps to +-2^30
    assert q[:, 3].tolist() == [Q_MAX, Q_MAX // 2, -Q_MAX]
    assert q[0, 4] == int(np.rint(-1e-3 * 2.0 ** 39)) and np.abs(q).max() <= Q_MAX
    # ties to even: 2^-31 multiples beside a column maximum of 1
    t = np.array([[1.0], [0.5 * 2.0 ** -30], [1.5 * 2.0 ** -30], [2.5 * 2.0 ** -30], [-0.5 * 2.0 ** -30], [-1.5 * 2.0 ** -30]])
    (q,), e = geno_quantize(t)
    assert e.tolist() == [0] and q[:, 0].tolist() == [Q_MAX, 0, 2, 2, 0, -2]
    # shared exponents over two matrices: the larger one sets them
    (qa, qb), e = geno_quantize(np.array([[0.5, 1.0]]), np.array([[3.0, -0.25]]))
    assert e.tolist() == [2, 0] and qa.tolist() == [[Q_MAX // 8, Q_MAX]] and qb.tolist() == [[3 * Q_MAX // 4, -Q_MAX // 4]]
    for bad in (np.array([[np.inf]]), np.array([[np.nan]]), np.zeros((2, 65)), np.zeros((2, 0))):
        with pytest.raises(LdxError):
            geno_quantize(bad)
    with pytest.raises(LdxError):
        geno_quantize(np.zeros((2, 2)), np.zeros((2, 3)))


def test_symbols_and_argument_rules():
    from ld_tools_amd import _lib

    lib = _lib.lib
    assert hasattr(lib, "ldx_geno_matmul_dev") and hasattr(lib, "ldx_geno_rmatmul_dev")
    assert "ldx_geno_matmul_dev" in _lib.SIGNATURES and "ldx_geno_rmatmul_dev" in _lib.SIGNATURES
    assert _lib.GENO_MAX_COLS == 64 and _lib.GENO_MAX_SLICE_SNPS == 1 << 22 and 384 * _lib.GENO_MAX_SLICE_SNPS < 1 << 31
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data                      # a non-null pointer: every call below returns before it is used
    ARG, UNSUPPORTED = -1, -3

    def fwd(store=p, tables=p, n_ind=4, n_snps=100, w=p, wc=None, ld_w=8, k=8, y=p, ld_y=8, accumulate=0, n_slices=0):
        return lib.ldx_geno_matmul_dev(store, tables, n_ind, n_snps, w, wc, ld_w, k, y, ld_y, accumulate, n_slices, None)

    def rev(alt=p, ref=p, n_snps=100, n_hap=8, keep=None, u=p, ld_u=8, k=8, z=p, zc=p, ld_z=8):
        return lib.ldx_geno_rmatmul_dev(alt, ref, n_snps, n_hap, keep, u, ld_u, k, z, zc, ld_z, None)

    for name in ("store", "tables", "w", "y"):
        assert fwd(**{name: None}) == ARG
    assert fwd(k=0) == ARG and fwd(k=65, ld_w=65, ld_y=65) == ARG
    assert fwd(ld_w=7) == ARG and fwd(ld_y=7) == ARG
    assert fwd(n_ind=0) == ARG and fwd(n_snps=0) == ARG
    assert fwd(n_ind=_lib.MAX_HAPS // 2 + 1) == UNSUPPORTED
    assert fwd(n_snps=_lib.KING_MAX_STORE_SNPS + 1) == ARG
    assert fwd(n_snps=_lib.GENO_MAX_SLICE_SNPS + 1, n_slices=1) == ARG          # one slice would pass the bound
    assert b"LDX_GENO_MAX_SLICE_SNPS" in lib.ldx_last_error()
    for name in ("alt", "ref", "u", "z", "zc"):
        assert rev(**{name: None}) == ARG
    assert rev(n_hap=7) == ARG and rev(n_hap=0) == ARG and rev(n_snps=0) == ARG
    assert rev(n_hap=_lib.MAX_HAPS + 2) == UNSUPPORTED
    assert rev(k=0) == ARG and rev(k=65, ld_u=65, ld_z=65) == ARG
    assert rev(ld_u=7) == ARG and rev(ld_z=7) == ARG
    header = (__import__("pathlib").Path(__file__).resolve().parents[1] / "include" / "ldx.h").read_text()
    assert "genotype products" in header and "NOT validated against PLINK 2, GCTA or FastPCA" in header
    assert _lib.lib.ldx_version() == 102          # additive symbols: the ABI number stays


# ---- sample_pca_host against the dense eigendecomposition ------------------------------------------------------------------------
# The bounds (tests/ld_geno_exact.py) were set with the definition: the method quantises to 2^-31 per entry, and a numpy restatement
# of the algorithm gave 2.4e-10 on the full-rank panel and 5e-11 on the structured one, so 1e-8 (eigenvalues) and 1e-7 (residuals),
# relative to lambda_1, leave about 40x; the top two eigenvalues of the structured panel are nearly equal, hence residuals, not vectors.
def test_pca_host_full_rank():
    from ld_tools_amd import sample_pca_host

    codes = full_rank_codes()
    check_full_rank(sample_pca_host(codes, n_pcs=40, n_iter=1), codes)


def test_pca_host_structured():
    from ld_tools_amd import sample_pca_host

    codes = structured_panel()
    pca = sample_pca_host(codes, n_pcs=4, loadings=True)
    check_structured(pca, codes)
    # the loadings are X^T u / sqrt(M lambda): unit vectors, and projecting the training individuals returns the vectors
    assert np.allclose(np.linalg.norm(pca.loadings[:, :2], axis=0), 1.0, atol=1e-6)
    assert np.abs(pca.project(codes)[:, :2] - pca.eigenvectors[:, :2]).max() <= 1e-6


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("impute", ["mean", "zero"])
def test_score_host_against_dense(impute, k):
    from ld_tools_amd import polygenic_score_host

    codes = panel_codes(9, 400, seed=5, holes="3%")
    keep = np.random.default_rng(1).random(400) < 0.9
    # a weight is quantised to 2^-31 of its column's scale, so a sum of 400 terms is off by about 20 x 2^-31 x max |beta|: weights
    # of one sign (scores of the order of 100 max |beta|) keep that an order of magnitude inside the bound, 1e-9 max |score|
    beta = np.random.default_rng(2).uniform(0.5, 1.0, size=(400, k)) * np.array([1.0, -1e-3, 50.0])[:k]
    h0, h1 = codes[:, 0::2], codes[:, 1::2]
    called = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1)) & keep[:, None]
    g = ((h0 == 1).astype(np.float64) + (h1 == 1)) * called
    n = called.sum(axis=1)
    two_p = np.where(n > 0, g.sum(axis=1) / np.maximum(n, 1), 0.0)
    filled = g + (~called & (keep & (n > 0))[:, None]) * two_p[:, None] if impute == "mean" else g
    want = filled.T @ beta
    got = polygenic_score_host(codes, beta if k > 1 else beta[:, 0], keep=keep, impute=impute)
    assert got.sum.shape == (9, k) and got.sum.dtype == np.float64
    assert np.abs(got.sum - want).max() <= 1e-9 * np.abs(want).max()
    assert got.allele_ct.dtype == np.int64 and np.array_equal(got.allele_ct, 2 * called.sum(axis=0))

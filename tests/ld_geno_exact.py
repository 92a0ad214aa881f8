"""Helpers of the genotype-product tests (include/ldx.h, "genotype products"): an oracle that loops over the allele codes on
Python ints and shares nothing with the host mirrors of ld_tools_amd, the structured panels of the PCA tests, and the dense
float64 GRM the PCA is compared with.  No tests here."""
import numpy as np

from ld_king_exact import panel_codes  # noqa: F401  (the unstructured panels)

Q_MAX = 1 << 30


def _genotype(c0, c1):
    """(dosage, called) of one individual at one SNP from its two allele codes."""
    if c0 in (0, 1) and c1 in (0, 1):
        return int(c0) + int(c1), 1
    return 0, 0


def loop_matmul(codes, q_w, q_wc=None, keep=None):
    """y [n_ind][k] as lists of Python ints."""
    n_snps, n_hap = len(codes), len(codes[0])
    k = len(q_w[0])
    y = [[0] * k for _ in range(n_hap // 2)]
    for i in range(n_snps):
        if keep is not None and not keep[i]:
            continue
        for a in range(n_hap // 2):
            g, c = _genotype(codes[i][2 * a], codes[i][2 * a + 1])
            for col in range(k):
                y[a][col] += g * int(q_w[i][col]) + (c * int(q_wc[i][col]) if q_wc is not None else 0)
    return y


def loop_rmatmul(codes, q_u, keep=None):
    """(z, zc) [n_snps][k] as lists of Python ints."""
    n_snps, n_hap = len(codes), len(codes[0])
    k = len(q_u[0])
    z = [[0] * k for _ in range(n_snps)]
    zc = [[0] * k for _ in range(n_snps)]
    for i in range(n_snps):
        if keep is not None and not keep[i]:
            continue
        for a in range(n_hap // 2):
            g, c = _genotype(codes[i][2 * a], codes[i][2 * a + 1])
            for col in range(k):
                z[i][col] += g * int(q_u[a][col])
                zc[i][col] += c * int(q_u[a][col])
    return z, zc


def random_weights(rng, n, k):
    """int32 [n, k], uniform in [-2^30, 2^30], the two ends included somewhere when there is room."""
    q = rng.integers(-Q_MAX, Q_MAX + 1, size=(n, k), dtype=np.int64).astype(np.int32)
    if q.size >= 2:
        q.reshape(-1)[0], q.reshape(-1)[-1] = Q_MAX, -Q_MAX
    return q


def structured_codes(n_ind, n_snps, seed, n_pop=3, fst=0.1, holes=False):
    """int8 [n_snps, 2 n_ind]: individual a belongs to population a mod n_pop; base frequencies f uniform in [0.05, 0.5]; each
    population's frequency is f + N(0, fst f (1 - f)) clipped to [0.01, 0.99]; with holes 3 % of the genotypes are missing."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.5, size=n_snps)
    fp = np.clip(f[:, None] + rng.standard_normal((n_snps, n_pop)) * np.sqrt(fst * f * (1.0 - f))[:, None], 0.01, 0.99)
    pop = np.arange(n_ind) % n_pop
    codes = (rng.random((n_snps, 2 * n_ind)) < np.repeat(fp[:, pop], 2, axis=1)).astype(np.int8)
    if holes:
        codes[np.repeat(rng.random((n_snps, n_ind)) < 0.03, 2, axis=1)] = 2
    return codes


def dense_grm(codes, keep=None):
    """(K float64 [n_ind, n_ind], M): X X^T / M with X_ia = c_ia (g_ia - 2 p_i) / sqrt(2 p_i (1 - p_i)), p_i = a_i / (2 n_i), over
    the kept SNPs with calls and 0 < p < 1 -- plain float64 from the codes."""
    c = np.asarray(codes)
    h0, h1 = c[:, 0::2], c[:, 1::2]
    called = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1))
    if keep is not None:
        called = called & np.asarray(keep, dtype=bool)[:, None]
    g = ((h0 == 1).astype(np.float64) + (h1 == 1)) * called
    n = called.sum(axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(n > 0, g.sum(axis=1) / (2.0 * n), 0.0)
    v = 2.0 * p * (1.0 - p)
    use = (n > 0) & (v > 0)
    X = (called[use] * (g[use] - 2.0 * p[use, None])) / np.sqrt(v[use])[:, None]
    M = int(use.sum())
    return X.T @ X / M, M


# ---- the two PCA panels and their checks against the dense eigendecomposition (host and GPU tests share them) -------------------
def full_rank_codes():
    return panel_codes(40, 600, seed=1, holes="3%")


def structured_panel():
    return structured_codes(150, 3000, seed=2, n_pop=3, fst=0.1, holes=True)


def check_full_rank(pca, codes):
    K, M = dense_grm(codes)
    lam = np.linalg.eigvalsh(K)[::-1]
    assert pca.n_used == M and pca.eigenvalues.shape == (40,)
    err = np.abs(pca.eigenvalues - lam).max() / lam[0]
    print("full rank: max eigenvalue error / lambda_1 =", err)
    assert err <= 1e-8


def check_structured(pca, codes):
    K, M = dense_grm(codes)
    lam = np.linalg.eigvalsh(K)[::-1]
    assert pca.n_used == M and pca.eigenvectors.shape == (150, 4)
    err = np.abs(pca.eigenvalues[:2] - lam[:2]).max() / lam[0]
    res = [np.abs(K @ pca.eigenvectors[:, j] - pca.eigenvalues[j] * pca.eigenvectors[:, j]).max() / lam[0] for j in range(2)]
    print("structured: eigenvalue error / lambda_1 =", err, " residuals / lambda_1 =", res)
    assert err <= 1e-8 and max(res) <= 1e-7
    big = np.argmax(np.abs(pca.eigenvectors), axis=0)
    assert (pca.eigenvectors[big, np.arange(4)] > 0).all()                 # the sign rule
    assert np.allclose(np.linalg.norm(pca.eigenvectors, axis=0), 1.0, atol=1e-12)

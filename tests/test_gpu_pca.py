"""GPU: sample_pca and polygenic_score (ld_tools_amd.ops) against their host mirrors BIT FOR BIT -- every device step is an exact
integer product or a single IEEE operation -- and against the dense float64 eigendecomposition within the bounds that
tests/test_geno_host.py states; the PLINK-style drivers on a small written fileset."""
import functools

import numpy as np
import pytest

from ld_geno_exact import check_full_rank, check_structured, full_rank_codes, panel_codes, structured_panel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PANELS = {"full_rank": (full_rank_codes, dict(n_pcs=40)), "structured": (structured_panel, dict(n_pcs=4))}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def codes_of(name):
    return PANELS[name][0]()


def same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_pca(a, b):
    return (a.n_used == b.n_used and same_bits(a.eigenvalues, b.eigenvalues) and same_bits(a.eigenvectors, b.eigenvectors)
            and same_bits(a.loadings, b.loadings) and same_bits(a.two_p, b.two_p) and same_bits(a.inv_sd, b.inv_sd))


@pytest.mark.parametrize("name", list(PANELS))
def test_pca_equals_the_host_mirror_bit_for_bit(gpu, name):
    from ld_tools_amd import PackedPanel, sample_pca, sample_pca_host

    codes, kw = codes_of(name), PANELS[name][1]
    dev = sample_pca(PackedPanel.from_codes(codes, gpu), loadings=True, **kw)
    ref = sample_pca_host(codes, loadings=True, **kw)
    assert same_pca(dev, ref)
    assert dev.eigenvalues.shape == (kw["n_pcs"],) and dev.loadings.shape == (codes.shape[0], kw["n_pcs"])
    # a held-out third: components of the first two thirds of the individuals, the last third projected on them
    n_ind = codes.shape[1] // 2
    cut = 2 * (2 * n_ind // 3)
    train, held = np.ascontiguousarray(codes[:, :cut]), np.ascontiguousarray(codes[:, cut:])
    n_pcs = min(kw["n_pcs"], cut // 2)
    dev = sample_pca(PackedPanel.from_codes(train, gpu), n_pcs=n_pcs, loadings=True)
    ref = sample_pca_host(train, n_pcs=n_pcs, loadings=True)
    assert same_pca(dev, ref)
    got = dev.project(PackedPanel.from_codes(held, gpu))
    assert got.shape == (n_ind - cut // 2, n_pcs) and same_bits(got, ref.project(held))


def test_pca_full_rank_against_dense(gpu):
    from ld_tools_amd import PackedPanel, sample_pca

    codes = codes_of("full_rank")
    check_full_rank(sample_pca(PackedPanel.from_codes(codes, gpu), n_pcs=40, n_iter=1), codes)


def test_pca_structured_against_dense(gpu):
    from ld_tools_amd import PackedPanel, sample_pca

    codes = codes_of("structured")
    check_structured(sample_pca(PackedPanel.from_codes(codes, gpu), n_pcs=4), codes)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("impute", ["mean", "zero"])
def test_score_equals_the_host_mirror(gpu, impute, k):
    from ld_tools_amd import PackedPanel, polygenic_score, polygenic_score_host

    codes = panel_codes(131, 700, seed=31, holes="3%")
    codes[17] = 2                                                        # a kept SNP without a call
    keep = np.random.default_rng(5).random(700) < 0.9
    beta = np.random.default_rng(6).standard_normal((700, k)) * np.array([1.0, 1e-5, 400.0])[:k]
    beta = beta if k > 1 else beta[:, 0]
    dev = polygenic_score(PackedPanel.from_codes(codes, gpu), beta, keep=keep, impute=impute)
    ref = polygenic_score_host(codes, beta, keep=keep, impute=impute)
    assert same_bits(dev.sum, ref.sum) and dev.sum.shape == (131, k)
    assert np.array_equal(dev.sums, ref.sums) and np.array_equal(dev.exps, ref.exps)
    assert dev.allele_ct.dtype == np.int64 and np.array_equal(dev.allele_ct, ref.allele_ct)


# ---- the drivers on a small written fileset -----------------------------------------------------------------------------------------
N_VAR, N_SAMPLES = 500, 45


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    from ld_tools_amd import plink

    codes = panel_codes(N_SAMPLES, N_VAR, seed=41, holes="none")
    codes[:, 4:6] = codes[:, 0:2]                                          # individual 2 duplicates individual 0
    gone = np.random.default_rng(6).random((N_VAR, N_SAMPLES)) < 0.03
    codes[np.repeat(gone, 2, axis=1)] = 2
    prefix = str(tmp_path_factory.mktemp("pca") / "study")
    fid, iid = [f"FAM{s // 3}" for s in range(N_SAMPLES)], [f"ID{s:03d}" for s in range(N_SAMPLES)]
    ids = [f"rs{v}" for v in range(N_VAR)]
    bim = {"chrom": ["7"] * N_VAR, "ids": ids, "pos": [1000 + 150 * v for v in range(N_VAR)], "a1": ["G"] * N_VAR, "a2": ["A"] * N_VAR}
    plink.write_bfile(prefix, plink.codes_bed_host(codes, alt="a1"), bim, {"fid": fid, "iid": iid})
    return prefix, plink.canonical_codes(codes), fid, iid, ids


def read_table(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        return head, [line.rstrip("\n").split("\t") for line in f]


def test_bfile_pca_files(gpu, study):
    from ld_tools_amd import king_cell_host, king_cutoff, sample_counts_host, sample_pca_host
    from ld_tools_amd.drivers import plink as dp

    prefix, codes, fid, iid, _ = study
    table = dp.bfile_pca(prefix, out=prefix + ".all", n_pcs=5)
    ref = sample_pca_host(codes, n_pcs=5)
    assert same_bits(table.coords, ref.eigenvectors) and table.in_pca.all()
    head, rows = read_table(prefix + ".all.eigenvec")
    assert head == ["#FID", "IID"] + [f"PC{j}" for j in range(1, 6)] and [r[:2] for r in rows] == [list(x) for x in zip(fid, iid)]
    assert same_bits(np.array([[float(v) for v in r[2:]] for r in rows]), ref.eigenvectors)
    with open(prefix + ".all.eigenval") as f:
        assert same_bits(np.array([float(line) for line in f]), ref.eigenvalues)
    assert dp.main(["pca", "--bfile", prefix, "--out", prefix + ".cli", "--pca", "5"]) == 0
    assert open(prefix + ".cli.eigenvec").read() == open(prefix + ".all.eigenvec").read()
    # relatives dropped first: the duplicate pair loses one individual, which is projected
    table = dp.bfile_pca(prefix, out=prefix + ".unrel", n_pcs=3, king_cutoff=0.35)
    N, HH, IBS0, HET = sample_counts_host(codes)
    inside, _ = king_cutoff(king_cell_host(N, HH, IBS0, HET, HET.T), 0.35)
    assert np.array_equal(table.in_pca, inside) and inside.sum() == N_SAMPLES - 1
    cols = lambda m: np.stack([2 * np.flatnonzero(m), 2 * np.flatnonzero(m) + 1], axis=1).reshape(-1)  # noqa: E731
    ref = sample_pca_host(np.ascontiguousarray(codes[:, cols(inside)]), n_pcs=3, loadings=True)
    want = np.empty((N_SAMPLES, 3))
    want[inside], want[~inside] = ref.eigenvectors, ref.project(np.ascontiguousarray(codes[:, cols(~inside)]))
    assert same_bits(table.coords, want)
    _, rows = read_table(prefix + ".unrel.eigenvec")
    assert same_bits(np.array([[float(v) for v in r[2:]] for r in rows]), want)


def test_bfile_score_files(gpu, study, capsys):
    from ld_tools_amd import polygenic_score_host
    from ld_tools_amd.drivers import plink as dp

    prefix, codes, fid, iid, ids = study
    rng = np.random.default_rng(8)
    picked = rng.permutation(N_VAR)[:200]
    w = rng.standard_normal(200)
    allele = np.where(rng.random(200) < 0.5, "G", "A")                     # G is a1 = code 1; A is the other allele
    allele[:3] = "T"                                                       # no allele of the variant
    path = prefix + ".weights"
    with open(path, "w") as f:
        f.write("SNP\tA1\tBETA\n")
        f.writelines(f"{ids[v]}\t{a}\t{x!r}\n" for v, a, x in zip(picked.tolist(), allele.tolist(), w.tolist()))
        f.write("rs_unknown\tG\t1.0\n")
    beta, offset, keep = np.zeros(N_VAR), np.zeros(N_VAR), np.zeros(N_VAR, dtype=bool)
    for v, a, x in zip(picked[3:], allele[3:], w[3:]):
        keep[v] = True
        beta[v], offset[v] = (x, 0.0) if a == "G" else (-x, 2.0 * x)
    for impute in ("mean", "zero"):
        table = dp.bfile_score(prefix, path, out=prefix + "." + impute, impute=impute)
        ref = polygenic_score_host(codes, beta, keep=keep, impute=impute, offset=offset)
        assert (table.n_matched, table.n_lines) == (197, 201)
        assert same_bits(table.scores.sum, ref.sum) and np.array_equal(table.scores.allele_ct, ref.allele_ct)
        head, rows = read_table(f"{prefix}.{impute}.sscore")
        assert head == ["#FID", "IID", "ALLELE_CT", "SCORE1_SUM"] and [r[:2] for r in rows] == [list(x) for x in zip(fid, iid)]
        assert [int(r[2]) for r in rows] == ref.allele_ct.tolist()
        assert same_bits(np.array([[float(r[3])] for r in rows]), ref.sum)
    # a weight on the other allele is the same score of the flipped dosage: sum w (2 - g) over the called genotypes
    h0, h1 = codes[:, 0::2], codes[:, 1::2]
    called = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1)) & keep[:, None]
    g = ((h0 == 1).astype(np.float64) + (h1 == 1)) * called
    w_full = np.zeros(N_VAR)
    w_full[picked[3:]] = w[3:]
    on_a1 = np.zeros(N_VAR, dtype=bool)
    on_a1[picked[3:]] = allele[3:] == "G"
    dense = (np.where(on_a1[:, None], g, (2.0 - g) * called) * w_full[:, None]).sum(axis=0)
    assert np.abs(ref.sum[:, 0] - dense).max() <= 1e-6 * np.abs(dense).max()
    assert dp.main(["score", "--bfile", prefix, "--out", prefix + ".cli", "--score", path]) == 0
    assert "197 of 201 weight lines matched" in capsys.readouterr().out
    assert open(prefix + ".cli.sscore").read() == open(prefix + ".mean.sscore").read()

"""GPU: drivers/plink.py's bfile_glm and the ``glm`` subcommand on a small written fileset -- two phenotypes whose missing rows
differ (two groups of complete rows), covariates from bfile_pca's .eigenvec; the .glm.linear files are then fed to the ``clump``
subcommand as they stand; the binary-phenotype refusal."""
import numpy as np
import pytest

import ld_glm_exact as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_VAR, N_SAMPLES = 200, 60


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def study(gpu, tmp_path_factory):
    from ld_tools_amd import plink
    from ld_tools_amd.drivers import plink as dp

    codes = X.glm_codes(N_SAMPLES, N_VAR, seed=51, miss=0.03)
    codes[:, 1::2][(codes[:, 0::2] == 2)] = 2                      # a .bed has no half-missing genotype
    codes[:, 0::2][(codes[:, 1::2] == 2)] = 2
    for v in range(1, N_VAR, 2):                                   # pairs of variants in LD, so that clumps have members
        same = np.random.default_rng(v).random(N_SAMPLES) < 0.9
        codes[v][np.repeat(same, 2)] = codes[v - 1][np.repeat(same, 2)]
    codes = plink.canonical_codes(codes)
    prefix = str(tmp_path_factory.mktemp("glm") / "study")
    fid, iid = [f"FAM{s // 2}" for s in range(N_SAMPLES)], [f"ID{s:03d}" for s in range(N_SAMPLES)]
    ids = [f"rs{v}" for v in range(N_VAR)]
    bim = {"chrom": ["5"] * N_VAR, "ids": ids, "pos": [1000 + 100 * v for v in range(N_VAR)], "a1": ["G"] * N_VAR, "a2": ["A"] * N_VAR}
    plink.write_bfile(prefix, plink.codes_bed_host(codes, alt="a1"), bim, {"fid": fid, "iid": iid})
    dp.bfile_pca(prefix, out=prefix, n_pcs=3)
    g, _ = X.planes(codes)
    rng = np.random.default_rng(52)
    Y = rng.standard_normal((N_SAMPLES, 2))
    Y[:, 0] += 1.2 * g[10] + 0.9 * g[120]
    Y[:, 1] += 1.0 * g[61]
    text = [[repr(float(Y[s, 0])), repr(float(Y[s, 1]))] for s in range(N_SAMPLES)]
    for s in (3, 17):
        text[s][0] = "NA"
    for s in (17, 40, 41):
        text[s][1] = "-9"
    order = rng.permutation(N_SAMPLES)[:-2]                        # shuffled lines; two individuals have no line at all
    pheno = prefix + ".pheno"
    with open(pheno, "w") as f:
        f.write("#FID IID height weight\n" + "".join(f"{fid[s]} {iid[s]} {text[s][0]} {text[s][1]}\n" for s in order))
    absent = np.setdiff1d(np.arange(N_SAMPLES), order)
    rows = [np.setdiff1d(np.arange(N_SAMPLES), np.concatenate([absent, gone])) for gone in ((3, 17), (17, 40, 41))]
    return prefix, codes, ids, pheno, Y, rows


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def read_table(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        return head, [line.rstrip("\n").split("\t") for line in f]


def test_bfile_glm_groups_files_and_clump(study, tmp_path):
    from ld_tools_amd import ld_glm_host, plink
    from ld_tools_amd.drivers import plink as dp
    from ld_tools_amd.drivers.glm import GLM_COLUMNS

    prefix, codes, ids, pheno, Y, rows = study
    tables = dp.bfile_glm(prefix, pheno, covar=prefix + ".eigenvec", out=prefix + ".api")
    assert [t.names for t in tables] == [["height"], ["weight"]]                    # two sets of complete rows: two sweeps
    covar = plink.read_covar(prefix + ".eigenvec")[3]
    for j, (table, r) in enumerate(zip(tables, rows)):
        ref = ld_glm_host(codes, Y[r, j], covar[r], individuals=r)
        res = table.result
        assert res.df == len(r) - 4 - 1 and (res.flags.cpu().numpy() != 6).all()
        for name in ("beta", "se", "t"):
            assert same_bits(getattr(res, name).cpu().numpy(), getattr(ref, name).numpy()), name
        assert np.array_equal(res.flags.cpu().numpy(), ref.flags.numpy()) and np.array_equal(res.n_obs, ref.n_obs)
        head, lines = read_table(f"{prefix}.api.{table.names[0]}.glm.linear")
        assert tuple(head) == GLM_COLUMNS and [ln[2] for ln in lines] == ids and all(ln[6] == "ADD" for ln in lines)
        ok = np.isin(res.flags.cpu().numpy()[:, 0], (0, 5))
        assert [ln[8] == "NA" for ln in lines] == (~ok).tolist()
        assert same_bits([float(ln[8]) for ln, o in zip(lines, ok) if o], res.beta.cpu().numpy()[ok, 0])
        assert [int(ln[7]) for ln in lines] == res.n_obs.tolist()
    # the command line writes the same files
    assert dp.main(["glm", "--bfile", prefix, "--out", prefix + ".cli", "--pheno", pheno, "--covar", prefix + ".eigenvec"]) == 0
    for name in ("height", "weight"):
        assert open(f"{prefix}.cli.{name}.glm.linear").read() == open(f"{prefix}.api.{name}.glm.linear").read()
    assert dp.main(["glm", "--bfile", prefix, "--out", prefix + ".one", "--pheno", pheno, "--pheno-name", "weight",
                    "--covar", prefix + ".eigenvec", "--covar-name", "PC1,PC2", "--vif", "20"]) == 0
    one = dp.bfile_glm(prefix, pheno, covar=prefix + ".eigenvec", pheno_names=["weight"], covar_names=["PC1", "PC2"], max_vif=20.0)
    assert len(one) == 1 and one[0].result.design.n_cov == 3
    _, lines = read_table(prefix + ".one.weight.glm.linear")
    assert same_bits([float(ln[11]) for ln in lines if ln[11] != "NA"],
                     one[0].result.p.cpu().numpy()[np.isin(one[0].result.flags.cpu().numpy()[:, 0], (0, 5)), 0])
    # the clump subcommand reads the .glm.linear file as it stands
    clump = ["--clump-p1", "1e-3", "--clump-p2", "0.05", "--clump-r2", "0.3", "--clump-kb", "1"]
    for table in tables:
        name = table.names[0]
        assert dp.main(["clump", "--bfile", prefix, "--out", f"{prefix}.{name}", "--clump", f"{prefix}.api.{name}.glm.linear",
                        "--clump-snp-field", "ID", "--clump-field", "P", *clump]) == 0
        with open(f"{prefix}.{name}.clumped") as f:
            index = [ln.split()[2] for ln in f.read().splitlines()[1:] if ln.strip()]
        want = dp.bfile_clump(prefix, table.result.p.cpu().numpy()[:, 0], p1=1e-3, p2=0.05, r2=0.3, window_bp=1000)
        assert index == [ids[k] for k, _ in want.clumps.clumps()] and len(index) >= 1
    assert "rs10" in open(f"{prefix}.height.clumped").read() and "rs61" in open(f"{prefix}.weight.clumped").read()


def test_binary_phenotypes_are_refused(study):
    from ld_tools_amd import LdxError
    from ld_tools_amd.drivers import plink as dp

    prefix, codes, ids, _, Y, _ = study
    bf = dp.load_bfile(prefix)
    for values in ((1.0, 2.0), (0.0, 1.0)):
        cc = np.where(Y[:, 0] > 0, values[1], values[0])
        cc[5] = np.nan
        table = (bf.fid, bf.iid, ["cc", "height"], np.stack([cc, Y[:, 0]], axis=1))
        with pytest.raises(LdxError, match="case/control"):
            dp.bfile_glm(bf, table)
        tables = dp.bfile_glm(bf, table, allow_binary=True)
        assert [t.names for t in tables] == [["cc"], ["height"]] and tables[0].result.df == N_SAMPLES - 1 - 1 - 1
    assert [t.names for t in dp.bfile_glm(bf, table, pheno_names=["height"])] == [["height"]]
    with pytest.raises(LdxError, match="no phenotype named"):
        dp.bfile_glm(bf, table, pheno_names=["bmi"])

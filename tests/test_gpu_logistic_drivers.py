"""GPU: drivers/plink.py's bfile_logistic and the ``logistic`` subcommand on a small written fileset -- two case/control
phenotypes, one coded 1 / 2 and one 0 / 1, whose missing rows differ (two groups of complete rows), covariates from bfile_pca's
.eigenvec; the .glm.logistic files are then fed to the ``clump`` subcommand as they stand; the refusals of other codings."""
import math

import numpy as np
import pytest

import ld_logistic_exact as X
from ld_tools_amd import ld_glm_logistic  # noqa: F401  (the feature under test)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_VAR, N_SAMPLES = 200, 120


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

    codes = X.logit_codes(N_SAMPLES, N_VAR, seed=51, miss=0.03)
    codes[:, 1::2][(codes[:, 0::2] == 2)] = 2                      # a .bed has no half-missing genotype
    codes[:, 0::2][(codes[:, 1::2] == 2)] = 2
    for v in range(1, N_VAR, 2):                                   # pairs of variants in LD, so that clumps have members
        same = np.random.default_rng(v).random(N_SAMPLES) < 0.9
        codes[v][np.repeat(same, 2)] = codes[v - 1][np.repeat(same, 2)]
    codes = plink.canonical_codes(codes)
    prefix = str(tmp_path_factory.mktemp("logistic") / "study")
    fid, iid = [f"FAM{s // 2}" for s in range(N_SAMPLES)], [f"ID{s:03d}" for s in range(N_SAMPLES)]
    ids = [f"rs{v}" for v in range(N_VAR)]
    bim = {"chrom": ["5"] * N_VAR, "ids": ids, "pos": [1000 + 100 * v for v in range(N_VAR)], "a1": ["G"] * N_VAR, "a2": ["A"] * N_VAR}
    plink.write_bfile(prefix, plink.codes_bed_host(codes, alt="a1"), bim, {"fid": fid, "iid": iid})
    dp.bfile_pca(prefix, out=prefix, n_pcs=3)
    g, _ = X.planes(codes)
    rng = np.random.default_rng(52)
    eta = np.stack([-0.8 + 1.6 * g[10], -1.0 + 2.2 * g[61]], axis=1)
    Y = (rng.random((N_SAMPLES, 2)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.int64)
    text = [[str(Y[s, 0] + 1), str(Y[s, 1])] for s in range(N_SAMPLES)]     # "asthma" coded 1 / 2, "t2d" coded 0 / 1
    for s in (3, 17):
        text[s][0] = "NA"
    for s in (17, 40, 41):
        text[s][1] = "-9"
    order = rng.permutation(N_SAMPLES)[:-2]                        # shuffled lines; two individuals have no line at all
    pheno = prefix + ".pheno"
    with open(pheno, "w") as f:
        f.write("#FID IID asthma t2d\n" + "".join(f"{fid[s]} {iid[s]} {text[s][0]} {text[s][1]}\n" for s in order))
    absent = np.setdiff1d(np.arange(N_SAMPLES), order)
    rows = [np.setdiff1d(np.arange(N_SAMPLES), np.concatenate([absent, gone])) for gone in ((3, 17), (17, 40, 41))]
    return prefix, codes, ids, pheno, Y, rows


def read_table(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        return head, [line.rstrip("\n").split("\t") for line in f]


def test_bfile_logistic_groups_files_and_clump(study):
    from ld_tools_amd import ld_glm_logistic_host, plink
    from ld_tools_amd.drivers import plink as dp
    from ld_tools_amd.drivers.glm import LOGISTIC_COLUMNS

    prefix, codes, ids, pheno, Y, rows = study
    tables = dp.bfile_logistic(prefix, pheno, covar=prefix + ".eigenvec", out=prefix + ".api")
    assert [t.names for t in tables] == [["asthma"], ["t2d"]]                       # two sets of complete rows: two groups
    covar = plink.read_covar(prefix + ".eigenvec")[3]
    for j, (table, r) in enumerate(zip(tables, rows)):
        ref = ld_glm_logistic_host(codes, Y[r, j], covar[r], individuals=r)
        res = table.result
        flags = res.flags.cpu().numpy()[:, 0]
        assert res.design.n_cov == 3 and res.design.n_ind == len(r)
        assert np.array_equal(flags, ref.flags.numpy()[:, 0]) and np.array_equal(res.n_obs, ref.n_obs)
        ok = flags == 0
        beta, se = res.beta.cpu().numpy()[:, 0], res.se.cpu().numpy()[:, 0]
        assert ok.sum() >= 150 and (np.abs(beta[ok] - ref.beta.numpy()[ok, 0]) <= 2.0 ** -39 * se[ok]).all()
        head, lines = read_table(f"{prefix}.api.{table.names[0]}.glm.logistic")
        assert tuple(head) == LOGISTIC_COLUMNS and [ln[2] for ln in lines] == ids and all(ln[6] == "ADD" for ln in lines)
        assert [ln[8] == "NA" for ln in lines] == (~ok).tolist() and [ln[12] == "." for ln in lines] == ok.tolist()
        assert [float(ln[8]) for ln, o in zip(lines, ok) if o] == [math.exp(b) for b in beta[ok]]
        assert [float(ln[9]) for ln, o in zip(lines, ok) if o] == se[ok].tolist()
        assert [int(ln[7]) for ln in lines] == res.n_obs.tolist()
    # the command line writes the same files
    assert dp.main(["logistic", "--bfile", prefix, "--out", prefix + ".cli", "--pheno", pheno, "--covar", prefix + ".eigenvec"]) == 0
    for name in ("asthma", "t2d"):
        assert open(f"{prefix}.cli.{name}.glm.logistic").read() == open(f"{prefix}.api.{name}.glm.logistic").read()
    assert dp.main(["logistic", "--bfile", prefix, "--out", prefix + ".one", "--pheno", pheno, "--pheno-name", "t2d",
                    "--covar", prefix + ".eigenvec", "--covar-name", "PC1,PC2", "--vif", "20"]) == 0
    one = dp.bfile_logistic(prefix, pheno, covar=prefix + ".eigenvec", pheno_names=["t2d"], covar_names=["PC1", "PC2"], max_vif=20.0)
    assert len(one) == 1 and one[0].result.design.n_cov == 2
    _, lines = read_table(prefix + ".one.t2d.glm.logistic")
    assert [float(ln[11]) for ln in lines if ln[11] != "NA"] == one[0].result.p.cpu().numpy()[one[0].result.flags.cpu().numpy()[:, 0] == 0, 0].tolist()
    # the clump subcommand reads the .glm.logistic file as it stands
    clump = ["--clump-p1", "1e-3", "--clump-p2", "0.05", "--clump-r2", "0.3", "--clump-kb", "1"]
    for table in tables:
        name = table.names[0]
        assert dp.main(["clump", "--bfile", prefix, "--out", f"{prefix}.{name}", "--clump", f"{prefix}.api.{name}.glm.logistic",
                        "--clump-snp-field", "ID", "--clump-field", "P", *clump]) == 0
        with open(f"{prefix}.{name}.clumped") as f:
            index = [ln.split()[2] for ln in f.read().splitlines()[1:] if ln.strip()]
        want = dp.bfile_clump(prefix, table.result.p.cpu().numpy()[:, 0], p1=1e-3, p2=0.05, r2=0.3, window_bp=1000)
        assert index == [ids[k] for k, _ in want.clumps.clumps()] and len(index) >= 1
    assert "rs10" in open(f"{prefix}.asthma.clumped").read() and "rs61" in open(f"{prefix}.t2d.clumped").read()


def test_other_codings_are_refused_and_glm_points_here(study):
    from ld_tools_amd import LdxError
    from ld_tools_amd.drivers import plink as dp

    prefix, codes, ids, _, Y, _ = study
    bf = dp.load_bfile(prefix)
    height = np.random.default_rng(1).standard_normal(N_SAMPLES)
    for values in (height, Y[:, 0] * 2.0, Y[:, 0] + 2.0):
        with pytest.raises(LdxError, match="case/control"):
            dp.bfile_logistic(bf, (bf.fid, bf.iid, ["x"], values[:, None]))
    with pytest.raises(LdxError, match="bfile_logistic"):
        dp.bfile_glm(bf, (bf.fid, bf.iid, ["cc"], Y[:, :1].astype(np.float64)))
    with pytest.raises(LdxError, match="no phenotype named"):
        dp.bfile_logistic(bf, (bf.fid, bf.iid, ["cc"], Y[:, :1].astype(np.float64)), pheno_names=["bmi"])
    with pytest.raises(LdxError, match="covariates are more than 13"):
        dp.bfile_logistic(bf, (bf.fid, bf.iid, ["cc"], Y[:, :1].astype(np.float64)),
                          covar=(bf.fid, bf.iid, [f"c{k}" for k in range(14)], np.random.default_rng(2).standard_normal((N_SAMPLES, 14))))
    tables = dp.bfile_logistic(bf, (bf.fid, bf.iid, ["cc"], Y[:, :1].astype(np.float64)))
    assert [t.names for t in tables] == [["cc"]] and tables[0].result.design.n_cov == 0

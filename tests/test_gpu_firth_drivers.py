"""GPU: drivers/plink.py's bfile_logistic(firth=) and the ``logistic --firth`` subcommand on a small written fileset whose odd
variants are rare and carried by cases alone (no finite maximum-likelihood fit): the .glm.logistic.hybrid and .glm.firth files,
their columns, a FIRTH? = Y line carrying the Firth numbers, OR = exp(beta); both files are then fed to the ``clump`` subcommand as
they stand."""
import math

import numpy as np
import pytest

import ld_firth_exact as F
from ld_tools_amd import FIRTH_MODES, ld_glm_logistic  # noqa: F401  (the feature under test)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def study(gpu, tmp_path_factory):
    from ld_tools_amd import plink

    codes, Y, C = F.rare_panel(n_ind=120, n_snps=40, n_cov=2)
    codes[:, 1::2][(codes[:, 0::2] == 2)] = 2                      # a .bed has no half-missing genotype
    codes[:, 0::2][(codes[:, 1::2] == 2)] = 2
    codes = plink.canonical_codes(codes)
    n_snps, n_ind = codes.shape[0], codes.shape[1] // 2
    prefix = str(tmp_path_factory.mktemp("firth") / "study")
    fid, iid = [f"FAM{s // 2}" for s in range(n_ind)], [f"ID{s:03d}" for s in range(n_ind)]
    ids = [f"rs{v}" for v in range(n_snps)]
    bim = {"chrom": ["5"] * n_snps, "ids": ids, "pos": [1000 + 100 * v for v in range(n_snps)], "a1": ["G"] * n_snps, "a2": ["A"] * n_snps}
    plink.write_bfile(prefix, plink.codes_bed_host(codes, alt="a1"), bim, {"fid": fid, "iid": iid})
    pheno, covar = prefix + ".pheno", prefix + ".covar"
    with open(pheno, "w") as f:
        f.write("#FID IID cc\n" + "".join(f"{fid[s]} {iid[s]} {int(Y[s, 0]) + 1}\n" for s in range(n_ind)))
    with open(covar, "w") as f:
        f.write("#FID IID C1 C2\n" + "".join(f"{fid[s]} {iid[s]} {float(C[s, 0])!r} {float(C[s, 1])!r}\n" for s in range(n_ind)))
    return prefix, codes, ids, pheno, covar, Y[:, 0], C


def read_table(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        return head, [line.rstrip("\n").split("\t") for line in f]


def test_hybrid_and_firth_files_and_clump(study):
    from ld_tools_amd import ld_glm_logistic_host
    from ld_tools_amd.drivers import plink as dp
    from ld_tools_amd.drivers.glm import HYBRID_COLUMNS, LOGISTIC_COLUMNS

    prefix, codes, ids, pheno, covar, y, C = study
    tables = dp.bfile_logistic(prefix, pheno, covar=covar, out=prefix + ".api", firth="fallback")
    assert [t.names for t in tables] == [["cc"]]
    res = tables[0].result
    flags, mark = res.flags.cpu().numpy()[:, 0], res.firth.cpu().numpy()[:, 0]
    beta, se, p = (getattr(res, k).cpu().numpy()[:, 0] for k in ("beta", "se", "p"))
    ref = ld_glm_logistic_host(codes, y, C, firth="fallback")
    assert np.array_equal(flags, ref.flags.numpy()[:, 0]) and np.array_equal(mark, ref.firth.numpy()[:, 0])
    assert mark[1::2].all() and mark.sum() >= 10 and (flags == 0).all()              # every rare variant is refitted, none is lost
    assert (np.abs(beta - ref.beta.numpy()[:, 0]) <= 2.0 ** -39 * se).all()
    head, lines = read_table(prefix + ".api.cc.glm.logistic.hybrid")
    assert tuple(head) == HYBRID_COLUMNS and head[6] == "FIRTH?" and [ln[2] for ln in lines] == ids
    assert [ln[6] for ln in lines] == ["Y" if m else "N" for m in mark] and all(ln[7] == "ADD" and ln[13] == "." for ln in lines)
    assert [float(ln[9]) for ln in lines] == [math.exp(b) for b in beta] and [float(ln[10]) for ln in lines] == se.tolist()
    assert [float(ln[12]) for ln in lines] == p.tolist() and [int(ln[8]) for ln in lines] == res.n_obs.tolist()
    # a refitted line carries the Firth numbers: those of the scan that fits every variant that way
    every = dp.bfile_logistic(prefix, pheno, covar=covar, firth="always")[0].result
    k = int(np.flatnonzero(mark)[0])
    assert float(lines[k][9]) == math.exp(float(every.beta[k, 0])) and float(lines[k][10]) == float(every.se[k, 0])
    # without firth= the same variants have no numbers
    plain = dp.bfile_logistic(prefix, pheno, covar=covar, out=prefix + ".api")[0].result
    assert plain.firth is None and (plain.flags.cpu().numpy()[mark == 1, 0] == 5).all()
    assert [ln[12] for ln in read_table(prefix + ".api.cc.glm.logistic")[1]][k] == "NO_FINITE_MAXIMISER"
    # the command line: --firth always writes .glm.firth, --firth fallback the same hybrid file
    assert dp.main(["logistic", "--bfile", prefix, "--out", prefix + ".cli", "--pheno", pheno, "--covar", covar, "--firth", "always"]) == 0
    head, flines = read_table(prefix + ".cli.cc.glm.firth")
    assert tuple(head) == LOGISTIC_COLUMNS and [ln[2] for ln in flines] == ids and all(ln[12] == "." for ln in flines)
    assert [float(ln[8]) for ln in flines] == [math.exp(b) for b in every.beta.cpu().numpy()[:, 0]]
    assert [float(ln[9]) for ln in flines] == every.se.cpu().numpy()[:, 0].tolist()
    assert dp.main(["logistic", "--bfile", prefix, "--out", prefix + ".cli", "--pheno", pheno, "--covar", covar, "--firth", "fallback"]) == 0
    assert open(prefix + ".cli.cc.glm.logistic.hybrid").read() == open(prefix + ".api.cc.glm.logistic.hybrid").read()
    # the clump subcommand reads both files as they stand
    clump = ["--clump-p1", "0.2", "--clump-p2", "0.5", "--clump-r2", "0.3", "--clump-kb", "1"]
    for path, pv in ((prefix + ".api.cc.glm.logistic.hybrid", p), (prefix + ".cli.cc.glm.firth", every.p.cpu().numpy()[:, 0])):
        assert dp.main(["clump", "--bfile", prefix, "--out", path, "--clump", path, "--clump-snp-field", "ID", "--clump-field", "P",
                        *clump]) == 0
        with open(path + ".clumped") as f:
            index = [ln.split()[2] for ln in f.read().splitlines()[1:] if ln.strip()]
        want = dp.bfile_clump(prefix, pv, p1=0.2, p2=0.5, r2=0.3, window_bp=1000)
        assert index == [ids[v] for v, _ in want.clumps.clumps()] and len(index) >= 1

"""GPU: the QC drivers and subcommands (ld_tools_amd/drivers/qc.py, drivers/plink.py: hardy, missing, het, model, qc) on a
synthetic fileset of 200 individuals x 300 variants written by make_bed: the parsed columns of every file equal the operators'
results on the same panel, the qc masks go to bfile_prune and bfile_king, and clump reads the .assoc.fisher."""
import numpy as np
import pytest

import ld_qc_exact as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_IND, N_SNPS, CHROM = 200, 300, "6"


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def study(gpu, tmp_path_factory):
    """(prefix, phenotype path, loaded fileset, case vector): whole genotypes missing only, as a .bed holds them."""
    from ld_tools_amd import PackedPanel
    from ld_tools_amd.drivers import plink as shell

    codes = X.qc_codes(N_IND, N_SNPS, seed=12)
    rng = np.random.default_rng(4)
    gone = rng.random((N_SNPS, N_IND)) < 0.03
    gone[:, 7] |= rng.random(N_SNPS) < 0.3                     # an individual --mind drops
    gone[11] |= rng.random(N_IND) < 0.4                        # a variant --geno drops
    codes[np.repeat(gone, 2, axis=1)] = 2
    root = tmp_path_factory.mktemp("qc")
    prefix = str(root / "study")
    bim = {"chrom": [CHROM] * N_SNPS, "ids": [f"rs{100 + k}" for k in range(N_SNPS)], "pos": [1000 + 37 * k for k in range(N_SNPS)],
           "a1": ["G"] * N_SNPS, "a2": ["A"] * N_SNPS}
    fam = {"fid": [f"F{k // 3}" for k in range(N_IND)], "iid": [f"I{k}" for k in range(N_IND)]}
    shell.make_bed(prefix, PackedPanel.from_codes(codes, device=gpu), bim=bim, fam=fam)
    case = X.case_vector(N_IND, seed=8)
    pheno = root / "study.pheno"
    pheno.write_text("#FID IID CC QT\n" + "".join(
        f"{f} {i} {'NA' if np.isnan(c) else int(c) + 1} {0.1 * k:.1f}\n" for k, (f, i, c) in enumerate(zip(fam["fid"], fam["iid"], case))))
    return prefix, str(pheno), shell.load_bfile(prefix), case


def table(path, sep="\t"):
    lines = [ln.split(sep) if sep else ln.split() for ln in open(path).read().splitlines()]
    return lines[0], lines[1:]


def num(cells):
    return np.array([np.nan if c == "NA" else float(c) for c in cells])


def u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def test_hardy_subcommand(study, tmp_path):
    from ld_tools_amd import ld_hardy
    from ld_tools_amd.drivers import plink as shell, qc as W

    prefix, _, bf, _ = study
    out = str(tmp_path / "o")
    assert shell.main(["hardy", "--bfile", prefix, "--out", out, "--midp"]) == 0
    head, rows = table(out + ".hardy")
    res = ld_hardy(bf.panel, midp=True)
    c = u32(res.counts)[:, 0]
    assert tuple(head) == W.HARDY_COLUMNS and len(rows) == N_SNPS
    assert [r[1] for r in rows] == bf.ids and {r[2] for r in rows} == {"G"} and {r[3] for r in rows} == {"A"}
    assert np.array_equal(np.array([[int(v) for v in r[4:7]] for r in rows]), np.stack([c[:, 2], c[:, 1], c[:, 0] - c[:, 1] - c[:, 2]], axis=1))
    for col, want in ((7, res.o_het), (8, res.e_het), (9, res.p)):
        assert np.array_equal(num([r[col] for r in rows]), want[:, 0].cpu().numpy(), equal_nan=True)
    assert rows[7][7:] == ["NA", "NA", "NA"] and rows[3][9] == "1.0"          # no call; monomorphic


def test_missing_and_het_subcommands(study, tmp_path):
    from ld_tools_amd import geno_snp_counts, ld_test_missing, sample_qc
    from ld_tools_amd.drivers import plink as shell, qc as W

    prefix, pheno, bf, case = study
    out = str(tmp_path / "o")
    assert shell.main(["missing", "--bfile", prefix, "--out", out, "--pheno", pheno, "--pheno-name", "CC"]) == 0
    assert shell.main(["het", "--bfile", prefix, "--out", out]) == 0
    called, qc, tm = u32(geno_snp_counts(bf.panel))[:, 0], sample_qc(bf.panel), ld_test_missing(bf.panel, case)
    head, rows = table(out + ".vmiss")
    assert tuple(head) == W.VMISS_COLUMNS and [int(r[2]) for r in rows] == (N_IND - called).tolist()
    assert {r[3] for r in rows} == {str(N_IND)} and np.array_equal(num([r[4] for r in rows]), (N_IND - called) / N_IND)
    head, rows = table(out + ".smiss")
    assert tuple(head) == W.SMISS_COLUMNS and [(r[0], r[1]) for r in rows] == list(zip(bf.fid, bf.iid))
    assert [int(r[2]) for r in rows] == (N_SNPS - qc.called).tolist() and np.array_equal(num([r[4] for r in rows]), qc.f_miss)
    head, rows = table(out + ".missing")
    assert tuple(head) == W.TEST_MISSING_COLUMNS
    for col, want in ((2, tm.f_miss_case), (3, tm.f_miss_ctrl), (4, tm.p)):
        assert np.array_equal(num([r[col] for r in rows]), want.cpu().numpy(), equal_nan=True)
    assert float(rows[11][4]) < 1.0
    head, rows = table(out + ".het")
    assert tuple(head) == W.HET_COLUMNS and [int(r[2]) for r in rows] == (qc.called - qc.het).tolist()
    assert np.array_equal(num([r[3] for r in rows]), qc.e_hom) and [int(r[4]) for r in rows] == qc.called.tolist()
    assert np.array_equal(num([r[5] for r in rows]), qc.f, equal_nan=True)


def test_model_subcommand_and_clump(study, tmp_path):
    from ld_tools_amd import MODEL_TESTS, LdxError, ld_model
    from ld_tools_amd.drivers import plink as shell, qc as W

    prefix, pheno, bf, case = study
    out = str(tmp_path / "o")
    assert shell.main(["model", "--bfile", prefix, "--out", out, "--pheno", pheno, "--pheno-name", "CC", "--cell", "3"]) == 0
    res = ld_model(bf.panel, case, min_cell=3)
    head, rows = table(out + ".model")
    assert tuple(head) == W.MODEL_COLUMNS and len(rows) == 5 * N_SNPS
    chisq, p, flags = res.chisq.cpu().numpy(), res.p.cpu().numpy(), res.flags.cpu().numpy()
    cells = W.model_cells(res.case_counts, res.ctrl_counts)
    for j, test in enumerate(W.MODEL_ORDER):
        t, part = MODEL_TESTS.index(test), rows[j::5]
        assert {r[4] for r in part} == {test} and [r[1] for r in part] == bf.ids
        assert [r[5] for r in part] == cells[test][0] and [r[6] for r in part] == cells[test][1]
        assert np.array_equal(num([r[7] for r in part]), chisq[:, t], equal_nan=True)
        assert np.array_equal(num([r[9] for r in part]), p[:, t], equal_nan=True)
        assert [r[8] for r in part] == ["NA" if f else str(W.MODEL_DF[test]) for f in flags[:, t]]
    assert set(np.unique(flags).tolist()) >= {0, 1, 2} and (flags[:, 2] == 3).any()
    head, rows = table(out + ".assoc.fisher")
    assert tuple(head) == W.FISHER_COLUMNS and [r[1] for r in rows] == bf.ids and [int(r[2]) for r in rows] == bf.pos.tolist()
    assert np.array_equal(num([r[7] for r in rows]), res.fisher_p.cpu().numpy(), equal_nan=True)
    odds = res.odds.cpu().numpy()
    assert np.array_equal(num([r[8] for r in rows]), odds, equal_nan=True)
    # clump reads the file; a variant without a test has no p there
    assert shell.main(["clump", "--bfile", prefix, "--out", out, "--clump", out + ".assoc.fisher", "--clump-snp-field", "SNP",
                       "--clump-field", "P", "--clump-p1", "0.05", "--clump-p2", "0.5"]) == 0
    fp = res.fisher_p.cpu().numpy()
    lines = open(out + ".clumped").read().splitlines()
    index = [ln.split()[2] for ln in lines[1:] if ln.split()]
    assert index and set(index) <= {i for i, v in zip(bf.ids, fp) if v <= 0.05}
    with pytest.raises(LdxError, match="bfile_glm"):
        shell.bfile_model(bf, pheno, pheno_name="QT")


def test_qc_subcommand_and_its_masks(study, tmp_path):
    from ld_tools_amd import sample_qc_mask, snp_qc_mask
    from ld_tools_amd.drivers import plink as shell

    prefix, pheno, bf, case = study
    out = str(tmp_path / "o")
    argv = ["qc", "--bfile", prefix, "--out", out, "--geno", "0.1", "--maf", "0.15", "--hwe", "0.001", "--mind", "0.1", "--pheno", pheno,
            "--pheno-name", "CC"]
    assert shell.main(argv) == 0
    ind = sample_qc_mask(bf.panel, mind_max=0.1)
    assert not ind[7] and ind.sum() >= N_IND - 3
    rows = np.flatnonzero(ind)
    sub = bf.panel.select(haplotypes=np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1))
    snps = snp_qc_mask(sub, maf_min=0.15, geno_max=0.1, hwe_min=0.001, hwe_group=case[ind] == 0.0).cpu().numpy().astype(bool)
    assert not snps[[3, 5, 7, 11]].any() and 50 < snps.sum() < N_SNPS
    assert open(out + ".qc.in").read().split() == [i for i, o in zip(bf.ids, snps) if o]
    assert open(out + ".qc.out").read().split() == [i for i, o in zip(bf.ids, snps) if not o]
    assert [tuple(ln.split()) for ln in open(out + ".qc.keep")] == [(f, i) for f, i, o in zip(bf.fid, bf.iid, ind) if o]
    masks = shell.bfile_qc(bf, geno=0.1, maf=0.15, hwe=0.001, mind=0.1, pheno=pheno, pheno_name="CC")
    assert np.array_equal(masks.extract, snps) and np.array_equal(masks.individuals, ind) and masks.snps.dtype == torch.uint8
    pruned = shell.bfile_prune(prefix, r2=0.5, window_bp=2000, missing="pairwise", extract=masks.extract, keep=masks.individuals)
    assert pruned.rs_ids == [i for i, o in zip(bf.ids, snps) if o] and 0 < int(pruned.pruned.keep.sum()) <= snps.sum()
    king = shell.bfile_king(prefix, keep=masks.individuals, extract=masks.extract)
    assert king.counts.n_ind == int(ind.sum()) and king.counts.n_snps == int(snps.sum())
    from ld_tools_amd import sample_counts
    direct = sample_counts(sub, keep=masks.snps)            # the device mask as an operator's keep=
    assert torch.equal(direct.counts, king.counts.counts)

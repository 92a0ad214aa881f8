"""The PLINK-fileset drivers (ld_tools_amd/drivers/plink.py) against the VCF drivers on the same genotypes: what the existing
writers write from a ``bfile_*`` table is byte-identical to what they write from the VCF driver's.

The genotypes: 60 variants x 40 diploid samples with LD blocks, phased calls (hets in both orders) and about 3 % missing
calls, whole genotypes only (a .bed has no half-missing call).  The fileset is written with A1 = the VCF's ALT allele and
read with alt="a1", so code 1 means the same allele on both sides."""
import gzip
from pathlib import Path

import numpy as np
import pytest

from fakevcf import FakeRecord, FakeVcf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHROM, N_VAR, N_SAMPLES = "6", 60, 40


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def study(gpu, tmp_path_factory):
    """(vcf, sample names, VCF rows, fileset prefix, codes, p-values)."""
    from ld_tools_amd import plink, synth

    codes = synth.synth_codes_host(N_VAR, 2 * N_SAMPLES, seed=5).astype(np.int8)
    rng = np.random.default_rng(8)
    gone = rng.random((N_VAR, N_SAMPLES)) < 0.03
    gone[3, :4] = True
    codes[np.repeat(gone, 2, axis=1)] = 2
    names = [f"HG{200 + s:05d}" for s in range(N_SAMPLES)]
    poss = [5000 + 211 * v + (v % 5) * 13 for v in range(N_VAR)]
    ids = [f"rs{7000 + v}" for v in range(N_VAR)]
    records = []
    for v in range(N_VAR):
        samples = {name: {"GT": tuple(None if c == 2 else int(c) for c in codes[v, 2 * s:2 * s + 2])}
                   for s, name in enumerate(names)}
        records.append(FakeRecord(CHROM, poss[v], ids[v], "A", ("G",), {"VT": ("SNP",)}, samples))
    prefix = str(tmp_path_factory.mktemp("bfile") / "study")
    bim = {"chrom": [CHROM] * N_VAR, "ids": ids, "pos": poss, "a1": ["G"] * N_VAR, "a2": ["A"] * N_VAR}    # A1 = ALT
    fam = {"fid": [f"FAM{s // 4}" for s in range(N_SAMPLES)], "iid": names, "sex": [str(1 + s % 2) for s in range(N_SAMPLES)]}
    plink.write_bfile(prefix, plink.codes_bed_host(codes, alt="a1"), bim, fam)
    pvalues = 10.0 ** -rng.uniform(0, 8, size=N_VAR)
    return FakeVcf(records), names, [[poss[v], ids[v]] for v in range(N_VAR)], prefix, codes, pvalues


def read(path):
    path = str(path)
    return gzip.open(path, "rb").read() if path.endswith(".gz") else Path(path).read_bytes()


def test_ld_table_matches_the_vcf_driver(study, tmp_path):
    from ld_tools_amd import drivers

    vcf, names, rows, prefix, _, _ = study
    for missing in (None, "pairwise"):
        side, hits = drivers.em_window_hits(vcf, CHROM, rows, names, r2=0.1, window_bp=4000, missing=missing)
        n_vcf = drivers.write_ld_table(str(tmp_path / "vcf.ld"), side, side, hits)
        bside, bhits = drivers.bfile_ld_table(prefix, r2=0.1, window_bp=4000, missing=missing)
        n_bed = drivers.write_ld_table(str(tmp_path / "bed.ld"), bside, bside, bhits)
        assert n_vcf == n_bed > 10
        assert read(tmp_path / "vcf.ld") == read(tmp_path / "bed.ld")
        assert bside.poss == side.poss and bside.alt_freqs == side.alt_freqs


def test_clump_matches_the_vcf_driver(study, tmp_path):
    from ld_tools_amd import drivers

    vcf, names, rows, prefix, _, p = study
    kw = dict(p1=1e-3, p2=0.05, r2=0.2, window_bp=5000, em=True, missing="pairwise")
    a = drivers.clump(vcf, CHROM, rows, names, p, **kw)
    b = drivers.bfile_clump(prefix, p, **kw)
    drivers.write_clumped(str(tmp_path / "vcf.clumped"), a)
    drivers.write_clumped(str(tmp_path / "bed.clumped"), b)
    assert read(tmp_path / "vcf.clumped") == read(tmp_path / "bed.clumped")
    assert len(a.clumps.index) >= 2 and any(m.size for _, m in a.clumps.clumps())
    default = drivers.bfile_clump(prefix, p, p1=1e-3, p2=0.05, r2=0.2, window_bp=5000)       # the default form is the EM r
    assert np.array_equal(default.clumps.owner, drivers.clump(vcf, CHROM, rows, names, p, p1=1e-3, p2=0.05, r2=0.2,
                                                              window_bp=5000, em=True).clumps.owner)


def test_prune_matches_the_vcf_driver(study, tmp_path):
    from ld_tools_amd import drivers

    vcf, names, rows, prefix, _, _ = study
    a = drivers.prune(vcf, CHROM, rows, names, r2=0.2, window_bp=5000, dosage=True)
    b = drivers.bfile_prune(prefix, r2=0.2, window_bp=5000, dosage=True)
    pa, pb = drivers.write_prune(str(tmp_path / "vcf"), a), drivers.write_prune(str(tmp_path / "bed"), b)
    for x, y in zip(pa, pb):
        assert read(x) == read(y)
    assert 0 < int(a.pruned.keep.sum()) < N_VAR
    assert np.array_equal(drivers.bfile_prune(prefix, r2=0.2, window_bp=5000).pruned.keep, a.pruned.keep)   # default: dosage


def test_ld_scores_match_the_vcf_driver(study, tmp_path):
    from ld_tools_amd import LdxError, drivers

    vcf, names, rows, prefix, _, _ = study
    annot = (np.arange(N_VAR)[:, None] % np.array([2, 3])) == 0
    for missing in ("pairwise", "ref"):
        a = drivers.ld_scores(vcf, CHROM, rows, names, window_bp=6000, annot=annot, annot_names=["even", "third"], dosage=True,
                              missing=missing)
        b = drivers.bfile_ld_scores(prefix, window_bp=6000, annot=annot, annot_names=["even", "third"], dosage=True,
                                    missing=missing)
        pa, pb = drivers.write_ldscore(str(tmp_path / "vcf"), a), drivers.write_ldscore(str(tmp_path / "bed"), b)
        for x, y in zip(pa, pb):
            assert read(x) == read(y), (missing, x)
        assert len(read(pa[0]).splitlines()) > N_VAR // 2
    with pytest.raises(LdxError, match="missing"):                        # the panel has missing calls: say how to count them
        drivers.bfile_ld_scores(prefix, window_bp=6000)


def test_bands_match_the_vcf_drivers(study):
    from ld_tools_amd import drivers

    vcf, names, rows, prefix, _, _ = study
    a = drivers.band_matrix(vcf, CHROM, rows, names, window_bp=4000, dosage=True, missing="pairwise")
    b = drivers.bfile_band(prefix, window_bp=4000, missing="pairwise")
    assert torch.equal(a.band.values.view(torch.int32), b.band.values.view(torch.int32)) and a.band.n_cells > 0
    assert (b.refs, b.alts, b.alt_freqs, b.poss, b.rs_ids) == (a.refs, a.alts, a.alt_freqs, a.poss, a.rs_ids)
    ea = drivers.em_band(vcf, CHROM, rows, names, window_bp=4000, missing="pairwise")
    eb = drivers.bfile_em_band(prefix, window_bp=4000, missing="pairwise")
    assert torch.equal(ea.bands.r.values.view(torch.int32), eb.bands.r.values.view(torch.int32))
    assert torch.equal(ea.bands.dprime.values.view(torch.int32), eb.bands.dprime.values.view(torch.int32))
    assert eb.alt_freqs == ea.alt_freqs


def test_filters_select_what_the_host_selects(study):
    from ld_tools_amd import LdxError, PackedPanel, drivers, plink

    _, names, _, prefix, codes, _ = study
    bed = plink.BedFile(prefix)
    host = plink.bed_codes_host(bed.rows, bed.n_ind)
    assert np.array_equal(host, plink.canonical_codes(codes))
    # keep by (FID, IID), extract by ID: in the caller's order
    pairs = [(bed.fid[k], bed.iid[k]) for k in (31, 2, 17, 5, 6, 7, 38, 11, 12, 20, 21, 22)]
    wanted = [bed.ids[k] for k in range(0, N_VAR, 2)]
    bf = drivers.load_bfile(prefix, keep=pairs, extract=wanted)
    ki = np.array([31, 2, 17, 5, 6, 7, 38, 11, 12, 20, 21, 22])
    sub = host.reshape(N_VAR, N_SAMPLES, 2)[::2][:, ki].reshape(N_VAR // 2, -1)
    want = PackedPanel.from_codes(sub, bf.panel.device)
    assert torch.equal(bf.panel.alt, want.alt) and torch.equal(bf.panel.ref, want.ref) and torch.equal(bf.panel.acnt, want.acnt)
    assert bf.ids == wanted and bf.iid == [p[1] for p in pairs] and bf.fid == [p[0] for p in pairs]
    assert bf.pos.tolist() == bed.pos[::2].tolist() and bf.sex == [bed.sex[k] for k in ki]
    # --maf / --geno over the kept individuals, from the host codes
    ki2 = np.arange(5, 35)
    sub = host.reshape(N_VAR, N_SAMPLES, 2)[:, ki2].reshape(N_VAR, -1)
    a, r = (sub == 1).sum(1), (sub == 0).sum(1)
    maf_min, geno_max = 0.2, 0.04
    ok = (np.minimum(a, r) >= maf_min * (a + r)) & ((a + r) > 0) & ((sub.shape[1] - a - r) <= geno_max * sub.shape[1])
    assert 0 < ok.sum() < N_VAR and ((sub.shape[1] - a - r) > geno_max * sub.shape[1]).any()
    bf = drivers.load_bfile(prefix, chrom=CHROM, keep=ki2, maf_min=maf_min, geno_max=geno_max)
    assert bf.ids == [bed.ids[k] for k in np.flatnonzero(ok)] and bf.iid == [names[k] for k in ki2]
    want = PackedPanel.from_codes(sub[ok], bf.panel.device)
    for f in ("alt", "ref", "acnt", "rcnt", "fa", "fr", "q"):
        assert torch.equal(getattr(bf.panel, f), getattr(want, f)), f
    # the other allele as ALT: the complement panel
    other = drivers.load_bfile(prefix, alt="a2")
    assert other.alts == bed.a2 and other.refs == bed.a1
    assert torch.equal(other.panel.acnt, drivers.load_bfile(prefix).panel.rcnt)
    for bad in (dict(keep=[("FAM0", "nobody")]), dict(extract=["rs1"]), dict(chrom="7"), dict(extract=[N_VAR]),
                dict(keep=np.zeros(N_SAMPLES, dtype=bool)), dict(maf_min=0.6), dict(alt="ref")):
        with pytest.raises(LdxError):
            drivers.load_bfile(prefix, **bad)


def test_make_bed_of_a_pruned_set_reopens(study, tmp_path):
    from ld_tools_amd import PackedPanel, drivers, plink

    _, names, _, prefix, codes, _ = study
    bf = drivers.load_bfile(prefix)
    keep = drivers.bfile_prune(bf, r2=0.2, window_bp=5000).pruned.keep
    inds = np.arange(3, 40, 2)
    out = str(tmp_path / "pruned")
    paths = drivers.make_bed(out, bf, snps=keep, individuals=inds)
    assert [Path(p).suffix for p in paths] == [".bed", ".bim", ".fam"]
    again = plink.BedFile(out)
    assert again.ids == [bf.ids[k] for k in np.flatnonzero(keep)] and again.iid == [names[k] for k in inds]
    assert again.pos.tolist() == bf.pos[keep].tolist() and again.a1 == ["G"] * int(keep.sum()) and again.chrom == [CHROM] * int(keep.sum())
    want = plink.canonical_codes(codes).reshape(N_VAR, N_SAMPLES, 2)[keep][:, inds].reshape(int(keep.sum()), -1)
    assert np.array_equal(plink.bed_codes_host(again.rows, again.n_ind), want)
    reopened = drivers.load_bfile(out)
    ref = PackedPanel.from_codes(want, reopened.panel.device)
    assert torch.equal(reopened.panel.alt, ref.alt) and torch.equal(reopened.panel.ref, ref.ref)
    # a bare panel with its columns, written with the other allele as code 1: A2's homozygotes become A1's
    paths = drivers.make_bed(str(tmp_path / "bare"), ref, bim=again.bim(), fam=again.fam(), alt="a2")
    assert np.array_equal(plink.bed_codes_host(plink.BedFile(paths[0]).rows, again.n_ind, alt="a2"), want)


def test_the_haplotype_r_is_refused(study):
    from ld_tools_amd import LdxError, drivers

    _, _, _, prefix, _, p = study
    bf = drivers.load_bfile(prefix)
    for call in (lambda: drivers.bfile_clump(bf, p, dosage=False, em=False),
                 lambda: drivers.bfile_prune(bf, dosage=False, em=False),
                 lambda: drivers.bfile_ld_scores(bf, dosage=False, em=False, missing="pairwise"),
                 lambda: drivers.bfile_band(bf, dosage=False, em=False, missing="pairwise"),
                 lambda: drivers.bfile_em_band(bf, dosage=False, em=False),
                 lambda: drivers.bfile_ld_table(bf, dosage=False, em=False)):
        with pytest.raises(LdxError, match="no phase"):
            call()
    with pytest.raises(LdxError):
        drivers.bfile_clump(bf, p, dosage=True, em=True)


def test_command_line_writes_what_the_drivers_write(study, tmp_path):
    from ld_tools_amd import drivers, plink
    from ld_tools_amd.drivers import plink as shell

    _, names, rows, prefix, _, p = study
    out, ref = str(tmp_path / "cli"), str(tmp_path / "ref")
    common = ["--bfile", prefix, "--out", out]
    assert shell.main(["prune", *common, "--r2", "0.2", "--window-kb", "5"]) == 0
    want = drivers.write_prune(ref, drivers.bfile_prune(prefix, r2=0.2, window_bp=5000))
    assert read(out + ".prune.in") == read(want[0]) and read(out + ".prune.out") == read(want[1])
    assoc = tmp_path / "assoc.txt"
    assoc.write_text("CHR SNP P\n" + "".join(f"{CHROM} {rs} {v!r}\n" for (_, rs), v in zip(rows, p.tolist())))
    assert shell.main(["clump", *common, "--clump", str(assoc), "--clump-p1", "1e-3", "--clump-p2", "0.05", "--clump-r2", "0.2",
                       "--clump-kb", "5", "--missing", "pairwise"]) == 0
    drivers.write_clumped(ref + ".clumped", drivers.bfile_clump(prefix, p, p1=1e-3, p2=0.05, r2=0.2, window_bp=5000,
                                                                 missing="pairwise"))
    assert read(out + ".clumped") == read(ref + ".clumped")
    assert shell.main(["ld", *common, "--ld-window-kb", "4", "--ld-window-r2", "0.1", "--missing", "pairwise"]) == 0
    side, hits = drivers.bfile_ld_table(prefix, r2=0.1, window_bp=4000, missing="pairwise")
    drivers.write_ld_table(ref + ".ld", side, side, hits)
    assert read(out + ".ld") == read(ref + ".ld")
    assert shell.main(["l2", *common, "--ld-wind-kb", "6", "--missing", "pairwise"]) == 0
    want = drivers.write_ldscore(ref, drivers.bfile_ld_scores(prefix, window_bp=6000, missing="pairwise"))
    for x in want:
        assert read(out + x[len(ref):]) == read(x)
    keep, extract = tmp_path / "keep.txt", tmp_path / "extract.txt"
    bed = plink.BedFile(prefix)
    keep.write_text("".join(f"{bed.fid[k]} {bed.iid[k]}\n" for k in (4, 0, 9)))
    extract.write_text("".join(f"{bed.ids[k]}\n" for k in (2, 3, 50)))
    assert shell.main(["make-bed", *common, "--chr", CHROM, "--keep", str(keep), "--extract", str(extract)]) == 0
    small = plink.BedFile(out)
    assert small.iid == [names[k] for k in (4, 0, 9)] and small.ids == [bed.ids[k] for k in (2, 3, 50)]
    full = plink.bed_codes_host(bed.rows, bed.n_ind).reshape(N_VAR, N_SAMPLES, 2)
    assert np.array_equal(plink.bed_codes_host(small.rows, 3), full[[2, 3, 50]][:, [4, 0, 9]].reshape(3, -1))

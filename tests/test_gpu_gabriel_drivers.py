"""GPU: the Gabriel block drivers -- drivers.bfile_blocks and the ``blocks`` subcommand of ld_tools_amd.drivers.plink on a small
fileset written with write_bfile, drivers.gabriel_blocks on the same genotypes as a VCF, and write_gabriel_blocks.  The rows of
``.blocks.det`` are composed here from the host mirrors (ops.gabriel_candidates_host, ops.gabriel_pick_host) fed the device's
own bound bytes; members exclude the SNPs that are not kept."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_gabriel_cases as gc  # noqa: E402
from fakevcf import FakeRecord, FakeVcf  # noqa: E402

pytestmark = pytest.mark.gpu

CHROM, N_VAR, N_HAP = "7", 129, 254


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def study(gpu, tmp_path_factory):
    """(fileset prefix, codes, positions, ids, planted, vcf, sample names, VCF rows): gabriel_panel's first 129 SNPs with
    whole genotypes missing (a .bed has no half-missing call)."""
    from ld_tools_amd import plink

    codes, pos, where = gc.gabriel_panel(N_HAP, n=N_VAR)
    codes = np.array(codes)
    gone = (codes.reshape(N_VAR, -1, 2) == 2).any(axis=2)
    codes[np.repeat(gone, 2, axis=1)] = 2
    ids = [f"rs{9000 + v}" for v in range(N_VAR)]
    names = [f"NA{100 + s:05d}" for s in range(N_HAP // 2)]
    prefix = str(tmp_path_factory.mktemp("gabriel") / "study")
    bim = {"chrom": [CHROM] * N_VAR, "ids": ids, "pos": [int(p) for p in pos], "a1": ["G"] * N_VAR, "a2": ["A"] * N_VAR}
    fam = {"fid": names, "iid": names, "sex": ["1"] * len(names)}
    plink.write_bfile(prefix, plink.codes_bed_host(codes, alt="a1"), bim, fam)
    records = []
    for v in range(N_VAR):
        samples = {name: {"GT": tuple(None if c == 2 else int(c) for c in codes[v, 2 * s:2 * s + 2])}
                   for s, name in enumerate(names)}
        records.append(FakeRecord(CHROM, int(pos[v]), ids[v], "A", ("G",), {"VT": ("SNP",)}, samples))
    return prefix, codes, pos, ids, where, FakeVcf(records), names, [[int(pos[v]), ids[v]] for v in range(N_VAR)]


def mirror_rows(result, pos, ids, window, **params):
    """The .blocks.det rows and .blocks lines of the host mirrors on the device's own bound bytes."""
    from ld_tools_amd import ops
    kept = result.ci.kept.cpu().numpy().astype(bool)
    cands = ops.gabriel_candidates_host(result.ci.lo.cpu().numpy(), result.ci.hi.cpu().numpy(), pos, kept, window, **params)
    block_of, n_blocks = ops.gabriel_pick_host(cands, kept.size, kept)
    det, plain = ["CHR\tBP1\tBP2\tKB\tNSNPS\tSNPS\n"], []
    for b in range(n_blocks):
        members = np.flatnonzero(block_of == b)
        names = [ids[i] for i in members]
        bp1, bp2 = int(pos[members[0]]), int(pos[members[-1]])
        det.append("%s\t%d\t%d\t%.3f\t%d\t%s\n" % (CHROM, bp1, bp2, (bp2 - bp1 + 1) / 1000.0, members.size, "|".join(names)))
        plain.append("* " + " ".join(names) + "\n")
    return "".join(det), "".join(plain), block_of, kept


def test_bfile_blocks_and_the_writer(study, tmp_path):
    from ld_tools_amd import drivers, ops

    prefix, codes, pos, ids, where, _, _, _ = study
    table = drivers.bfile_blocks(prefix, window_bp=gc.WINDOW)
    assert table.chrom == CHROM and table.rs_ids == ids and table.poss == [int(p) for p in pos] and table.n == N_VAR
    assert table.result.ci.missing == "pairwise"                          # the default of the fileset driver
    det, plain, block_of, kept = mirror_rows(table.result, pos, ids, gc.WINDOW)
    paths = drivers.write_gabriel_blocks(str(tmp_path / "bed"), table.result, table.rs_ids, table.chrom)
    assert Path(paths[0]).read_text() == plain and Path(paths[1]).read_text() == det
    assert table.result.n_blocks == len(plain.splitlines()) >= 8 and np.array_equal(table.result.block_of, block_of)
    # a SNP the MAF rule drops lies between a block's ends and is not listed
    rare = where["rare_snp"][0]
    assert not kept[rare] and block_of[rare - 1] == block_of[rare + 1] < ops.NO_BLOCK
    row = det.splitlines()[1 + int(block_of[rare - 1])].split("\t")
    assert ids[rare] not in row[5].split("|") and ids[rare - 1] in row[5].split("|") and int(row[4]) == len(row[5].split("|"))
    assert int(row[1]) < int(pos[rare]) < int(row[2])
    listed = [name for line in plain.splitlines() for name in line.split()[1:]]
    assert len(listed) == len(set(listed)) == int((block_of < ops.NO_BLOCK).sum()) and not set(listed) & {ids[i] for i in np.flatnonzero(~kept)}
    # the other form, other parameters, a keep mask
    keep = np.ones(N_VAR, dtype=bool)
    keep[10:14] = False
    other = drivers.bfile_blocks(prefix, window_bp=200_000, missing=None, maf_min=0.1, keep_snps=keep, cuts=(75, 60, 55, 65))
    det2, plain2, block2, kept2 = mirror_rows(other.result, pos, ids, 200_000, cuts=(75, 60, 55, 65))
    paths2 = drivers.write_gabriel_blocks(str(tmp_path / "other"), other.result, other.rs_ids, other.chrom)
    assert Path(paths2[1]).read_text() == det2 and Path(paths2[0]).read_text() == plain2 and not kept2[10:14].any()
    assert other.result.ci.missing is None


def test_the_vcf_driver_gives_the_same_blocks(study, tmp_path):
    from ld_tools_amd import drivers

    prefix, _, pos, ids, _, vcf, names, rows = study
    a = drivers.gabriel_blocks(vcf, CHROM, rows, names, window_bp=gc.WINDOW, missing="pairwise")
    b = drivers.bfile_blocks(prefix, window_bp=gc.WINDOW)
    assert a.rs_ids == b.rs_ids and a.poss == b.poss and a.chrom == b.chrom
    pa = drivers.write_gabriel_blocks(str(tmp_path / "vcf"), a.result, a.rs_ids, a.chrom)
    pb = drivers.write_gabriel_blocks(str(tmp_path / "bed"), b.result, b.rs_ids, b.chrom)
    for x, y in zip(pa, pb):
        assert Path(x).read_bytes() == Path(y).read_bytes() and Path(x).stat().st_size > 100


def test_the_blocks_subcommand(study, tmp_path):
    from ld_tools_amd import drivers
    from ld_tools_amd.drivers import plink as shell

    prefix, _, pos, ids, _, _, _, _ = study
    out, ref = str(tmp_path / "cli"), str(tmp_path / "ref")
    assert shell.main(["blocks", "--bfile", prefix, "--out", out]) == 0
    table = drivers.bfile_blocks(prefix)
    want = drivers.write_gabriel_blocks(ref, table.result, table.rs_ids, table.chrom)
    assert Path(out + ".blocks").read_bytes() == Path(want[0]).read_bytes()
    assert Path(out + ".blocks.det").read_bytes() == Path(want[1]).read_bytes()
    assert Path(out + ".blocks.det").read_text() == mirror_rows(table.result, pos, ids, 500_000)[0]
    assert shell.main(["blocks", "--bfile", prefix, "--out", out, "--blocks-max-kb", "200", "--blocks-min-maf", "0.1",
                       "--missing", "ref"]) == 0
    other = drivers.bfile_blocks(prefix, window_bp=200_000, missing=None, maf_min=0.1)
    assert Path(out + ".blocks.det").read_text() == mirror_rows(other.result, pos, ids, 200_000)[0]

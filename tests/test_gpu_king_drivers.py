"""GPU: the relatedness drivers on a synthetic PLINK fileset: bfile_king's counts and tables against the host oracle on the
fileset's genotypes, the pruned form against sample_counts on the panel of ld_prune's kept variants, and the ``king`` subcommand
in a fresh process against the drivers' own files."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
CHROM, N_VAR, N_SAMPLES = "3", 400, 24


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def study(gpu, tmp_path_factory):
    """(prefix, canonical codes, fid, iid): LD blocks, 3 % missing genotypes, individual 7 a copy of individual 2."""
    from ld_tools_amd import plink, synth

    codes = synth.synth_codes_host(N_VAR, 2 * N_SAMPLES, seed=12).astype(np.int8)
    codes[:, 14:16] = codes[:, 4:6]
    gone = np.random.default_rng(6).random((N_VAR, N_SAMPLES)) < 0.03
    codes[np.repeat(gone, 2, axis=1)] = 2
    prefix = str(tmp_path_factory.mktemp("king") / "study")
    fid, iid = [f"FAM{s // 3}" for s in range(N_SAMPLES)], [f"ID{s:03d}" for s in range(N_SAMPLES)]
    bim = {"chrom": [CHROM] * N_VAR, "ids": [f"rs{v}" for v in range(N_VAR)], "pos": [1000 + 150 * v for v in range(N_VAR)],
           "a1": ["G"] * N_VAR, "a2": ["A"] * N_VAR}
    plink.write_bfile(prefix, plink.codes_bed_host(codes, alt="a1"), bim, {"fid": fid, "iid": iid})
    return prefix, plink.canonical_codes(codes), fid, iid


def host_pairs(counts, kin_min=None):
    from ld_tools_amd import RelatedPairs, king_cell_host

    N, HH, IBS0, HET = counts
    kin = king_cell_host(N, HH, IBS0, HET, HET.T)
    a, b = np.nonzero(np.tril(np.ones_like(N, dtype=bool), -1) & (True if kin_min is None else kin >= np.float32(kin_min)))
    return RelatedPairs(a, b, kin[a, b], N[a, b], HH[a, b], IBS0[a, b])


def test_bfile_king_equals_the_host_oracle(study, tmp_path):
    from ld_tools_amd import drivers, king_cell_host, king_cutoff, sample_counts_host
    from ld_tools_amd.drivers.king import KIN0_HEADER, kin0_lines

    prefix, codes, fid, iid = study
    want = sample_counts_host(codes)
    out = str(tmp_path / "all")
    table = drivers.bfile_king(prefix, out=out, cutoff=0.177, matrix=True)
    assert (table.fid, table.iid) == (fid, iid) and table.counts.n_snps == N_VAR
    assert np.array_equal(table.counts.counts.cpu().numpy().view(np.uint32).astype(np.int64), want)
    lines = kin0_lines(fid, iid, host_pairs(want))
    assert len(lines) == N_SAMPLES * (N_SAMPLES - 1) // 2
    assert Path(out + ".kin0").read_text() == KIN0_HEADER + "\n" + "".join(x + "\n" for x in lines)
    dup = [x for x in lines if x.startswith("FAM0\tID002\tFAM2\tID007\t")]
    assert len(dup) == 1 and dup[0].endswith("\t0\t0.5")                    # the copy: no opposite homozygote, kinship 0.5
    N, HH, IBS0, HET = want
    kin = king_cell_host(N, HH, IBS0, HET, HET.T)
    keep, _ = king_cutoff(kin, 0.177)
    assert not keep.all() and not (keep[2] and keep[7])                      # of the two copies at most one stays
    ids = lambda sel: "#FID\tIID\n" + "".join(f"{fid[k]}\t{iid[k]}\n" for k in np.flatnonzero(sel))  # noqa: E731
    assert Path(out + ".king.cutoff.in.id").read_text() == ids(keep)
    assert Path(out + ".king.cutoff.out.id").read_text() == ids(~keep)
    assert Path(out + ".king.id").read_text() == ids(np.ones(N_SAMPLES, dtype=bool))
    rows = Path(out + ".king").read_text().split("\n")[:-1]
    assert len(rows) == N_SAMPLES - 1 and rows[6].split("\t")[2] == "0.5" and [len(r.split("\t")) for r in rows] == list(range(1, N_SAMPLES))
    # a filtered table, individuals and variants selected at load
    inds, snps = np.array([2, 7, 9, 10, 20]), np.arange(0, N_VAR, 3)
    sub = codes.reshape(N_VAR, N_SAMPLES, 2)[snps][:, inds].reshape(snps.size, -1)
    table = drivers.bfile_king(prefix, out=str(tmp_path / "sub"), keep=inds, extract=snps, kin_min=0.3)
    assert np.array_equal(table.counts.counts.cpu().numpy().view(np.uint32).astype(np.int64), sample_counts_host(sub))
    assert Path(str(tmp_path / "sub") + ".kin0").read_text().split("\n")[1:-1] == kin0_lines(
        [fid[k] for k in inds], [iid[k] for k in inds], host_pairs(sample_counts_host(sub), 0.3))


def test_pruned_form_counts_the_kept_variants(study):
    from ld_tools_amd import drivers, sample_counts, sample_counts_host

    prefix, codes, _, _ = study
    bf = drivers.load_bfile(prefix)
    keep = drivers.bfile_prune(bf, r2=0.2, window_bp=5000, missing="pairwise").pruned.keep
    assert 0 < int(keep.sum()) < N_VAR
    table = drivers.bfile_king(bf, prune_r2=0.2, prune_window_bp=5000, prune_missing="pairwise")
    assert np.array_equal(table.snp_mask, keep) and table.counts.n_snps == N_VAR
    assert torch.equal(table.counts.counts, sample_counts(bf.panel.select(snps=keep)).counts)
    assert np.array_equal(table.counts.counts.cpu().numpy().view(np.uint32).astype(np.int64), sample_counts_host(codes, keep))


def test_king_subcommand_in_a_fresh_process(study, tmp_path):
    from ld_tools_amd import drivers

    prefix, _, _, _ = study
    out, ref = str(tmp_path / "cli"), str(tmp_path / "ref")
    run = subprocess.run([sys.executable, "-m", "ld_tools_amd.drivers.plink", "king", "--bfile", prefix, "--out", out,
                          "--king-table-filter", "0.05", "--king-cutoff", "0.177", "--prune-r2", "0.2", "--prune-window-kb", "5",
                          "--missing", "pairwise"], cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    drivers.bfile_king(prefix, out=ref, prune_r2=0.2, prune_window_bp=5000, prune_missing="pairwise", kin_min=0.05, cutoff=0.177)
    for ext in (".kin0", ".king.cutoff.in.id", ".king.cutoff.out.id"):
        assert Path(out + ext).read_bytes() == Path(ref + ext).read_bytes(), ext
    assert len(Path(out + ".kin0").read_text().split("\n")) > 2

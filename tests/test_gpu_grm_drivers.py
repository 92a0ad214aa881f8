"""GPU: the GRM drivers on a synthetic PLINK fileset: bfile_grm streamed in three chunks against grm_table on the whole panel and
against the host mirror on the fileset's genotypes, file for file, and the ``grm`` subcommand in a fresh process against the
driver's own files."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
N_VAR, N_SAMPLES, CHUNK = 700, 24, 300     # chunks of 300, 300 and 100 variants
GCTA = (".grm.bin", ".grm.N.bin", ".grm.id")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def study(gpu, tmp_path_factory):
    """(prefix, canonical codes, fid, iid): two chromosomes, 3 % missing genotypes, individual 7 a copy of individual 2, the
    rarest variants in the last chunk (so that the largest coefficient, and with it the exponent, is not the first chunk's)."""
    from ld_tools_amd import plink

    rng = np.random.default_rng(12)
    f = np.concatenate([rng.uniform(0.2, 0.5, size=N_VAR - 50), rng.uniform(0.02, 0.05, size=50)])
    codes = (rng.random((N_VAR, 2 * N_SAMPLES)) < f[:, None]).astype(np.int8)
    codes[:, 14:16] = codes[:, 4:6]
    codes[np.repeat(rng.random((N_VAR, N_SAMPLES)) < 0.03, 2, axis=1)] = 2
    prefix = str(tmp_path_factory.mktemp("grm") / "study")
    fid, iid = [f"FAM{s // 3}" for s in range(N_SAMPLES)], [f"ID{s:03d}" for s in range(N_SAMPLES)]
    bim = {"chrom": ["3"] * 400 + ["4"] * (N_VAR - 400), "ids": [f"rs{v}" for v in range(N_VAR)],
           "pos": [1000 + 150 * v for v in range(N_VAR)], "a1": ["G"] * N_VAR, "a2": ["A"] * N_VAR}
    plink.write_bfile(prefix, plink.codes_bed_host(codes, alt="a1"), bim, {"fid": fid, "iid": iid})
    return prefix, plink.canonical_codes(codes), fid, iid


def same_files(a, b, exts):
    for ext in exts:
        assert Path(a + ext).read_bytes() == Path(b + ext).read_bytes(), ext


def test_streamed_fileset_equals_the_whole_panel(study, tmp_path):
    from ld_tools_amd import drivers, grm_cutoff, ld_grm_host
    from ld_tools_amd.drivers.grm import grm_table, write_grm_bin, write_grm_cutoff, write_rel

    prefix, codes, fid, iid = study
    bf = drivers.load_bfile(prefix)
    whole, chunks = str(tmp_path / "whole"), str(tmp_path / "chunks")
    table = grm_table(bf.panel, list(zip(fid, iid)), maf_min=0.03)
    write_grm_bin(whole, table), write_rel(whole, table), write_grm_cutoff(whole, table, 0.2)
    streamed = drivers.bfile_grm(prefix, out=chunks, maf_min=0.03, cutoff=0.2, chunk_snps=CHUNK)
    drivers.bfile_grm(prefix, out=chunks, maf_min=0.03, fmt="rel", chunk_snps=CHUNK)
    assert (streamed.fid, streamed.iid) == (fid, iid)
    assert streamed.result.exp == table.result.exp and streamed.result.n_live == table.result.n_live
    assert torch.equal(streamed.result.S, table.result.S) and torch.equal(streamed.result.counts.counts, table.result.counts.counts)
    same_files(whole, chunks, GCTA + (".rel", ".rel.id", ".grm.cutoff.in.id", ".grm.cutoff.out.id"))
    # ... and the host mirror on the fileset's genotypes
    want = ld_grm_host(codes, maf_min=0.03)
    assert want.exp == table.result.exp and 0 < want.n_live < N_VAR
    grm = want.grm()
    low = np.tril_indices(N_SAMPLES)
    assert np.array_equal(np.fromfile(chunks + ".grm.bin", dtype="<f4").view(np.int32), grm[low].view(np.int32))
    assert np.array_equal(np.fromfile(chunks + ".grm.N.bin", dtype="<f4"), want.N[low].astype(np.float32))
    assert Path(chunks + ".grm.id").read_text() == "".join(f"{a}\t{b}\n" for a, b in zip(fid, iid))
    assert grm[7, 2] > 0.8                                                               # the copy
    keep, _ = grm_cutoff(grm, 0.2)
    assert not keep.all() and not (keep[2] and keep[7])
    ids = lambda sel: "#FID\tIID\n" + "".join(f"{fid[k]}\t{iid[k]}\n" for k in np.flatnonzero(sel))  # noqa: E731
    assert Path(chunks + ".grm.cutoff.in.id").read_text() == ids(keep)
    assert Path(chunks + ".grm.cutoff.out.id").read_text() == ids(~keep)
    # a loaded fileset, and selections at the file: individuals, variants, one chromosome
    loaded = str(tmp_path / "loaded")
    drivers.bfile_grm(bf, out=loaded, maf_min=0.03)
    same_files(whole, loaded, GCTA)
    inds, snps = np.array([2, 7, 9, 10, 20]), np.arange(0, N_VAR, 3)
    sub = drivers.bfile_grm(prefix, keep=inds, extract=snps, chrom="4", chunk_snps=40)
    rows = snps[snps >= 400]
    want = ld_grm_host(codes.reshape(N_VAR, N_SAMPLES, 2)[rows][:, inds].reshape(rows.size, -1))
    assert sub.iid == [iid[k] for k in inds] and sub.result.exp == want.exp
    assert np.array_equal(sub.grm().view(np.int32), want.grm().view(np.int32))


def test_grm_subcommand_in_a_fresh_process(study, tmp_path):
    from ld_tools_amd import drivers

    prefix, _, _, _ = study
    out, ref = str(tmp_path / "cli"), str(tmp_path / "ref")
    run = subprocess.run([sys.executable, "-m", "ld_tools_amd.drivers.plink", "grm", "--bfile", prefix, "--out", out, "--maf", "0.03",
                          "--grm-cutoff", "0.2", "--chunk-snps", str(CHUNK)], cwd=str(ROOT), capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    drivers.bfile_grm(prefix, out=ref, maf_min=0.03, cutoff=0.2)
    same_files(out, ref, GCTA + (".grm.cutoff.in.id", ".grm.cutoff.out.id"))
    assert Path(out + ".grm.bin").stat().st_size == 4 * N_SAMPLES * (N_SAMPLES + 1) // 2
    run = subprocess.run([sys.executable, "-m", "ld_tools_amd.drivers.plink", "grm", "--bfile", prefix, "--out", out, "--maf", "0.03",
                          "--format", "rel"], cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    drivers.bfile_grm(prefix, out=ref, maf_min=0.03, fmt="rel")
    same_files(out, ref, (".rel", ".rel.id"))

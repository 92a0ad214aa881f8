"""PLINK .bed/.bim/.fam on the host: the two converters of ld_tools_amd/plink.py (the specification the device kernels are
tested against), the fileset reader and writer, and the ABI of the two new entries.  No GPU."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("ldx_bed_unpack_dev", "ldx_bed_pack_dev")


def clear_pad(rows, n_ind):
    out = np.array(rows, dtype=np.uint8, copy=True)
    if n_ind % 4:
        out[:, (n_ind - 1) // 4] &= (1 << (2 * (n_ind % 4))) - 1
    return out[:, : (n_ind + 3) // 4]


def test_hand_decoded_literals():
    from ld_tools_amd import plink

    # 0xdc = 11 01 11 00, individual 0 in the low bits: hom A1, hom A2, missing, hom A2
    x = np.array([[0xDC]], dtype=np.uint8)
    assert plink.bed_codes_host(x, 4).tolist() == [[1, 1, 0, 0, 2, 2, 0, 0]]
    assert plink.bed_codes_host(x, 4, alt="a2").tolist() == [[0, 0, 1, 1, 2, 2, 1, 1]]
    assert plink.bed_codes_host(x, 4).dtype == np.int8
    # 0x36 = 00 11 01 10: het, missing, hom A2 -- and a pad field that n_ind = 3 must ignore, whatever it holds
    for pad in (0x00, 0x40, 0x80, 0xC0):
        y = np.array([[0x36 | pad]], dtype=np.uint8)
        assert plink.bed_codes_host(y, 3).tolist() == [[1, 0, 2, 2, 0, 0]]
        assert plink.bed_codes_host(y, 3, alt="a2").tolist() == [[1, 0, 2, 2, 1, 1]]
    # the inverse writes the pad field as zero
    assert plink.codes_bed_host(np.array([[1, 0, 2, 2, 0, 0]], dtype=np.int8)).tolist() == [[0x36]]
    assert plink.codes_bed_host(np.array([[0, 1, 2, 0, 1, 1]], dtype=np.int8), alt="a2").tolist() == [[0x36]]   # het either order; half-missing


@pytest.mark.parametrize("n_ind", [1, 3, 4, 5, 64, 131])
@pytest.mark.parametrize("alt", ["a1", "a2"])
def test_round_trips(n_ind, alt):
    from ld_tools_amd import plink

    rng = np.random.default_rng(n_ind)
    rows = rng.integers(0, 256, size=(9, plink.row_bytes(n_ind)), dtype=np.uint8)
    codes = plink.bed_codes_host(rows, n_ind, alt=alt)
    assert codes.shape == (9, 2 * n_ind) and set(np.unique(codes)) <= {0, 1, 2}
    assert np.array_equal(plink.codes_bed_host(codes, alt=alt), clear_pad(rows, n_ind))
    # random codes over {0, 1, 2} come back in the canonical form: (1, 1), (0, 0), a het as (1, 0), anything else (2, 2)
    c = rng.integers(0, 3, size=(9, 2 * n_ind)).astype(np.int8)
    x, y = c[:, 0::2], c[:, 1::2]
    want = np.full_like(c, 2)
    hom = (x == y) & (x < 2)
    het = (x + y == 1) & (x < 2) & (y < 2)
    want[:, 0::2] = np.where(hom, x, np.where(het, 1, 2))
    want[:, 1::2] = np.where(hom, y, np.where(het, 0, 2))
    got = plink.bed_codes_host(plink.codes_bed_host(c, alt=alt), n_ind, alt=alt)
    assert np.array_equal(got, want) and np.array_equal(plink.canonical_codes(c), want)


def test_wider_rows_are_accepted_and_alt_is_checked():
    from ld_tools_amd import LdxError, plink

    rows = np.random.default_rng(1).integers(0, 256, size=(4, 5), dtype=np.uint8)
    assert np.array_equal(plink.bed_codes_host(rows, 7), plink.bed_codes_host(rows[:, :2], 7))
    with pytest.raises(LdxError):
        plink.bed_codes_host(rows, 21)             # 6 bytes needed
    with pytest.raises(LdxError):
        plink.bed_codes_host(rows, 7, alt="ref")
    with pytest.raises(LdxError):
        plink.codes_bed_host(np.zeros((2, 3), dtype=np.int8))


def test_keep_permutation_repeats_and_mask():
    from ld_tools_amd import LdxError, plink

    n_ind = 23
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 256, size=(6, plink.row_bytes(n_ind)), dtype=np.uint8)
    full = plink.bed_codes_host(rows, n_ind).reshape(6, n_ind, 2)
    perm = rng.permutation(n_ind)
    assert np.array_equal(plink.bed_codes_host(rows, n_ind, keep=perm), full[:, perm].reshape(6, -1))
    rep = np.array([3, 3, 22, 0, 3])
    assert np.array_equal(plink.bed_codes_host(rows, n_ind, keep=rep, alt="a2"),
                          plink.bed_codes_host(rows, n_ind, alt="a2").reshape(6, n_ind, 2)[:, rep].reshape(6, -1))
    mask = rng.random(n_ind) < 0.4
    mask[2] = True
    assert np.array_equal(plink.bed_codes_host(rows, n_ind, keep=mask), full[:, np.flatnonzero(mask)].reshape(6, -1))
    for bad in (np.array([0, n_ind]), np.array([-1]), np.zeros(n_ind + 1, dtype=bool), np.array([], dtype=np.int64),
                np.array([0.5])):
        with pytest.raises(LdxError):
            plink.bed_codes_host(rows, n_ind, keep=bad)


def make_fileset(tmp_path, n_snps=7, n_ind=10, seed=3):
    from ld_tools_amd import plink

    rng = np.random.default_rng(seed)
    rows = clear_pad(rng.integers(0, 256, size=(n_snps, plink.row_bytes(n_ind)), dtype=np.uint8), n_ind)
    bim = {"chrom": ["1"] * 4 + ["X"] * (n_snps - 4), "ids": [f"rs{100 + k}" for k in range(n_snps)],
           "cm": [0, 0.5, 1.25, 2, 0, 0, 3.5][:n_snps], "pos": [1000 + 37 * k for k in range(n_snps)],
           "a1": ["A", "C", "G", "T", "AT", "G", "C"][:n_snps], "a2": ["G", "T", "A", "C", "A", "GTT", "T"][:n_snps]}
    fam = {"fid": [f"F{k // 2}" for k in range(n_ind)], "iid": [f"I{k}" for k in range(n_ind)],
           "father": ["0"] * n_ind, "mother": ["0"] * (n_ind - 1) + ["I0"], "sex": [str(1 + k % 2) for k in range(n_ind)],
           "pheno": ["-9", "1", "2", "0.37", "-9", "1", "1", "2", "2", "NA"][:n_ind]}
    prefix = str(tmp_path / "study")
    paths = plink.write_bfile(prefix, rows, bim, fam)
    return prefix, paths, rows, bim, fam


def test_bedfile_reads_what_write_bfile_wrote(tmp_path):
    from ld_tools_amd import BedFile, plink

    prefix, paths, rows, bim, fam = make_fileset(tmp_path)
    assert [Path(p).name for p in paths] == ["study.bed", "study.bim", "study.fam"]
    raw = Path(paths[0]).read_bytes()
    assert raw[:3] == bytes([0x6C, 0x1B, 0x01]) and len(raw) == 3 + 7 * 3 and raw[3:] == rows.tobytes()
    for opened in (BedFile(prefix), BedFile(prefix + ".bed"), BedFile(Path(prefix))):
        assert (opened.n_snps, opened.n_ind) == (7, 10)
        assert opened.chrom == bim["chrom"] and opened.ids == bim["ids"] and opened.a1 == bim["a1"] and opened.a2 == bim["a2"]
        assert opened.cm.dtype == np.float64 and opened.cm.tolist() == [float(v) for v in bim["cm"]]
        assert opened.pos.dtype == np.int64 and opened.pos.tolist() == bim["pos"]
        for name in ("fid", "iid", "father", "mother", "sex", "pheno"):
            assert getattr(opened, name) == fam[name], name
        assert isinstance(opened.rows, np.memmap) and opened.rows.dtype == np.uint8 and opened.rows.shape == (7, 3)
        assert np.array_equal(opened.rows, rows)
        assert np.array_equal(plink.bed_codes_host(opened.rows, opened.n_ind), plink.bed_codes_host(rows, 10))
    sub = opened.bim([4, 1])
    assert sub["ids"] == ["rs104", "rs101"] and sub["pos"].tolist() == [1148, 1037]
    assert opened.fam([9])["pheno"] == ["NA"]
    # defaults of the writer: FID = IID, parents 0, sex 0, phenotype -9, cM 0
    p2 = str(tmp_path / "plain")
    plink.write_bfile(p2, rows, {k: bim[k] for k in ("chrom", "ids", "pos", "a1", "a2")}, {"iid": fam["iid"]})
    plain = BedFile(p2)
    assert plain.fid == fam["iid"] and plain.pheno == ["-9"] * 10 and plain.sex == ["0"] * 10 and plain.cm.tolist() == [0.0] * 7


def test_malformed_filesets_raise(tmp_path):
    from ld_tools_amd import BedFile, LdxError, plink

    prefix, paths, rows, bim, fam = make_fileset(tmp_path)
    bed, bimp, famp = (Path(p) for p in paths)
    good = {p: p.read_bytes() for p in (bed, bimp, famp)}

    def restore():
        for p, data in good.items():
            p.write_bytes(data)

    def refused(match=None):
        with pytest.raises(LdxError, match=match):
            BedFile(prefix)
        restore()

    bed.write_bytes(good[bed][:-1])                                  # a short file
    refused("bytes")
    bed.write_bytes(good[bed] + b"\0")                               # a long one
    refused("bytes")
    bed.write_bytes(good[bed][:2])                                   # not even the magic
    refused("magic")
    bed.write_bytes(b"\x6c\x1b\x00" + good[bed][3:])                 # individual-major: its own message
    refused("individual-major")
    bed.write_bytes(b"\x6c\x1a\x01" + good[bed][3:])
    refused("magic")
    bimp.write_text(good[bimp].decode().replace("rs102\t", "rs102\textra\t"))   # a line with seven fields
    refused("fields")
    bimp.write_text(good[bimp].decode().replace("\t1074\t", "\tabc\t"))
    refused("numeric")
    bimp.write_text("".join(good[bimp].decode().splitlines(True)[:-1]))         # .bim and .bed disagree
    refused("bytes")
    famp.write_text(good[famp].decode() + "F9 I10 0 0 1\n")                     # a .fam line with five fields
    refused("fields")
    famp.write_text(good[famp].decode() + "F9 I10 0 0 1 -9\nF9 I11 0 0 1 -9\nF9 I12 0 0 1 -9\n")   # 13 individuals: 4 bytes a row
    refused("bytes")
    bimp.unlink()
    with pytest.raises(LdxError):
        BedFile(prefix)
    restore()
    assert BedFile(prefix).n_snps == 7
    with pytest.raises(LdxError):
        plink.write_bfile(prefix + "x", rows[:, :2], bim, fam)
    with pytest.raises(LdxError):
        plink.write_bfile(prefix + "x", rows, bim, {"iid": fam["iid"][:8]})        # 8 individuals: 2 bytes a row


def test_new_symbols_are_declared_exported_and_bound():
    import ld_tools_amd
    from ld_tools_amd import _lib, build

    raw = (ROOT / "include" / "ldx.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ldx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/ldx.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libldx.so"
    for name, n_args in (("ldx_bed_unpack_dev", 14), ("ldx_bed_pack_dev", 10)):
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", text)
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1])
    assert _lib.version() == 102                                           # new symbols only: no version bump
    assert "#define LDX_VERSION 102" in raw.replace("  ", " ")
    assert "ldx_bed.hip" in build.SOURCES
    for name in ("plink", "BedFile", "bed_codes_host", "codes_bed_host", "write_bfile"):
        assert name in ld_tools_amd.__all__ and hasattr(ld_tools_amd, name)
    assert callable(ld_tools_amd.PackedPanel.from_bed) and callable(ld_tools_amd.PackedPanel.to_bed)
    from ld_tools_amd import drivers
    for name in ("load_bfile", "bfile_ld_table", "bfile_clump", "bfile_prune", "bfile_ld_scores", "bfile_band",
                 "bfile_em_band", "make_bed", "Bfile"):
        assert callable(getattr(drivers, name)), name


def test_entries_refuse_bad_arguments_before_any_launch():
    from ld_tools_amd import _lib

    L, E_ARG, E_UNSUP = _lib.lib, -1, -3
    p = 0x1000                                                             # never dereferenced: every call returns first

    def unpack(bed=p, row_bytes=16, n_src=64, n_rows=128, idx=None, n_dst=64, a2=0, row0=0, n_panel=128, alt=p, ref=p,
               acnt=p, rcnt=p):
        return L.ldx_bed_unpack_dev(bed, row_bytes, n_src, n_rows, idx, n_dst, a2, row0, n_panel, alt, ref, acnt, rcnt, None)

    assert unpack(bed=None) == E_ARG and unpack(ref=None) == E_ARG and unpack(rcnt=None) == E_ARG
    assert unpack(row_bytes=15) == E_ARG                                   # below ceil(64 / 4)
    assert unpack(n_dst=32) == E_ARG                                       # identity needs n_ind_dst == n_ind_src
    assert unpack(a2=2) == E_ARG
    assert unpack(row0=64, n_panel=256) == E_ARG                           # row0 is no multiple of 128
    assert unpack(row0=129, n_rows=1, n_panel=130) == E_ARG
    assert unpack(n_rows=100, n_panel=300) == E_ARG                        # a ragged chunk that does not reach the end
    assert unpack(row0=128, n_rows=128, n_panel=200) == E_ARG              # past the panel
    assert unpack(n_src=0) == E_ARG and unpack(n_rows=0) == E_ARG
    assert unpack(n_src=5121, n_dst=5121, row_bytes=1281) == E_UNSUP       # 2 n_ind_dst > LDX_MAX_HAPS
    assert unpack(idx=p, n_src=500_000, row_bytes=125_000, n_dst=5121) == E_UNSUP

    def pack(alt=p, ref=p, n_snps=300, n_hap=128, row0=0, n_rows=300, bed=p, row_bytes=16, a2=0):
        return L.ldx_bed_pack_dev(alt, ref, n_snps, n_hap, row0, n_rows, bed, row_bytes, a2, None)

    assert pack(ref=None) == E_ARG and pack(bed=None) == E_ARG
    assert pack(n_hap=127) == E_ARG                                        # odd
    assert pack(row0=299, n_rows=2) == E_ARG and pack(row0=300, n_rows=1) == E_ARG and pack(n_rows=0) == E_ARG
    assert pack(row_bytes=15) == E_ARG and pack(a2=-1) == E_ARG
    assert pack(n_hap=10242, row_bytes=1281) == E_UNSUP


def test_cli_help_exits_zero():
    out = subprocess.run([sys.executable, "-m", "ld_tools_amd.drivers.plink", "--help"], cwd=str(ROOT), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    for word in ("ld", "clump", "prune", "l2", "make-bed"):
        assert word in out.stdout

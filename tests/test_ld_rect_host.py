"""CPU: rectangular LD -- the ABI of the four new entries, the argument rules that are checked before a device is touched
(include/ldx.h, "rectangular LD"; ops.ld_rect, ops.ld_rect_hits), the host mirror of the hit rule (ops.rect_hits_host), the
test panels' own properties, and the plumbing of drivers/rect.py as far as it runs without a device.  No kernel is launched
here."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import fakevcf  # noqa: E402
import ld_dosage_exact as dx  # noqa: E402
import ld_exact as lx  # noqa: E402
import ld_rect_cases as rc  # noqa: E402

NEW_SYMBOLS = ["ldx_ld_rect_dev", "ldx_ld_rect_dosage_dev", "ldx_ld_rect_hits_dev", "ldx_ld_rect_hits_dosage_dev"]
E_ARG, E_UNSUPPORTED = -1, -3


def test_new_symbols_are_declared_bound_and_exported():
    from ld_tools_amd import _lib
    text = (ROOT / "include" / "ldx.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ldx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/ldx.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libldx.so"
    assert _lib.version() == 102                                           # new symbols only: no version bump
    assert "#define LDX_VERSION 102" in (ROOT / "include" / "ldx.h").read_text().replace("  ", " ")
    import ld_tools_amd
    for name in ("ld_rect", "ld_rect_hits", "LDRectHits", "rect_hits_host"):
        assert name in ld_tools_amd.__all__ and hasattr(ld_tools_amd, name)
    from ld_tools_amd import drivers
    for name in ("rect_matrix", "write_rect_matrix"):
        assert hasattr(drivers, name)


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every rule of the header's table returns its code, with a message that names the argument, before a device is touched."""
    from ld_tools_amd import _lib
    lib = _lib.lib
    big = C.create_string_buffer(4096 + 256)
    ptr = (C.addressof(big) + 255) // 256 * 256   # a non-null, 256-byte-aligned stand-in for every pointer (never read)

    def err():
        return lib.ldx_last_error().decode()

    def dense(alt_i=ptr, acnt_i=ptr, rcnt_i=ptr, n_i=100, alt_j=ptr, acnt_j=ptr, rcnt_j=ptr, n_j=50, n_hap=64, out=ptr,
              ld_out=50):
        return lib.ldx_ld_rect_dev(alt_i, acnt_i, rcnt_i, n_i, alt_j, acnt_j, rcnt_j, n_j, n_hap, out, ld_out, None)

    def dense_d(alt_i=ptr, gstat_i=ptr, n_i=100, alt_j=ptr, gstat_j=ptr, n_j=50, n_hap=64, out=ptr, ld_out=50):
        return lib.ldx_ld_rect_dosage_dev(alt_i, gstat_i, n_i, alt_j, gstat_j, n_j, n_hap, out, ld_out, None)

    def hits(alt_i=ptr, acnt_i=ptr, rcnt_i=ptr, n_i=100, alt_j=ptr, acnt_j=ptr, rcnt_j=ptr, n_j=50, n_hap=64, bound=0.2,
             buf=ptr, cap=256, n_hits=ptr):
        return lib.ldx_ld_rect_hits_dev(alt_i, acnt_i, rcnt_i, n_i, alt_j, acnt_j, rcnt_j, n_j, n_hap, bound, buf, cap, n_hits,
                                        None)

    def hits_d(alt_i=ptr, gstat_i=ptr, n_i=100, alt_j=ptr, gstat_j=ptr, n_j=50, n_hap=64, bound=0.2, buf=ptr, cap=256,
               n_hits=ptr):
        return lib.ldx_ld_rect_hits_dosage_dev(alt_i, gstat_i, n_i, alt_j, gstat_j, n_j, n_hap, bound, buf, cap, n_hits, None)

    who = {dense: "ldx_ld_rect_dev", dense_d: "ldx_ld_rect_dosage_dev", hits: "ldx_ld_rect_hits_dev",
           hits_d: "ldx_ld_rect_hits_dosage_dev"}

    def said(fn, message):
        """the WHOLE message, word for word (callers match on the words)"""
        return err() == f"{who[fn]}: {message}"

    # null pointers, each named
    for fn, names in ((dense, ("alt_i", "acnt_i", "rcnt_i", "alt_j", "acnt_j", "rcnt_j", "out")),
                      (dense_d, ("alt_i", "gstat_i", "alt_j", "gstat_j", "out")),
                      (hits, ("alt_i", "acnt_i", "rcnt_i", "alt_j", "acnt_j", "rcnt_j", "n_hits")),
                      (hits_d, ("alt_i", "gstat_i", "alt_j", "gstat_j", "n_hits"))):
        for name in names:
            assert fn(**{name: None}) == E_ARG, (fn.__name__, name)
            assert said(fn, f"{name} is a null pointer"), err()
    for fn in (hits, hits_d):
        assert fn(buf=None) == E_ARG and said(fn, "hits is a null pointer but hit_cap is 256"), err()
        for bad, shown in ((0.0, "0"), (-0.5, "-0.5"), (float("nan"), "nan")):
            assert fn(bound=bad) == E_ARG and said(fn, f"r2_bound must be a float32 > 0 (got {shown})"), err()
        assert fn(bound=0.0, buf=None, n_hits=None, n_i=0) == E_ARG and said(fn, "n_hits is a null pointer")   # the first rule
        assert fn(bound=0.0, buf=None, n_i=0) == E_ARG and said(fn, "hits is a null pointer but hit_cap is 256")
        assert fn(bound=0.0, n_i=0) == E_ARG and said(fn, "r2_bound must be a float32 > 0 (got 0)")
    # shapes
    plane = "{} is a bit plane of 4 GiB or more (16777216 SNPs x 10240 haplotypes)"
    for fn in (dense, dense_d, hits, hits_d):
        wide = {"ld_out": 1 << 26} if fn in (dense, dense_d) else {}
        assert fn(n_i=0) == E_ARG and said(fn, "n_i is 0"), err()
        assert fn(n_j=0) == E_ARG and said(fn, "n_j is 0"), err()
        assert fn(n_i=0, n_j=0, n_hap=0) == E_ARG and said(fn, "n_i is 0"), err()
        assert fn(n_hap=0) == E_ARG and said(fn, "n_hap is 0"), err()
        assert fn(n_hap=_lib.MAX_HAPS + 2) == E_UNSUPPORTED and said(fn, "n_hap 10242 > LDX_MAX_HAPS 10240"), err()
        assert fn(n_i=1 << 24, n_hap=10240) == E_UNSUPPORTED and said(fn, plane.format("alt_i")), err()
        assert fn(n_j=1 << 24, n_hap=10240, **wide) == E_UNSUPPORTED and said(fn, plane.format("alt_j")), err()
        assert fn(n_i=1 << 24, n_j=1 << 24, n_hap=10240, **wide) == E_UNSUPPORTED and said(fn, plane.format("alt_i")), err()
        assert fn(n_i=1 << 26, n_j=1 << 26, n_hap=64, **wide) == E_UNSUPPORTED, err()
        assert said(fn, "n_i x n_j = 67108864 x 67108864 needs 2^31 or more tiles of 256 x 128"), err()
    for fn in (dense, dense_d):
        assert fn(ld_out=49) == E_ARG and said(fn, "ld_out 49 < n_j 50"), err()
        assert fn(ld_out=49, n_i=0) == E_ARG and said(fn, "ld_out 49 < n_j 50"), err()
    for fn in (dense_d, hits_d):
        for n_hap in (63, _lib.MAX_HAPS + 1):                                # (parity speaks before the limit)
            assert fn(n_hap=n_hap) == E_ARG, err()
            assert said(fn, f"n_hap {n_hap} is odd (dosage pairs haplotypes 2k and 2k + 1 into individuals)"), err()
    for fn in (dense, hits):
        assert fn(n_hap=63, n_i=0) == E_ARG and said(fn, "n_i is 0")        # (an odd n_hap is fine for haplotype r)


def test_python_argument_rules_come_before_the_device():
    import torch
    from ld_tools_amd import LdxError, PackedPanel, ops
    z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731

    def host_panel(n_snps, n_hap, device=None):
        mk = (lambda n, dt: torch.zeros(n, dtype=dt, device=device)) if device else z
        return PackedPanel(n_snps, n_hap, mk(1, torch.uint8), mk(1, torch.uint8), mk(128, torch.int32), mk(128, torch.int32),
                           mk(128, torch.float64), mk(128, torch.float64), mk(128, torch.float64))

    a, b, odd = host_panel(10, 64), host_panel(7, 62), host_panel(10, 63)
    for fn in (ops.ld_rect, ops.ld_rect_hits):
        with pytest.raises(LdxError, match="haplotype count"):
            fn(a, b)
        with pytest.raises(LdxError, match="even n_hap"):
            fn(odd, odd, dosage=True)
        with pytest.raises(LdxError, match="different devices"):
            fn(a, host_panel(7, 64, device="meta"))
        with pytest.raises(LdxError, match="PackedPanel"):
            fn(a, "chr7")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(LdxError, match="threshold"):
            ops.ld_rect_hits(a, a, r2=bad)
    with pytest.raises(LdxError, match="out must be"):
        ops.ld_rect(a, a, out=torch.zeros((10, 9)))
    with pytest.raises(LdxError, match="out must be"):
        ops.ld_rect(a, a, out=torch.zeros((10, 12), dtype=torch.float64))
    with pytest.raises(LdxError, match="out must be"):
        ops.ld_rect(a, a, out=torch.zeros((12, 10)).t())
    if not torch.cuda.is_available():                                       # valid arguments: only now the device is asked for
        with pytest.raises(LdxError, match="HIP device"):
            ops.ld_rect(a, a)
        with pytest.raises(LdxError, match="HIP device"):
            ops.ld_rect_hits(a, a)


def test_rect_hits_host_on_a_hand_made_matrix():
    from ld_tools_amd import LdxError, ops
    t = 0.25
    on = np.float32(0.5)                                   # 0.5 *f32 0.5 == 0.25 exactly: on the bound
    below = np.nextafter(on, np.float32(0))                # its square rounds below 0.25
    above = np.nextafter(on, np.float32(1))
    assert np.multiply(on, on, dtype=np.float32) == np.float32(t) > np.multiply(below, below, dtype=np.float32)
    r = np.array([[-0.0, 0.0, on, below],
                  [-on, above, -below, 1.0],
                  [0.7, -1.0, -0.0, -above]], dtype=np.float32)
    loose, strict = ops.r2_bound(t), ops.r2_bound(t, strict=True)
    assert float(loose) == t and strict == np.nextafter(np.float32(t), np.float32(1))
    i, j = ops.rect_hits_host(r, loose)
    assert i.dtype == np.int64 and j.dtype == np.int64
    assert list(zip(i.tolist(), j.tolist())) == [(0, 2), (1, 0), (1, 1), (1, 3), (2, 0), (2, 1), (2, 3)]
    i, j = ops.rect_hits_host(r, strict)                   # the two cells exactly on the bound leave
    assert list(zip(i.tolist(), j.tolist())) == [(1, 1), (1, 3), (2, 0), (2, 1), (2, 3)]
    # -0.0f is never a hit and +0.0f only fails the bound: a bound of 0 (which the device entries refuse) tells them apart
    i, j = ops.rect_hits_host(r, np.float32(0))
    got = set(zip(i.tolist(), j.tolist()))
    assert (0, 1) in got and (0, 0) not in got and (2, 2) not in got and len(got) == r.size - 2
    i, j = ops.rect_hits_host(r, ops.r2_bound(1.0))        # 1.0 not strict: exactly +-1
    assert list(zip(i.tolist(), j.tolist())) == [(1, 3), (2, 1)]
    assert ops.rect_hits_host(r, ops.r2_bound(1.0, strict=True))[0].size == 0
    assert ops.rect_hits_host(np.zeros((0, 4), dtype=np.float32), loose)[0].size == 0
    with pytest.raises(LdxError, match="float32"):
        ops.rect_hits_host(r.astype(np.float64), loose)


def test_the_gpu_tests_panels_hold_what_the_tests_rely_on():
    """The planted-copy density of tests/test_gpu_ld_rect.py, pinned on the CPU with the exact oracle: cells at exactly +1 and
    -1 across the edge cases, degenerate and zero-numerator cells, and for the hits panel an expected set (from the oracle's r
    rounded to float32, which differs from a conforming kernel's cells by at most 4 ulps) that is neither empty, nor within
    reach of half the cells, nor within one batch of 256 at r^2 >= 0.2."""
    plus = minus = 0
    for shape, n_hap in rc.EDGE_CASES:
        ci, cj = rc.pair_codes(shape[0], shape[1], n_hap, seed=1000 * shape[0] + shape[1] + n_hap)
        assert ci.shape == (shape[0], n_hap) and cj.shape == (shape[1], n_hap) and ci.dtype == cj.dtype == np.int8
        ex = lx.Exact(np.concatenate([ci, cj]))
        blk = (slice(0, shape[0]), slice(shape[0], None))
        one = (ex.num2[blk] == ex.den2[blk]) & ~ex.degenerate[blk]
        plus += int((one & (ex.num[blk] > 0)).sum())
        minus += int((one & (ex.num[blk] < 0)).sum())
        if min(shape) >= 5:
            assert ex.degenerate[blk].any() and (~ex.degenerate[blk]).any()
    assert plus >= 10 and minus >= 10
    shape, n_hap = rc.HITS_CASE
    ci, cj = rc.pair_codes(shape[0], shape[1], n_hap, seed=1000 * shape[0] + shape[1] + n_hap, family=rc.FAMILY)
    ex = lx.Exact(np.concatenate([ci, cj]))
    r2 = ex.r2_64[:shape[0], shape[0]:]
    cells = shape[0] * shape[1]
    assert 256 * 2 < int((r2 >= 0.21).sum()) and int((r2 >= 0.19).sum()) < cells // 4
    assert int((r2 == 1.0).sum()) >= 5
    assert int(((r2 > 0.3) & (r2 < 0.9)).sum()) >= 10
    codes, rows, cols = rc.triangle_panel()
    exd = lx.Exact(codes)
    assert (~exd.live[rows]).any() and set(rows.tolist()) & set(cols.tolist()) and len(set(rows.tolist())) < rows.size
    assert (codes == 2).any() and (~exd.live).sum() >= 8


BLOCK_ATTRS = ("num", "den2", "num2", "degenerate", "zero_num", "r64", "r2_64")


@pytest.mark.parametrize("shape", rc.SHAPES, ids=str)
def test_exact_block_is_the_off_diagonal_block_of_the_stacked_oracle(shape):
    """ExactBlock / DosageExactBlock (the oracles of the walk cases, whose stacked squares would be too heavy) against
    Exact(stacked) / DosageExact(stacked): every attribute a cell check reads, equal."""
    n_i, n_j = shape
    ci, cj = rc.pair_codes(n_i, n_j, 254, seed=rc.pair_seed(shape, 254))
    stacked = np.concatenate([ci, cj])
    for block, full in ((lx.ExactBlock(ci, cj), lx.Exact(stacked)), (dx.DosageExactBlock(ci, cj), dx.DosageExact(stacked))):
        assert isinstance(block, lx.ExactBlock)
        for name in BLOCK_ATTRS:
            got, want = getattr(block, name), getattr(full, name)[:n_i, n_i:]
            assert got.shape == (n_i, n_j) and got.dtype == want.dtype, name
            assert np.array_equal(got, want), (type(block).__name__, name)
    # the other orientation is the transpose
    back = lx.ExactBlock(cj, ci)
    assert np.array_equal(back.num, lx.ExactBlock(ci, cj).num.T) and np.array_equal(back.den2, lx.ExactBlock(ci, cj).den2.T)


def test_walk_cases_cover_what_they_must():
    """The walk of rect_kernel (tile_of): bands of 16 I blocks of 256 rows.  The table must hold a band of exactly 16 blocks
    that is the whole grid, a band index >= 2, a last band shorter than 16 after a full one (of one block, of one ROW, and of
    two blocks), and the long side on J under one partial band."""
    assert (rc.I_BLOCK, rc.BAND_BLOCKS) == (256, 16)
    bands = {case: rc.walk_bands(case[0][0]) for case in rc.WALK_CASES}
    assert len(bands) == len(rc.WALK_CASES) == 5
    assert [16] in bands.values()                                          # one full band, nothing after it
    assert any(len(b) >= 3 for b in bands.values())                        # a band index >= 2
    assert any(len(b) >= 2 and b[-2] == 16 and b[-1] < 16 for b in bands.values())
    assert bands[((4096, 130), 64)] == [16] and bands[((4097, 130), 254)] == [16, 1] and 4097 % rc.I_BLOCK == 1
    assert bands[((4353, 257), 254)] == [16, 2] and bands[((8200, 130), 64)] == [16, 16, 1]
    assert bands[((130, 4353), 254)] == [1] and (4353 + 127) // 128 == 35
    assert rc.WALK_HITS_CASE in rc.WALK_CASES and rc.WALK_SWAPPED in rc.WALK_CASES
    for (shape, n_hap) in rc.WALK_CASES:
        assert n_hap % 2 == 0                                              # the dosage form applies
        assert shape[0] % rc.I_BLOCK != 0 or shape == (4096, 130)          # partial last blocks but for the exact band
    # the planted copies reach across the sides at size, and the swapped case is the hits case's transpose
    ci, cj = rc.walk_codes(*rc.WALK_HITS_CASE)
    si, sj = rc.walk_codes(*rc.WALK_SWAPPED)
    assert ci.shape == (4353, 254) and cj.shape == (257, 254) and si.shape == (130, 254) and sj.shape == (4353, 254)
    assert np.array_equal(si, cj[:130]) and np.array_equal(sj, ci)
    ex = lx.ExactBlock(ci, cj)
    one = (ex.num2 == ex.den2) & ~ex.degenerate
    assert int((one & (ex.num > 0)).sum()) >= 10 and int((one & (ex.num < 0)).sum()) >= 10
    assert ex.degenerate.any() and ex.zero_num.any()
    rows_hit = np.flatnonzero(one.any(axis=1))
    assert (rows_hit >= 4096).any() and (rows_hit < 4096).any()            # |r| = 1 cells in both bands
    hits = int((ex.r2_64 >= 0.21).sum())
    assert 0 < hits and int((ex.r2_64 >= 0.19).sum()) < ex.num.size // 4


# ---- drivers/rect.py without a device ----------------------------------------------------------------------------------------
def two_chromosomes(**kw):
    a, names = fakevcf.make_chromosome(chrom="6", n_variants=48, seed=11)
    b, names_b = fakevcf.make_chromosome(chrom="7", n_variants=37, seed=23, first_pos=5000, step=211, **kw)
    assert names == names_b
    return fakevcf.FakeVcf(a.records + b.records), names


def rs_rows(vcf, chrom):
    seen, rows = set(), []
    for rec in vcf.records:
        if rec.chrom == chrom and rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
            seen.add(rec.id)
            rows.append([rec.pos, rec.id])
    return rows


def test_rect_driver_reads_both_sides_and_refuses_what_it_must():
    from ld_tools_amd import LdxError
    from ld_tools_amd.drivers import rect
    vcf, names = two_chromosomes()
    rows_i, rows_j = rs_rows(vcf, "6"), rs_rows(vcf, "7")
    si, sj = rect.read_sides(vcf, "6", rows_i[::-1], "7", rows_j + [[12, "rs1"]], names)   # (a row without a record is left out)
    assert si.n == len(rows_i) and sj.n == len(rows_j) and (si.chrom, sj.chrom) == ("6", "7")
    assert si.poss == sorted(p for p, _ in rows_i) and sj.poss == sorted(p for p, _ in rows_j)
    assert si.rs_ids == [rs for _, rs in sorted(rows_i[::-1], key=lambda r: r[0])]   # (stable: ties keep the caller's order)
    assert si.codes.shape == (si.n, 2 * (len(names) - 1)) and sj.codes.shape == (sj.n, si.codes.shape[1])   # (no record carries sample 7)
    assert si.codes.dtype == np.int8 and set(np.unique(si.codes).tolist()) <= {0, 1, 2}
    # the same file for both sides, or one per side
    ti, tj = rect.read_sides((vcf, vcf), "6", rows_i[::-1], "7", rows_j, names)
    assert np.array_equal(ti.codes, si.codes) and np.array_equal(tj.codes, sj.codes)
    # two lists of one chromosome
    ui, uj = rect.read_sides(vcf, "6", rows_i[:10], "6", rows_i[5:], names)
    assert ui.n == 10 and uj.n == len(rows_i) - 5 and np.array_equal(ui.codes[5:], uj.codes[:5])
    with pytest.raises(LdxError, match="no variant of the columns"):
        rect.read_sides(vcf, "6", rows_i, "7", [[12, "rs1"]], names)
    with pytest.raises(LdxError, match="no variant of the rows"):
        rect.read_sides(vcf, "8", rows_i, "7", rows_j, names)
    # mixed ploidy inside one side
    ragged, _ = two_chromosomes(haploid_from=20)
    with pytest.raises(LdxError, match="mixed ploidy"):
        rect.read_sides(ragged, "6", rows_i, "7", rs_rows(ragged, "7"), names)
    # mixed ploidy between the sides: every record of chromosome 7 haploid for every second sample
    between, _ = two_chromosomes(haploid_from=0)
    with pytest.raises(LdxError, match="mixed ploidy between the two sides"):
        rect.read_sides(between, "6", rows_i, "7", rs_rows(between, "7"), names)
    # samples that differ between the sides: chromosome 7's records lack one more sample
    fewer, _ = two_chromosomes()
    for rec in fewer.records:
        if rec.chrom == "7":
            rec.samples.pop(names[3])
    with pytest.raises(LdxError, match="samples differ between the two sides"):
        rect.read_sides(fewer, "6", rows_i, "7", rows_j, names)
    # ... and inside one side
    some, _ = two_chromosomes()
    some.records[-1].samples.pop(names[3])
    with pytest.raises(LdxError, match="carry different samples"):
        rect.read_sides(some, "6", rows_i, "7", rows_j, names)
    with pytest.raises(LdxError, match="no genotype of the selected samples"):
        rect.read_sides(vcf, "6", rows_i, "7", rows_j, ["nobody"])


def test_write_rect_matrix_files_names_and_headers(tmp_path):
    from ld_tools_amd.drivers import rect
    from ld_tools_amd.drivers.rmatrix import VARIANTS_HEADER
    vcf, names = two_chromosomes()
    si, sj = rect.read_sides(vcf, "6", rs_rows(vcf, "6"), "7", rs_rows(vcf, "7"), names)
    si.alt_freqs = [round(float((row == 1).sum()) / row.size, 4) for row in si.codes]
    sj.alt_freqs = [round(float((row == 1).sum()) / row.size, 4) for row in sj.codes]
    r = np.random.default_rng(3).uniform(-1, 1, (si.n, sj.n)).astype(np.float32)
    r[0, 0], r[1, 1] = -0.0, 0.0
    m = rect.RectMatrix(si, sj, False, r)                   # (a host array stands in for the device tensor)
    base = str(tmp_path / "lead_x_chr7")
    paths = rect.write_rect_matrix(base, m, rows_per_block=5)
    assert paths == [base + ".npy", base + ".rows.tsv", base + ".cols.tsv"]
    got = np.load(paths[0], mmap_mode="r")
    assert got.shape == (si.n, sj.n) and got.dtype == np.float32
    assert np.array_equal(np.asarray(got).view(np.uint32), r.view(np.uint32))
    for path, side in ((paths[1], si), (paths[2], sj)):
        lines = Path(path).read_text().splitlines(keepends=True)
        assert lines[0] == VARIANTS_HEADER and len(lines) == side.n + 1
        fields = [ln.rstrip("\n").split("\t") for ln in lines[1:]]
        assert [int(f[0]) for f in fields] == list(range(side.n))
        assert [f[1] for f in fields] == side.rs_ids and [int(f[2]) for f in fields] == side.poss
        assert [f[3] for f in fields] == side.refs and [f[4] for f in fields] == side.alts
        assert [float(f[5]) for f in fields] == side.alt_freqs

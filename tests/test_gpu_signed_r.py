"""GPU: signed-r cells (LDX_OUT_R32) -- against independent definitions, across the three triangle kernels, the block export
ldx_triangle_r_block_dev and the drivers/rmatrix.py writer.

Contract (include/ldx.h): cell = float32 of (n n11 - a_i a_j) / sqrt(a_i r_i a_j r_j) within 4 float32 ulps, +0.0 exactly
when the numerator is 0, -0.0 for a degenerate SNP (a r == 0); bit-identical on every kernel.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import fakevcf  # noqa: E402

pytestmark = pytest.mark.gpu

PATHS = ("popcount", "mfma", "fp4")


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    from ld_tools_amd import _lib

    buf = __import__("ctypes").create_string_buffer(64)
    _lib.check(_lib.lib.ldx_device_arch(0, buf, 64))
    assert buf.value.decode().startswith("gfx950"), buf.value
    return torch.device("cuda", 0)


def lower_index(n, dev, fmt="r32"):
    """(rows, cols, flat strip index) of every cell i > j of an n-SNP triangle, as device tensors."""
    import torch

    from ld_tools_amd._lib import lib
    ij = torch.tril_indices(n, n, -1, device=dev)
    i, j = ij[0], ij[1]
    G = lib.ldx_padded_snps(n) // 8
    t, g = j // 128, i // 8
    u = t * G - 8 * t * (t - 1) + (g - 16 * t)
    c = j % 128
    if fmt == "ld32":
        off = (i % 8) * 128 + (c // 64) * 64 + (c % 32) * 2 + (c // 32) % 2
    else:
        off = (i % 8) * 128 + (c % 32) * 4 + c // 32
    return i, j, u * 1024 + off


def ulp_err(got32, exact64):
    """|got - exact| in float32 ulps of the exact value (exact != 0)."""
    import torch
    _, ex = torch.frexp(exact64)
    ulp = torch.ldexp(torch.ones_like(exact64), (ex - 24).to(torch.int32))
    return (got32.double() - exact64).abs() / ulp


def is_neg_zero(x):
    import torch
    return (x == 0) & torch.signbit(x)


def is_pos_zero(x):
    import torch
    return (x == 0) & ~torch.signbit(x)


def inject_degenerate(codes, rows):
    """Rows: all REF, all ALT, ALT + missing only (no REF), REF + missing only (no ALT)."""
    kinds = [np.int8(0), np.int8(1), None, None]
    for k, r in enumerate(rows):
        if k % 4 == 2:
            codes[r] = np.where(codes[r] == 0, 2, codes[r]).astype(np.int8)
            codes[r, 0] = 1
        elif k % 4 == 3:
            codes[r] = np.where(codes[r] == 1, 2, codes[r]).astype(np.int8)
            codes[r, 0] = 0
        else:
            codes[r] = kinds[k % 4]
    return codes


def corrcoef_check(codes, res, dev):
    """Every cell of a missing-free panel vs np.corrcoef of the 0/1 rows (float64); monomorphic rows give -0.0."""
    import torch
    n = codes.shape[0]
    x = codes.astype(np.float64)
    poly = (x.min(axis=1) != x.max(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        cc = np.corrcoef(x) if n > 1 else np.ones((1, 1))
    i, j, idx = lower_index(n, dev)
    got = res.r32[idx]
    exact = torch.from_numpy(cc).to(dev)[i, j]
    deg = ~(torch.from_numpy(poly).to(dev)[i] & torch.from_numpy(poly).to(dev)[j])
    assert bool(is_neg_zero(got[deg]).all())
    ok = ~deg
    e, g = exact[ok], got[ok]
    # np.corrcoef's own float64 error (~1e-16 absolute after its centring) bounds what the comparison can resolve
    nz = e.abs() > 1e-12
    assert bool((ulp_err(g[nz], e[nz]) <= 4.0).all()), float(ulp_err(g[nz], e[nz]).max())
    assert bool(((g[~nz].double() - e[~nz]).abs() <= 1e-12).all())


@pytest.mark.parametrize("shape", [(500, 5008), (300, 1008), (257, 37)])
def test_r32_equals_corrcoef_without_missing_codes(gpu, shape):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = shape
    codes = synth.synth_codes_host(n, h, seed=3 + n)
    codes[7] = 0                                      # monomorphic rows: -0.0
    codes[n - 2] = 1
    p = PackedPanel.from_codes(codes, gpu)
    corrcoef_check(codes, ops.ld_triangle(p, fmt="r32"), gpu)


@pytest.fixture(scope="module")
def bench_panel(gpu):
    """10 000 x 5008 with missing codes and injected degenerate rows (the bench shape)."""
    from ld_tools_amd import PackedPanel, synth
    codes = synth.synth_codes_host(10_000, 5008, seed=17, miss=0.004)
    codes = inject_degenerate(codes, [0, 5, 127, 128, 129, 4097, 7000, 9998, 9999])
    h = np.arange(5008)
    codes[300] = (h < 2504).astype(np.int8)           # with row 301: n11 = 1252 = a a / n, a zero numerator
    codes[301] = (h % 2 == 0).astype(np.int8)
    return PackedPanel.from_codes(codes, gpu)


def test_r32_with_missing_codes_and_degenerate_snps(gpu, bench_panel):
    import torch

    from ld_tools_amd import ops
    p = bench_panel
    n, nh = p.n_snps, p.n_hap
    res = ops.ld_triangle(p, fmt="r32")
    n11 = ops.pair_counts(p)                          # exact counts, pinned to the oracle elsewhere
    a = p.acnt[:n].double()
    r = p.rcnt[:n].double()
    i, j, idx = lower_index(n, gpu)
    got = res.r32[idx]
    num = nh * n11[i, j].double() - a[i] * a[j]
    den2 = a[i] * r[i] * a[j] * r[j]
    deg = den2 == 0
    assert int(deg.sum()) > 0
    assert bool(is_neg_zero(got[deg]).all())
    zero = (num == 0) & ~deg
    assert int(zero.sum()) > 0
    assert bool(is_pos_zero(got[zero]).all())
    live = ~deg & ~zero
    exact = num[live] / torch.sqrt(den2[live])
    assert bool((ulp_err(got[live], exact) <= 4.0).all()), float(ulp_err(got[live], exact).max())
    assert bool(((got[live] > 0) == (num[live] > 0)).all())
    del n11, num, den2, exact
    # r^2 against the unrounded r^2 of the ld32 path (calc_ld.py:86-90)
    raw = ops.ld_triangle(p, fmt="ld32", want_raw=True)
    _, _, idx32 = lower_index(n, gpu, "ld32")
    rsq = raw.raw[idx32, 0]
    g2 = got.double() ** 2
    nzr = rsq != 0
    # the reference's d = f11 - fa1 fa2 is a rounding residue where n n11 == a1 a2: r^2 ~ 1e-30 there, r = +0.0
    assert bool(((g2[nzr] - rsq[nzr]).abs() <= 2e-6 * rsq[nzr] + 1e-20).all())
    assert bool((got[~nzr] == 0).all())


def _cells_bits(p, path, **kw):
    from ld_tools_amd import ops
    return ops.ld_triangle(p, fmt="r32", path=path, **kw).r32.view(dtype=__import__("torch").int32).clone()


def test_three_kernels_bit_identical_bench(gpu, bench_panel):
    import torch
    base = _cells_bits(bench_panel, "popcount")
    for path in ("mfma", "fp4", None):
        assert torch.equal(_cells_bits(bench_panel, path), base), path


@pytest.mark.parametrize("n_hap", [1, 37, 1008, 5008, 10240])
def test_three_kernels_bit_identical_edges(gpu, n_hap):
    import torch

    from ld_tools_amd import PackedPanel, ops, synth
    for n in (1, 2, 127, 128, 129, 1000):
        codes = synth.synth_codes_host(n, n_hap, seed=n + n_hap, miss=0.01)
        if n > 2:
            codes = inject_degenerate(codes, [1, n - 1])
        p = PackedPanel.from_codes(codes, gpu)
        base = _cells_bits(p, "popcount")
        for path in ("mfma", "fp4"):
            assert torch.equal(_cells_bits(p, path), base), (n, n_hap, path)
        if n_hap == 1 and n > 1:                      # one haplotype: every SNP is degenerate
            _, _, idx = lower_index(n, gpu)
            cells = ops.ld_triangle(p, fmt="r32").r32[idx]
            assert bool(is_neg_zero(cells).all())


def test_ragged_unit_ranges_and_buffer_reuse(gpu):
    import torch

    from ld_tools_amd import PackedPanel, ops, synth
    p = PackedPanel.from_codes(synth.synth_codes_host(3000, 1008, seed=5, miss=0.003), gpu)
    full = ops.ld_triangle(p, fmt="r32")
    U = p.n_units
    for path in PATHS:
        cuts = [0, 1, 77, 1000, 1001, U // 2 + 3, U - 5, U]
        pieces = [ops.ld_triangle(p, unit_range=(a, b), fmt="r32", path=path).r32 for a, b in zip(cuts, cuts[1:])]
        assert torch.equal(torch.cat(pieces).view(torch.int32), full.r32.view(torch.int32)), path
        out = ops.ld_triangle(p, fmt="r32", path=path)
        first = out.r32.view(torch.int32).clone()
        again = ops.ld_triangle(p, fmt="r32", path=path, out=out)
        assert again is out
        assert torch.equal(out.r32.view(torch.int32), first)
        assert torch.equal(first, full.r32.view(torch.int32))


def test_rejections(gpu):
    from ld_tools_amd import LdxError, PackedPanel, ops, synth
    p = PackedPanel.from_codes(synth.synth_codes_host(300, 100, seed=2), gpu)
    with pytest.raises(LdxError):
        ops.ld_triangle(p, fmt="r32", want_raw=True)
    with pytest.raises(LdxError):
        ops.ld_triangle(p, fmt="r32", want_n11=True)
    res = ops.ld_triangle(p, fmt="r32")
    assert res.fmt == "r32" and res.cells is res.r32 and res.r32.dtype.is_floating_point
    with pytest.raises(LdxError):
        res.dense()
    with pytest.raises(LdxError):
        res.dense_values()
    with pytest.raises(LdxError):
        res.k_and_int0([0])
    shard = ops.ld_triangle(p, fmt="r32", unit_range=(0, 10))
    with pytest.raises(LdxError):
        shard.r_matrix()
    with pytest.raises(LdxError):
        ops.ld_triangle(p, fmt="k16").r_matrix()
    with pytest.raises(LdxError):
        res.r_matrix(rows=(0, 301))
    with pytest.raises(LdxError):                      # `out` of another format
        ops.ld_triangle(p, fmt="k16", out=res)


def test_block_export(gpu):
    import torch

    from ld_tools_amd import PackedPanel, ops, synth
    n = 3000
    codes = synth.synth_codes_host(n, 1008, seed=9, miss=0.003, miss_rows=0.5)
    codes = inject_degenerate(codes, [3, 128, 1500, 2999])
    p = PackedPanel.from_codes(codes, gpu)
    res = ops.ld_triangle(p, fmt="r32")
    full = res.r_matrix()
    assert full.shape == (n, n) and full.dtype == torch.float32
    bits = full.view(torch.int32)
    assert torch.equal(bits, bits.t().contiguous())
    i, j, idx = lower_index(n, gpu)
    assert torch.equal(full[i, j].view(torch.int32), res.r32[idx].view(torch.int32))
    a = p.acnt[:n].cpu().numpy().astype(np.float64)
    r = p.rcnt[:n].cpu().numpy().astype(np.float64)
    d = torch.diagonal(full).cpu().numpy()
    deg = a * r == 0
    complete = (a + r == 1008) & ~deg
    assert deg.sum() >= 4 and complete.sum() > 100 and (~deg & ~complete).sum() > 100
    assert np.all(d[complete] == 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = ((1008 - a) / r).astype(np.float32)
    assert np.array_equal(d[~deg].view(np.int32), want[~deg].view(np.int32))
    assert np.all((d[deg] == 0) & np.signbit(d[deg]))
    for rows, cols in [((129, 1300), (2999, 3000)), ((0, n), (0, n)), ((5, 5), (0, 10)), ((0, 10), (7, 7)),
                       ((1234, 2999), (17, 2222)), ((2000, 2100), (1, 129)), ((0, 1), (0, 3000)), ((2890, 3000), (2890, 3000))]:
        blk = res.r_matrix(rows=rows, cols=cols)
        assert blk.shape == (rows[1] - rows[0], cols[1] - cols[0])
        assert torch.equal(blk.view(torch.int32), bits[rows[0]:rows[1], cols[0]:cols[1]]), (rows, cols)


def test_rmatrix_driver(gpu, tmp_path):
    from ld_tools_amd.drivers import r_matrix, triangle_matrix, write_r_matrix
    from ld_tools_amd.drivers.rmatrix import VARIANTS_HEADER
    vcf, names = fakevcf.make_chromosome()
    seen, rows = set(), []
    for rec in vcf.records:
        if rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
            seen.add(rec.id)
            rows.append([rec.pos, rec.id])
    rows = rows[::-1]                                  # the driver sorts by position
    m = r_matrix(vcf, "6", rows, names)
    base = str(tmp_path / "chr6_r")
    n = m.n
    assert n == len(rows)
    paths = write_r_matrix(base, m, rows_per_block=7)
    assert paths == [base + ".npy", base + ".variants.tsv"]
    got = np.load(base + ".npy", mmap_mode="r")
    assert got.shape == (n, n) and got.dtype == np.float32
    assert np.array_equal(np.asarray(got).view(np.int32), m.result.r_matrix().cpu().numpy().view(np.int32))
    tri = triangle_matrix(vcf, "6", rows, names)
    lines = Path(base + ".variants.tsv").read_text().splitlines(keepends=True)
    assert lines[0] == VARIANTS_HEADER and len(lines) == n + 1
    fields = [ln.rstrip("\n").split("\t") for ln in lines[1:]]
    assert [f[1] for f in fields] == tri.rs_ids_srtd
    assert [int(f[2]) for f in fields] == tri.poss_srtd
    assert [f[3] + "/" + f[4] for f in fields] == tri.alleles
    assert [float(f[5]) for f in fields] == tri.alt_freqs
    # a row without a matching record is left out of both files
    m2 = r_matrix(vcf, "6", rows + [[12, "rs1"]], names)
    assert m2.rs_ids == m.rs_ids


def test_rmatrix_driver_refuses_mixed_ploidy(gpu):
    from ld_tools_amd import LdxError
    from ld_tools_amd.drivers import r_matrix
    vcf, names = fakevcf.make_chromosome(haploid_from=30)
    rows = [[rec.pos, rec.id] for rec in vcf.records if rec.id.startswith("rs") and ";" not in rec.id][:40]
    with pytest.raises(LdxError, match="mixed ploidy"):
        r_matrix(vcf, "6", rows, names)

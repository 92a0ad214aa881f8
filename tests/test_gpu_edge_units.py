"""GPU: the FP4 triangle kernel's edge units -- diagonal units, the partly padded last row group, the all-padding row
group and the last tile's padding columns -- against the popcount kernel, every cell bit for bit.

These units run the fp32 tier with the cells outside the triangle forced to zero (csrc/ldx_mfma.hip, epilogue_f32,
`edge`), and a unit of padding rows only skips its matrix work and stores zero cells.  Every output is poisoned before
the launch, so a cell the kernel leaves unwritten fails the comparison.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL_N = [1, 2, 63, 64, 65, 127, 128, 129, 191, 255, 257, 4097]
LARGE_N = [9999, 10000, 10047, 10048, 10049]
HAPS = [1, 64, 1008, 5008, 10240]
FORMATS = ["k16", "ld32", "k16r", "k16d"]


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)

    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(-1).view(__import__("torch").uint8)


def _poisoned(panel, fmt, path, unit_range=None):
    """ld_triangle into buffers filled with -1 first: a cell the kernel does not write stays -1."""
    from ld_tools_amd import ld_triangle

    res = ld_triangle(panel, fmt=fmt, path=path, unit_range=unit_range)
    res.cells.fill_(-1)
    return ld_triangle(panel, fmt=fmt, path=path, unit_range=unit_range, out=res)


def _edge_codes(n, h, seed):
    """Synthetic codes with degenerate and odd SNPs on the tiles' diagonals and in the last real rows."""
    from ld_tools_amd import synth

    codes = synth.synth_codes_host(n, h, seed=seed, miss=0.002)
    special = sorted({r for r in (0, 1, 62, 63, 64, 127, 128, 129, 190, n - 6, n - 3, n - 2, n - 1) if 0 <= r < n})
    for k, r in enumerate(special):
        kind = k % 5
        if kind == 0:
            codes[r] = 0                       # monomorphic REF: degenerate, int-0 cells
        elif kind == 1:
            codes[r] = 1                       # monomorphic ALT
        elif kind == 2:
            codes[r] = 2                       # nothing but missing codes
        elif kind == 3:
            codes[r, ::7] = 2                  # many missing codes: parks in the fp32 tier
        else:
            codes[r, 3:6] = 2                  # a few missing codes: ordinary
    return codes


def _check(panel, fmts, tag, unit_range=None):
    import torch

    for fmt in fmts:
        got = _poisoned(panel, fmt, "fp4", unit_range)
        want = _poisoned(panel, fmt, "popcount", unit_range)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got.cells), _bits(want.cells)), (tag, fmt, unit_range)


@pytest.mark.parametrize("n", SMALL_N)
def test_edge_units_small_panels(gpu, n):
    from ld_tools_amd import PackedPanel

    for h in HAPS:
        p = PackedPanel.from_codes(_edge_codes(n, h, seed=100 + n + h))
        _check(p, FORMATS, (n, h))


@pytest.mark.parametrize("n", LARGE_N)
def test_edge_units_large_panels(gpu, n):
    from ld_tools_amd import PackedPanel

    for h in (1008, 5008) if n != 10048 else HAPS:
        p = PackedPanel.from_codes(_edge_codes(n, h, seed=7 * n + h))
        _check(p, FORMATS if h == 5008 else ["k16", "k16r"], (n, h))


@pytest.mark.parametrize("n,h", [(129, 1008), (1111, 777), (4097, 5008), (10049, 1008)])
def test_edge_units_ranges_inside_first_passes(gpu, n, h):
    """Unit ranges that start and end inside tiles' first passes (the diagonal units): the pieces, concatenated, equal
    the whole triangle of the popcount kernel."""
    import torch

    from ld_tools_amd import PackedPanel
    from ld_tools_amd._lib import lib

    p = PackedPanel.from_codes(_edge_codes(n, h, seed=n + 3 * h))
    total = p.n_units
    T = (n + 127) // 128
    cuts = {0, total}
    for t in sorted({0, T // 2, T - 1}):
        tb = int(lib.ldx_triangle_tile_base(n, t))
        for off in (3, 8, 29):                     # inside the first 64-row unit, on its boundary, inside the second
            if 0 < tb + off < total:
                cuts.add(tb + off)
    cuts = sorted(cuts)
    for fmt in ("k16", "ld32"):
        want = _poisoned(p, fmt, "popcount")
        pieces = [_poisoned(p, fmt, "fp4", (a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
        got = torch.cat([x.cells for x in pieces])
        assert torch.equal(_bits(got), _bits(want.cells)), (n, h, fmt, cuts)


@pytest.mark.parametrize("n,h", [(65, 1008), (257, 5008), (1111, 777), (10000, 5008)])
def test_edge_units_half_height_tickets(gpu, n, h):
    """Every pass halved, and a mix: the half-height units of the edge (a last real group of 32 rows or fewer, a padding
    half) give the same cells."""
    from ld_tools_amd import PackedPanel
    from ld_tools_amd._lib import lib

    p = PackedPanel.from_codes(_edge_codes(n, h, seed=n * h % 9973))
    try:
        for short in (1000000, 37):
            lib.ldx_debug_force_short_passes(short)
            _check(p, ("k16", "ld32", "k16d"), (n, h, short))
    finally:
        lib.ldx_debug_force_short_passes(-1)


def test_edge_rows_of_the_bench_panel_against_the_oracle(gpu):
    """10 000 x 5008 with degenerate and odd SNPs near the diagonal and at the end: rows through the diagonal units and the
    last real rows, all their cells, against the C oracle."""
    from ld_tools_amd import PackedPanel, ld_triangle
    from oracle import c_oracle

    n, h = 10000, 5008
    codes = _edge_codes(n, h, seed=2024)
    p = PackedPanel.from_codes(codes)
    res = ld_triangle(p, fmt="k16", path="fp4")
    o = c_oracle.Panel(codes)
    for r0 in (63, 64, 128, 129, 9983, 9984, 9994, 9997, 9998, 9999):
        t = o.triangle(r0, r0 + 1, libm_pow=True)
        cols = np.arange(r0, dtype=np.int64)
        kk, int0, esc = res.k_and_int0(res.cell_index(np.full(r0, r0), cols))
        want_k = np.stack([np.rint(t["rsq_rnd"][r0, :r0] * 1e4), np.rint(t["dp_rnd"][r0, :r0] * 1e4)], axis=1)
        ok = ~esc
        assert np.array_equal(kk[ok], want_k[ok].astype(np.int64)), r0
        assert np.array_equal(int0[:, 0], (t["flags"][r0, :r0] & 2) != 0), r0
        assert np.array_equal(int0[:, 1], (t["flags"][r0, :r0] & 1) != 0), r0

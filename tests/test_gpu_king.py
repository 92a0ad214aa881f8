"""GPU: sample relatedness (include/ldx.h, "sample relatedness") against the host oracle: the four count planes exactly and the
kinship / IBS cells bit for bit, over shapes that cross an accumulator tile, a wave, one and two workgroup tiles, one MFMA
K-step, one chunk, one K-block and the minimum slice; with holes (shortcut and general tiles, and both in one matrix) and with
forced K slices; the special panels; the invariances; the cells on tuples; the argument rules."""
import ctypes as C

import numpy as np
import pytest

from ld_king_exact import HOLES, N_IND, N_SLICES, N_SNPS, N_SNPS_LONG, panel_codes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def ints(sc):
    return sc.counts.cpu().numpy().view(np.uint32).astype(np.int64)


def host_cells(counts):
    from ld_tools_amd import ibs_cell_host, king_cell_host

    N, HH, IBS0, HET = counts
    return king_cell_host(N, HH, IBS0, HET, HET.T), ibs_cell_host(N, HH, IBS0, HET, HET.T)


def check_cells(sc, want):
    kin, ibs = host_cells(want)
    assert np.array_equal(bits(sc.kinship().cpu().numpy()), bits(kin))
    assert np.array_equal(bits(sc.ibs().cpu().numpy()), bits(ibs))


def same(a, b):
    return torch.equal(a.counts, b.counts) and torch.equal(a.kinship().view(torch.int32), b.kinship().view(torch.int32)) \
        and torch.equal(a.ibs().view(torch.int32), b.ibs().view(torch.int32))


@pytest.mark.parametrize("holes", HOLES)
@pytest.mark.parametrize("n_ind", N_IND)
def test_counts_exact_and_cells_bit_for_bit(gpu, n_ind, holes):
    from ld_tools_amd import PackedPanel, sample_counts, sample_counts_host

    for n_snps in N_SNPS:
        codes = panel_codes(n_ind, n_snps, seed=1000 * n_ind + n_snps, holes=holes)
        want = sample_counts_host(codes)
        panel = PackedPanel.from_codes(codes, gpu)
        for n_slices in N_SLICES:
            sc = sample_counts(panel, n_slices=n_slices)
            assert sc.n_snps == n_snps and sc.n_ind == n_ind
            assert np.array_equal(ints(sc), want), (n_snps, n_slices)
        check_cells(sc, want)
        ibs1 = want[3] + want[3].T - 2 * want[1]
        assert np.array_equal(sc.ibs1.cpu().numpy(), ibs1) and np.array_equal(sc.ibs2.cpu().numpy(), want[0] - ibs1 - want[2])


@pytest.mark.parametrize("holes", ["none", "3%"])
@pytest.mark.parametrize("n_ind", [3, 129])
def test_around_the_minimum_slice(gpu, n_ind, holes):
    """The kernel's minimum slice length +-1 and the first panel the automatic choice cuts in two, with forced slice counts."""
    from ld_tools_amd import PackedPanel, sample_counts, sample_counts_host

    codes = panel_codes(n_ind, max(N_SNPS_LONG), seed=77 + n_ind, holes=holes)
    for n_snps in N_SNPS_LONG:
        want = sample_counts_host(codes[:n_snps])
        panel = PackedPanel.from_codes(codes[:n_snps], gpu)
        for n_slices in N_SLICES:
            assert np.array_equal(ints(sample_counts(panel, n_slices=n_slices)), want), (n_snps, n_slices)
    check_cells(sample_counts(panel), want)


def test_medium_panel(gpu):
    from ld_tools_amd import PackedPanel, sample_counts, sample_counts_host

    codes = panel_codes(300, 20000, seed=9, holes="3%")
    want = sample_counts_host(codes)
    sc = sample_counts(PackedPanel.from_codes(codes, gpu))
    assert np.array_equal(ints(sc), want)
    check_cells(sc, want)
    assert np.array_equal(ints(sample_counts(PackedPanel.from_codes(codes, gpu), store_snps=3001)), want)   # seven stores, accumulated


MOST_IND = 39 * 128 + 1   # 4993 individuals: T = 40 tile rows, 820 lower tiles, the most LDX_MAX_HAPS allows
_MOST = {}


def most_individuals(holes, gpu):
    """(codes, host counts as int32 [4, n_ind, n_ind], the same on the device) of the 4993-individual panel, once per ``holes``."""
    from ld_tools_amd import sample_counts_host

    if holes not in _MOST:
        codes = panel_codes(MOST_IND, 130, seed=4993 + len(holes), holes=holes)
        want = sample_counts_host(codes).astype(np.int32)      # counts <= 130; the int64 copy would be 800 MB
        _MOST[holes] = (codes, want, torch.from_numpy(want).to(gpu))
    return _MOST[holes]


@pytest.mark.parametrize("n_slices", [None, 2])
@pytest.mark.parametrize("holes", ["single", "3%"])
def test_every_tile_number_the_counts_kernel_can_be_given(gpu, holes, n_slices):
    """counts_kernel turns a workgroup number into a lower tile (ti, tj) with a square root and two correcting loops; the other
    cases reach 6 tiles.  Here all 820 of the largest panel, every count compared on the device.  With "single" the one
    missing genotype (individual 2496) makes tile row and column 19 general tiles amid shortcut tiles across the triangle."""
    from ld_tools_amd import PackedPanel, _lib, ibs_cell_host, king_cell_host, sample_counts

    assert (MOST_IND + 127) // 128 == (_lib.MAX_HAPS // 2 + 127) // 128 == 40 and 40 * 41 // 2 == 820   # no panel has more tiles
    codes, want, want_dev = most_individuals(holes, gpu)
    sc = sample_counts(PackedPanel.from_codes(codes, gpu), n_slices=n_slices)
    assert sc.n_ind == MOST_IND and sc.n_snps == 130
    if not torch.equal(sc.counts, want_dev):
        plane, a, b = (int(x) for x in torch.nonzero(sc.counts != want_dev)[0])
        raise AssertionError(f"plane {plane}, individuals ({a}, {b}), tile ({a // 128}, {b // 128}): {sc.counts[plane, a, b].item()} "
                             f"!= {want[plane, a, b]}")
    if holes == "single":
        assert 0 < (MOST_IND // 2) // 128 < 39 and int((want[0] != 130).sum()) == 2 * MOST_IND - 1
    # the cells: the last tile row (one individual) against every partner, and 10 000 seeded cells
    rng = np.random.default_rng(820)
    a = np.concatenate([np.full(MOST_IND, MOST_IND - 1), rng.integers(0, MOST_IND, size=10_000)])
    b = np.concatenate([np.arange(MOST_IND), rng.integers(0, MOST_IND, size=10_000)])
    tup = (want[0][a, b], want[1][a, b], want[2][a, b], want[3][a, b], want[3][b, a])
    ai, bi = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    assert np.array_equal(bits(sc.kinship()[ai, bi].cpu().numpy()), bits(king_cell_host(*tup)))
    assert np.array_equal(bits(sc.ibs()[ai, bi].cpu().numpy()), bits(ibs_cell_host(*tup)))


def test_special_panels(gpu):
    from ld_tools_amd import PackedPanel, sample_counts, sample_counts_host

    codes = panel_codes(140, 500, seed=21, holes="3%")
    codes[:, 2 * 5: 2 * 5 + 2] = 2                        # individual 5: every genotype missing
    codes[:, 2 * 131 + 1] = codes[:, 2 * 131]             # individual 131: no heterozygous call
    want = sample_counts_host(codes)
    sc = sample_counts(PackedPanel.from_codes(codes, gpu))
    assert np.array_equal(ints(sc), want)
    check_cells(sc, want)
    n, kin, ibs = ints(sc)[0], sc.kinship().cpu().numpy(), sc.ibs().cpu().numpy()
    minus0 = bits(np.float32(-0.0))
    assert (n[5] == 0).all() and (n[:, 5] == 0).all()
    assert (bits(kin[5]) == minus0).all() and (bits(kin[:, 5]) == minus0).all()
    assert (bits(ibs[5]) == minus0).all() and (bits(ibs[:, 5]) == minus0).all()
    assert (ints(sc)[3][131] == 0).all() and (bits(kin[131]) == minus0).all() and (bits(kin[:, 131]) == minus0).all()
    assert (ibs[131, np.arange(140) != 5] > 0).all()
    # a repeated individual of a selected panel: kinship exactly 0.5, whatever is missing
    panel = PackedPanel.from_codes(panel_codes(4, 300, seed=2, holes="3%"), gpu)
    twice = panel.select(haplotypes=np.array([0, 1, 2, 3, 4, 5, 6, 7, 2, 3]))
    kin = sample_counts(twice).kinship().cpu().numpy()
    assert kin[1, 4] == np.float32(0.5) and kin[4, 1] == np.float32(0.5) and kin[4, 4] == np.float32(0.5)
    assert np.array_equal(bits(kin[4, :4]), bits(kin[1, :4]))


def test_invariances(gpu):
    from ld_tools_amd import PackedPanel, sample_counts

    n_ind, n_snps = 70, 700
    codes = panel_codes(n_ind, n_snps, seed=33, holes="3%")
    panel = PackedPanel.from_codes(codes, gpu)
    base = sample_counts(panel)
    rng = np.random.default_rng(4)
    assert same(sample_counts(panel), base)                                              # repeated calls
    assert same(sample_counts(PackedPanel.from_codes(codes[rng.permutation(n_snps)], gpu)), base)   # permuted SNPs
    swap = np.arange(2 * n_ind).reshape(n_ind, 2)
    flip = rng.random(n_ind) < 0.5
    swap[flip] = swap[flip][:, ::-1]
    assert same(sample_counts(PackedPanel.from_codes(codes[:, swap.reshape(-1)], gpu)), base)       # rephased genotypes
    p = rng.permutation(n_ind)                                                           # permuted individuals
    cols = np.stack([2 * p, 2 * p + 1], axis=1).reshape(-1)
    moved = sample_counts(PackedPanel.from_codes(codes[:, cols], gpu))
    pt = torch.from_numpy(p).to(gpu)
    assert torch.equal(moved.counts, base.counts[:, pt][:, :, pt])
    assert torch.equal(moved.kinship().view(torch.int32), base.kinship()[pt][:, pt].view(torch.int32))
    mask = rng.random(n_snps) < 0.6                                                      # keep mask == the selected panel
    kept = sample_counts(panel, keep=mask)
    assert same(kept, sample_counts(panel.select(snps=mask)))
    assert kept.n_snps == n_snps and not torch.equal(kept.counts, base.counts)
    first = np.arange(n_snps) < 257                                                      # two calls over a split == one call
    part = sample_counts(panel.select(snps=first))
    both = sample_counts(panel.select(snps=~first), out=part)
    assert both is part and both.n_snps == n_snps and same(both, base)
    both = sample_counts(panel, keep=~first, out=sample_counts(panel, keep=first))
    assert torch.equal(both.counts, base.counts) and both.n_snps == 2 * n_snps


def test_cells_on_tuples(gpu):
    from ld_tools_amd import ibs_cell_host, king_cell_host, king_from_counts, sample_counts_host

    N, HH, IBS0, HET = sample_counts_host(panel_codes(40, 300, seed=8, holes="3%"))
    big = 2 ** 32 - 1
    cols = [np.concatenate([x.reshape(-1), extra]) for x, extra in
            ((N, [0, 5, big, big, big]), (HH, [0, 0, big, 1, 0]), (IBS0, [0, 2, 0, big - 1, 0]),
             (HET, [0, 0, big, 1, big - 1]), (HET.T, [0, 3, big, 1, 1]))]   # N = 0; m = 0; the largest legal counts
    kin, ibs = king_from_counts(*cols, device=gpu)
    assert np.array_equal(bits(kin.cpu().numpy()), bits(king_cell_host(*cols)))
    assert np.array_equal(bits(ibs.cpu().numpy()), bits(ibs_cell_host(*cols)))
    assert bits(kin.cpu().numpy()[-5:-3]).tolist() == [bits(np.float32(-0.0)).item()] * 2


def test_argument_rules(gpu):
    """The documented codes, returned before any HIP call: the pointers are never followed."""
    from ld_tools_amd import _lib

    lib, ptr = _lib.lib, 0x1000
    E_ARG, E_UNSUPPORTED = -1, -3
    planes = lambda **kw: lib.ldx_sample_planes_dev(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("alt", ptr), ("ref", ptr), ("n_snps", 100), ("n_hap", 8), ("keep", None), ("begin", 0), ("count", 100), ("store", ptr),
        ("tables", ptr), ("stream", None))])
    counts = lambda **kw: lib.ldx_sample_counts_dev(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("store", ptr), ("tables", ptr), ("n_ind", 4), ("n_snps", 100), ("counts", ptr), ("ld", 4), ("accumulate", 0), ("n_prior", 0),
        ("n_slices", 0), ("stream", None))])
    for bad in (dict(alt=None), dict(ref=None), dict(store=None), dict(tables=None), dict(n_hap=7), dict(n_hap=0), dict(count=0),
                dict(begin=1), dict(begin=100), dict(count=101)):
        assert planes(**bad) == E_ARG, bad
        assert b"ldx_sample_planes_dev" in lib.ldx_last_error()
    assert planes(n_hap=_lib.MAX_HAPS + 2) == E_UNSUPPORTED
    big = _lib.KING_MAX_SLICE_SNPS
    for bad in (dict(store=None), dict(tables=None), dict(counts=None), dict(n_ind=0), dict(n_snps=0), dict(ld=3),
                dict(n_prior=5), dict(accumulate=1, n_prior=2 ** 32 - 100), dict(n_snps=big + 1, n_slices=1),
                dict(n_snps=2 * big + 1, n_slices=2), dict(n_snps=_lib.KING_MAX_STORE_SNPS + 1)):
        assert counts(**bad) == E_ARG, bad
        assert b"ldx_sample_counts_dev" in lib.ldx_last_error()
    assert counts(n_ind=_lib.MAX_HAPS // 2 + 1, ld=_lib.MAX_HAPS) == E_UNSUPPORTED
    f32 = lambda n: (C.c_float * n)()  # noqa: E731
    assert lib.ldx_king_from_counts_dev(1, ptr, ptr, ptr, ptr, ptr, None, None, None) == E_ARG
    assert lib.ldx_king_from_counts_dev(1, None, ptr, ptr, ptr, ptr, C.addressof(f32(1)), None, None) == E_ARG
    assert lib.ldx_sample_cells_dev(ptr, 4, 3, ptr, ptr, 4, None) == E_ARG
    assert lib.ldx_sample_cells_dev(ptr, 4, 4, None, None, 4, None) == E_ARG
    assert lib.ldx_sample_cells_dev(None, 4, 4, ptr, ptr, 4, None) == E_ARG
    assert lib.ldx_sample_planes_bytes(129, 257) == 3 * 2 * 4 * 128 * 16 and lib.ldx_sample_tables_bytes(129) == (3 * 256 + 4) * 4

"""GPU: pairwise-complete LD on the band (ops.ld_band / ld_score / ld_neighbors / ld_prune with missing="pairwise";
include/ldx.h, "pairwise-complete bands") against the pairwise-complete rectangle bit for bit, the exact integer oracle
(tests/ld_pairwise_exact.py), the plain band operators where no call is missing, and the host mirrors of
tests/ld_pwband_cases.py.

Contract: the cell of SNPs i > j inside the window is ld_rect(panel, panel, missing="pairwise")[i, j] bit for bit -- within 4
float32 ulps of the exact r of the pair's integers, -0.0f exactly on a degenerate pair, +0.0f exactly where num = 0 --; sums
and lists are integer / bit-exact functions of those cells.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_band_cases as bc  # noqa: E402
import ld_exact as lx  # noqa: E402
import ld_pairwise_exact as px  # noqa: E402
import ld_pwband_cases as pb  # noqa: E402

pytestmark = pytest.mark.gpu

NEG0, POS0, ONE = np.uint32(0x80000000), np.uint32(0), np.float32(1.0).view(np.uint32)
ULPS = 4.0   # include/ldx.h: the bound of every r32 cell
FORMS = [False, True]
PW = pb.PW


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


def bits(t) -> np.ndarray:
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


_PACKED, _ORACLE = {}, {}


def packed(key, codes):
    from ld_tools_amd import PackedPanel
    if key not in _PACKED:
        _PACKED[key] = PackedPanel.from_codes(np.array(codes))   # (a copy: the codes are read-only)
    return _PACKED[key]


def oracle(key, codes, dosage):
    if (key, dosage) not in _ORACLE:
        _ORACLE[(key, dosage)] = px.PairwiseExactBlock(codes, codes, dosage)
    return _ORACLE[(key, dosage)]


def forms(n_hap):
    return FORMS if n_hap % 2 == 0 else [False]


def band_index(band):
    """(rows, cols) of the band's cells in layout order, as device int64 tensors."""
    import torch
    n = band.n_snps
    lo = band.lo.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    off = band.offsets
    length = torch.arange(n, device=lo.device) - lo
    assert int(off[n].item()) == band.n_cells == int(length.sum().item())
    rows = torch.repeat_interleave(torch.arange(n, device=lo.device), length)
    cols = torch.arange(band.n_cells, device=lo.device) - torch.repeat_interleave(off[:-1] - lo, length)
    return rows, cols


def assert_band_is_rect(band, panel, dosage, what):
    """values == ld_rect(panel, panel, missing="pairwise")[rows, cols], compared on the device; returns (rows, cols) on the host."""
    import torch
    from ld_tools_amd import ops
    rows, cols = band_index(band)
    sq = ops.ld_rect(panel, panel, dosage=dosage, missing=PW)
    want = sq.reshape(-1)[rows * panel.n_snps + cols]
    same = torch.equal(band.values.view(torch.int32), want.view(torch.int32))
    if not same:
        bad = torch.nonzero(band.values.view(torch.int32) != want.view(torch.int32))[0].item()
        raise AssertionError(f"{what}: cell {bad} = ({rows[bad].item()}, {cols[bad].item()}) is {band.values[bad].item()!r}, "
                             f"the rectangle has {want[bad].item()!r}")
    return rows.cpu().numpy(), cols.cpu().numpy()


def check_cells(got32, ex, rows, cols, what):
    b = np.ascontiguousarray(got32).view(np.uint32)
    deg, zero = ex.degenerate[rows, cols], ex.zero_num[rows, cols]
    assert np.array_equal(b == NEG0, deg), f"{what}: -0.0f <=> degenerate"
    assert np.array_equal(b == POS0, zero), f"{what}: +0.0f <=> num == 0"
    rest = ~deg & ~zero
    if rest.any():
        err = lx.ulp32_err(got32[rest], ex.r64[rows, cols][rest])
        print(f"{what}: {int(rest.sum())} cells, max error {float(err.max()):.3f} float32 ulps")
        assert float(err.max()) <= ULPS, f"{what}: {float(err.max())} ulps"


def check_diag(band, ex, what):
    live = np.diagonal(ex.v_x) > 0
    d = bits(band.diag)
    assert np.array_equal(d == ONE, live) and np.array_equal(d == NEG0, ~live), what
    return live


# ---- 1. band = rectangle = oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hap", pb.MAIN_HAPS)
def test_band_is_the_rectangle_and_the_oracle(gpu, n_hap):
    from ld_tools_amd import ops
    n = pb.N_MAIN
    codes, _ = pb.mixed_panel(n, n_hap)
    key = ("mixed", n, n_hap)
    p = packed(key, codes)
    pos = pb.ragged_positions(n)
    for dosage in forms(n_hap):
        what = f"mixed {n} x {n_hap}, dosage={dosage}"
        band = ops.ld_band(p, pos, window_bp=pb.MAIN_WINDOW, dosage=dosage, missing=PW)
        assert band.missing == PW and band.dosage == dosage and band.n_snps == n
        lo, off = ops.band_layout_host(pos, pb.MAIN_WINDOW)
        assert np.array_equal(band.layout()[0], lo.astype(np.int64)) and np.array_equal(band.layout()[1], off.astype(np.int64))
        rows, cols = assert_band_is_rect(band, p, dosage, what)
        ex = oracle(key, codes, dosage)
        check_cells(band.values.cpu().numpy(), ex, rows, cols, what)
        live = check_diag(band, ex, what)
        assert (~live).sum() >= 3 and live.sum() > n // 2
        assert bits(band.values)[(rows == px.ROW_DISJOINT + pb.SHIFT) & (cols == px.ROW_DISJOINT)].tolist() == [int(NEG0)]
        assert bits(band.values)[(rows == px.ROW_MONO + pb.SHIFT) & (cols == px.ROW_MONO)].tolist() == [int(NEG0)]
        plain = ops.ld_band(p, pos, window_bp=pb.MAIN_WINDOW, dosage=dosage)
        assert plain.missing is None and not np.array_equal(bits(plain.values), bits(band.values))


# ---- 2. no holes: the plain operators, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_hap", [254, 1008])
def test_without_holes_the_operators_are_the_plain_ones(gpu, n_hap):
    import torch
    from ld_tools_amd import ops
    n = pb.N_MAIN
    codes = pb.complete_panel(n, n_hap)
    p = packed(("complete", n, n_hap), codes)
    pos = pb.ragged_positions(n)
    ann = pb.annot_matrix(n)
    for dosage in FORMS:
        a, b = ops.ld_band(p, pos, window_bp=pb.MAIN_WINDOW, dosage=dosage, missing=PW), \
            ops.ld_band(p, pos, window_bp=pb.MAIN_WINDOW, dosage=dosage)
        assert np.array_equal(bits(a.values), bits(b.values)) and np.array_equal(bits(a.diag), bits(b.diag)), f"dosage={dosage}"
        assert (bits(a.diag) == NEG0).any() and (bits(a.values) == NEG0).any()
        for annot in (None, ann):
            sa = ops.ld_score(p, pos, window_bp=pb.MAIN_WINDOW, annot=annot, dosage=dosage, missing=PW)
            sb = ops.ld_score(p, pos, window_bp=pb.MAIN_WINDOW, annot=annot, dosage=dosage)
            assert torch.equal(sa.sums.view(torch.int64), sb.sums.view(torch.int64)), f"sums, dosage={dosage}"
            assert np.array_equal(sa.live, sb.live) and np.array_equal(sa.m, sb.m)
        na = ops.ld_neighbors(p, pos, window_bp=pb.MAIN_WINDOW, r2=pb.NBR_R2, dosage=dosage, missing=PW)
        nb = ops.ld_neighbors(p, pos, window_bp=pb.MAIN_WINDOW, r2=pb.NBR_R2, dosage=dosage)
        assert len(na) == len(nb) > 256 and torch.equal(na.hits, nb.hits) and torch.equal(na.offsets, nb.offsets)


# ---- 3. four tile kinds in one launch -------------------------------------------------------------------------------------------
def test_four_tile_kinds_in_one_launch(gpu):
    from ld_tools_amd import ops
    codes = pb.tiles_panel()
    n = codes.shape[0]
    key = ("tiles",)
    p = packed(key, codes)
    lo, _ = ops.band_layout_host(np.arange(n), pb.TILES_WINDOW_SNPS)
    assert pb.tile_kinds(codes, lo) == {(False, False), (True, False), (False, True), (True, True)}
    both = px.complete_rows(codes)
    for dosage in FORMS:
        what = f"tiles, dosage={dosage}"
        band = ops.ld_band(p, window_snps=pb.TILES_WINDOW_SNPS, dosage=dosage, missing=PW)
        rows, cols = assert_band_is_rect(band, p, dosage, what)
        check_cells(band.values.cpu().numpy(), oracle(key, codes, dosage), rows, cols, what)
        plain = ops.ld_band(p, window_snps=pb.TILES_WINDOW_SNPS, dosage=dosage)
        cc = both[rows] & both[cols]
        assert cc[(rows >= 256) & (rows < 384)].any()   # complete x complete pairs inside hole-bearing tiles
        assert np.array_equal(bits(band.values)[cc], bits(plain.values)[cc]), f"{what}: complete x complete cells are ld_band's"
        assert not np.array_equal(bits(band.values)[~cc], bits(plain.values)[~cc])


# ---- 4. the walk ----------------------------------------------------------------------------------------------------------------
def walk_case(gpu, key, codes, positions, window_bp, window_snps, what, with_oracle=False):
    import torch
    from ld_tools_amd import ops
    p = packed(key, codes)
    n_cells = None
    for dosage in forms(codes.shape[1]):
        band = ops.ld_band(p, positions, window_bp=window_bp, window_snps=window_snps, dosage=dosage, missing=PW)
        fill = 0x7FC12345   # a quiet NaN with a payload no kernel produces: every cell is written
        assert not bool((band.values.view(torch.int32) == fill).any().item())
        rows, cols = assert_band_is_rect(band, p, dosage, f"{what}, dosage={dosage}")
        if with_oracle:
            ex = oracle(key, codes, dosage)
            check_cells(band.values.cpu().numpy(), ex, rows, cols, f"{what}, dosage={dosage}")
            check_diag(band, ex, what)
        n_cells = band.n_cells
    return n_cells


def test_walk_clustered_positions_where_lo_jumps_inside_a_block(gpu):
    n, n_hap = 2700, 62
    codes, _ = pb.mixed_panel(n, n_hap)
    cells = walk_case(gpu, ("mixed", n, n_hap), codes, bc.clustered(n), 0, None, "clustered, window 0")
    assert cells == (2500 * 2499 + 15 * 14 + 184 * 183) // 2


def test_walk_the_everything_window_is_the_lower_triangle(gpu):
    n, n_hap = pb.N_MAIN, 1008
    codes, _ = pb.mixed_panel(n, n_hap)
    pos = pb.ragged_positions(n)
    cells = walk_case(gpu, ("mixed", n, n_hap), codes, pos, 1 << 60, None, "everything", with_oracle=True)
    assert cells == n * (n - 1) // 2


def test_walk_window_zero_on_distinct_positions_has_no_cell(gpu):
    import torch
    from ld_tools_amd import ops
    n, n_hap = 300, 254
    codes, _ = pb.mixed_panel(n, n_hap)
    p = packed(("mixed", n, n_hap), codes)
    for dosage in FORMS:
        band = ops.ld_band(p, bc.grid(n), window_bp=0, dosage=dosage, missing=PW)
        assert band.n_cells == 0 and band.values.numel() == 0
        live = check_diag(band, oracle(("mixed", n, n_hap), codes, dosage), "window 0")
        sc = ops.ld_score(p, bc.grid(n), window_bp=0, dosage=dosage, missing=PW)
        assert np.array_equal(sc.sums.cpu().numpy().view(np.uint64)[:, 0], np.where(live, np.uint64(1) << np.uint64(32), np.uint64(0)))
        assert np.array_equal(sc.live, live)
        nb = ops.ld_neighbors(p, bc.grid(n), window_bp=0, r2=pb.NBR_R2, dosage=dosage, missing=PW)
        assert len(nb) == 0 and not bool(torch.any(nb.offsets != 0).item())


@pytest.mark.parametrize("n", pb.WALK_SIZES)
def test_walk_sizes_on_the_tile_edges(gpu, n):
    n_hap = 62   # a single K-block
    codes, _ = pb.mixed_panel(n, n_hap)
    window_snps = 700 if n > 1000 else n   # 4226: six or seven slabs per I block; else everything
    cells = walk_case(gpu, ("mixed", n, n_hap), codes, None, None, window_snps, f"n = {n}", with_oracle=n <= 257)
    assert cells == sum(min(i, window_snps) for i in range(n))


def test_walk_the_largest_counts(gpu):
    n, n_hap = pb.BIG_CASE
    codes, _ = pb.mixed_panel(n, n_hap)
    key = ("mixed", n, n_hap)
    walk_case(gpu, key, codes, None, None, n, "10 240 haplotypes", with_oracle=True)
    assert int(oracle(key, codes, False).c.max()) == n_hap and int(oracle(key, codes, True).S.max()) == 2 * n_hap


def test_walk_more_tiles_than_the_grid(gpu):
    n, n_hap = pb.GRID_CASE
    codes, _ = pb.mixed_panel(n, n_hap)
    assert pb.tiles_walked(np.zeros(n, dtype=np.int64), n) > 1024
    cells = walk_case(gpu, ("mixed", n, n_hap), codes, None, None, n, "everything at 8269")
    assert cells == n * (n - 1) // 2


# ---- 5. scores --------------------------------------------------------------------------------------------------------------------
def main_band(dosage, n_hap=1008):
    from ld_tools_amd import ops
    n = pb.N_MAIN
    codes, _ = pb.mixed_panel(n, n_hap)
    p = packed(("mixed", n, n_hap), codes)
    pos = pb.ragged_positions(n)
    band = ops.ld_band(p, pos, window_bp=pb.MAIN_WINDOW, dosage=dosage, missing=PW)
    rows, cols = (t.cpu().numpy() for t in band_index(band))
    return codes, p, pos, band, rows, cols


@pytest.mark.parametrize("dosage", FORMS)
def test_scores_are_the_host_sums_of_the_band_cells(gpu, dosage):
    import torch
    from ld_tools_amd import _lib, ops
    from ld_tools_amd.panel import _stream_ptr
    codes, p, pos, band, rows, cols = main_band(dosage)
    n = p.n_snps
    values = band.values.cpu().numpy()
    live = bits(band.diag) == ONE
    ann = pb.annot_matrix(n)
    bits_a, k = ops.pack_annot(ann, n)
    for annot, ab, kk in ((None, None, 0), (ann, bits_a, k)):
        want = pb.expected_sums(n, rows, cols, values, live, ab, kk)
        sc = ops.ld_score(p, pos, window_bp=pb.MAIN_WINDOW, annot=annot, dosage=dosage, missing=PW)
        got = sc.sums.cpu().numpy().view(np.uint64)
        assert sc.missing == PW and got.shape == (n, 1 + kk)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"sums differ at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]} (annot={annot is not None})"
        assert np.array_equal(sc.live, live)
        assert np.array_equal(sc.m, ops.window_counts(pos, pb.MAIN_WINDOW, live, ab, kk))
    # a relaunch into a dirty buffer gives the same bytes: the entry itself, into a buffer of 0xAB bytes
    dirty = torch.full((n, 1 + k), -0x5454545454545455, dtype=torch.int64, device=gpu)
    ws = torch.empty(_lib.lib.ldx_ld_pw_band_workspace_bytes(n), dtype=torch.uint8, device=gpu)
    pos_d, ann_d = torch.as_tensor(pos).to(gpu), torch.as_tensor(bits_a).to(gpu)
    for _ in range(2):
        _lib.check(_lib.lib.ldx_ld_pw_score_dev(*ops._pw_panel(p, dosage), n, p.n_hap, int(dosage), pos_d.data_ptr(), pb.MAIN_WINDOW,
                                                ann_d.data_ptr(), k, band.diag.data_ptr(), dirty.data_ptr(), ws.data_ptr(),
                                                ws.numel(), _stream_ptr()), "ldx_ld_pw_score_dev")
        assert np.array_equal(dirty.cpu().numpy().view(np.uint64), want)


# ---- 6. neighbours ------------------------------------------------------------------------------------------------------------------
def assert_neighbors(nb, want, what):
    off, i, j, r, s = want
    h = nb.hits.cpu().numpy()
    assert h.shape == (i.size, 4), f"{what}: {h.shape[0]} records, {i.size} expected"
    assert np.array_equal(h[:, 0].astype(np.int64), i) and np.array_equal(h[:, 1].astype(np.int64), j), what
    assert np.array_equal(np.ascontiguousarray(h[:, 2]).view(np.uint32), r.view(np.uint32)), f"{what}: r bits"
    assert np.array_equal(np.ascontiguousarray(h[:, 3]).view(np.uint32), s.view(np.uint32)), f"{what}: s bits"
    assert np.array_equal(nb.offsets.cpu().numpy().astype(np.int64), off), what


@pytest.mark.parametrize("dosage", FORMS)
def test_neighbours_are_the_host_filter_of_the_band_and_agree_with_the_oracle(gpu, dosage):
    from ld_tools_amd import ops
    codes, p, pos, band, rows, cols = main_band(dosage)
    n = p.n_snps
    bound = ops.r2_bound(pb.NBR_R2)
    want = pb.expected_neighbors(n, rows, cols, band.values.cpu().numpy(), bound)
    nb = ops.ld_neighbors(p, pos, window_bp=pb.MAIN_WINDOW, r2=pb.NBR_R2, dosage=dosage, missing=PW)
    assert nb.missing == PW and nb.dosage == dosage and np.float32(nb.bound) == bound
    assert_neighbors(nb, want, f"neighbours, dosage={dosage}")
    kept = np.zeros((n, n), dtype=bool)
    kept[want[1], want[2]] = True
    cls = oracle(("mixed", n, 1008), codes, dosage).classes(pb.NBR_R2)
    inside = np.zeros((n, n), dtype=bool)
    inside[rows, cols] = inside[cols, rows] = True
    assert kept[inside & (cls == px.IN)].all() and not kept[inside & (cls == px.OUT)].any() and not kept[~inside].any()
    assert int((inside & (cls == px.IN)).sum()) >= 2 * pb.MIN_DECIDED_IN
    assert want[1].size > 256   # a buffer of one batch: the first run reserves more than it holds, the re-run gives the same CSR
    small = ops.ld_neighbors(p, pos, window_bp=pb.MAIN_WINDOW, r2=pb.NBR_R2, dosage=dosage, missing=PW, hit_capacity=256)
    assert_neighbors(small, want, f"neighbours from a 256-slot buffer, dosage={dosage}")
    # pruning on top: the strict lists, and the sequential rule on them
    pr = ops.ld_prune(p, pos, r2=pb.NBR_R2, window_bp=pb.MAIN_WINDOW, dosage=dosage, missing=PW)
    strict = pb.expected_neighbors(n, rows, cols, band.values.cpu().numpy(), ops.r2_bound(pb.NBR_R2, strict=True))
    assert pr.neighbors.missing == PW
    assert_neighbors(pr.neighbors, strict, f"prune lists, dosage={dosage}")
    live = bits(band.diag) == ONE
    state, _ = ops.select_host(strict[0], strict[2], pr.rank, live.astype(np.uint8))
    assert np.array_equal(pr.keep, state == ops.SEL_INDEX) and pr.keep.sum() > 0 and not pr.keep[~live].any()
    assert not kept_pairs_above(pr.keep, strict)


def kept_pairs_above(keep, lists) -> bool:
    """Is there a neighbour pair whose two SNPs are both kept?"""
    _, i, j, _, _ = lists
    return bool((keep[i] & keep[j]).any())


# ---- 7. invariances ---------------------------------------------------------------------------------------------------------------
def all_bytes(p, pos, dosage):
    from ld_tools_amd import ops
    band = ops.ld_band(p, pos, window_bp=pb.MAIN_WINDOW, dosage=dosage, missing=PW)
    sc = ops.ld_score(p, pos, window_bp=pb.MAIN_WINDOW, annot=pb.annot_matrix(p.n_snps), dosage=dosage, missing=PW)
    nb = ops.ld_neighbors(p, pos, window_bp=pb.MAIN_WINDOW, r2=pb.NBR_R2, dosage=dosage, missing=PW)
    return [bits(band.values), bits(band.diag), sc.sums.cpu().numpy().view(np.uint64), nb.hits.cpu().numpy(),
            nb.offsets.cpu().numpy()]


@pytest.mark.parametrize("dosage", FORMS)
def test_permuted_individuals_give_identical_bytes(gpu, dosage):
    n, n_hap = pb.N_MAIN, 254
    codes, _ = pb.mixed_panel(n, n_hap)
    pos = pb.ragged_positions(n)
    base = all_bytes(packed(("mixed", n, n_hap), codes), pos, dosage)
    other = all_bytes(packed(("permuted", n, n_hap), px.permute_individuals(codes, 5)), pos, dosage)
    for a, b in zip(base, other):
        assert np.array_equal(a, b)


def test_dosage_rephased_genotypes_give_identical_bytes(gpu):
    n, n_hap = pb.N_MAIN, 254
    codes, _ = pb.mixed_panel(n, n_hap)
    pos = pb.ragged_positions(n)
    re = px.rephase(codes, 8)
    assert not np.array_equal(re, codes)
    base = all_bytes(packed(("mixed", n, n_hap), codes), pos, True)
    other = all_bytes(packed(("rephased", n, n_hap), re), pos, True)
    for a, b in zip(base, other):
        assert np.array_equal(a, b)
    hap = all_bytes(packed(("rephased", n, n_hap), re), pos, False)
    assert not np.array_equal(hap[0], all_bytes(packed(("mixed", n, n_hap), codes), pos, False)[0])   # the haplotype form sees the phase


# ---- 8. composition: the stored band's consumers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dosage", FORMS)
def test_matvec_and_cross_score_on_a_pairwise_band(gpu, dosage):
    from ld_tools_amd import ops
    codes, p, pos, band, rows, cols = main_band(dosage)
    n = p.n_snps
    values, diag = band.values.cpu().numpy(), band.diag.cpu().numpy()
    x = np.random.default_rng(3).normal(size=(n, 3)).astype(np.float32)
    for power in (1, 2):
        prod = band.matvec(x, power=power)
        x32 = prod.x32.cpu().numpy()
        pv = ops.prod_values(values, power)
        got = prod.sums.cpu().numpy()
        for c in range(3):
            xc = np.ascontiguousarray(x32[:, c])
            own = ops.prod_terms(ops.prod_values(diag, power), xc)
            with np.errstate(over="ignore"):
                want = np.array(own, dtype=np.int64)
                np.add.at(want, rows, ops.prod_terms(pv, xc[cols]))
                np.add.at(want, cols, ops.prod_terms(pv, xc[rows]))
            assert np.array_equal(got[:, c], want), f"power {power}, column {c}"
    # ld_cross_score(b, b) is the pairwise score's column 0; to_dense carries the cells and the diagonal
    sc = ops.ld_score(p, pos, window_bp=pb.MAIN_WINDOW, dosage=dosage, missing=PW)
    assert np.array_equal(ops.ld_cross_score(band, band).sums.view(np.uint64), sc.sums.cpu().numpy().view(np.uint64)[:, 0])
    want_terms = bc.pair_sums(n, rows, cols, ops.cross_terms(values, values), ops.cross_terms(diag, diag))
    assert np.array_equal(ops.ld_cross_score(band, band).sums, want_terms)
    dense = band.to_dense((0, 300))
    sel = (rows < 300)
    assert np.array_equal(dense[rows[sel], cols[sel]].view(np.uint32), values[sel].view(np.uint32))
    assert np.array_equal(np.diagonal(dense).view(np.uint32), diag[:300].view(np.uint32))


# ---- 9. drivers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dosage", FORMS)
def test_drivers_pass_missing_through(gpu, dosage):
    import torch
    from test_gpu_ld_pairwise import rs_rows, vcf_with_missing_calls
    from ld_tools_amd import LdxError, ops
    from ld_tools_amd.drivers.band import band_matrix
    from ld_tools_amd.drivers.ldscore import _fetch_panel, ld_scores
    vcf, names = vcf_with_missing_calls()
    rows = rs_rows(vcf, "6")
    _, keep, _, _, panel = _fetch_panel("test", vcf, "6", rows, names, None, None)
    assert int(((panel.acnt[:panel.n_snps] + panel.rcnt[:panel.n_snps]) != panel.n_hap).sum()) > 0   # calls are missing
    tab = ld_scores(vcf, "6", rows, names, window_bp=2_000, dosage=dosage, missing=PW)
    m = band_matrix(vcf, "6", rows, names, window_bp=2_000, dosage=dosage, missing=PW)
    assert tab.scores.missing == PW and m.band.missing == PW and m.band.dosage == dosage and m.band.n_cells > 0
    pos = np.asarray(m.poss, dtype=np.int64)
    band = ops.ld_band(panel, pos, window_bp=2_000, dosage=dosage, missing=PW)
    assert np.array_equal(bits(m.band.values), bits(band.values)) and np.array_equal(bits(m.band.diag), bits(band.diag))
    sc = ops.ld_score(panel, pos, window_bp=2_000, dosage=dosage, missing=PW)
    assert torch.equal(tab.scores.sums.view(torch.int64), sc.sums.view(torch.int64))
    assert tab.scores.adjusted().shape == (len(keep), 1)   # n_obs as without missing=: n_hap, or n_hap / 2 with dosage
    if dosage:   # the plain dosage driver refuses the panel
        with pytest.raises(LdxError, match="missing='ref'"):
            band_matrix(vcf, "6", rows, names, window_bp=2_000, dosage=True)
    else:
        plain = band_matrix(vcf, "6", rows, names, window_bp=2_000)
        assert plain.band.missing is None and not np.array_equal(bits(plain.band.values), bits(m.band.values))


# ---- 10. past the first trip of the plan ---------------------------------------------------------------------------------------
# pb.PLAN_CASE: 258 I blocks, two of them in plan_kernel's second trip (ldx_band_plan.h): the carry between trips, prefix[Ti]
# after the loop, tile_at's search over 259 entries, rows up to 65 868.  The reference of every cell is the rectangle of a
# SELECTED panel, whose rows start at 0; three row blocks go to the exact oracle, one of them across the trip boundary.
PLAN_PANELS = ("plan", "mixed")
PLAN_FILL = 0x7FC12345   # walk_case's quiet NaN: a payload no kernel produces
_PLAN_BAND = {}


def plan_case(kind):
    n, n_hap = pb.PLAN_CASE
    codes = pb.plan_panel() if kind == "plan" else pb.mixed_panel(n, n_hap)[0]
    return ("plan", kind), codes, pb.ragged_positions(n)


def plan_layout():
    """(lo, offsets, rows, cols) of the plan case on the host, from band_layout_host; once per process."""
    from ld_tools_amd import ops
    if "layout" not in _PLAN_BAND:
        lo, off = ops.band_layout_host(pb.ragged_positions(pb.PLAN_CASE[0]), pb.PLAN_WINDOW)
        _PLAN_BAND["layout"] = (lo.astype(np.int64), off.astype(np.int64)) + bc.cell_rows_cols(lo, off)
    return _PLAN_BAND["layout"]


def plan_band(gpu, kind, dosage):
    """The stored band of the plan case, once per panel and form (the store test checks every cell of it)."""
    import torch
    from ld_tools_amd import ops
    if (kind, dosage) not in _PLAN_BAND:
        key, codes, pos = plan_case(kind)
        # a freed block of the values' size full of the fill pattern: the allocator hands it to the next request of that size,
        # so a cell the kernel leaves out is likely to show as the pattern and not as an earlier run's bytes
        filled = torch.full((pb.PLAN_CELLS,), PLAN_FILL, dtype=torch.int32, device=gpu)
        del filled
        _PLAN_BAND[(kind, dosage)] = ops.ld_band(packed(key, codes), pos, window_bp=pb.PLAN_WINDOW, dosage=dosage, missing=PW)
    return _PLAN_BAND[(kind, dosage)]


@pytest.mark.parametrize("dosage", FORMS)
@pytest.mark.parametrize("kind", PLAN_PANELS)
def test_past_the_first_trip_the_stored_band_is_the_rectangle_and_the_oracle(gpu, kind, dosage):
    import torch
    from ld_tools_amd import ops
    key, codes, pos = plan_case(kind)
    n = codes.shape[0]
    p = packed(key, codes)
    lo, off, rows, cols = plan_layout()
    what = f"plan case, {kind} panel, dosage={dosage}"
    band = plan_band(gpu, kind, dosage)
    assert band.n_snps == n and band.n_cells == pb.PLAN_CELLS
    assert np.array_equal(band.layout()[0], lo) and np.array_equal(band.layout()[1], off)
    got = band.values.view(torch.int32)
    assert not bool((got == PLAN_FILL).any().item()), f"{what}: a cell was not written"
    for (a, b), (c0, c1), cells, li, lj in bc.band_chunks(lo, off):
        sq = ops.ld_rect(p.select(snps=np.arange(a, b)), p.select(snps=np.arange(c0, c1)), dosage=dosage, missing=PW)
        want = sq.reshape(-1).view(torch.int32)[torch.from_numpy(li * (c1 - c0) + lj).to(gpu)]
        mine = got[int(cells[0]): int(cells[-1]) + 1]
        if not torch.equal(mine, want):
            k = int(torch.nonzero(mine != want)[0].item())
            raise AssertionError(f"{what}: cell {cells[k]} = ({a + li[k]}, {c0 + lj[k]}) is {band.values[int(cells[k])].item()!r}, "
                                 f"the rectangle of rows {a} .. {b - 1} has {sq[int(li[k]), int(lj[k])].item()!r}")
    # the exact oracle on three row blocks: the first rows, across the trip boundary (I blocks 255 | 256), the ragged last block
    values, diag = band.values.cpu().numpy(), bits(band.diag)
    edge = 256 * pb.PLAN_TRIP
    for a, b in ((0, 512), (edge - 256, edge + 256), (n - 333, n)):
        c0 = int(lo[a])
        ex = px.PairwiseExactBlock(codes[a:b], codes[c0:b], dosage)
        at = np.arange(off[a], off[b])
        check_cells(values[at], ex, rows[at] - a, cols[at] - c0, f"{what}, rows {a} .. {b - 1}")
        own = np.arange(b - a)
        live = ex.v_x[own, own + a - c0] > 0                                   # check_diag's rule on the block's own rows
        assert np.array_equal(diag[a:b] == ONE, live) and np.array_equal(diag[a:b] == NEG0, ~live), f"{what}: diag of rows {a} .."


@pytest.mark.parametrize("dosage", FORMS)
@pytest.mark.parametrize("kind", PLAN_PANELS)
def test_past_the_first_trip_scores_are_the_host_sums_of_the_band_cells(gpu, kind, dosage):
    from ld_tools_amd import ops
    key, codes, pos = plan_case(kind)
    n = codes.shape[0]
    lo, off, rows, cols = plan_layout()
    band = plan_band(gpu, kind, dosage)
    values, live = band.values.cpu().numpy(), bits(band.diag) == ONE
    bits_a, k = ops.pack_annot(pb.annot_matrix(n), n)
    sc = ops.ld_score(packed(key, codes), pos, window_bp=pb.PLAN_WINDOW, annot=pb.annot_matrix(n), dosage=dosage, missing=PW)
    got = sc.sums.cpu().numpy().view(np.uint64)
    want = pb.expected_sums(n, rows, cols, values, live, bits_a, k)
    assert got.shape == want.shape == (n, 1 + pb.N_ANNOT)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{kind}, dosage={dosage}: {bad.shape[0]} sums differ, the first at {bad[0].tolist()}: " \
                          f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    assert np.array_equal(sc.live, live)
    assert np.array_equal(sc.m, ops.window_counts(pos, pb.PLAN_WINDOW, live, bits_a, k))


@pytest.mark.parametrize("dosage", FORMS)
@pytest.mark.parametrize("kind", PLAN_PANELS)
def test_past_the_first_trip_neighbours_are_the_host_filter_of_the_band_cells(gpu, kind, dosage):
    from ld_tools_amd import ops
    key, codes, pos = plan_case(kind)
    n = codes.shape[0]
    lo, off, rows, cols = plan_layout()
    band = plan_band(gpu, kind, dosage)
    want = pb.expected_neighbors(n, rows, cols, band.values.cpu().numpy(), ops.r2_bound(pb.NBR_R2))
    nb = ops.ld_neighbors(packed(key, codes), pos, window_bp=pb.PLAN_WINDOW, r2=pb.NBR_R2, dosage=dosage, missing=PW)
    assert_neighbors(nb, want, f"plan case, {kind} panel, dosage={dosage}")
    assert int((want[1] >= 256 * pb.PLAN_TRIP).sum()) >= 1                     # a hit in a row of the second trip

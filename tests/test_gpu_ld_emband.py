"""GPU: EM LD on the band (ops.ld_em_band, ops.ld_neighbors / ld_clump / ld_prune with em=True; include/ldx.h, "EM on the
band") against the EM rectangle bit for bit, the 60-digit oracle on the cells' own integers, and the host mirrors of
tests/ld_emband_cases.py.

Contract: the r and D' cells of SNPs i > j inside the window are ld_em(panel, panel, missing=...)[i, j] bit for bit -- the same
five integers through the same em_cell --; the diagonal is +1 where 0 < A < 2 N over the SNP's own called individuals, else
-0.0; lists and selections are bit-exact functions of those cells.  No expected value comes from the band operators.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_band_cases as bc  # noqa: E402
import ld_emband_cases as eb  # noqa: E402
import ld_pairwise_exact as px  # noqa: E402
import ld_pwband_cases as pb  # noqa: E402
import ld_rect_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

NEG0, ONE = np.uint32(0x80000000), np.float32(1.0).view(np.uint32)
PW = eb.PW
MISSING = [None, PW]


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    from ld_tools_amd import _lib

    buf = C.create_string_buffer(64)
    _lib.check(_lib.lib.ldx_device_arch(0, buf, 64))
    assert buf.value.decode().startswith("gfx950"), buf.value
    return torch.device("cuda", 0)


def bits(t) -> np.ndarray:
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


_PACKED, _RECT = {}, {}


def packed(key, codes):
    from ld_tools_amd import PackedPanel
    if key not in _PACKED:
        _PACKED[key] = PackedPanel.from_codes(np.array(codes))   # (a copy: the codes are read-only)
    return _PACKED[key]


def rect(key, codes, missing):
    """The parent's only way to these cells: ld_em(panel, panel), both matrices on the host, once per panel and form."""
    from ld_tools_amd import ops
    if (key, missing) not in _RECT:
        out = ops.ld_em(packed(key, codes), missing=missing)
        _RECT[(key, missing)] = (out.r.cpu().numpy(), out.dprime.cpu().numpy())
    return _RECT[(key, missing)]


def main_case(missing, n_hap=1008):
    """Case 1's panel of each form: complete_panel for the plain form, mixed_panel for the pairwise form."""
    n = eb.N_MAIN
    kind = "mixed" if missing == PW else "complete"
    codes = eb.mixed_panel(n, n_hap) if missing == PW else eb.complete_panel(n, n_hap)
    return (kind, n, n_hap), codes, pb.ragged_positions(n)


def assert_band_is_rect(res, key, codes, missing, rows, cols, what):
    sq_r, sq_d = rect(key, codes, missing)
    for name, band, sq in (("r", res.r, sq_r), ("D'", res.dprime, sq_d)):
        if band is None:
            continue
        got, want = bits(band.values), bits(sq[rows, cols])
        assert got.shape == want.shape, f"{what}: {got.size} {name} cells, {want.size} expected"
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{what}: {bad.size} {name} cells differ from the rectangle, the first ({rows[bad[0]]}, {cols[bad[0]]}): "
                               f"{band.values[int(bad[0])].item()!r} != {sq[rows[bad[0]], cols[bad[0]]]!r}")


def assert_diag(res, codes, missing, what):
    live = eb.own_live(codes, missing == PW)
    for band in (res.r, res.dprime):
        if band is not None:
            d = bits(band.diag)
            assert np.array_equal(d == ONE, live) and np.array_equal(d == NEG0, ~live), what
    assert np.array_equal(res.live.cpu().numpy().astype(bool), live), what
    return live


# ---- 1. store = rectangle = oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("n_hap", eb.MAIN_HAPS)
def test_store_equals_the_rectangle(gpu, n_hap, missing):
    from ld_tools_amd import ops
    key, codes, pos = main_case(missing, n_hap)
    n = codes.shape[0]
    what = f"{key}, missing={missing}"
    res = ops.ld_em_band(packed(key, codes), pos, window_bp=eb.MAIN_WINDOW, missing=missing)
    assert res.r.em and res.dprime.em and res.r.missing == missing and res.r.n_snps == n and not res.r.dosage
    assert res.r.lo is res.dprime.lo and res.r.offsets is res.dprime.offsets and res.r.diag is res.dprime.diag
    lo, off, rows, cols = eb.band_cells(pos, eb.MAIN_WINDOW)
    assert np.array_equal(res.r.layout()[0], lo.astype(np.int64)) and np.array_equal(res.r.layout()[1], off.astype(np.int64))
    walked = eb.tiles_walked(lo, n)
    assert 6 < walked < 21   # I blocks meet two to four slabs: more than the diagonal, fewer than the triangle
    assert_band_is_rect(res, key, codes, missing, rows, cols, what)
    live = assert_diag(res, codes, missing, what)
    assert live[eb.ROW_HET] and bits(res.r.diag)[eb.ROW_HET] == ONE          # all-heterozygous: no dosage variance, a live EM SNP
    assert (~live).sum() >= 2 and live.sum() > n // 2
    N, A = eb.own_counts(codes, missing == PW)
    assert A[eb.ROW_HET] == N[eb.ROW_HET] == n_hap // 2
    pick = eb.sample_cells(rows, cols, live, eb.SAMPLED_CELLS, seed=n_hap)
    assert pick.size == eb.SAMPLED_CELLS
    counts = eb.pair_counts(codes, rows[pick], cols[pick], missing == PW)
    r, d = res.r.values.cpu().numpy()[pick], res.dprime.values.cpu().numpy()[pick]
    bad = eb.cells_pass_the_oracle(counts, r, d)
    assert not bad, f"{what}: {len(bad)} of {pick.size} sampled cells miss the oracle, the first {bad[0]}"
    # ... and they are the list epilogue's cells on those integers
    lr, ld_, _ = ops.ld_em_from_counts(*counts)
    assert np.array_equal(bits(lr), bits(r)) and np.array_equal(bits(ld_), bits(d))
    if missing == PW:
        plain = ops.ld_em_band(packed(key, codes), pos, window_bp=eb.MAIN_WINDOW)
        assert not np.array_equal(bits(plain.r.values), bits(res.r.values))   # a missing code counted as REF shows


# ---- 2. four tile kinds in one launch ---------------------------------------------------------------------------------------------
def test_four_tile_kinds_in_one_launch(gpu):
    from ld_tools_amd import ops
    codes = eb.tiles_panel()
    n = codes.shape[0]
    key = ("tiles",)
    p = packed(key, codes)
    lo, off, rows, cols = eb.band_cells(np.arange(n), eb.TILES_WINDOW_SNPS)
    assert eb.tile_kinds(codes, lo) == {(False, False), (True, False), (False, True), (True, True)}
    res = ops.ld_em_band(p, window_snps=eb.TILES_WINDOW_SNPS, missing=PW)
    assert_band_is_rect(res, key, codes, PW, rows, cols, "tiles")
    plain = ops.ld_em_band(p, window_snps=eb.TILES_WINDOW_SNPS)
    both = px.complete_rows(codes)
    cc = both[rows] & both[cols]
    assert cc[(rows >= 256) & (rows < 384)].any()   # complete x complete pairs inside hole-bearing tiles
    for a, b in ((res.r, plain.r), (res.dprime, plain.dprime)):
        assert np.array_equal(bits(a.values)[cc], bits(b.values)[cc]), "complete x complete cells are the plain form's"
    assert not np.array_equal(bits(res.r.values)[~cc], bits(plain.r.values)[~cc])


# ---- 3. no holes: the plain bytes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hap", eb.MAIN_HAPS)
def test_without_holes_the_pairwise_form_is_the_plain_one(gpu, n_hap):
    from ld_tools_amd import ops
    n = eb.N_MAIN
    codes = eb.complete_panel(n, n_hap)
    p = packed(("complete", n, n_hap), codes)
    pos = pb.ragged_positions(n)
    a, b = ops.ld_em_band(p, pos, window_bp=eb.MAIN_WINDOW, missing=PW), ops.ld_em_band(p, pos, window_bp=eb.MAIN_WINDOW)
    for x, y in ((a.r, b.r), (a.dprime, b.dprime)):
        assert np.array_equal(bits(x.values), bits(y.values)) and np.array_equal(bits(x.diag), bits(y.diag))
    assert (bits(a.r.diag) == NEG0).any() and (bits(a.r.values) == NEG0).any() and a.n_cells > 100_000


# ---- 4. more tiles than the grid, past row 4096, and the smallest panels --------------------------------------------------------------
def test_more_tiles_than_the_grid_and_past_row_4096(gpu):
    import torch
    from ld_tools_amd import ops
    n, n_hap = eb.GRID_CASE
    codes = eb.grid_panel()
    key = ("grid",)
    p = packed(key, codes)
    lo, off, rows, cols = eb.band_cells(np.arange(n), n)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert eb.tiles_walked(lo, n) == eb.GRID_TILES > 2 * cus, (eb.tiles_walked(lo, n), cus)
    assert not px.complete_rows(codes)[list(eb.GRID_HOLE_ROWS)].any() and (~px.complete_rows(codes)).sum() == 2
    for missing in MISSING:
        res = ops.ld_em_band(p, window_snps=n, missing=missing)
        assert res.n_cells == n * (n - 1) // 2
        assert_band_is_rect(res, key, codes, missing, rows, cols, f"everything at {n}, missing={missing}")
        assert_diag(res, codes, missing, f"everything at {n}")


@pytest.mark.parametrize("n", eb.SMALL_SIZES)
def test_smallest_panels(gpu, n):
    from ld_tools_amd import ops
    n_hap = 62
    codes = eb.plant_het(pb.mixed_panel(n, n_hap)[0])
    key = ("small", n)
    p = packed(key, codes)
    lo, off, rows, cols = eb.band_cells(np.arange(n), n)
    for missing in MISSING:
        res = ops.ld_em_band(p, window_snps=n, missing=missing)
        assert res.n_cells == n * (n - 1) // 2 == rows.size
        if n == 1:
            assert res.r.values.numel() == 0 and res.dprime.values.numel() == 0   # n_cells = 0: no launch
        else:
            assert_band_is_rect(res, key, codes, missing, rows, cols, f"n = {n}, missing={missing}")
        assert_diag(res, codes, missing, f"n = {n}")
        nb = ops.ld_neighbors(p, window_snps=n, r2=eb.NBR_R2, em=True, missing=missing)
        sq_r, sq_d = rect(key, codes, missing)
        want = eb.expected_neighbors(n, rows, cols, sq_r[rows, cols], sq_d[rows, cols], ops.r2_bound(eb.NBR_R2))
        assert_neighbors(nb, want, f"n = {n}, missing={missing}")


# ---- 5. windows -------------------------------------------------------------------------------------------------------------------
def test_windows_zero_and_beyond_the_maximum(gpu):
    from ld_tools_amd import ops
    key, codes, pos = main_case(PW, 254)
    n = codes.shape[0]
    p = packed(key, codes)
    lo, off, rows, cols = eb.band_cells(pos, 0)
    assert 0 < rows.size < n and (pos[rows] == pos[cols]).all()   # window 0: the duplicate positions' pairs only
    res = ops.ld_em_band(p, pos, window_bp=0, missing=PW)
    assert res.n_cells == rows.size
    assert_band_is_rect(res, key, codes, PW, rows, cols, "window 0")
    none = ops.ld_em_band(p, bc.grid(n), window_bp=0, missing=PW)
    assert none.n_cells == 0 and none.r.values.numel() == 0
    assert_diag(none, codes, PW, "window 0 on distinct positions")
    huge = ops.ld_em_band(p, pos, window_bp=ops.BAND_WINDOW_MAX * 4, missing=PW)   # clamped as in ld_band
    assert huge.r.window == ops.BAND_WINDOW_MAX and huge.n_cells == n * (n - 1) // 2
    lo, off, rows, cols = eb.band_cells(pos, ops.BAND_WINDOW_MAX * 4)
    assert_band_is_rect(huge, key, codes, PW, rows, cols, "a window past BAND_WINDOW_MAX")


# ---- 6. want_r / want_dprime ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", MISSING)
def test_each_band_alone_is_the_same_bytes(gpu, missing):
    from ld_tools_amd import LdxError, ops
    key, codes, pos = main_case(missing, 254)
    p = packed(key, codes)
    both = ops.ld_em_band(p, pos, window_bp=eb.MAIN_WINDOW, missing=missing)
    only_r = ops.ld_em_band(p, pos, window_bp=eb.MAIN_WINDOW, missing=missing, want_dprime=False)
    only_d = ops.ld_em_band(p, pos, window_bp=eb.MAIN_WINDOW, missing=missing, want_r=False)
    assert only_r.dprime is None and only_d.r is None
    assert np.array_equal(bits(only_r.r.values), bits(both.r.values))
    assert np.array_equal(bits(only_d.dprime.values), bits(both.dprime.values))
    assert np.array_equal(bits(only_d.dprime.diag), bits(both.r.diag))
    with pytest.raises(LdxError, match="neither r nor D' was asked for"):
        ops.ld_em_band(p, pos, window_bp=eb.MAIN_WINDOW, missing=missing, want_r=False, want_dprime=False)


# ---- 7. neighbours ----------------------------------------------------------------------------------------------------------------
def assert_neighbors(nb, want, what):
    off, i, j, r, d = want
    h = nb.hits.cpu().numpy()
    assert h.shape == (i.size, 4), f"{what}: {h.shape[0]} records, {i.size} expected"
    assert np.array_equal(h[:, 0].astype(np.int64), i) and np.array_equal(h[:, 1].astype(np.int64), j), what
    assert np.array_equal(np.ascontiguousarray(h[:, 2]).view(np.uint32), r.view(np.uint32)), f"{what}: r bits"
    assert np.array_equal(np.ascontiguousarray(h[:, 3]).view(np.uint32), d.view(np.uint32)), f"{what}: D' bits"
    assert np.array_equal(nb.offsets.cpu().numpy().astype(np.int64), off), what
    assert nb.em and np.array_equal(bits(nb.dprime), d.view(np.uint32)) and np.array_equal(bits(nb.r), r.view(np.uint32))


def main_lists(missing, strict=False, r2=eb.NBR_R2):
    """The host mirror of case 1's neighbour lists, from the rectangle's cells."""
    from ld_tools_amd import ops
    key, codes, pos = main_case(missing)
    n = codes.shape[0]
    lo, off, rows, cols = eb.band_cells(pos, eb.MAIN_WINDOW)
    sq_r, sq_d = rect(key, codes, missing)
    bound = ops.r2_bound(r2, strict=strict)
    return key, codes, pos, eb.expected_neighbors(n, rows, cols, sq_r[rows, cols], sq_d[rows, cols], bound), bound


@pytest.mark.parametrize("missing", MISSING)
def test_neighbours_are_the_host_filter_of_the_rectangle(gpu, missing):
    from ld_tools_amd import LdxError, ops
    key, codes, pos, want, bound = main_lists(missing)
    p = packed(key, codes)
    assert want[1].size > 256   # the planted copies of ld_codes: more than one batch of record slots
    nb = ops.ld_neighbors(p, pos, window_bp=eb.MAIN_WINDOW, r2=eb.NBR_R2, em=True, missing=missing)
    assert nb.missing == missing and not nb.dosage and np.float32(nb.bound) == bound
    assert_neighbors(nb, want, f"neighbours, missing={missing}")
    assert not (want[3].view(np.uint32) == NEG0).any()   # -0.0 is never a hit
    # a buffer of one batch: the first run reserves more than it holds, the re-run gives the same CSR
    small = ops.ld_neighbors(p, pos, window_bp=eb.MAIN_WINDOW, r2=eb.NBR_R2, em=True, missing=missing, hit_capacity=256)
    assert_neighbors(small, want, f"neighbours from a 256-slot buffer, missing={missing}")
    # strict at a threshold that is a float32: the bound is the next float32 (0.2 is none: there strict changes nothing)
    _, _, _, strict, sbound = main_lists(missing, strict=True, r2=0.25)
    nbs = ops.ld_neighbors(p, pos, window_bp=eb.MAIN_WINDOW, r2=0.25, strict=True, em=True, missing=missing)
    assert np.float32(nbs.bound) == sbound > np.float32(0.25) == ops.r2_bound(0.25)
    assert_neighbors(nbs, strict, f"strict neighbours, missing={missing}")
    # a non-EM list has no D'
    plain = ops.ld_neighbors(p, pos, window_bp=eb.MAIN_WINDOW, r2=eb.NBR_R2, missing=missing)
    assert not plain.em
    with pytest.raises(LdxError, match="em=True"):
        plain.dprime


# ---- 8. clump and prune -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", MISSING)
def test_clump_and_prune_are_the_sequential_rule_on_the_em_lists(gpu, missing):
    from ld_tools_amd import ops
    key, codes, pos, want, _ = main_lists(missing)
    _, _, _, strict, _ = main_lists(missing, strict=True)
    p = packed(key, codes)
    n = codes.shape[0]
    live = eb.own_live(codes, missing == PW)
    dosage_live = p.dosage_live() if missing is None else None
    assert live[eb.ROW_HET] and (dosage_live is None or not dosage_live[eb.ROW_HET])
    rng = np.random.default_rng(12)
    pv = rng.uniform(0.0, 0.02, size=n)
    pv[eb.ROW_HET] = 1e-9          # the all-heterozygous SNP leads a clump
    pv[::97] = np.nan
    cl = ops.ld_clump(p, pos, pv, p1=1e-2, p2=2e-2, r2=eb.NBR_R2, window_bp=eb.MAIN_WINDOW, em=True, missing=missing)
    assert cl.neighbors.em and cl.neighbors.missing == missing
    assert_neighbors(cl.neighbors, want, f"clump lists, missing={missing}")
    rank, member_ok = ops.clump_ranks(pv, 1e-2, 2e-2, live)
    state, owner = ops.select_host(want[0], want[2], rank, member_ok)
    idx = np.flatnonzero(state == ops.SEL_INDEX)
    idx = idx[np.argsort(rank[idx], kind="stable")]
    assert np.array_equal(cl.index, idx) and np.array_equal(cl.owner, owner)
    assert cl.index[0] == eb.ROW_HET and np.array_equal(cl.degenerate, np.flatnonzero(~live))
    assert (cl.owner[~live] == -1).all() and idx.size > 10
    pr = ops.ld_prune(p, pos, r2=eb.NBR_R2, window_bp=eb.MAIN_WINDOW, em=True, missing=missing)
    assert_neighbors(pr.neighbors, strict, f"prune lists, missing={missing}")
    N, A = eb.own_counts(codes, missing == PW)
    f = A / np.maximum(2.0 * N, 1.0)
    want_rank = ops.priority_ranks(np.minimum(f, 1.0 - f), live)
    assert np.array_equal(pr.rank, want_rank)
    state, _ = ops.select_host(strict[0], strict[2], want_rank, live.astype(np.uint8))
    assert np.array_equal(pr.keep, state == ops.SEL_INDEX) and pr.keep.sum() > 0
    assert not pr.keep[~live].any()                         # monomorphic SNPs are never kept
    maf = np.minimum(f, 1.0 - f)
    assert maf[eb.ROW_HET] == 0.5                            # the all-heterozygous SNP takes part, among the first
    assert want_rank[eb.ROW_HET] == int((live[:eb.ROW_HET] & (maf[:eb.ROW_HET] == 0.5)).sum())
    assert not (pr.keep[strict[1]] & pr.keep[strict[2]]).any()


# ---- 9. invariances ---------------------------------------------------------------------------------------------------------------
def all_bytes(p, pos, missing):
    from ld_tools_amd import ops
    res = ops.ld_em_band(p, pos, window_bp=eb.MAIN_WINDOW, missing=missing)
    nb = ops.ld_neighbors(p, pos, window_bp=eb.MAIN_WINDOW, r2=eb.NBR_R2, em=True, missing=missing)
    return [bits(res.r.values), bits(res.dprime.values), bits(res.r.diag), nb.hits.cpu().numpy(), nb.offsets.cpu().numpy()]


@pytest.mark.parametrize("missing", MISSING)
def test_permuted_individuals_and_rephased_genotypes_give_identical_bytes(gpu, missing):
    key, codes, pos = main_case(missing, 254)
    base = all_bytes(packed(key, codes), pos, missing)
    re = px.rephase(codes, 8)
    assert not np.array_equal(re, codes)
    for name, other in (("permuted", px.permute_individuals(codes, 5)), ("rephased", re)):
        got = all_bytes(packed((name,) + key, other), pos, missing)
        for a, b in zip(base, got):
            assert np.array_equal(a, b), name


def test_the_r_band_is_a_band_like_any_other(gpu):
    from ld_tools_amd import ops
    n, n_hap = 300, 254
    codes = eb.mixed_panel(n, n_hap)
    p = packed(("mixed", n, n_hap), codes)
    pos = pb.ragged_positions(n)
    res = ops.ld_em_band(p, pos, window_bp=eb.MAIN_WINDOW, missing=PW)
    dense = res.r.to_dense()
    assert np.array_equal(dense.view(np.uint32), dense.T.copy().view(np.uint32))
    lo, off, rows, cols = eb.band_cells(pos, eb.MAIN_WINDOW)
    assert np.array_equal(dense[rows, cols].view(np.uint32), bits(res.r.values))
    assert np.array_equal(np.diagonal(dense).view(np.uint32), bits(res.r.diag))
    inside = np.zeros((n, n), dtype=bool)
    inside[rows, cols] = inside[cols, rows] = True
    np.fill_diagonal(inside, True)
    assert not dense[~inside].any()
    x = np.random.default_rng(3).normal(size=n).astype(np.float32)
    prod = res.r.matvec(x)
    x32 = np.ascontiguousarray(prod.x32.cpu().numpy().reshape(n))
    with np.errstate(over="ignore"):
        want = np.array([ops.prod_terms(dense[i][inside[i]], x32[inside[i]]).sum() for i in range(n)], dtype=np.int64)
    assert np.array_equal(prod.sums.cpu().numpy().reshape(n), want)
    indptr, indices, data = res.r.to_csr()
    assert indptr[-1] == 2 * res.n_cells + n and np.array_equal(res.r.row(n - 1)[1].view(np.uint32),
                                                                 bits(res.r.values)[int(off[n - 1]):])


# ---- 10. argument rules -----------------------------------------------------------------------------------------------------------
def test_argument_rules(gpu):
    import torch
    from ld_tools_amd import PackedPanel, _lib, ops
    lib = _lib.lib
    n, h = 300, 254
    codes = eb.mixed_panel(n, h)
    p = packed(("mixed", n, h), codes)
    ws_bytes = lib.ldx_ld_em_band_workspace_bytes(n)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=gpu)
    ptr = buf.data_ptr()
    side = [p.alt.data_ptr(), p.ref.data_ptr(), p.acnt.data_ptr(), p.rcnt.data_ptr()]
    names = ("alt", "ref", "acnt", "rcnt")
    who = ""

    def refused(rc_, code, message):
        """the code and the WHOLE message, word for word (callers match on the words)"""
        assert rc_ == code, (rc_, code, message, lib.ldx_last_error().decode())
        assert lib.ldx_last_error().decode() == f"{who}: {message}"

    E_ARG, E_UNSUPPORTED = -1, -3
    assert _lib.E_NAMES[E_ARG] == "LDX_E_ARG" and _lib.E_NAMES[E_UNSUPPORTED] == "LDX_E_UNSUPPORTED"
    null, odd = "{} is a null pointer", "n_hap 255 is odd (haplotypes 2k and 2k + 1 are the two alleles of individual k)"
    plane = "alt is a bit plane of 4 GiB or more (4194304 SNPs x 10240 haplotypes)"
    pw_only = {"ref": "ref is a null pointer (the pairwise form reads both planes)",
               "rcnt": "rcnt is a null pointer (the pairwise form reads both count tables)"}
    band = dict(side=side, n_snps=n, n_hap=h, pairwise=1, positions=ptr, window=5, workspace=ptr, workspace_bytes=ws_bytes)

    def store(**kw):
        a = dict(band, lo=ptr, offsets=ptr, values_r=ptr, values_dprime=ptr, n_cells=5)
        a.update(kw)
        return lib.ldx_ld_em_band_dev(*a["side"], a["n_snps"], a["n_hap"], a["pairwise"], a["positions"], a["window"], a["lo"],
                                      a["offsets"], a["values_r"], a["values_dprime"], a["n_cells"], a["workspace"],
                                      a["workspace_bytes"], None)

    def nbr(**kw):
        a = dict(band, r2_bound=0.2, hits=ptr, hit_cap=256, n_hits=ptr)
        a.update(kw)
        return lib.ldx_ld_em_neighbors_dev(*a["side"], a["n_snps"], a["n_hap"], a["pairwise"], a["positions"], a["window"],
                                           a["r2_bound"], a["hits"], a["hit_cap"], a["n_hits"], a["workspace"],
                                           a["workspace_bytes"], None)

    def without(k):
        return side[:k] + [None] + side[k + 1:]

    for fn, name in ((store, "ldx_ld_em_band_dev"), (nbr, "ldx_ld_em_neighbors_dev")):
        who = name
        for k, arg in enumerate(names):
            refused(fn(side=without(k)), E_ARG, pw_only.get(arg, null.format(arg)))
        refused(fn(side=without(0), pairwise=0), E_ARG, null.format("alt"))
        refused(fn(positions=None), E_ARG, null.format("positions"))
        refused(fn(workspace=None), E_ARG, null.format("workspace"))
        refused(fn(window=-1), E_ARG, "window -1 is negative")
        refused(fn(n_snps=0), E_ARG, "n_snps is 0")
        refused(fn(n_hap=0), E_ARG, "n_hap is 0")
        refused(fn(n_hap=255), E_ARG, odd)
        refused(fn(n_hap=10242), E_UNSUPPORTED, "n_hap 10242 > LDX_MAX_HAPS 10240")
        refused(fn(n_snps=1 << 22, n_hap=10240), E_UNSUPPORTED, plane)
        refused(fn(workspace_bytes=ws_bytes - 1), E_ARG, f"workspace_bytes {ws_bytes - 1} < {ws_bytes}")
    who = "ldx_ld_em_band_dev"
    refused(store(lo=None), E_ARG, null.format("lo"))
    refused(store(offsets=None), E_ARG, null.format("offsets"))
    refused(store(values_r=None, values_dprime=None), E_ARG, "values_r and values_dprime are both null pointers but n_cells is 5")
    # ref / rcnt may be null in the plain form; n_cells = 0 is LDX_OK and launches nothing (the buffers hold no plan)
    assert store(side=[side[0], None, side[2], None], pairwise=0, n_cells=0, values_r=None, values_dprime=None) == 0
    assert store(n_cells=0) == 0
    torch.cuda.synchronize()
    assert not bool(buf.any().item())
    who = "ldx_ld_em_neighbors_dev"
    refused(nbr(r2_bound=0.0), E_ARG, "r2_bound must be a float32 > 0 (got 0)")
    refused(nbr(r2_bound=float("nan")), E_ARG, "r2_bound must be a float32 > 0 (got nan)")
    refused(nbr(hits=None), E_ARG, "hits is a null pointer but hit_cap is 256")
    refused(nbr(n_hits=None), E_ARG, null.format("n_hits"))
    who = "ldx_em_snp_stats_dev"

    def stats(**kw):
        a = dict(side=side, n_snps=n, n_hap=h, pairwise=1, N=ptr, A=ptr, diag=ptr, live=ptr)
        a.update(kw)
        return lib.ldx_em_snp_stats_dev(*a["side"], a["n_snps"], a["n_hap"], a["pairwise"], a["N"], a["A"], a["diag"], a["live"], None)

    for k, arg in enumerate(names):
        refused(stats(side=without(k)), E_ARG, pw_only.get(arg, null.format(arg)))
    for arg in ("N", "A", "diag"):
        refused(stats(**{arg: None}), E_ARG, null.format(arg))
    refused(stats(n_snps=0), E_ARG, "n_snps is 0")
    refused(stats(n_hap=255), E_ARG, odd)
    refused(stats(n_hap=10242), E_UNSUPPORTED, "n_hap 10242 > LDX_MAX_HAPS 10240")
    # the plain form reads neither ref nor rcnt, and `live` may be left out
    big = torch.zeros(4 * n, dtype=torch.int32, device=gpu)
    assert stats(side=[side[0], None, side[2], None], pairwise=0, N=big.data_ptr(), A=big[n:].data_ptr(), diag=big[2 * n:].data_ptr(),
                 live=None) == 0
    assert np.array_equal(big[:n].cpu().numpy(), np.full(n, h // 2)) and np.array_equal(big[n:2 * n].cpu().numpy(), p.alt_counts())
    # the stats against the integers of the codes
    for pairwise in (False, True):
        N, A, diag, live = ops.em_snp_stats(p, pairwise)
        wn, wa = eb.own_counts(codes, pairwise)
        assert np.array_equal(N.cpu().numpy(), wn) and np.array_equal(A.cpu().numpy(), wa)
        assert np.array_equal(live.cpu().numpy().astype(bool), eb.own_live(codes, pairwise))
    # the Python layer's own rules, before the device is touched
    pos = pb.ragged_positions(n)
    odd_panel = PackedPanel.from_codes(rc.random_codes(4, 255, np.random.default_rng(1)))
    with pytest.raises(_lib.LdxError, match="even n_hap"):
        ops.ld_em_band(odd_panel, window_snps=4)
    with pytest.raises(_lib.LdxError, match='missing must be None or "pairwise"'):
        ops.ld_em_band(p, pos, missing="complete")
    for fn, more in ((ops.ld_neighbors, {}), (ops.ld_prune, {}), (ops.ld_clump, {"pvalues": np.full(n, 1e-5)})):
        with pytest.raises(_lib.LdxError, match="em=True and dosage=True"):
            fn(p, pos, em=True, dosage=True, **more)
        with pytest.raises(_lib.LdxError, match="FP4 band only"):
            fn(p, pos, em=True, path="mfma", **more)
        with pytest.raises(_lib.LdxError, match='missing must be None or "pairwise"'):
            fn(p, pos, em=True, missing="complete", **more)
        with pytest.raises(_lib.LdxError, match="even n_hap"):
            fn(odd_panel, np.arange(4), em=True, **{k: v[:4] for k, v in more.items()})


# ---- 11. driver -------------------------------------------------------------------------------------------------------------------
def test_drivers_on_a_chromosome_with_missing_calls(gpu, tmp_path):
    from test_gpu_ld_pairwise import rs_rows, vcf_with_missing_calls
    from ld_tools_amd import ops
    from ld_tools_amd.drivers import clump, em_band, em_window_hits, prune, write_em_band, write_ld_table
    from ld_tools_amd.drivers.clump import chrom_panel
    vcf, names = vcf_with_missing_calls()
    rows_in = rs_rows(vcf, "6")
    panel, _, rs_ids, poss = chrom_panel(vcf, "6", rows_in, names, "test")
    n = panel.n_snps
    assert int(((panel.acnt[:n] + panel.rcnt[:n]) != panel.n_hap).sum()) > 0   # calls are missing
    pos = np.asarray(poss, dtype=np.int64)
    window, r2 = 2_000, 0.05
    lo, off, rows, cols = eb.band_cells(pos, window)
    for missing in MISSING:
        sq = ops.ld_em(panel, missing=missing)
        sq_r, sq_d = sq.r.cpu().numpy(), sq.dprime.cpu().numpy()
        m = em_band(vcf, "6", rows_in, names, window_bp=window, missing=missing)
        assert m.rs_ids == rs_ids and m.poss == poss and m.bands.r.missing == missing and 0 < m.bands.n_cells == rows.size
        assert np.array_equal(bits(m.bands.r.values), bits(sq_r[rows, cols]))
        assert np.array_equal(bits(m.bands.dprime.values), bits(sq_d[rows, cols]))
        paths = write_em_band(str(tmp_path / f"em_{missing}"), m)
        assert np.array_equal(np.load(paths[0]).view(np.uint32), bits(sq_r[rows, cols]))
        assert np.array_equal(np.load(paths[1]).view(np.uint32), bits(sq_d[rows, cols]))
        assert np.array_equal(np.load(paths[2]), off) and np.array_equal(np.load(paths[3]), lo)
        assert np.array_equal(np.load(paths[4]).view(np.uint32), bits(m.bands.r.diag))
        assert len(open(paths[5]).read().splitlines()) == n + 1
        side, hits = em_window_hits(vcf, "6", rows_in, names, r2=r2, window_bp=window, missing=missing)
        want = eb.expected_neighbors(n, rows, cols, sq_r[rows, cols], sq_d[rows, cols], ops.r2_bound(r2))
        once = want[1] < want[2]
        gi, gj, gr = hits.pairs()
        assert once.sum() > 0 and hits.em and hits.missing == missing
        assert np.array_equal(gi, want[1][once]) and np.array_equal(gj, want[2][once])
        assert np.array_equal(gr.view(np.uint32), want[3][once].view(np.uint32))
        assert np.array_equal(bits(hits.dprime), want[4][once].view(np.uint32))
        path = str(tmp_path / f"em_{missing}.ld")
        assert write_ld_table(path, side, side, hits) == int(once.sum())
        lines = open(path).read().splitlines()[1:]
        listed = [tuple(ln.split("\t")[:2]) for ln in lines]
        assert len(set(listed)) == len(listed) == int(once.sum())                      # each in-window pair once
        assert not {(b, a) for a, b in listed} & set(listed)
        assert listed == [(rs_ids[a], rs_ids[b]) for a, b in zip(want[1][once], want[2][once])]
    # the selections pass em through
    pv = np.linspace(1e-6, 1e-3, len(rows_in))
    ct = clump(vcf, "6", rows_in, names, pv, p1=1e-2, p2=1e-2, r2=r2, window_bp=window, em=True, missing=PW)
    pt = prune(vcf, "6", rows_in, names, r2=r2, window_bp=window, em=True, missing=PW)
    assert ct.clumps.neighbors.em and ct.clumps.neighbors.missing == PW and pt.pruned.neighbors.em
    direct = ops.ld_prune(panel, pos, r2=r2, window_bp=window, em=True, missing=PW)
    assert np.array_equal(pt.pruned.keep, direct.keep)


# ---- 12. past the first trip of the plan --------------------------------------------------------------------------------------
# eb.PLAN_CASE: 258 I blocks of 128 rows, two of them in plan_kernel's second trip (ldx_band_plan.h): the carry between trips,
# prefix[Ti] after the loop, tile_at's search over 259 entries, rows up to 32 972.  The reference of every cell is the EM
# rectangle of a SELECTED panel, whose rows start at 0; sampled cells of the last I blocks go to the 60-digit oracle.
PLAN_PANELS = ("plan", "mixed")
PLAN_FILL = 0x7FC12345   # a quiet NaN with a payload no kernel produces
_PLAN = {}


def plan_case(kind):
    n, n_hap = eb.PLAN_CASE
    codes = eb.plan_panel() if kind == "plan" else eb.mixed_panel(n, n_hap)
    return ("plan", kind), codes, pb.ragged_positions(n)


def plan_layout():
    """(lo, offsets, rows, cols) of the plan case on the host, int64, from band_layout_host; once per process."""
    if "layout" not in _PLAN:
        lo, off, rows, cols = eb.band_cells(pb.ragged_positions(eb.PLAN_CASE[0]), eb.PLAN_WINDOW)
        _PLAN["layout"] = (lo.astype(np.int64), off.astype(np.int64), rows, cols)
    return _PLAN["layout"]


def plan_bands(gpu, kind, missing):
    """ld_em_band of the plan case, once per panel and form (the store test checks every cell of it)."""
    import torch
    from ld_tools_amd import ops
    if (kind, missing) not in _PLAN:
        key, codes, pos = plan_case(kind)
        # two freed blocks of the values' size full of the fill pattern: the allocator hands them to the next requests of that
        # size, so a cell the kernel leaves out is likely to show as the pattern and not as an earlier run's bytes
        filled = [torch.full((eb.PLAN_CELLS,), PLAN_FILL, dtype=torch.int32, device=gpu) for _ in range(2)]
        del filled
        _PLAN[(kind, missing)] = ops.ld_em_band(packed(key, codes), pos, window_bp=eb.PLAN_WINDOW, missing=missing)
    return _PLAN[(kind, missing)]


@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("kind", PLAN_PANELS)
def test_past_the_first_trip_the_store_is_the_rectangle_and_the_oracle(gpu, kind, missing):
    import torch
    from ld_tools_amd import ops
    key, codes, pos = plan_case(kind)
    n = codes.shape[0]
    p = packed(key, codes)
    lo, off, rows, cols = plan_layout()
    what = f"plan case, {kind} panel, missing={missing}"
    res = plan_bands(gpu, kind, missing)
    assert res.r.n_snps == n and res.n_cells == eb.PLAN_CELLS
    assert np.array_equal(res.r.layout()[0], lo) and np.array_equal(res.r.layout()[1], off)
    got = {"r": res.r.values.view(torch.int32), "D'": res.dprime.values.view(torch.int32)}
    for name, g in got.items():
        assert not bool((g == PLAN_FILL).any().item()), f"{what}: a cell of {name} was not written"
    for (a, b), (c0, c1), cells, li, lj in bc.band_chunks(lo, off):
        sq = ops.ld_em(p.select(snps=np.arange(a, b)), p.select(snps=np.arange(c0, c1)), missing=missing)
        at = torch.from_numpy(li * (c1 - c0) + lj).to(gpu)
        for name, m in (("r", sq.r), ("D'", sq.dprime)):
            want = m.reshape(-1).view(torch.int32)[at]
            mine = got[name][int(cells[0]): int(cells[-1]) + 1]
            if not torch.equal(mine, want):
                k = int(torch.nonzero(mine != want)[0].item())
                raise AssertionError(f"{what}: {name} cell {cells[k]} = ({a + li[k]}, {c0 + lj[k]}) has the bits {mine[k].item():#x}, "
                                     f"the rectangle of rows {a} .. {b - 1} has {want[k].item():#x}")
    live = assert_diag(res, codes, missing, what)
    # the 60-digit oracle on seeded cells of I blocks 255 and above, on their own five integers (a tie passes either way)
    cand = np.flatnonzero(live[rows] & live[cols] & (rows >= eb.PLAN_SAMPLED_FROM))
    pick = np.sort(np.random.default_rng(255).choice(cand, size=eb.PLAN_SAMPLED_CELLS, replace=False))
    assert (rows[pick] >= 128 * eb.PLAN_TRIP).sum() >= 50                      # in the second trip's own rows too
    counts = eb.pair_counts(codes, rows[pick], cols[pick], missing == PW)
    r, d = res.r.values.cpu().numpy()[pick], res.dprime.values.cpu().numpy()[pick]
    bad = eb.cells_pass_the_oracle(counts, r, d)
    assert not bad, f"{what}: {len(bad)} of {pick.size} sampled cells miss the oracle, the first {bad[0]}"


@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("kind", PLAN_PANELS)
def test_past_the_first_trip_neighbours_are_the_host_filter_of_the_band_cells(gpu, kind, missing):
    from ld_tools_amd import ops
    key, codes, pos = plan_case(kind)
    n = codes.shape[0]
    lo, off, rows, cols = plan_layout()
    res = plan_bands(gpu, kind, missing)
    want = eb.expected_neighbors(n, rows, cols, res.r.values.cpu().numpy(), res.dprime.values.cpu().numpy(),
                                 ops.r2_bound(eb.NBR_R2))
    nb = ops.ld_neighbors(packed(key, codes), pos, window_bp=eb.PLAN_WINDOW, r2=eb.NBR_R2, em=True, missing=missing)
    assert_neighbors(nb, want, f"plan case, {kind} panel, missing={missing}")
    assert int((want[1] >= 128 * eb.PLAN_TRIP).sum()) >= 1                     # a hit in a row of the second trip

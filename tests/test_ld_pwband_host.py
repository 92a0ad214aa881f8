"""CPU: pairwise-complete LD on the band (include/ldx.h, "pairwise-complete bands") -- the expected band cells, sums and lists
of one small case from the numpy mirrors (tests/ld_pwband_cases.py) against the exact oracle (tests/ld_pairwise_exact.py), the
ABI of the five new entries, the argument rules that come before the device, and the properties of the GPU tests' panels.  No
kernel is launched here."""
import ctypes as C
import re
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

NEW_SYMBOLS = ["ldx_ld_pw_band_workspace_bytes", "ldx_pw_snp_stats_dev", "ldx_ld_pw_band_dev", "ldx_ld_pw_score_dev",
               "ldx_ld_pw_neighbors_dev"]
E_ARG, E_UNSUPPORTED = -1, -3
NEG0, POS0 = np.uint32(0x80000000), np.uint32(0)
SMALL = (300, 254)   # the pinned case: two I blocks, three slabs


# ---- 1. the expected band, sums and lists of one small case against the oracle ----------------------------------------------
@pytest.mark.parametrize("dosage", [False, True])
def test_expected_band_sums_and_lists_against_the_oracle(dosage):
    from ld_tools_amd import ops
    n, n_hap = SMALL
    codes, done = pb.mixed_panel(n, n_hap)
    assert set(done) == {"individual", "half", "disjoint", "mono"}
    pos = pb.ragged_positions(n)
    window = 1500
    exp = pb.expected_band(codes, pos, window, dosage)
    ex = px.PairwiseExactBlock(codes, codes, dosage)
    rows, cols = exp["rows"], exp["cols"]
    # the layout: every pair i > j with pos_i - pos_j <= window once, nothing else
    want = np.argwhere((np.subtract.outer(pos, pos) <= window) & np.tri(n, k=-1, dtype=bool))
    assert np.array_equal(np.stack([rows, cols], axis=1), want) and int(exp["offsets"][n]) == len(want) > 10 * n
    # counts equal, cells within 4 ulps, the signed zeros exactly
    assert np.array_equal(exp["counts"], ex.counts)
    b = exp["values"].view(np.uint32)
    deg, zero = ex.degenerate[rows, cols], ex.zero_num[rows, cols]
    assert np.array_equal(b == NEG0, deg) and np.array_equal(b == POS0, zero)
    assert deg.any() and (b == POS0).sum() == zero.sum()
    rest = ~deg & ~zero
    assert float(lx.ulp32_err(exp["values"][rest], ex.r64[rows, cols][rest]).max()) <= 4.0
    # the planted pairs lie inside the window
    for i, j in ((px.ROW_DISJOINT + pb.SHIFT, px.ROW_DISJOINT), (px.ROW_MONO + pb.SHIFT, px.ROW_MONO)):
        at = np.flatnonzero((rows == i) & (cols == j))
        assert at.size == 1 and b[at[0]] == NEG0
    assert int(ex.counts[0][px.ROW_DISJOINT + pb.SHIFT, px.ROW_DISJOINT]) == 0
    # the diagonal: live over the SNP's own called set
    v_own = np.diagonal(ex.v_x)
    assert np.array_equal(exp["live"], v_own > 0) and np.array_equal(v_own, np.diagonal(ex.v_y))
    assert np.array_equal(exp["diag"].view(np.uint32) == np.float32(1.0).view(np.uint32), exp["live"])
    assert np.array_equal(exp["diag"].view(np.uint32) == NEG0, ~exp["live"]) and (~exp["live"]).sum() >= 3
    # sums: the uint64 sum of score_terms over the window, own term included -- against a dense restatement
    ann = pb.annot_matrix(n)
    bits, k = ops.pack_annot(ann, n)
    sums = pb.expected_sums(n, rows, cols, exp["values"], exp["live"], bits, k).view(np.int64)
    lo_w, hi_w = ops.window_bounds(pos, window)
    dense = np.zeros((n, n), dtype=np.int64)
    dense[rows, cols] = dense[cols, rows] = ops.score_terms(exp["values"]).astype(np.int64)
    dense[np.arange(n), np.arange(n)] = np.where(exp["live"], 1 << 32, 0)
    inside = (np.arange(n)[None, :] >= lo_w[:, None]) & (np.arange(n)[None, :] < hi_w[:, None])
    assert not dense[~inside].any()
    assert np.array_equal(sums[:, 0], dense.sum(axis=1))
    for c in range(k):
        assert np.array_equal(sums[:, 1 + c], dense[:, ann[:, c]].sum(axis=1))
    assert (sums[:, 3] != sums[:, 0]).any()
    # lists: both orientations, sorted, r and s bits; the oracle decides
    bound = ops.r2_bound(pb.NBR_R2)
    off, i, j, r, s = pb.expected_neighbors(n, rows, cols, exp["values"], bound)
    assert i.size % 2 == 0 and i.size > 0 and np.array_equal(np.lexsort((j, i)), np.arange(i.size))
    assert int(off[n]) == i.size and np.array_equal(np.diff(off), np.bincount(i, minlength=n))
    kept = np.zeros((n, n), dtype=bool)
    kept[i, j] = True
    assert np.array_equal(kept, kept.T) and not np.diagonal(kept).any()
    cls = ex.classes(pb.NBR_R2)
    band = np.zeros((n, n), dtype=bool)
    band[rows, cols] = band[cols, rows] = True
    assert kept[band & (cls == px.IN)].all() and not kept[band & (cls == px.OUT)].any() and not kept[~band].any()
    assert np.array_equal(s.view(np.uint32), np.multiply(r, r, dtype=np.float32).view(np.uint32))


def test_a_panel_without_holes_gives_the_plain_band():
    """No missing code: the expected pairwise band is ops' plain r32 arithmetic on n_hap and the allele counts."""
    n, n_hap = 200, 254
    codes = pb.complete_panel(n, n_hap)
    assert px.complete_rows(codes).all()
    pos = pb.ragged_positions(n)
    for dosage in (False, True):
        exp = pb.expected_band(codes, pos, 1000, dosage)
        assert (exp["counts"][0] == (n_hap // 2 if dosage else n_hap)).all()
        plain = px.PairwiseExactBlock(codes, codes, dosage)
        assert np.array_equal(exp["live"], ~np.diagonal(plain.degenerate))


# ---- 2. the GPU tests' panels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dosage", [False, True])
def test_neighbours_panel_is_decided_by_the_oracle(dosage):
    """Under the oracle alone: at least MIN_DECIDED_IN in-window pairs decided IN and at most AMBIGUOUS_SHARE_MAX of the
    in-window pairs left open at NBR_R2, on the panel and window tests/test_gpu_ld_pwband.py uses."""
    from ld_tools_amd import ops
    n, n_hap = pb.N_MAIN, 1008
    codes, _ = pb.mixed_panel(n, n_hap)
    lo, off = ops.band_layout_host(pb.ragged_positions(n), pb.MAIN_WINDOW)
    rows, cols = bc.cell_rows_cols(lo, off)
    cls = px.PairwiseExactBlock(codes, codes, dosage).classes(pb.NBR_R2)[rows, cols]
    n_in, amb = int((cls == px.IN).sum()), int((cls == px.AMBIGUOUS).sum())
    print(f"dosage={dosage}: {n_in} in, {amb} ambiguous of {cls.size} in-window pairs")
    assert n_in >= pb.MIN_DECIDED_IN and amb <= pb.AMBIGUOUS_SHARE_MAX * cls.size
    assert 2 * n_in > 256                                                   # more than one batch of slots


def test_the_panels_hold_what_the_gpu_tests_rely_on():
    from ld_tools_amd import ops
    n = pb.N_MAIN
    pos = pb.ragged_positions(n)
    assert (np.diff(pos) >= 0).all() and (np.diff(pos) == 0).any()           # non-decreasing, with duplicates
    lo, off = ops.band_layout_host(pos, pb.MAIN_WINDOW)
    reach = np.arange(n) - lo
    assert 128 < int(reach.max()) < 384 and pb.tiles_walked(lo, n) >= 9    # several slabs per I block, none of them the whole row
    for n_hap in pb.MAIN_HAPS:
        codes, done = pb.mixed_panel(n, n_hap)
        assert set(done) == {"individual", "half", "disjoint", "mono"}
        holes = ~px.complete_rows(codes)
        assert 0.5 < holes.mean() < 0.8 and (codes[-1] == 2).all() and (codes[n // 2] == 1).all() and (codes[1] == 0).all()
        assert pb.tile_kinds(codes, lo) == {(True, True)}                    # every tile takes the general loop
    assert pb.MAIN_HAPS[0] < 256 < pb.MAIN_HAPS[1] and pb.MAIN_HAPS[2] % 2 == 1
    # the four tile kinds, and tiles that are only partly in the window
    codes = pb.tiles_panel()
    holes = ~px.complete_rows(codes)
    assert holes[pb.HOLE_ROWS].any() and not holes[:256].any() and not holes[384:].any()
    lo_t, _ = ops.band_layout_host(np.arange(n), pb.TILES_WINDOW_SNPS)
    assert pb.tile_kinds(codes, lo_t) == {(False, False), (True, False), (False, True), (True, True)}
    assert int(lo_t[512]) % 128 != 0 and int(lo_t[699]) > 128 * (int(lo_t[512]) // 128)   # a first slab that is partly outside
    # the walk: lo jumps inside an I block with clustered positions and window 0
    lo_c, _ = ops.band_layout_host(bc.clustered(2700), 0)
    jumps = np.flatnonzero(np.diff(lo_c.astype(np.int64)) > 0) + 1
    assert jumps.tolist() == [2500, 2501, 2516] and 2304 < 2500 < 2560
    lo_0, off_0 = ops.band_layout_host(bc.grid(300), 0)
    assert int(off_0[300]) == 0 and np.array_equal(lo_0, np.arange(300))      # window 0 on distinct positions: no cell
    # the grid case: more tiles than two workgroups on each of 256 compute units
    ng, _ = pb.GRID_CASE
    assert pb.tiles_walked(np.zeros(ng, dtype=np.int64), ng) > 1024
    assert pb.WALK_SIZES == (1, 257, 4226)
    # the largest counts
    big, _ = pb.mixed_panel(*pb.BIG_CASE)
    assert (big[65] == 1).all()
    assert int(px.PairwiseExactBlock(big[60:70], big[60:70]).c.max()) == pb.BIG_CASE[1]
    assert int(px.PairwiseExactBlock(big[60:70], big[60:70], True).S.max()) == 2 * pb.BIG_CASE[1]


def test_the_plan_case_lies_past_the_first_trip_of_the_plan():
    """PLAN_CASE from band_layout_host alone: 258 I blocks of 256 rows, so two of them in plan_kernel's second trip, with the
    four tile kinds among their tiles; and band_chunks covers the band once."""
    from ld_tools_amd import ops
    n, n_hap = pb.PLAN_CASE
    assert n == 65_869 and n_hap == 62
    pos = pb.ragged_positions(n)
    lo, off = ops.band_layout_host(pos, pb.PLAN_WINDOW)
    lo = lo.astype(np.int64)
    blocks = (n + 255) // 256
    assert blocks == 258 > pb.PLAN_TRIP and n - 256 * 257 == 77                # one full and one ragged block past the trip
    assert int(off[n]) == pb.PLAN_CELLS == 1_669_273 and int((np.arange(n) - lo).max()) == pb.PLAN_REACH == 41
    assert pb.tiles_walked(lo, n) == pb.PLAN_TILES == 772 > 2 * 256            # more than two workgroups on each of 256 CUs
    assert pb.tiles_walked(lo, n, pb.PLAN_TRIP) == pb.PLAN_TILES_PAST == 5 >= 4
    assert any(lo[256 * ti] // 128 < (256 * ti) // 128 for ti in range(pb.PLAN_TRIP, blocks))   # a first slab that is not its own
    codes = pb.plan_panel()
    assert codes.shape == pb.PLAN_CASE
    holes = ~px.complete_rows(codes)
    assert holes[pb.PLAN_HOLE_ROWS].any() and int(holes.sum()) == int(holes[pb.PLAN_HOLE_ROWS].sum())   # one slab, nothing else
    assert pb.PLAN_HOLE_ROWS.start % 128 == 0 and pb.PLAN_HOLE_ROWS.stop - pb.PLAN_HOLE_ROWS.start == 128
    assert pb.PLAN_HOLE_ROWS.start // 256 == pb.PLAN_TRIP
    assert pb.tile_kinds(codes, lo, pb.PLAN_TRIP) == {(False, False), (True, False), (False, True), (True, True)}
    assert pb.tile_kinds(pb.mixed_panel(n, n_hap)[0], lo, pb.PLAN_TRIP) == {(True, True)}
    # the chunks: every cell once, in layout order, inside its chunk's rectangle, at its own (row, column)
    rows, cols = bc.cell_rows_cols(lo, off)
    seen = []
    for (a, b), (c0, c1), cells, li, lj in bc.band_chunks(lo, off):
        assert 0 < b - a <= bc.CHUNK_ROWS and c1 == b and c0 == lo[a] and c1 - c0 <= bc.CHUNK_ROWS + pb.PLAN_REACH
        assert np.array_equal(rows[cells], a + li) and np.array_equal(cols[cells], c0 + lj)
        assert (li < b - a).all() and (lj >= 0).all() and (lj < c1 - c0).all()
        seen.append(cells)
    assert len(seen) == 17 and np.array_equal(np.concatenate(seen), np.arange(pb.PLAN_CELLS))


# ---- 3. the ABI and the argument rules --------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    from ld_tools_amd import _lib
    raw = (ROOT / "include" / "ldx.h").read_text()
    assert "pairwise-complete bands" in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ldx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/ldx.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libldx.so"
    assert _lib.version() == 102                                           # new symbols only: no version bump
    assert "#define LDX_VERSION 102" in raw.replace("  ", " ")
    ws = _lib.lib.ldx_ld_pw_band_workspace_bytes
    assert ws(1) >= 16 + 4 and ws(100_000) >= 8 * (391 + 1) + 4 * 100_000 and ws(100_000) % 256 == 0


def test_entries_refuse_bad_arguments_before_any_launch():
    from ld_tools_amd import _lib
    lib = _lib.lib
    big = C.create_string_buffer(4096 + 256)
    ptr = (C.addressof(big) + 255) // 256 * 256   # a non-null stand-in for every pointer (never read)
    panel = ("alt", "ref", "acnt", "rcnt")
    ws_bytes = lib.ldx_ld_pw_band_workspace_bytes(100)

    def call(entry, tail, **kw):
        a = {name: ptr for name in panel}
        a.update(hom=None, n_snps=100, n_hap=64, dosage=0, positions=ptr, window=10, workspace=ptr, workspace_bytes=ws_bytes)
        a.update(tail)
        a.update(kw)
        if a["dosage"] and "hom" not in kw:
            a["hom"] = ptr
        head = [a[name] for name in panel + ("hom", "n_snps", "n_hap", "dosage", "positions", "window")]
        return getattr(lib, entry)(*head, *[a[name] for name in tail], a["workspace"], a["workspace_bytes"], None)

    def store(**kw):
        return call("ldx_ld_pw_band_dev", dict(lo=ptr, offsets=ptr, values=ptr, n_cells=5), **kw)

    def score(**kw):
        return call("ldx_ld_pw_score_dev", dict(annot=None, n_annot=0, diag=ptr, sums=ptr), **kw)

    def nbr(**kw):
        return call("ldx_ld_pw_neighbors_dev", dict(r2_bound=0.2, hits=ptr, hit_cap=256, n_hits=ptr), **kw)

    who = {store: "ldx_ld_pw_band_dev", score: "ldx_ld_pw_score_dev", nbr: "ldx_ld_pw_neighbors_dev"}

    def said(fn, message):
        return lib.ldx_last_error().decode() == f"{who[fn]}: {message}"

    for fn, extra in ((store, ("lo", "offsets")), (score, ("diag", "sums")), (nbr, ("n_hits",))):
        for name in panel + extra + ("positions", "workspace"):
            assert fn(**{name: None}) == E_ARG and said(fn, f"{name} is a null pointer"), lib.ldx_last_error()
        assert fn(dosage=1, hom=None) == E_ARG and lib.ldx_last_error().decode().startswith(f"{who[fn]}: hom is a null pointer")
        assert fn(n_snps=0) == E_ARG and said(fn, "n_snps is 0")
        assert fn(n_hap=0) == E_ARG and said(fn, "n_hap is 0")
        assert fn(window=-1) == E_ARG and said(fn, "window -1 is negative")
        for n_hap in (63, _lib.MAX_HAPS + 1):                                    # parity speaks before the limit
            assert fn(n_hap=n_hap, dosage=1) == E_ARG
            assert said(fn, f"n_hap {n_hap} is odd (dosage pairs haplotypes 2k and 2k + 1 into individuals)")
        assert fn(n_hap=63, n_snps=0) == E_ARG and said(fn, "n_snps is 0")        # an odd n_hap is fine for haplotype r
        assert fn(n_hap=_lib.MAX_HAPS + 2) == E_UNSUPPORTED and said(fn, "n_hap 10242 > LDX_MAX_HAPS 10240")
        assert fn(n_snps=1 << 24, n_hap=10240) == E_UNSUPPORTED
        assert said(fn, "alt is a bit plane of 4 GiB or more (16777216 SNPs x 10240 haplotypes)")
        assert fn(workspace_bytes=ws_bytes - 1) == E_ARG and said(fn, f"workspace_bytes {ws_bytes - 1} < {ws_bytes}")
    assert store(values=None) == E_ARG and said(store, "values is a null pointer but n_cells is 5")
    assert score(n_annot=9, annot=ptr) == E_ARG and said(score, "n_annot 9 > 8")
    assert score(n_annot=2) == E_ARG and said(score, "annot is a null pointer but n_annot is 2")
    assert nbr(hits=None) == E_ARG and said(nbr, "hits is a null pointer but hit_cap is 256")
    for bad, shown in ((0.0, "0"), (-0.5, "-0.5"), (float("nan"), "nan")):
        assert nbr(r2_bound=bad) == E_ARG and said(nbr, f"r2_bound must be a float32 > 0 (got {shown})")

    def stats(**kw):
        a = dict(alt=ptr, ref=ptr, acnt=ptr, rcnt=ptr, n_snps=100, n_hap=64, dosage=0, diag=ptr, live=None)
        a.update(kw)
        return lib.ldx_pw_snp_stats_dev(*[a[k] for k in ("alt", "ref", "acnt", "rcnt", "n_snps", "n_hap", "dosage", "diag", "live")],
                                        None)

    for name in panel + ("diag",):
        assert stats(**{name: None}) == E_ARG and lib.ldx_last_error().decode() == f"ldx_pw_snp_stats_dev: {name} is a null pointer"
    assert stats(n_snps=0) == E_ARG and stats(n_hap=63, dosage=1) == E_ARG and stats(n_hap=10242) == E_UNSUPPORTED


def test_python_argument_rules_come_before_the_device():
    import torch
    from ld_tools_amd import LdxError, PackedPanel, ops
    from ld_tools_amd.drivers.band import band_matrix
    from ld_tools_amd.drivers.ldscore import ld_scores

    def host_panel(n_snps, n_hap):
        z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731
        return PackedPanel(n_snps, n_hap, z(1, torch.uint8), z(1, torch.uint8), z(128, torch.int32), z(128, torch.int32),
                           z(128, torch.float64), z(128, torch.float64), z(128, torch.float64))

    a, odd = host_panel(10, 64), host_panel(10, 63)
    pos = np.arange(10, dtype=np.int64)
    p = np.full(10, 0.5)
    calls = {
        "ld_band": lambda **kw: ops.ld_band(a, pos, **kw),
        "ld_score": lambda **kw: ops.ld_score(a, pos, **kw),
        "ld_neighbors": lambda **kw: ops.ld_neighbors(a, pos, **kw),
        "ld_prune": lambda **kw: ops.ld_prune(a, pos, **kw),
        "ld_clump": lambda **kw: ops.ld_clump(a, pos, p, **kw),
    }
    for name, fn in calls.items():
        for bad in ("ref", "complete", "Pairwise", 1, True, ""):
            with pytest.raises(LdxError, match=f"{name}: missing must be"):
                fn(missing=bad)
        for path in ("mfma", "popcount", "auto"):
            with pytest.raises(LdxError, match=f"{name}: missing=\"pairwise\" runs on the FP4 band only"):
                fn(missing="pairwise", path=path)
        if not torch.cuda.is_available():                                   # valid arguments: only now the device is asked for
            for kw in (dict(missing="pairwise"), dict(missing="pairwise", path="fp4")):
                with pytest.raises(LdxError, match="HIP device"):
                    fn(**kw)
    with pytest.raises(LdxError, match=r"regions= together with missing=\"pairwise\".*ld_band\(missing=\"pairwise\"\)"):
        ops.ld_score(a, pos, regions=np.zeros(10, dtype=np.int64), missing="pairwise")
    for fn in (ops.ld_band, ops.ld_score, ops.ld_neighbors):
        with pytest.raises(LdxError, match="even n_hap"):
            fn(odd, pos, dosage=True, missing="pairwise")
    for drv in (ld_scores, band_matrix):
        with pytest.raises(LdxError, match="missing must be"):
            drv(None, "6", [], [], missing="drop")
        with pytest.raises(LdxError, match="missing='ref' belongs to dosage=True"):
            drv(None, "6", [], [], missing="ref")
    # the new fields have defaults
    assert ops.LDBand(None, torch.zeros(1), None, None, None, 0).missing is None
    assert ops.LDScores(None, None, 0, 2, None, 0).missing is None
    assert ops.LDNeighbors(None, None, 1, 0, np.float32(0.2)).missing is None

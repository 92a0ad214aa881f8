"""CPU: EM LD on the band (include/ldx.h, "EM on the band") -- the cases module of the GPU tests pinned on hand-checked layouts
(tests/ld_emband_cases.py: the 128-row walk, the four tile kinds, the 561 tiles of the grid case, the all-heterozygous row), the
ABI of the four new entries, their argument rules (which come before any HIP call), and the Python-side refusals that need no
device.  No kernel is launched here."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_band_cases as bc  # noqa: E402
import ld_em_exact as emx  # noqa: E402
import ld_em_pairwise_exact as epx  # noqa: E402
import ld_emband_cases as eb  # noqa: E402
import ld_pairwise_exact as px  # noqa: E402
import ld_pwband_cases as pb  # noqa: E402

NEW_SYMBOLS = ["ldx_ld_em_band_workspace_bytes", "ldx_em_snp_stats_dev", "ldx_ld_em_band_dev", "ldx_ld_em_neighbors_dev"]
E_ARG, E_UNSUPPORTED = -1, -3


# ---- 1. the cases module ------------------------------------------------------------------------------------------------------
def test_tiles_walked_on_hand_checked_layouts():
    # the everything window: the lower triangle of 128 x 128 tiles, the diagonal tiles included
    for n, want in ((1, 1), (128, 1), (129, 3), (700, 21), (4100, 33 * 34 // 2)):
        assert eb.tiles_walked(np.zeros(n, dtype=np.int64), n) == want, n
    # window 0 on distinct positions: lo[i] = i, every I block meets its own slab only
    assert eb.tiles_walked(np.arange(700), 700) == 6
    # 300 SNPs each side at n = 700: blocks 0 .. 2 reach slab 0 (1 + 2 + 3), lo[384] = 84 -> slabs 0 .. 3, lo[512] = 212 ->
    # 1 .. 4, lo[640] = 340 -> 2 .. 5
    lo = np.maximum(0, np.arange(700) - 300)
    assert eb.tiles_walked(lo, 700) == 1 + 2 + 3 + 4 + 4 + 4
    # a layout whose lo jumps inside a block counts from the block's FIRST row
    lo = np.where(np.arange(300) < 130, 0, 256)
    assert eb.tiles_walked(lo, 300) == 1 + 2 + 1
    from ld_tools_amd import ops
    assert eb.tiles_walked(ops.band_layout_host(np.arange(700), 300)[0], 700) == 18


def test_the_four_tile_kinds_of_case_2():
    from ld_tools_amd import ops
    codes = eb.tiles_panel()
    n = codes.shape[0]
    assert n == 700 and codes.shape[1] == 1008
    holes = ~px.complete_rows(codes)
    assert holes[pb.HOLE_ROWS].any() and not holes[:256].any() and not holes[384:].any()   # slab 2 and nothing else
    lo, _ = ops.band_layout_host(np.arange(n), eb.TILES_WINDOW_SNPS)
    assert eb.tile_kinds(codes, lo) == {(False, False), (True, False), (False, True), (True, True)}
    # without the window's reach (window 0) no clean block meets the slab with holes
    assert eb.tile_kinds(codes, np.arange(n)) == {(False, False), (True, True)}


def test_the_grid_case_has_561_tiles_and_two_hole_rows():
    n, n_hap = eb.GRID_CASE
    assert eb.tiles_walked(np.zeros(n, dtype=np.int64), n) == eb.GRID_TILES == 561 > 2 * 256   # an MI355X has 256 CUs
    codes = eb.grid_panel()
    assert codes.shape == (n, n_hap)
    holes = np.flatnonzero(~px.complete_rows(codes))
    assert sorted(holes.tolist()) == sorted(eb.GRID_HOLE_ROWS) and max(eb.GRID_HOLE_ROWS) > 4096 and min(eb.GRID_HOLE_ROWS) < 128
    assert eb.own_live(codes, True)[list(eb.GRID_HOLE_ROWS)].all()


def test_the_plan_case_lies_past_the_first_trip_of_the_plan():
    """PLAN_CASE from band_layout_host alone: 258 I blocks of 128 rows, so two of them in plan_kernel's second trip, with the
    four tile kinds among their tiles; and band_chunks covers the band once."""
    from ld_tools_amd import ops
    n, n_hap = eb.PLAN_CASE
    assert n == 32_973 and n_hap == 62
    pos = pb.ragged_positions(n)
    lo, off = ops.band_layout_host(pos, eb.PLAN_WINDOW)
    lo = lo.astype(np.int64)
    blocks = (n + 127) // 128
    assert blocks == 258 > eb.PLAN_TRIP and n - 128 * 257 == 77                # one full and one ragged block past the trip
    assert int(off[n]) == eb.PLAN_CELLS == 836_438 and int((np.arange(n) - lo).max()) == eb.PLAN_REACH == 38
    assert eb.tiles_walked(lo, n) == eb.PLAN_TILES == 515 > 2 * 256            # more than two workgroups on each of 256 CUs
    assert eb.tiles_walked(lo, n, eb.PLAN_TRIP) == eb.PLAN_TILES_PAST == 4
    assert any(lo[128 * ti] // 128 < ti for ti in range(eb.PLAN_TRIP, blocks))   # a first slab that is not the block's own
    codes = eb.plan_panel()
    assert codes.shape == eb.PLAN_CASE
    holes = ~px.complete_rows(codes)
    assert holes[eb.PLAN_HOLE_ROWS].any() and int(holes.sum()) == int(holes[eb.PLAN_HOLE_ROWS].sum())   # one slab, nothing else
    assert (eb.PLAN_HOLE_ROWS.start, eb.PLAN_HOLE_ROWS.stop) == (128 * eb.PLAN_TRIP, 128 * eb.PLAN_TRIP + 128)
    assert eb.tile_kinds(codes, lo, eb.PLAN_TRIP) == {(False, False), (True, False), (False, True), (True, True)}
    assert eb.tile_kinds(eb.mixed_panel(n, n_hap), lo, eb.PLAN_TRIP) == {(True, True)}
    live = eb.own_live(codes, True)
    rows, cols = bc.cell_rows_cols(lo, off)
    assert int((live[rows] & live[cols] & (rows >= eb.PLAN_SAMPLED_FROM)).sum()) > eb.PLAN_SAMPLED_CELLS
    # the chunks: every cell once, in layout order, inside its chunk's rectangle, at its own (row, column)
    seen = []
    for (a, b), (c0, c1), cells, li, lj in bc.band_chunks(lo, off):
        assert 0 < b - a <= bc.CHUNK_ROWS and c1 == b and c0 == lo[a] and c1 - c0 <= bc.CHUNK_ROWS + eb.PLAN_REACH
        assert np.array_equal(rows[cells], a + li) and np.array_equal(cols[cells], c0 + lj)
        assert (li < b - a).all() and (lj >= 0).all() and (lj < c1 - c0).all()
        seen.append(cells)
    assert len(seen) == 9 and np.array_equal(np.concatenate(seen), np.arange(eb.PLAN_CELLS))


@pytest.mark.parametrize("kind", ["mixed", "complete"])
def test_the_all_heterozygous_row_is_live_for_the_em_only(kind):
    n, n_hap = 300, 254
    codes = eb.mixed_panel(n, n_hap) if kind == "mixed" else eb.complete_panel(n, n_hap)
    assert not codes.flags.writeable
    row = codes[eb.ROW_HET]
    assert (row[0::2] == 0).all() and (row[1::2] == 1).all()
    for pairwise in (False, True):
        N, A = eb.own_counts(codes, pairwise)
        live = eb.own_live(codes, pairwise)
        assert N[eb.ROW_HET] == A[eb.ROW_HET] == n_hap // 2 and live[eb.ROW_HET]
        assert not live[1] and not live[n // 2] and not live[n - 1]   # rc.special_rows: all REF, all ALT, all missing
        assert (N <= n_hap // 2).all() and (A <= 2 * N).all()
    # the dosage form sees no variance there: N (A + 2 HA) - A^2 = N * N - N^2 = 0
    _, g, hom = px.ind_planes(codes[eb.ROW_HET:eb.ROW_HET + 1])
    assert int(hom.sum()) == 0 and int(g.sum()) ** 2 == (n_hap // 2) * int(g.sum())
    # its own pair: em_cell's tie rule would give r = -1 there, which is why the diagonal is defined and not computed
    counts = eb.pair_counts(codes, [eb.ROW_HET], [eb.ROW_HET], True)[:, 0]
    assert counts.tolist() == [n_hap // 2, n_hap // 2, n_hap // 2, n_hap // 2, n_hap // 2]
    # no copy of ld_codes reads the row
    base = pb.mixed_panel(n, n_hap)[0] if kind == "mixed" else pb.complete_panel(n, n_hap)
    assert np.array_equal(np.delete(codes, eb.ROW_HET, axis=0), np.delete(base, eb.ROW_HET, axis=0))


def test_the_mirrors_on_a_small_case():
    n, n_hap = 40, 62
    codes = eb.plant_het(pb.mixed_panel(n, n_hap)[0][:, :n_hap])
    rows, cols = np.array([5, 30, 39, 33]), np.array([4, 2, 38, 7])
    for pairwise in (False, True):
        counts = eb.pair_counts(codes, rows, cols, pairwise)
        src = codes if pairwise else np.where(codes == 1, 1, 0).astype(np.int8)
        assert np.array_equal(counts, epx.loop_counts(src, src)[:, rows, cols])
        N, A = eb.own_counts(codes, pairwise)
        full = epx.pair_counts(src, src)
        assert np.array_equal(N, np.diagonal(full[0])) and np.array_equal(A, np.diagonal(full[1]))
    # expected_neighbors: both orientations, sorted by (i, j), -0.0 never a hit, D' in the fourth column
    r = np.array([0.9, -0.0, -0.5, 0.1], dtype=np.float32)
    d = np.array([1.0, -0.0, 0.75, 0.3], dtype=np.float32)
    off, i, j, rr, dd = eb.expected_neighbors(n, rows, cols, r, d, np.float32(0.2))
    assert i.tolist() == [4, 5, 38, 39] and j.tolist() == [5, 4, 39, 38]
    assert rr.tolist() == [np.float32(0.9), np.float32(0.9), -0.5, -0.5] and dd.tolist() == [1.0, 1.0, 0.75, 0.75]
    assert off[0] == 0 and off[-1] == 4 and off[5] == 1 and off[6] == 2 and off[39] == 3
    # the oracle check refuses a wrong cell and accepts the fp64 restatement's
    from ld_tools_amd import ops
    tup = np.array([[20], [17], [22], [21], [5]])
    _, rv, dv = ops.em_host(20, 17, 22, 21, 5)
    assert not eb.cells_pass_the_oracle(tup, [np.float32(rv)], [np.float32(dv)])
    assert eb.cells_pass_the_oracle(tup, [np.float32(rv) + np.float32(1e-3)], [np.float32(dv)])
    assert emx.cells_ok(emx.solve(20, 17, 22, 21, 5), np.float32(rv), np.float32(dv))


# ---- 2. the ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    import ld_tools_amd
    from ld_tools_amd import _lib
    raw = (ROOT / "include" / "ldx.h").read_text()
    assert "EM on the band" in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ldx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/ldx.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libldx.so"
    ws = _lib.lib.ldx_ld_em_band_workspace_bytes
    assert ws(1) >= 16 + 4 and ws(100_000) >= 8 * (782 + 1) + 4 * 100_000 and ws(100_000) % 256 == 0
    for name in ("ld_em_band", "LDEmBand", "em_snp_stats"):
        assert name in ld_tools_amd.__all__ and hasattr(ld_tools_amd, name)
    from ld_tools_amd import drivers
    for name in ("em_band", "write_em_band", "em_window_hits", "EmBand"):
        assert hasattr(drivers, name)


def test_entries_refuse_bad_arguments_before_any_launch():
    from ld_tools_amd import _lib
    lib = _lib.lib
    big = C.create_string_buffer(4096 + 256)
    ptr = (C.addressof(big) + 255) // 256 * 256   # a non-null stand-in for every pointer (never read)
    panel = ("alt", "ref", "acnt", "rcnt")
    ws_bytes = lib.ldx_ld_em_band_workspace_bytes(100)

    def call(entry, tail, **kw):
        a = {name: ptr for name in panel}
        a.update(n_snps=100, n_hap=64, pairwise=1, positions=ptr, window=10, workspace=ptr, workspace_bytes=ws_bytes)
        a.update(tail)
        a.update(kw)
        head = [a[name] for name in panel + ("n_snps", "n_hap", "pairwise", "positions", "window")]
        return getattr(lib, entry)(*head, *[a[name] for name in tail], a["workspace"], a["workspace_bytes"], None)

    def store(**kw):
        return call("ldx_ld_em_band_dev", dict(lo=ptr, offsets=ptr, values_r=ptr, values_dprime=ptr, n_cells=5), **kw)

    def nbr(**kw):
        return call("ldx_ld_em_neighbors_dev", dict(r2_bound=0.2, hits=ptr, hit_cap=256, n_hits=ptr), **kw)

    who = {store: "ldx_ld_em_band_dev", nbr: "ldx_ld_em_neighbors_dev"}
    odd = "n_hap {} is odd (haplotypes 2k and 2k + 1 are the two alleles of individual k)"
    pw_only = {"ref": "ref is a null pointer (the pairwise form reads both planes)",
               "rcnt": "rcnt is a null pointer (the pairwise form reads both count tables)"}

    def said(fn, message):
        return lib.ldx_last_error().decode() == f"{who[fn]}: {message}"

    for fn, extra in ((store, ("lo", "offsets")), (nbr, ("n_hits",))):
        for name in panel + extra + ("positions", "workspace"):
            assert fn(**{name: None}) == E_ARG and said(fn, pw_only.get(name, f"{name} is a null pointer")), lib.ldx_last_error()
        for name in ("alt", "acnt"):                                              # the plain form needs these two ...
            assert fn(**{name: None}, pairwise=0) == E_ARG and said(fn, f"{name} is a null pointer")
        assert fn(ref=None, rcnt=None, pairwise=0, n_snps=0) == E_ARG and said(fn, "n_snps is 0")   # ... and not the other two
        assert fn(n_snps=0) == E_ARG and said(fn, "n_snps is 0")
        assert fn(n_hap=0) == E_ARG and said(fn, "n_hap is 0")
        assert fn(window=-1) == E_ARG and said(fn, "window -1 is negative")
        for n_hap in (63, _lib.MAX_HAPS + 1):                                    # parity speaks before the limit
            for pairwise in (0, 1):
                assert fn(n_hap=n_hap, pairwise=pairwise) == E_ARG and said(fn, odd.format(n_hap))
        assert fn(n_hap=_lib.MAX_HAPS + 2) == E_UNSUPPORTED and said(fn, "n_hap 10242 > LDX_MAX_HAPS 10240")
        assert fn(n_snps=1 << 24, n_hap=10240) == E_UNSUPPORTED
        assert said(fn, "alt is a bit plane of 4 GiB or more (16777216 SNPs x 10240 haplotypes)")
        assert fn(workspace_bytes=ws_bytes - 1) == E_ARG and said(fn, f"workspace_bytes {ws_bytes - 1} < {ws_bytes}")
    assert store(values_r=None, values_dprime=None) == E_ARG
    assert said(store, "values_r and values_dprime are both null pointers but n_cells is 5")
    # n_cells = 0 is LDX_OK and launches nothing (no device here, and the pointers lead nowhere), with or without values
    assert store(n_cells=0) == 0 and store(n_cells=0, values_r=None, values_dprime=None) == 0
    assert store(n_cells=0, ref=None, rcnt=None, pairwise=0) == 0
    assert nbr(hits=None) == E_ARG and said(nbr, "hits is a null pointer but hit_cap is 256")
    for bad, shown in ((0.0, "0"), (-0.5, "-0.5"), (float("nan"), "nan")):
        assert nbr(r2_bound=bad) == E_ARG and said(nbr, f"r2_bound must be a float32 > 0 (got {shown})")

    def stats(**kw):
        a = dict(alt=ptr, ref=ptr, acnt=ptr, rcnt=ptr, n_snps=100, n_hap=64, pairwise=1, N=ptr, A=ptr, diag=ptr, live=None)
        a.update(kw)
        order = ("alt", "ref", "acnt", "rcnt", "n_snps", "n_hap", "pairwise", "N", "A", "diag", "live")
        return lib.ldx_em_snp_stats_dev(*[a[k] for k in order], None)

    for name in panel + ("N", "A", "diag"):
        assert stats(**{name: None}) == E_ARG
        assert lib.ldx_last_error().decode() == "ldx_em_snp_stats_dev: " + pw_only.get(name, f"{name} is a null pointer")
    assert stats(n_snps=0) == E_ARG and stats(n_hap=10242) == E_UNSUPPORTED
    assert stats(n_hap=63, pairwise=0) == E_ARG and lib.ldx_last_error().decode() == "ldx_em_snp_stats_dev: " + odd.format(63)


# ---- 3. the Python layer ------------------------------------------------------------------------------------------------------
def test_python_argument_rules_come_before_the_device():
    import torch
    from ld_tools_amd import LdxError, PackedPanel, ops
    from ld_tools_amd.drivers import em_band  # noqa: F401  (importable without a device)

    def host_panel(n_snps, n_hap):
        z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731
        return PackedPanel(n_snps, n_hap, z(1, torch.uint8), z(1, torch.uint8), z(128, torch.int32), z(128, torch.int32),
                           z(128, torch.float64), z(128, torch.float64), z(128, torch.float64))

    a, odd = host_panel(10, 64), host_panel(10, 63)
    pos = np.arange(10, dtype=np.int64)
    p = np.full(10, 0.5)
    calls = {
        "ld_neighbors": lambda panel=a, **kw: ops.ld_neighbors(panel, pos, em=True, **kw),
        "ld_prune": lambda panel=a, **kw: ops.ld_prune(panel, pos, em=True, **kw),
        "ld_clump": lambda panel=a, **kw: ops.ld_clump(panel, pos, p, em=True, **kw),
    }
    for name, fn in calls.items():
        for bad in ("ref", "complete", "Pairwise", 1, True, ""):
            with pytest.raises(LdxError, match=f"{name}: missing must be"):
                fn(missing=bad)
        with pytest.raises(LdxError, match=f"{name}: em=True and dosage=True exclude each other"):
            fn(dosage=True)
        for path in ("mfma", "popcount", "auto"):
            with pytest.raises(LdxError, match=f"{name}: em=True runs on the FP4 band only"):
                fn(path=path)
        for missing in (None, "pairwise"):
            with pytest.raises(LdxError, match=f"{name}: the EM needs an even n_hap \\(got 63\\)"):
                fn(panel=odd, missing=missing)
        if not torch.cuda.is_available():                                   # valid arguments: only now the device is asked for
            for kw in (dict(), dict(missing="pairwise"), dict(path="fp4")):
                with pytest.raises(LdxError, match="HIP device"):
                    fn(**kw)
    with pytest.raises(LdxError, match="ld_em_band: missing must be"):
        ops.ld_em_band(a, pos, missing="complete")
    with pytest.raises(LdxError, match="ld_em_band: the EM needs an even n_hap"):
        ops.ld_em_band(odd, pos)
    with pytest.raises(LdxError, match="ld_em_band: neither r nor D' was asked for"):
        ops.ld_em_band(a, pos, want_r=False, want_dprime=False)
    with pytest.raises(LdxError, match="even n_hap"):
        ops.em_snp_stats(odd)
    if not torch.cuda.is_available():
        with pytest.raises(LdxError, match="HIP device"):
            ops.ld_em_band(a, pos, missing="pairwise")
    # the new fields have defaults, and D' is an EM list's only
    assert ops.LDBand(None, torch.zeros(1), None, None, None, 0).em is False
    nb = ops.LDNeighbors(None, torch.zeros((2, 4), dtype=torch.int32), 1, 0, np.float32(0.2))
    assert nb.em is False and nb.missing is None
    with pytest.raises(LdxError, match="em=True"):
        nb.dprime
    em_nb = ops.LDNeighbors(None, torch.zeros((2, 4), dtype=torch.int32), 1, 0, np.float32(0.2), em=True)
    assert em_nb.dprime.dtype == torch.float32 and em_nb.dprime.shape == (2,)
    assert ops.LDEmBand(None, None, None).r is None

"""GPU: Gabriel's D' confidence bounds on the EM band and the blocks picked from them (ops.ld_dprime_ci, ops.ld_ci_from_counts,
ops.ld_gabriel_blocks; include/ldx.h, "Gabriel blocks").

Contract: every byte of the two bound bands is the list epilogue's (ldx_ld_ci_from_counts_dev: the same device function) on the
pair's five integers from the CPU (ld_em_pairwise_exact.pair_counts), 0xFF where a SNP is not kept or the cell lies outside the
window; sampled cells equal the 60-digit definition (tests/ld_ci_exact.py) unless that calls the tuple fragile, and at most 0.5 %
of a sample may be fragile; blocks, block count and candidate count are the host mirrors' on the DEVICE's own bytes, exactly --
it is integer logic from there on.  Sizes sit on the band kernel's loops: 128 x 128 tiles, 256-haplotype K-blocks.

Section 6 drives the integer kernels of csrc/ldx_gabriel.hip directly, on made-up bound bytes (tests/ld_gabriel_kernel_cases.py):
the candidate list slot by slot against the layout and the host mirror, the pick against the host mirror, both against the plain
loops of tests/ld_gabriel_cases.py where those are cheap.  tests/test_ld_gabriel_host.py proves without a GPU that each input
reaches the depth it is there for.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_ci_exact as cx  # noqa: E402
import ld_dosage_exact as dx  # noqa: E402
import ld_em_pairwise_exact as epx  # noqa: E402
import ld_emband_cases as eb  # noqa: E402
import ld_gabriel_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

PW = eb.PW
MISSING = [None, PW]
SAMPLED = eb.SAMPLED_CELLS          # 400
FRAGILE_CAP = 0.005


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


_PACKED = {}


def packed(key, codes):
    from ld_tools_amd import PackedPanel
    if key not in _PACKED:
        _PACKED[key] = PackedPanel.from_codes(np.array(codes))   # (a copy: the codes are read-only)
    return _PACKED[key]


def form(codes, missing):
    """The codes as the form counts them: plain = a missing code is REF."""
    codes = np.asarray(codes)
    return codes if missing == PW else np.where(codes == 1, 1, 0).astype(np.int8)


def host_kept(codes, missing, keep=None, maf_min=0.05):
    from ld_tools_amd import ops
    N, A = eb.own_counts(form(codes, missing), True)
    return ops.gabriel_kept_host(N, A, keep, maf_min)


def raw_ci_band(panel, pos, window, kept, band_lo, offsets, n_cells, pairwise, fill):
    """ldx_ld_em_ci_band_dev into two buffers that hold ``fill`` in every byte."""
    import torch
    from ld_tools_amd import _lib, ops
    dev = panel.device
    lo = torch.full((n_cells,), fill, dtype=torch.uint8, device=dev)
    hi = torch.full((n_cells,), fill, dtype=torch.uint8, device=dev)
    ws = torch.empty(_lib.lib.ldx_ld_em_band_workspace_bytes(panel.n_snps), dtype=torch.uint8, device=dev)
    pos_d = torch.as_tensor(np.asarray(pos, dtype=np.int64)).to(dev)
    kept_d = torch.as_tensor(np.asarray(kept).astype(np.uint8)).to(dev)
    _lib.check(_lib.lib.ldx_ld_em_ci_band_dev(*ops._em_panel(panel, pairwise), panel.n_snps, panel.n_hap, int(pairwise),
                                              pos_d.data_ptr(), int(window), kept_d.data_ptr(), band_lo.data_ptr(),
                                              offsets.data_ptr(), lo.data_ptr(), hi.data_ptr(), n_cells, ws.data_ptr(), ws.numel(),
                                              None), "ldx_ld_em_ci_band_dev")
    torch.cuda.synchronize()
    return lo.cpu().numpy(), hi.cpu().numpy()


def check_against_the_oracle(counts, lo, hi, what, capped=True):
    """The cells of ``counts`` [5, m] against ld_ci_exact; returns the number of fragile tuples (``capped``: at most 0.5 %)."""
    fragile, bad = 0, []
    for k in range(counts.shape[1]):
        t = tuple(int(v) for v in counts[:, k])
        want_lo, want_hi, frag = cx.bounds_fast(*t)
        if frag:
            fragile += 1
        elif (int(lo[k]), int(hi[k])) != (want_lo, want_hi):
            bad.append((t, (int(lo[k]), int(hi[k])), (want_lo, want_hi)))
    print(f"{what}: {counts.shape[1]} sampled cells, {fragile} fragile, {len(bad)} mismatches")
    assert not bad, f"{what}: {len(bad)} cells miss the definition, the first {bad[0]}"
    assert not capped or fragile <= FRAGILE_CAP * counts.shape[1], (what, fragile)
    return fragile


# ---- 1. the bounds on the band ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("n_hap", eb.MAIN_HAPS)
def test_every_cell_is_the_list_epilogue_on_the_cpu_counts(gpu, n_hap, missing):
    from ld_tools_amd import ops
    codes, pos, where = gc.gabriel_panel(n_hap)
    n = codes.shape[0]
    what = f"gabriel_panel({n_hap}), missing={missing}"
    panel = packed(("gabriel", n_hap), codes)
    ci = ops.ld_dprime_ci(panel, pos, window_bp=gc.WINDOW, missing=missing)
    band_lo, off, rows, cols = eb.band_cells(pos, gc.WINDOW)
    assert ci.n_cells == rows.size and ci.n_snps == n and ci.lo.dtype == ci.hi.dtype == __import__("torch").uint8
    assert np.array_equal(ci.layout()[0], band_lo.astype(np.int64)) and np.array_equal(ci.layout()[1], off.astype(np.int64))
    assert 3 < eb.tiles_walked(band_lo, n) <= 6 and (band_lo[-1] > 0)          # diagonal and off-diagonal tiles, cut by the window
    kept = host_kept(codes, missing)
    assert np.array_equal(ci.kept.cpu().numpy().astype(bool), kept) and not kept[where["rare_snp"][0]] and kept.sum() > n - 5
    got_lo, got_hi = ci.lo.cpu().numpy(), ci.hi.cpu().numpy()
    run = kept[rows] & kept[cols]
    assert ((got_lo[~run] == ops.NO_CI) & (got_hi[~run] == ops.NO_CI)).all() and (~run).sum() >= 100, what
    counts = epx.pair_counts(form(codes, missing), form(codes, missing))[:, rows[run], cols[run]]
    want_lo, want_hi = (t.cpu().numpy() for t in ops.ld_ci_from_counts(*counts))
    bad = np.flatnonzero((got_lo[run] != want_lo) | (got_hi[run] != want_hi))
    assert bad.size == 0, (f"{what}: {bad.size} cells differ from the list epilogue, the first ({rows[run][bad[0]]}, "
                           f"{cols[run][bad[0]]}): {(got_lo[run][bad[0]], got_hi[run][bad[0]])} != {(want_lo[bad[0]], want_hi[bad[0]])}")
    assert (want_lo != ops.NO_CI).all() and (want_lo <= want_hi).all() and want_hi.max() == 100 and want_lo.max() >= 90
    # the definition itself, on a seeded sample
    pick = np.sort(np.random.default_rng(n_hap).choice(counts.shape[1], size=SAMPLED, replace=False))
    check_against_the_oracle(counts[:, pick], want_lo[pick], want_hi[pick], what)
    # the same pairs whichever SNP comes first
    swap_lo, swap_hi = (t.cpu().numpy() for t in ops.ld_ci_from_counts(*counts[[0, 2, 1, 3, 4]][:, pick]))
    assert np.array_equal(swap_lo, want_lo[pick]) and np.array_equal(swap_hi, want_hi[pick])
    # a relaunch into dirty buffers gives the same bytes: every cell of the layout is written
    again_lo, again_hi = raw_ci_band(panel, pos, gc.WINDOW, kept, ci.band_lo, ci.offsets, ci.n_cells, missing == PW, 0x5A)
    assert np.array_equal(again_lo, got_lo) and np.array_equal(again_hi, got_hi), what
    dense_lo, dense_hi = ci.to_dense()
    assert np.array_equal(dense_lo, gc.dense_from_band(got_lo, band_lo, off, n)) and np.array_equal(dense_lo, dense_lo.T)
    assert dense_hi[0, n - 1] == ops.NO_CI and dense_lo[5, 5] == ops.NO_CI
    s70, rec = ci.strong(70).cpu().numpy(), ci.recombinant().cpu().numpy()
    assert np.array_equal(s70, (got_lo != 0xFF) & (got_lo >= 70) & (got_hi >= 98)) and np.array_equal(rec, got_hi < 90)
    assert s70.sum() > 100 and rec.sum() > 100 and not (s70 & rec).any()


def test_cells_of_a_wider_layout_outside_the_window_are_no_interval(gpu):
    """A layout made for twice the window: its cells beyond the window's first column are written, with 0xFF."""
    import torch
    from ld_tools_amd import ops
    codes, pos, _ = gc.gabriel_panel(254)
    n = codes.shape[0]
    panel = packed(("gabriel", 254), codes)
    wide_lo, wide_off, rows, cols = eb.band_cells(pos, 2 * gc.WINDOW)
    inside = pos[rows] - pos[cols] <= gc.WINDOW
    assert (~inside).sum() > 1000
    kept = np.ones(n, dtype=bool)
    lo_d = torch.as_tensor(wide_lo.astype(np.int32)).to(panel.device)
    off_d = torch.as_tensor(wide_off.astype(np.int64)).to(panel.device)
    got_lo, got_hi = raw_ci_band(panel, pos, gc.WINDOW, kept, lo_d, off_d, rows.size, True, 0x11)
    assert (got_lo[~inside] == ops.NO_CI).all() and (got_hi[~inside] == ops.NO_CI).all()
    ci = ops.ld_dprime_ci(panel, pos, window_bp=gc.WINDOW, missing=PW, maf_min=0.0)
    live = eb.own_live(codes, True)
    ok = inside & live[rows] & live[cols]
    narrow = gc.dense_from_band(ci.lo.cpu().numpy(), *(a.astype(np.int64) for a in ci.layout()), n)
    assert np.array_equal(got_lo[ok], narrow[rows[ok], cols[ok]]) and (got_lo[ok] != ops.NO_CI).all()


# ---- 2. past the first round of the grid -----------------------------------------------------------------------------------------
def test_the_grid_case_on_sampled_cells(gpu):
    """4100 x 62 with an everything window: 561 tiles, more than two workgroups per CU; rows past 4096."""
    from ld_tools_amd import ops
    n, n_hap = eb.GRID_CASE
    codes = eb.grid_panel()
    panel = packed(("grid",), codes)
    ci = ops.ld_dprime_ci(panel, window_snps=n, missing=PW)
    assert ci.n_cells == n * (n - 1) // 2
    kept = host_kept(codes, PW)
    assert np.array_equal(ci.kept.cpu().numpy().astype(bool), kept) and kept.sum() > n // 4 and not kept.all()
    rng = np.random.default_rng(62)
    dropped = np.maximum(np.flatnonzero(~kept)[:20], 1)                   # pairs with a SNP that is not kept: (k, k - 1), or (1, 0)
    rows = np.concatenate([rng.integers(1, n, size=300), rng.integers(4000, n, size=100), dropped,
                           np.array(eb.GRID_HOLE_ROWS + (4099,))])
    cols = (rng.random(rows.size) * rows).astype(np.int64)
    cols[400:400 + dropped.size] = dropped - 1
    cols[-1] = eb.GRID_HOLE_ROWS[1]                                       # both hole-carrying rows in one pair
    at = rows * (rows - 1) // 2 + cols                                    # lo[i] = 0: offsets[i] = i (i - 1) / 2
    got_lo, got_hi = ci.lo.cpu().numpy()[at], ci.hi.cpu().numpy()[at]
    run = kept[rows] & kept[cols]
    assert run.sum() >= 150 and (~run).sum() >= 1
    assert (got_lo[~run] == ops.NO_CI).all() and (got_hi[~run] == ops.NO_CI).all()
    counts = eb.pair_counts(codes, rows[run], cols[run], True)
    want_lo, want_hi = (t.cpu().numpy() for t in ops.ld_ci_from_counts(*counts))
    assert np.array_equal(got_lo[run], want_lo) and np.array_equal(got_hi[run], want_hi)
    # (31 individuals: small tables tie often, so the fragile share is reported, not capped -- the cap is test 1's)
    check_against_the_oracle(counts[:, :150], want_lo[:150], want_hi[:150], "grid case", capped=False)


# ---- 3. invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", MISSING)
def test_bounds_do_not_depend_on_phase_or_on_the_order_of_individuals(gpu, missing):
    from ld_tools_amd import ops
    codes, pos, _ = gc.gabriel_panel(254)
    n_hap = codes.shape[1]
    base = ops.ld_dprime_ci(packed(("gabriel", 254), codes), pos, window_bp=gc.WINDOW, missing=missing)
    other = dx.rephase(codes, seed=254)                                   # swapped alleles within calls, individuals permuted
    perm = np.random.default_rng(8).permutation(n_hap // 2)
    moved = np.ascontiguousarray(np.array(codes).reshape(-1, n_hap // 2, 2)[:, perm].reshape(-1, n_hap))
    assert not np.array_equal(other, codes) and not np.array_equal(moved, codes)
    for name, c in (("rephased", other), ("permuted", moved)):
        res = ops.ld_dprime_ci(packed(("gabriel", 254, name), c), pos, window_bp=gc.WINDOW, missing=missing)
        assert np.array_equal(res.lo.cpu().numpy(), base.lo.cpu().numpy()), name
        assert np.array_equal(res.hi.cpu().numpy(), base.hi.cpu().numpy()), name


def test_list_epilogue_on_hand_tuples(gpu):
    from ld_tools_amd import ops
    tuples = np.array([(127, 100, 100, 200, 0), (127, 100, 154, 0, 0), (127, 127, 127, 127, 127), (127, 120, 120, 210, 30),
                       (127, 0, 100, 0, 0), (127, 254, 100, 200, 0), (127, 300, 10, 0, 0), (127, 10, 10, 3, 0), (0, 0, 0, 0, 0),
                       (5120, 5120, 5120, 5120, 5120), (5120, 10000, 10000, 20000, 0)], dtype=np.int64).T
    lo, hi = (t.cpu().numpy() for t in ops.ld_ci_from_counts(*tuples))
    assert (lo[0], hi[0]) == (97, 100) and lo.dtype == np.uint8
    assert (lo[4:9] == ops.NO_CI).all() and (hi[4:9] == ops.NO_CI).all()
    for k in (0, 1, 2, 3, 9, 10):
        want_lo, want_hi, frag = cx.bounds_fast(*tuples[:, k])
        assert frag or (lo[k], hi[k]) == (want_lo, want_hi), tuples[:, k]
    one_n = ops.ld_ci_from_counts(127, tuples[1, :4], tuples[2, :4], tuples[3, :4], tuples[4, :4])
    assert np.array_equal(one_n[0].cpu().numpy(), lo[:4]) and np.array_equal(one_n[1].cpu().numpy(), hi[:4])


# ---- 4. blocks -------------------------------------------------------------------------------------------------------------------
def assert_blocks_are_the_mirrors(res, pos, window, what, **params):
    """block_of, n_blocks and n_candidates against the host mirrors fed the device's own bound bytes and kept mask."""
    from ld_tools_amd import ops
    kept = res.ci.kept.cpu().numpy().astype(bool)
    n = kept.size
    cands = ops.gabriel_candidates_host(res.ci.lo.cpu().numpy(), res.ci.hi.cpu().numpy(), pos, kept, window, **params)
    block_of, n_blocks = ops.gabriel_pick_host(cands, n, kept)
    assert res.n_candidates == cands.shape[0], (what, res.n_candidates, cands.shape[0])
    assert res.n_blocks == n_blocks and np.array_equal(res.block_of, block_of), what
    member = block_of < ops.NO_BLOCK
    assert res.sizes.sum() == member.sum() and (res.sizes >= 2).all() and res.starts.size == res.ends.size == n_blocks
    for b in range(n_blocks):
        inside = np.flatnonzero(block_of == b)
        assert (res.starts[b], res.ends[b], res.sizes[b]) == (inside[0], inside[-1], inside.size)
    assert np.array_equal(res.spans_bp, np.asarray(pos)[res.ends] - np.asarray(pos)[res.starts])
    assert (np.diff(res.starts) > 0).all() and (res.starts[1:] > res.ends[:-1]).all()
    return block_of, cands


@pytest.mark.parametrize("missing", MISSING)
def test_blocks_of_the_planted_panel(gpu, missing):
    from ld_tools_amd import ops
    codes, pos, where = gc.gabriel_panel(254)
    panel = packed(("gabriel", 254), codes)
    res = ops.ld_gabriel_blocks(panel, pos, window_bp=gc.WINDOW, missing=missing)
    block_of, cands = assert_blocks_are_the_mirrors(res, pos, gc.WINDOW, f"planted, missing={missing}")
    assert res.n_blocks >= 20 and res.n_candidates > 10 * res.n_blocks and {2, 3, 4} <= set(res.sizes.tolist()) and res.sizes.max() >= 5
    rare = where["rare_snp"][0]
    assert block_of[rare] == ops.NOT_KEPT and block_of[rare - 1] == block_of[rare + 1] < ops.NO_BLOCK
    assert (block_of == ops.NO_BLOCK).any()
    # other parameters: integer logic on the same bytes
    params = dict(cuts=(75, 60, 55, 65), max_spans=(8000, 12000, 40000, None), min_informative=(1, 2, 4, 5), strong_share=(3, 4),
                  cand_cut=60, strong_hi=97, recomb_hi=85)
    other = ops.ld_gabriel_blocks(panel, pos, window_bp=gc.WINDOW, missing=missing, **params)
    assert_blocks_are_the_mirrors(other, pos, gc.WINDOW, "other parameters", **params)
    assert not np.array_equal(other.block_of, res.block_of)


def test_blocks_with_keep_and_a_window_in_snps(gpu):
    from ld_tools_amd import ops
    codes, pos, _ = gc.gabriel_panel(254)
    n = codes.shape[0]
    panel = packed(("gabriel", 254), codes)
    keep = np.random.default_rng(4).random(n) > 0.2
    res = ops.ld_gabriel_blocks(panel, pos, window_bp=gc.WINDOW, missing=PW, keep=keep, maf_min=0.1)
    assert np.array_equal(res.ci.kept.cpu().numpy().astype(bool), host_kept(codes, PW, keep, 0.1))
    block_of, _ = assert_blocks_are_the_mirrors(res, pos, gc.WINDOW, "keep")
    assert (block_of[~keep] == ops.NOT_KEPT).all() and res.n_blocks >= 10
    snps = ops.ld_gabriel_blocks(panel, window_snps=20, missing=PW)
    # positions 0 .. n - 1: every span is below the two- and three-SNP caps, the window alone cuts
    assert_blocks_are_the_mirrors(snps, np.arange(n), 20, "window_snps")
    assert snps.n_blocks >= 10 and snps.spans_bp.max() <= 20


def test_blocks_of_a_random_panel_and_of_tiny_panels(gpu):
    from ld_tools_amd import ops
    codes, pos = gc.random_panel(200, 254)
    res = ops.ld_gabriel_blocks(packed(("random", 200), codes), pos, window_bp=50_000)
    assert_blocks_are_the_mirrors(res, pos, 50_000, "random panel")
    print(f"random panel: {res.n_blocks} blocks of {res.n_candidates} candidates")
    assert res.n_blocks <= 10                                              # few or none: chance pairs only
    for n in eb.SMALL_SIZES:                                               # 1 and 129
        small, small_pos, _ = gc.gabriel_panel(254, n=n)
        out = ops.ld_gabriel_blocks(packed(("gabriel", 254, n), small), small_pos, window_bp=gc.WINDOW, missing=PW)
        assert_blocks_are_the_mirrors(out, small_pos, gc.WINDOW, f"n = {n}")
        assert out.block_of.shape == (n,) and (out.n_blocks > 5 if n > 1 else (out.n_blocks, out.n_candidates) == (0, 0))
    one = ops.ld_gabriel_blocks(packed(("gabriel", 254, 1), gc.gabriel_panel(254, n=1)[0]), window_snps=5)
    assert one.block_of.tolist() in ([ops.NO_BLOCK], [ops.NOT_KEPT]) and one.ci.n_cells == 0


def test_the_operators_refuse_dosage_and_haplotype_paths(gpu):
    from ld_tools_amd import LdxError, ops
    codes, pos, _ = gc.gabriel_panel(254)
    panel = packed(("gabriel", 254), codes)
    for kw in (dict(dosage=True), dict(path="mfma"), dict(missing="zero")):
        with pytest.raises(LdxError):
            ops.ld_gabriel_blocks(panel, pos, window_bp=gc.WINDOW, **kw)
    with pytest.raises(LdxError):
        ops.ld_gabriel_blocks(panel, pos, window_bp=gc.WINDOW, cuts=(1, 2))


# ---- 5. past the first trip of the plan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("kind", ["plan", "mixed"])
def test_past_the_first_trip_every_byte_is_the_list_epilogue_on_the_cpu_counts(gpu, kind, missing):
    """eb.PLAN_CASE: 258 I blocks, two of them in plan_kernel's second trip (ldx_band_plan.h).  Every byte of both bands against
    the list epilogue on the CPU's five integers, which are counted block by block of 512 rows.  (No sample goes to the
    60-digit definition here: at 31 individuals small tables tie too often for the 0.5 % cap, as the grid case notes, and the
    list epilogue is held to the definition by test 1.)"""
    import ld_band_cases as bc
    import ld_pwband_cases as pb
    from ld_tools_amd import ops
    n, n_hap = eb.PLAN_CASE
    codes = eb.plan_panel() if kind == "plan" else eb.mixed_panel(n, n_hap)
    pos = pb.ragged_positions(n)
    what = f"plan case, {kind} panel, missing={missing}"
    panel = packed(("plan", kind), codes)
    ci = ops.ld_dprime_ci(panel, pos, window_bp=eb.PLAN_WINDOW, missing=missing)
    band_lo, off, rows, cols = eb.band_cells(pos, eb.PLAN_WINDOW)
    assert ci.n_cells == rows.size == eb.PLAN_CELLS and ci.n_snps == n
    assert np.array_equal(ci.layout()[0], band_lo.astype(np.int64)) and np.array_equal(ci.layout()[1], off.astype(np.int64))
    kept = host_kept(codes, missing)
    assert np.array_equal(ci.kept.cpu().numpy().astype(bool), kept) and kept.sum() > n // 4 and not kept.all()
    got_lo, got_hi = ci.lo.cpu().numpy(), ci.hi.cpu().numpy()
    run = kept[rows] & kept[cols]
    assert (run & (rows >= 128 * eb.PLAN_TRIP)).sum() >= 100 and (~run & (rows >= 128 * eb.PLAN_TRIP)).sum() >= 100
    assert ((got_lo[~run] == ops.NO_CI) & (got_hi[~run] == ops.NO_CI)).all(), what
    f = form(codes, missing)
    counts = np.empty((5, eb.PLAN_CELLS), dtype=np.int64)
    for (a, b), (c0, c1), cells, li, lj in bc.band_chunks(band_lo, off, 512):
        counts[:, cells] = epx.pair_counts(f[a:b], f[c0:c1])[:, li, lj]
    want_lo, want_hi = (t.cpu().numpy() for t in ops.ld_ci_from_counts(*counts[:, run]))
    bad = np.flatnonzero((got_lo[run] != want_lo) | (got_hi[run] != want_hi))
    assert bad.size == 0, (f"{what}: {bad.size} cells differ from the list epilogue, the first ({rows[run][bad[0]]}, "
                           f"{cols[run][bad[0]]}): {(got_lo[run][bad[0]], got_hi[run][bad[0]])} != {(want_lo[bad[0]], want_hi[bad[0]])}")
    has = want_lo != ops.NO_CI                                                # (a kept pair may be monomorphic within its joint set)
    assert has.mean() > 0.9 and np.array_equal(has, want_hi != ops.NO_CI) and (want_lo[has] <= want_hi[has]).all()
    # a relaunch into dirty buffers gives the same bytes: every cell of the layout is written
    again_lo, again_hi = raw_ci_band(panel, pos, eb.PLAN_WINDOW, kept, ci.band_lo, ci.offsets, ci.n_cells, missing == PW, 0x5A)
    assert np.array_equal(again_lo, got_lo) and np.array_equal(again_hi, got_hi), what


# ---- 6. the candidate and pick kernels, directly (tests/ld_gabriel_kernel_cases.py) ---------------------------------------------
# No panel and no EM: made-up bound bytes, so that the chunks of pick_kernel settle at depth, the lists run over many chunks and
# the trips of the scans over several multiples of 256.  Every device array is a view of one poisoned allocation with gaps
# between the views (kc.Kernels): a stray write fails an assertion there.
import ld_gabriel_kernel_cases as kc  # noqa: E402

_KERNELS = {}


def kernels(gpu, name, keep="case", layout=None):
    """The carve of a case, made once (its outputs and workspaces stay dirty from launch to launch)."""
    key = (name, keep if isinstance(keep, str) else "none" if keep is None else "all", layout is not None)
    if key not in _KERNELS:
        _KERNELS[key] = kc.Kernels(gpu, kc.case(name), keep=keep, layout=layout)
    return _KERNELS[key]


def assert_the_list_and_the_pick(res, name, what, params=None, all_kept=False, brute=False):
    """The three comparisons of every direct case.  ``params``: what the kernels were given (None: the defaults);
    the mirrors get the same."""
    c = kc.case(name)
    first, last, _ = kc.column_major(c["band_lo"], c["off"])
    # the list in full: one slot per cell, column-major, every slot written
    assert res.cand_span.shape == res.cand_first.shape == res.cand_last.shape == (c["n_cells"],) == first.shape, what
    assert not (res.cand_first == 0xA5A5A5A5).any() and not (res.cand_last == 0xA5A5A5A5).any(), what
    assert not (res.cand_span.view(np.uint64) == 0xA5A5A5A5A5A5A5A5).any(), what
    assert np.array_equal(res.cand_first, first) and np.array_equal(res.cand_last, last), what
    cands, block_of, n_blocks = kc.mirrors(name, params, all_kept)
    live = res.cand_span >= 0
    got = np.stack([res.cand_first[live].astype(np.int64), res.cand_last[live].astype(np.int64), res.cand_span[live]], axis=1)
    assert np.array_equal(got, cands), (what, got.shape, cands.shape)
    assert (res.cand_span[~live] == -1).all(), what
    # the pick
    assert np.array_equal(res.block_of, block_of), (what, np.flatnonzero(res.block_of != block_of)[:8])
    assert res.n_out.tolist() == [n_blocks, cands.shape[0]], (what, res.n_out, n_blocks, cands.shape[0])
    if brute:
        valid, _, brute_blocks, accepted, _ = kc.brute(name, params, all_kept)
        assert [tuple(v) for v in got.tolist()] == valid and np.array_equal(res.block_of, brute_blocks), what
        assert int(res.n_out[0]) == len(accepted), what
    return cands, block_of, n_blocks


@pytest.mark.parametrize("params", [None, kc.OTHER], ids=["default", "other"])
@pytest.mark.parametrize("name", ["random257", "random513"])
def test_kernels_on_random_bounds_equal_the_mirrors_and_the_plain_loops(gpu, name, params):
    res = kernels(gpu, name).run(params or {})
    cands, _, n_blocks = assert_the_list_and_the_pick(res, name, f"{name}, {params}", params, brute=True)
    assert cands.shape[0] >= 100 and n_blocks >= 15


@pytest.mark.parametrize("name", ["long3000", "wide600"])
def test_kernels_over_many_chunks_of_candidates(gpu, name):
    """Blocks accepted in one chunk kill candidates many chunks later (tests/test_ld_gabriel_host.py shows that they do)."""
    res = kernels(gpu, name).run({})
    cands, _, _ = assert_the_list_and_the_pick(res, name, name)
    assert cands.shape[0] > 10 * kc.CHUNK


@pytest.mark.parametrize("n,window", kc.CHAINS)
def test_kernels_on_chains_of_tied_candidates(gpu, n, window):
    """Every span ties and every candidate overlaps the next: up to 256 rounds per chunk, and the order is the slot order under
    the caller's stable sort alone."""
    from ld_tools_amd import ops
    name = f"chain{n}w{window}"
    res = kernels(gpu, name).run({})
    assert_the_list_and_the_pick(res, name, name, brute=n <= 601)
    if window == 1:                                           # without any mirror: (0, 1), (2, 3), ...
        even = n - n % 2
        assert np.array_equal(res.block_of[:even], np.arange(even) // 2) and res.n_out.tolist() == [n // 2, n - 1]
        assert n % 2 == 0 or res.block_of[n - 1] == ops.NO_BLOCK


@pytest.mark.parametrize("name", [f"trip{n}" for n in kc.TRIP_SIZES] + ["valid256of512", "valid512of699", "full256", "full512"])
def test_kernels_at_trip_and_chunk_boundaries(gpu, name):
    res = kernels(gpu, name).run({})
    assert_the_list_and_the_pick(res, name, name, brute=True)


@pytest.mark.parametrize("name", ["random257", "random513"])
def test_a_null_keep_is_every_snp_kept_and_null_params_are_the_defaults(gpu, name):
    n = kc.case(name)["n"]
    both = kernels(gpu, name, keep=None).run({})
    assert_the_list_and_the_pick(both, name, f"{name}, no keep", all_kept=True, brute=True)
    ones = kernels(gpu, name, keep=np.ones(n, dtype=bool))
    want = ones.run({})
    for r in (ones.run({}, cand_keep=False), ones.run({}, pick_keep=False), both):      # one call with a null keep, the other without
        assert all(np.array_equal(a, b) for a, b in zip(r, want))
    assert not np.array_equal(want.block_of, kc.mirrors(name)[1])
    # the candidates ignore a keep they do not get; the pick then only marks the SNPs that ITS keep drops
    mixed = kernels(gpu, name).run({}, cand_keep=False)
    dropped = ~kc.case(name)["kept"]
    assert np.array_equal(mixed.cand_span, want.cand_span) and (mixed.block_of[dropped] == 0xFFFFFFFF).all()
    assert np.array_equal(mixed.block_of[~dropped], want.block_of[~dropped]) and np.array_equal(mixed.n_out, want.n_out)
    # a null parameter pointer
    null = kernels(gpu, name).run(None)
    assert_the_list_and_the_pick(null, name, f"{name}, null params")
    assert all(np.array_equal(a, b) for a, b in zip(null, kernels(gpu, name).run({})))


def test_kernels_with_spans_above_32_bits(gpu):
    res = kernels(gpu, "scaled513").run(kc.SCALED)
    cands, _, _ = assert_the_list_and_the_pick(res, "scaled513", "scaled", kc.SCALED, brute=True)
    base = kernels(gpu, "random513").run({})
    live = base.cand_span >= 0
    assert np.array_equal(res.cand_first, base.cand_first) and np.array_equal(res.cand_last, base.cand_last)
    assert np.array_equal(res.cand_span >= 0, live) and np.array_equal(res.cand_span[live], base.cand_span[live] << 33)
    assert np.array_equal(res.block_of, base.block_of) and np.array_equal(res.n_out, base.n_out)
    assert res.cand_span.max() > 1 << 32


@pytest.mark.parametrize("name", ["long3000", "wide600"])
def test_a_relaunch_into_dirty_buffers_changes_nothing(gpu, name):
    """`used`, `start`, the suffix counts, the column offsets and the list hold the run before, then 0x00, then 0xFF."""
    k = kc.Kernels(gpu, kc.case(name))
    first = k.run({})
    assert_the_list_and_the_pick(first, name, f"{name}, poisoned")
    fills = [None, 0x00, 0xFF]
    for fill in fills:
        if fill is not None:
            k.refill(fill)
        again = k.run({})
        assert all(np.array_equal(a, b) for a, b in zip(again, first)), fill
    # and after another parameter set's run
    k.run(kc.OTHER)
    assert all(np.array_equal(a, b) for a, b in zip(k.run({}), first))


def test_no_pair_in_any_window_at_size(gpu):
    from ld_tools_amd import ops
    c = kc.case("empty700")
    res = kernels(gpu, "empty700").run({})
    assert res.cand_span.size == res.cand_first.size == res.cand_last.size == 0
    assert np.array_equal(res.block_of, np.where(c["kept"], ops.NO_BLOCK, ops.NOT_KEPT).astype(np.uint32))
    assert res.n_out.tolist() == [0, 0]
    assert_the_list_and_the_pick(res, "empty700", "empty")


def test_a_foreign_layout_writes_nothing_beyond_the_list(gpu):
    """The layout of a wider window with bands, list and n_cells of the narrow one: the guards `at >= n_cells` and
    `slot >= n_cells` of the kernels.  Values are unspecified; nothing past slot n_cells - 1 -- a gap of the carve -- is written."""
    from ld_tools_amd import ops
    c = kc.case("random513")
    wide = ops.band_layout_host(c["pos"], 3 * c["window"])
    assert int(wide[1][-1]) > 2 * c["n_cells"] and (wide[0] <= c["band_lo"]).all()
    res = kc.Kernels(gpu, c, layout=wide).run({}, pick=False)      # (run asserts the gaps)
    assert res.cand_span.shape == (c["n_cells"],) and res.block_of is None


def test_the_pick_alone_scans_the_inside_of_a_candidate(gpu):
    """A list of the caller's: a candidate whose ends are free and whose inside is blocks of the chunk before (kc.nested_list)."""
    span, first, last, block_of, n_out = kc.nested_list()
    k = kernels(gpu, "chain600w1")
    for keep in (True, False):
        res = k.pick_list(span, first, last, keep=keep)
        assert np.array_equal(res.block_of, block_of) and res.n_out.tolist() == n_out
        assert np.array_equal(res.cand_span, span) and np.array_equal(res.cand_first, first) and np.array_equal(res.cand_last, last)

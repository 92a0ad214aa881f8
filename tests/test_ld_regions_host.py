"""CPU: the host side of the LD-region family -- ops.cross_host against the exact profiles of tests/ld_regions_exact.py and
the definition as a double loop, ops.split_host against the enumeration of every admissible cut set, region_positions, the
LDRegions bookkeeping, the .bed / .regions.det writer, and the header's declarations."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_regions_exact as rx  # noqa: E402


def r32_square(ex):
    return ex.r64.astype(np.float32)


@pytest.mark.parametrize("key", ["lr700", (129, 333), (300, 64), (2, 64), (1, 64)], ids=str)
def test_cross_host_against_exact_profiles(key):
    from ld_tools_amd import ops
    _, ex = rx.panel(key)
    n = ex.n_snps
    r32 = r32_square(ex)
    worst = 0.0
    for pos, w in rx.cases(key):
        exact, pairs = rx.exact_cross(ex, pos, w)
        sides, cross = ops.cross_host(r32, pos, w, live=ex.live)
        assert sides.dtype == np.uint64 and sides.shape == (n, 2) and cross.dtype == np.uint64 and cross.shape == (n + 1,)
        assert cross[0] == 0 and cross[n] == 0 and pairs[0] == 0 and pairs[n] == 0
        assert int(sides[:, 0].astype(object).sum()) == int(sides[:, 1].astype(object).sum())
        assert np.array_equal(ops.cross_pairs(pos, w, ex.live), pairs), (key, w)
        err = np.abs(cross.astype(np.float64) / ops.SCORE_SCALE - exact)
        b = rx.bound(exact, pairs)
        assert (err <= b).all(), (key, w)
        worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
    print(f"{key}: worst |cross - exact| / bound = {worst:.3g}")


@pytest.mark.parametrize("key", [(129, 333), (2, 64), (1, 64)], ids=str)
def test_cross_host_equals_the_double_loop(key):
    from ld_tools_amd import ops
    _, ex = rx.panel(key)
    r32 = r32_square(ex)[:40, :40]
    n = r32.shape[0]
    for pos, w in rx.cases(key):
        pos = pos[:n]
        sides, cross = ops.cross_host(r32, pos, w)
        assert np.array_equal(cross, rx.cross_loops(r32, pos, w)), (key, w)
        # the halves against their definitions, and without `live` the same array (a degenerate cell's term is 0)
        t = ops.score_terms(r32).astype(object)
        near = np.tril(pos[:, None] - pos[None, :] <= w, -1)
        assert [int(v) for v in sides[:, 0]] == [int((t[i] * near[i]).sum()) for i in range(n)]
        assert [int(v) for v in sides[:, 1]] == [int((t[:, j] * near[:, j]).sum()) for j in range(n)]
        live = ex.live[:n]
        assert np.array_equal(ops.cross_host(r32, pos, w, live=live)[1], cross)


def test_split_host_against_every_admissible_cut_set():
    from ld_tools_amd import ops
    feasible = infeasible = tied = 0
    for cross, mn, mx in rx.split_cases():
        n = cross.size - 1
        want = rx.brute_split(cross >> np.uint64(16), mn, mx)
        assert (want is not None) == ops.split_feasible(n, mn, mx), (n, mn, mx)
        if want is None:
            infeasible += 1
            with pytest.raises(ops._lib.LdxError):
                ops.split_host(cross, mn, mx)
            continue
        feasible += 1
        cuts, total = ops.split_host(cross, mn, mx)
        assert total == want[0], (n, mn, mx)
        assert tuple(cuts.tolist()) == want[1], (n, mn, mx, cross >> np.uint64(16))
        assert rx.admissible(n, cuts.tolist(), mn, mx)
        tied += int(not (cross >> np.uint64(16)).any())
    assert feasible > 100 and infeasible > 20 and tied > 20
    for bad in ((0, 3), (4, 3)):
        with pytest.raises(ops._lib.LdxError):
            ops.split_host(np.zeros(9, dtype=np.uint64), *bad)


def test_split_host_tie_rule_and_sums_beyond_2_53():
    from ld_tools_amd import ops
    # all-zero costs, regions of 2 .. 3 over 7 SNPs: prev[7] is the largest feasible p in [4, 5], 5; prev[5] the largest in
    # [2, 3], 3; prev[3] the largest feasible one in [0, 1], 0
    cuts, total = ops.split_host(np.zeros(8, dtype=np.uint64), 2, 3)
    assert cuts.tolist() == [3, 5] and total == 0
    # sums above 2^53 are still compared exactly (the plain loop goes on in Python integers): with regions of 1 .. 2 SNPs
    # the optimum skips the dearer SNP of every pair, and the costs differ in their last bit only
    odd = ((1 << 47) + 1) << 16
    cross = np.full(600, odd, dtype=np.uint64)
    cross[2::2] -= np.uint64(1 << 16)
    cuts, total = ops.split_host(cross, 1, 2)
    assert cuts.tolist() == list(range(2, 599, 2)) and total == 299 * (1 << 47) > (1 << 53)


def test_region_positions():
    from ld_tools_amd import ops
    rng = np.random.default_rng(5)
    pos = np.sort(rng.integers(1, 5000, size=60)).astype(np.int64)
    reg = np.repeat(np.arange(5), [7, 20, 1, 30, 2])
    for w in (0, 1, 250, 10_000, None):
        shifted, win = ops.region_positions(pos, reg, w)
        spans = [pos[reg == k][-1] - pos[reg == k][0] for k in range(5)]
        assert win == (max(spans) if w is None else w)
        assert shifted.dtype == np.int64 and (np.diff(shifted) >= 0).all()
        same = reg[:, None] == reg[None, :]
        d, d0 = shifted[:, None] - shifted[None, :], pos[:, None] - pos[None, :]
        assert np.array_equal(d[same], d0[same])                       # within a region: unchanged
        assert (np.abs(d[~same]) > win).all()                          # across a boundary: out of every window
    for bad in (reg + 1, reg[::-1].copy(), np.where(np.arange(60) == 30, 0, reg)):
        with pytest.raises(ops._lib.LdxError):
            ops.region_positions(pos, bad, 100)
    with pytest.raises(ops._lib.LdxError):
        ops.region_positions(pos, reg[:-1], 100)
    with pytest.raises(ops._lib.LdxError, match="2\\^62"):
        ops.region_positions(pos, reg, 1 << 60)
    with pytest.raises(ops._lib.LdxError, match="2\\^62"):
        ops.region_positions(pos - pos[-1] + (1 << 62) - 4, reg, 0)    # the last SNP lands on 2^62
    edge, _ = ops.region_positions(pos - pos[-1] + (1 << 62) - 5, reg, 0)
    assert int(edge[-1]) == (1 << 62) - 1
    ok, _ = ops.region_positions(pos, reg, (1 << 59) - 5000)           # 4 (2^59 - 4999) + pos < 2^62
    assert int(ok[-1]) < (1 << 62)


def toy_regions():
    """Five regions over 12 SNPs, an LDCross over host arrays beside them."""
    import torch
    from ld_tools_amd import ops
    pos = np.array([10, 20, 20, 35, 50, 61, 70, 88, 90, 95, 120, 130], dtype=np.int64)
    cross = np.zeros(13, dtype=np.uint64)
    cross[[2, 5, 6, 10]] = np.array([1 << 31, 3 << 32, 0, (1 << 32) + (1 << 30)], dtype=np.uint64)
    cr = ops.LDCross(torch.zeros(1), torch.zeros(1), pos, 100, 64)
    cr._host = (np.zeros(12), np.zeros(12), cross.astype(np.float64) / ops.SCORE_SCALE)
    return ops.LDRegions(np.array([2, 5, 6, 10], dtype=np.int64), 12, pos, 100, 1, 5, cr)


def test_regions_bookkeeping():
    res = toy_regions()
    assert res.n_regions == 5 and res.starts.tolist() == [0, 2, 5, 6, 10] and res.ends.tolist() == [1, 4, 5, 9, 11]
    assert res.sizes.tolist() == [2, 3, 1, 4, 2] and res.region_of.tolist() == [0, 0, 1, 1, 1, 2, 3, 3, 3, 3, 4, 4]
    assert res.spans_bp.tolist() == [10, 30, 0, 25, 10]
    assert res.cross_at_cuts.tolist() == [0.5, 3.0, 0.0, 1.25] and res.total_cross == 4.75


def test_writer_golden(tmp_path):
    from ld_tools_amd.drivers import write_regions
    res = toy_regions()
    bed, det = write_regions(str(tmp_path / "a"), res, chrom="7")
    assert bed.endswith("a.bed") and det.endswith("a.regions.det")
    assert Path(bed).read_text() == ("chr\tstart\tstop\n" "chr7\t10\t20\n" "chr7\t20\t61\n" "chr7\t61\t70\n" "chr7\t70\t120\n"
                                     "chr7\t120\t131\n")
    assert Path(det).read_text() == ("CHR\tBP1\tBP2\tKB\tNSNPS\tCUT_R2\n" "7\t10\t20\t0.011\t2\t0.0000\n"
                                     "7\t20\t50\t0.031\t3\t0.5000\n" "7\t61\t61\t0.001\t1\t3.0000\n"
                                     "7\t70\t95\t0.026\t4\t0.0000\n" "7\t120\t130\t0.011\t2\t1.2500\n")
    b2, d2 = write_regions(str(tmp_path / "b"), res, chrom="7")
    assert Path(b2).read_bytes() == Path(bed).read_bytes() and Path(d2).read_bytes() == Path(det).read_bytes()


def test_header_and_exports():
    import ld_tools_amd
    from ld_tools_amd import _lib
    header = (ROOT / "include" / "ldx.h").read_text()
    for sym in ("ldx_ld_cross_dev", "ldx_ld_cross_workspace_bytes", "ldx_ld_cross_scan_dev", "ldx_ld_split_dev",
                "ldx_ld_split_workspace_bytes"):
        assert sym in header and sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
    assert "Berisa & Pickrell" in header and "additive" in header.lower() and "2^32" in header
    for name in ("ld_cross", "ld_regions", "LDCross", "LDRegions", "cross_host", "split_host", "region_positions"):
        assert name in ld_tools_amd.__all__ and hasattr(ld_tools_amd, name)
    assert _lib.lib.ldx_ld_split_workspace_bytes(1000) >= 20 * 1001
    assert _lib.lib.ldx_ld_cross_workspace_bytes(1000, 64) == _lib.lib.ldx_ld_score_workspace_bytes(1000, 64)


def test_case_list_is_the_one_the_gpu_tests_expect():
    assert rx.PANELS == ["lr1000", "lr700"] + [(n, h) for h in (64, 333) for n in (1, 2, 127, 128, 129, 300)]
    for key in rx.PANELS:
        assert len(rx.cases(key)) == 7
    _, ex = rx.panel("lr700")
    pos = 1 + 100 * np.arange(700, dtype=np.int64)
    exact, pairs = rx.exact_cross(ex, pos, 12900)
    assert pairs.max() > 129 * 60 and exact.max() > 50.0     # LD that reaches across 128-column tiles crosses the cuts

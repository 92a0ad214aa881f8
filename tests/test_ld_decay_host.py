"""CPU: the host side of LD decay -- ops.decay_host against the exact histograms of tests/ld_decay_exact.py, LDDecay's
rebin / adjusted / mean, the .stat.gz writer, and the properties of the case list that tests/test_gpu_ld_decay.py relies on."""
import gzip
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_decay_exact as dx  # noqa: E402
import ld_exact as lx  # noqa: E402


def fake_result(sums_u64, counts, width, window, n_hap=100):
    """An LDDecay over host arrays (what the lazy properties would have fetched)."""
    import torch
    from ld_tools_amd import ops
    s = np.asarray(sums_u64, dtype=np.uint64)
    res = ops.LDDecay(torch.zeros(s.size), torch.zeros(s.size), width, window, n_hap)
    res._counts = np.asarray(counts, dtype=np.int64)
    res._sum_r2 = s.astype(np.float64) / ops.SCORE_SCALE
    return res


@pytest.mark.parametrize("key", ["lr700", (129, 333), (300, 64), (2, 64), (1, 64)], ids=str)
def test_decay_host_against_exact_histograms(key):
    from ld_tools_amd import ops
    _, ex = dx.panel(key)
    r32 = ex.r64.astype(np.float32)
    keep = dx.keep_mask(ex.n_snps)
    worst = 0.0
    for pos, w, bw in dx.cases(key):
        for k in (None, keep):
            counts, exact = dx.exact_decay(ex, pos, w, bw, k)
            sums, cnt = ops.decay_host(r32, pos, w, bw, keep=k, live=ex.live)
            assert sums.dtype == np.uint64 and cnt.dtype == np.uint64 and sums.shape == (dx.n_bins(w, bw),)
            assert np.array_equal(cnt.astype(np.int64), counts), (key, w, bw)
            err = np.abs(sums.astype(np.float64) / ops.SCORE_SCALE - exact)
            b = dx.bound(exact, counts)
            assert (err <= b).all(), (key, w, bw)
            worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
    print(f"{key}: worst |sum - exact| / bound = {worst:.3g}")


def test_decay_host_bins_are_integer_floors():
    from ld_tools_amd import ops
    bw = 3_000_000_007
    pos = np.array([0, bw - 1, bw, 2 * bw - 1, 2 * bw, 2 * bw], dtype=np.int64)
    r = np.full((6, 6), 0.5, dtype=np.float32)
    sums, cnt = ops.decay_host(r, pos, 2 * bw, bw)
    d = (pos[:, None] - pos[None, :])[np.tril_indices(6, -1)]
    assert np.array_equal(cnt, np.bincount(d // bw, minlength=3).astype(np.uint64)) and int(cnt.sum()) == 15
    assert np.array_equal(sums, cnt * np.uint64(1 << 30))
    with pytest.raises(ops._lib.LdxError):
        ops.decay_host(r, pos, 10, 0)


def test_rebin_conserves_and_refuses_bad_edges():
    from ld_tools_amd import ops
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 50, size=26)
    sums = rng.integers(0, 1 << 40, size=26).astype(np.uint64)
    res = fake_result(sums, counts, 10, 250)
    assert res.n_bins == 26 and np.array_equal(res.distance, 10 * np.arange(26))
    s, c = res.rebin([0, 10, 50, 100, 260])
    assert c.tolist() == [counts[0], counts[1:5].sum(), counts[5:10].sum(), counts[10:].sum()]
    assert np.allclose(s, [res.sum_r2[0], res.sum_r2[1:5].sum(), res.sum_r2[5:10].sum(), res.sum_r2[10:].sum()], rtol=1e-14)
    assert c.sum() == counts.sum() and np.isclose(s.sum(), res.sum_r2.sum(), rtol=1e-14)
    s2, c2 = res.rebin([0, 1000])                       # an edge beyond the last bin stands for its end
    assert c2.tolist() == [counts.sum()]
    for bad in ([0, 15, 30], [0, 50, 50], [50, 10], [0], [0.0, 10.0], [-10, 10]):
        with pytest.raises(ops._lib.LdxError):
            res.rebin(bad)


def test_mean_and_adjusted():
    from ld_tools_amd import ops
    res = fake_result([1 << 31, 0, 3 << 32], [2, 0, 4], 5, 14, n_hap=102)
    assert np.array_equal(res.counts, [2, 0, 4]) and np.array_equal(res.sum_r2, [0.5, 0.0, 3.0])
    m = res.mean_r2
    assert m[0] == 0.25 and np.isnan(m[1]) and m[2] == 0.75
    a = res.adjusted()
    assert np.isclose(a[0], 101 / 100 * 0.25 - 1 / 100) and np.isnan(a[1]) and np.isclose(a[2], 101 / 100 * 0.75 - 1 / 100)
    assert np.isclose(res.adjusted(52)[0], 51 / 50 * 0.25 - 1 / 50)
    with pytest.raises(ops._lib.LdxError):
        res.adjusted(2)


def test_writer_is_byte_stable(tmp_path):
    from ld_tools_amd.drivers import write_decay
    res = fake_result([1 << 31, 0, 3 << 32], [2, 0, 4], 5, 12)
    p1 = write_decay(str(tmp_path / "a"), res)
    p2 = write_decay(str(tmp_path / "b"), res)
    assert p1.endswith("a.stat.gz") and Path(p1).read_bytes() == Path(p2).read_bytes()
    text = gzip.open(p1, "rt").read()
    assert text == "#Dist\tMean_r^2\tSum_r^2\tNumberPairs\n5\t0.250000\t0.5000\t2\n13\t0.750000\t3.0000\t4\n"
    p3 = write_decay(str(tmp_path / "c"), res, rebin=[0, 10, 15])
    assert gzip.open(p3, "rt").read() == "#Dist\tMean_r^2\tSum_r^2\tNumberPairs\n10\t0.250000\t0.5000\t2\n13\t0.750000\t3.0000\t4\n"


def test_too_many_bins_names_the_smallest_width():
    from ld_tools_amd import ops
    assert ops.decay_bins(250_000, 1000) == 251 and ops.decay_bins(250_000, 245) == 1021 and ops.decay_bins(0, 5) == 1
    assert ops.decay_bins(250_000, 250_000 // 1024 + 1) <= 1024 < ops.decay_bins(250_000, 250_000 // 1024)
    assert ops.decay_bins(1 << 60, 1 << 52) == 2


# ---- what tests/test_gpu_ld_decay.py relies on ---------------------------------------------------------------------------
def test_case_list_is_the_one_the_gpu_tests_expect():
    assert dx.PANELS == ["lr1000", "lr700"] + [(n, h) for h in (64, 333) for n in (1, 2, 127, 128, 129, 300)]
    assert dx.bin_widths(300) == [1, 7, 100, 300, 301] and dx.bin_widths(0) == [1, 7, 100]
    assert dx.bin_widths(12900) == [100, 12900, 12901] and dx.bin_widths(2) == [1, 7, 100, 2, 3]
    for key in dx.PANELS:
        cs = dx.cases(key)
        assert all(1 <= dx.n_bins(w, bw) <= dx.MAX_BINS for _, w, bw in cs)
        assert len({(w, id(pos)) for pos, w, _ in cs}) <= 7
        assert any(dx.n_bins(w, bw) == 2 for _, w, bw in cs) and any(dx.n_bins(w, bw) == 1 and w > 0 for _, w, bw in cs)


@pytest.mark.parametrize("key", [k for k in dx.PANELS if isinstance(k, str) or k[0] >= 127], ids=str)
def test_cases_sit_on_bin_edges_and_window_edges(key):
    """Per panel of 127 SNPs or more: for every width > 1 some case has pairs at d = k width (k >= 1) and some case pairs at
    d = k width - 1; the grid cases with the window as the width have pairs at d == window alone in the last bin (w = 300
    everywhere, 100 x 129 where the panel is longer than 129 SNPs); degenerate SNPs are present, so `live` matters.
    (Not EVERY case has a pair on an edge: the grid's distances are multiples of 100, so its width-7 cases with w = 300 have
    none, and neither has the window that ends between two grid points.)"""
    _, ex = dx.panel(key)
    n = ex.n_snps
    assert 0 < int((~ex.live).sum()) < n // 4
    on, below = set(), set()
    for pos, w, bw in dx.cases(key):
        _, _, d = dx.pairs(ex, pos, w)
        if bw > 1 and ((d % bw == 0) & (d > 0)).any():
            on.add(bw)
        if bw > 1 and (d % bw == bw - 1).any():
            below.add(bw)
        if pos[1] - pos[0] == 100 and pos[-1] == 1 + 100 * (n - 1) and bw == w and (w == 300 or (w == 12900 and n > 130)):
            counts, _ = dx.exact_decay(ex, pos, w, bw)
            assert counts.shape == (2,) and counts[1] == (d == w).sum() > 0 and counts[0] > 0
    assert {7, 100} <= on and {7, 100} <= below, (on, below)


@pytest.mark.parametrize("key", ["lr1000", "lr700"])
def test_long_range_cases_fill_bins_with_tile_crossing_ld(key):
    """More than one bin holds pairs of different 128-column tiles, and pairs with r^2 >= 0.2 among them."""
    _, ex = dx.panel(key)
    n = ex.n_snps
    pos = 1 + 100 * np.arange(n, dtype=np.int64)
    assert any(p is not None and np.array_equal(p, pos) and w == 12900 and bw == 100 for p, w, bw in dx.cases(key))
    rows, cols, d = dx.pairs(ex, pos, 12900)
    cross = rows // 128 != cols // 128
    strong = cross & (ex.r2_64[rows, cols] >= 0.2)
    assert np.unique(d[cross] // 100).size > 100 and np.unique(d[strong] // 100).size > 1

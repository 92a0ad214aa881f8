"""GPU: ld_decay (ldx_ld_decay_dev) -- per-distance-bin sums of r^2 and pair counts on the matrix-pipe band.

1. against the exact oracle (tests/ld_decay_exact.py: integers from the allele codes): counts equal, and
   |sum_r2[b] - exact[b]| <= 2^-19 exact[b] + counts[b] 2^-33 (derived there), every case, both paths;
2. integer equality with ops.decay_host over the r32 square, fp4 == mfma, launch 2 == launch 1, pre-filled outputs;
3. the two identities of include/ldx.h against ld_score on the same window;
4. keep masks; 5. argument errors; and bin edges at distances a float32 or a rounded reciprocal would misplace.
Tests 1, 3 and 4 reach the allele codes (through the oracle); test 2 compares with the r32 triangle.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_decay_exact as dx  # noqa: E402

pytestmark = pytest.mark.gpu

BANDS = ("fp4", "mfma")
EQUALITY_PANELS = ["lr1000", "lr700", (129, 333), (300, 64), (2, 64)]


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


def pack(codes, gpu):
    from ld_tools_amd import PackedPanel
    return PackedPanel.from_codes(np.array(codes), gpu)


def raw(res):
    return res.sums.cpu().numpy(), res.counts_dev.cpu().numpy()


# ---- 1. the exact oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", dx.PANELS, ids=str)
def test_decay_against_exact_counts_and_r2_sums(gpu, key):
    from ld_tools_amd import ops
    codes, ex = dx.panel(key)
    p = pack(codes, gpu)
    worst = 0.0
    for pos, w, bw in dx.cases(key):
        counts, exact = dx.exact_decay(ex, pos, w, bw)
        b = dx.bound(exact, counts)
        for path in BANDS:
            res = ops.ld_decay(p, pos, window_bp=w, bin_bp=bw, path=path)
            assert res.counts.shape == counts.shape and res.n_bins == dx.n_bins(w, bw)
            assert np.array_equal(res.counts, counts), (key, w, bw, path)
            err = np.abs(res.sum_r2 - exact)
            worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
            assert (err <= b).all(), (key, w, bw, path)
            assert np.array_equal(np.isnan(res.mean_r2), counts == 0)
    print(f"{key}: {len(dx.cases(key))} cases, worst |sum_r2 - exact| / bound = {worst:.3g}")


# ---- 2. integer equality -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", EQUALITY_PANELS, ids=str)
def test_decay_equals_the_host_histogram_of_the_r32_square(gpu, key):
    import torch
    from ld_tools_amd import _lib, ops
    codes, ex = dx.panel(key)
    n = ex.n_snps
    p = pack(codes, gpu)
    R = ops.ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()
    ws = torch.empty(_lib.lib.ldx_ld_decay_workspace_bytes(n, p.n_hap), dtype=torch.uint8, device=gpu)
    for pos, w, bw in dx.cases(key):
        want_s, want_c = ops.decay_host(R, pos, w, bw, live=ex.live)
        first = None
        for path in BANDS:
            for launch in range(2):
                s, c = raw(ops.ld_decay(p, pos, window_bp=w, bin_bp=bw, path=path, workspace=ws))
                assert np.array_equal(s, want_s) and np.array_equal(c, want_c), (key, w, bw, path, launch)
                first = (s, c) if first is None else first
                assert np.array_equal(s, first[0]) and np.array_equal(c, first[1])
        # outputs full of ones come back the same: the call writes them
        nb = want_s.size
        sums = torch.full((nb,), -1, dtype=torch.int64, device=gpu).view(torch.uint64)
        counts = torch.full((nb,), -1, dtype=torch.int64, device=gpu).view(torch.uint64)
        ops._decay_launch(p, torch.as_tensor(pos).to(gpu), w, bw, None, ops.PATHS["fp4"], sums, counts, ws)
        assert np.array_equal(sums.cpu().numpy(), want_s) and np.array_equal(counts.cpu().numpy(), want_c), (key, w, bw)


def test_decay_in_snp_units(gpu):
    from ld_tools_amd import ops
    codes, ex = dx.panel((300, 64))
    p = pack(codes, gpu)
    R = ops.ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()
    for w, bw in ((299, 1), (130, 7), (5, 2)):
        want_s, want_c = ops.decay_host(R, np.arange(300), w, bw, live=ex.live)
        s, c = raw(ops.ld_decay(p, window_snps=w, bin_bp=bw))
        assert np.array_equal(s, want_s) and np.array_equal(c, want_c)


# ---- bin edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bw", [3, 1000, 3_000_000_007, (1 << 42) + 1])
def test_bins_are_exact_at_k_width_and_k_width_minus_1(gpu, bw):
    """Positions in clusters {k bw - 1, k bw, k bw + 1} around every multiple of the width (k up to 43, distances up to 2^47 for
    the largest width: beyond float32, and products q bw that a double rounds): every d = k bw lands in bin k and every
    d = k bw - 1 in bin k - 1."""
    from ld_tools_amd import ops
    codes, ex = dx.panel((129, 333))
    p = pack(codes, gpu)
    k = np.arange(129, dtype=np.int64) // 3
    pos = 7 + k * bw + (np.arange(129) % 3 - 1)
    pos[0] = 7                        # (7 - 1 would still be fine; keep the first cluster {7, 7, 8}: a duplicate)
    assert (np.diff(pos) >= 0).all()
    R = ops.ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()
    for w in (42 * bw, 42 * bw - 1, 5 * bw, bw, bw - 1):
        counts, exact = dx.exact_decay(ex, pos, w, bw)
        want_s, want_c = ops.decay_host(R, pos, w, bw, live=ex.live)
        assert np.array_equal(want_c.astype(np.int64), counts)
        rows, cols, d = dx.pairs(ex, pos, w)
        assert (d % bw == bw - 1).any() and (w < bw or ((d % bw == 0) & (d > 0)).any())
        for path in BANDS:
            s, c = raw(ops.ld_decay(p, pos, window_bp=w, bin_bp=bw, path=path))
            assert np.array_equal(c, want_c) and np.array_equal(s, want_s), (bw, w, path)


def test_windows_and_widths_beyond_2_52(gpu):
    from ld_tools_amd import ops
    codes, ex = dx.panel((129, 333))
    p = pack(codes, gpu)
    pos = np.cumsum(np.full(129, 1 << 40, dtype=np.int64))
    counts, _ = dx.exact_decay(ex, pos, 1 << 52, 1 << 52)
    res = ops.ld_decay(p, pos, window_bp=1 << 60, bin_bp=1 << 52)         # the window acts as 2^52: two bins
    assert res.n_bins == 2 and np.array_equal(res.counts, counts)
    one = ops.ld_decay(p, pos, window_bp=1 << 60, bin_bp=(1 << 62) + 12345)  # one bin
    assert one.n_bins == 1 and one.counts[0] == counts.sum()


# ---- 3. the identities against ld_score ----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["lr1000", (129, 64), (300, 333)], ids=str)
def test_identities_with_ld_score(gpu, key):
    from ld_tools_amd import ops
    import ld_exact as lx
    codes, ex = dx.panel(key)
    n = ex.n_snps
    p = pack(codes, gpu)
    diag = ops.ld_triangle(p, fmt="r32").r_matrix().cpu().numpy().diagonal()
    self_terms = int(ops.score_terms(diag).astype(object).sum())
    for pos, w, bw in dx.cases(key):
        s, c = raw(ops.ld_decay(p, pos, window_bp=w, bin_bp=bw))
        win = lx.window_mask(pos, w) & ex.live[:, None] & ex.live[None, :]
        assert int(c.astype(object).sum()) == (int(win.sum()) - int(ex.live.sum())) // 2
        score = ops.ld_score(p, pos, window_bp=w).sums.cpu().numpy()[:, 0]
        assert 2 * int(s.astype(object).sum()) + self_terms == int(score.astype(object).sum()), (key, w, bw)


# ---- 4. keep masks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["lr700", (129, 333), (300, 64)], ids=str)
def test_keep_masks(gpu, key):
    from ld_tools_amd import ops
    codes, ex = dx.panel(key)
    n = ex.n_snps
    p = pack(codes, gpu)
    keep = dx.keep_mask(n)
    assert (~ex.live & keep).any() and 0.6 < keep.mean() < 0.8       # degenerate rows among the kept
    for pos, w, bw in dx.cases(key):
        counts, exact = dx.exact_decay(ex, pos, w, bw, keep)
        for path in BANDS:
            res = ops.ld_decay(p, pos, window_bp=w, bin_bp=bw, keep=keep, path=path)
            assert np.array_equal(res.counts, counts), (key, w, bw, path)
            assert (np.abs(res.sum_r2 - exact) <= dx.bound(exact, counts)).all(), (key, w, bw, path)
        none = ops.ld_decay(p, pos, window_bp=w, bin_bp=bw, keep=np.zeros(n, dtype=bool))
        s, c = raw(none)
        assert not s.any() and not c.any() and s.shape == counts.shape


# ---- 5. errors -----------------------------------------------------------------------------------------------------------
def test_errors_and_the_single_snp_panel(gpu):
    import torch
    from ld_tools_amd import _lib, ops
    codes, ex = dx.panel((129, 64))
    p = pack(codes, gpu)
    pos = 1 + 100 * np.arange(129, dtype=np.int64)
    with pytest.raises(_lib.LdxError):
        ops.ld_decay(p, pos, window_bp=1000, bin_bp=0)
    with pytest.raises(_lib.LdxError, match="smallest admissible bin_bp for this window is 2"):
        ops.ld_decay(p, pos, window_bp=1024, bin_bp=1)               # 1025 bins
    assert ops.ld_decay(p, pos, window_bp=1023, bin_bp=1).n_bins == 1024
    assert ops.ld_decay(p, pos, window_bp=1024, bin_bp=2).n_bins == 513
    with pytest.raises(_lib.LdxError, match="UNSUPPORTED"):
        ops.ld_decay(p, pos, window_bp=1000, bin_bp=100, path="popcount")
    with pytest.raises(_lib.LdxError):
        ops.ld_decay(p, pos, window_bp=1000, bin_bp=100, keep=np.ones(5, dtype=bool))
    # the C entry point refuses a bin count that does not match the window, and a width of 0
    ws = torch.empty(_lib.lib.ldx_ld_decay_workspace_bytes(129, 64), dtype=torch.uint8, device=gpu)
    out = torch.zeros(16, dtype=torch.int64, device=gpu)
    posd = torch.as_tensor(pos).to(gpu)
    for w, bw, nb in ((1000, 100, 10), (1000, 0, 11), (1 << 20, 1, 1025)):
        rc = _lib.lib.ldx_ld_decay_dev(p.alt.data_ptr(), p.acnt.data_ptr(), p.rcnt.data_ptr(), p.fa.data_ptr(), p.fr.data_ptr(),
                                       129, 64, posd.data_ptr(), w, bw, None, 0, out.data_ptr(), out.data_ptr(), nb,
                                       ws.data_ptr(), ws.numel(), None)
        assert rc == -1, (w, bw, nb)
    # one SNP: no pair, zeros
    c1, _ = dx.panel((1, 64))
    one = ops.ld_decay(pack(c1, gpu), np.array([5], dtype=np.int64), window_bp=300, bin_bp=100)
    s, c = raw(one)
    assert s.shape == (4,) and not s.any() and not c.any() and np.isnan(one.mean_r2).all()

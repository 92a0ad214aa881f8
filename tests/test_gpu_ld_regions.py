"""GPU: LD-independent regions -- ld_cross (ldx_ld_cross_dev: the band with one-sided sums, and the scan), ldx_ld_split_dev
(the optimal cuts), ld_regions and the ``regions=`` keyword of ld_score / ld_matvec / ld_ridge.

1. against the exact oracle (tests/ld_regions_exact.py: integers from the allele codes): pairs equal, and
   |cross_r2[k] - exact[k]| <= 2^-19 exact[k] + pairs[k] 2^-33 at every cut, every case, both paths;
2. integer equality with ops.cross_host over the r32 square, fp4 == mfma, launch 2 == launch 1, pre-filled outputs;
3. the identities of include/ldx.h against ld_score and ld_decay on the same window;
4. the split kernel alone against ops.split_host, uploaded profiles; 5. ld_regions end to end; 6. ``regions=``;
7. argument errors.
Tests 1 and 3 reach the allele codes (through the oracle and the other kernels); test 2 compares with the r32 triangle.
"""
import sys
import time
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_regions_exact as rx  # noqa: E402

pytestmark = pytest.mark.gpu

BANDS = ("fp4", "mfma")
EQUALITY_PANELS = ["lr1000", "lr700", (129, 333), (300, 64), (128, 64), (127, 333), (2, 64), (1, 64)]


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
    return res.sides.cpu().numpy(), res.cross.cpu().numpy()


def r32_square(p):
    from ld_tools_amd import ops
    return ops.ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()


# ---- 1. the exact oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", rx.PANELS, ids=str)
def test_cross_against_exact_counts_and_r2_sums(gpu, key):
    from ld_tools_amd import ops
    codes, ex = rx.panel(key)
    n = ex.n_snps
    p = pack(codes, gpu)
    worst = 0.0
    for pos, w in rx.cases(key):
        exact, pairs = rx.exact_cross(ex, pos, w)
        b = rx.bound(exact, pairs)
        for path in BANDS:
            res = ops.ld_cross(p, pos, window_bp=w, path=path)
            assert res.cross_r2.shape == (n + 1,) and res.left.shape == (n,) and res.right.shape == (n,)
            assert np.array_equal(res.pairs, pairs), (key, w, path)
            err = np.abs(res.cross_r2 - exact)
            worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
            assert (err <= b).all(), (key, w, path)
            assert np.array_equal(np.isnan(res.mean_r2), pairs == 0)
            assert res.cross_r2[0] == 0 and res.cross_r2[n] == 0
    print(f"{key}: {len(rx.cases(key))} cases, worst |cross_r2 - exact| / bound = {worst:.3g}")


# ---- 2. integer equality -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", EQUALITY_PANELS, ids=str)
def test_cross_equals_the_host_sums_of_the_r32_square(gpu, key):
    import torch
    from ld_tools_amd import _lib, ops
    codes, ex = rx.panel(key)
    n = ex.n_snps
    p = pack(codes, gpu)
    R = r32_square(p)
    ws = torch.empty(_lib.lib.ldx_ld_cross_workspace_bytes(n, p.n_hap), dtype=torch.uint8, device=gpu)
    for pos, w in rx.cases(key):
        want_s, want_c = ops.cross_host(R, pos, w, live=ex.live)
        for path in BANDS:
            for launch in range(2):
                s, c = raw(ops.ld_cross(p, pos, window_bp=w, path=path, workspace=ws))
                assert np.array_equal(s, want_s), (key, w, path, launch)
                assert np.array_equal(c, want_c), (key, w, path, launch)
        # outputs full of ones come back the same: the call writes them
        sides = torch.full((n, 2), -1, dtype=torch.int64, device=gpu).view(torch.uint64)
        cross = torch.full((n + 1,), -1, dtype=torch.int64, device=gpu).view(torch.uint64)
        ops._cross_launch(p, torch.as_tensor(pos).to(gpu), w, ops.PATHS["fp4"], sides, cross, ws)
        assert np.array_equal(sides.cpu().numpy(), want_s) and np.array_equal(cross.cpu().numpy(), want_c), (key, w)


def test_cross_in_snp_units_and_the_scan_alone(gpu):
    import torch
    from ld_tools_amd import _lib, ops
    codes, ex = rx.panel((300, 64))
    p = pack(codes, gpu)
    R = r32_square(p)
    for w in (299, 130, 5, 0):
        want_s, want_c = ops.cross_host(R, np.arange(300), w)
        s, c = raw(ops.ld_cross(p, window_snps=w))
        assert np.array_equal(s, want_s) and np.array_equal(c, want_c)
    # the scan over uploaded one-sided sums: more than one tile of 4096 SNPs, a ragged tail, values that wrap on the way
    rng = np.random.default_rng(3)
    for n in (1, 4095, 4096, 4097, 3 * 4096 + 77):
        sides = rng.integers(0, 1 << 63, size=(n, 2), dtype=np.int64).astype(np.uint64)
        want = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(sides[:, 1] - sides[:, 0], dtype=np.uint64)])
        out = torch.full((n + 1,), -1, dtype=torch.int64, device=gpu)
        _lib.check(_lib.lib.ldx_ld_cross_scan_dev(torch.as_tensor(sides.view(np.int64)).to(gpu).data_ptr(), n, out.data_ptr(),
                                                  None))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want), n


# ---- 3. the identities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["lr1000", (129, 64), (300, 333)], ids=str)
def test_identities_with_ld_score_and_ld_decay(gpu, key):
    from ld_tools_amd import ops
    codes, ex = rx.panel(key)
    p = pack(codes, gpu)
    self_terms = ops.score_terms(r32_square(p).diagonal())
    for pos, w in rx.cases(key):
        s, _ = raw(ops.ld_cross(p, pos, window_bp=w))
        score = ops.ld_score(p, pos, window_bp=w).sums.cpu().numpy()[:, 0]
        assert np.array_equal(s[:, 0] + s[:, 1] + self_terms, score), (key, w)
        decay = ops.ld_decay(p, pos, window_bp=w, bin_bp=max(1, w)).sums.cpu().numpy()
        assert int(s[:, 0].astype(object).sum()) == int(decay.astype(object).sum()) == int(s[:, 1].astype(object).sum())


# ---- 4. the split kernel alone ---------------------------------------------------------------------------------------------
def run_split(gpu, cross, mn, mx):
    """(cuts int64, n_out [count, flag]) of ldx_ld_split_dev over an uploaded profile; the outputs start full of ones."""
    import torch
    from ld_tools_amd import _lib, ops
    n = cross.size - 1
    cd = torch.as_tensor(np.ascontiguousarray(cross).view(np.int64)).to(gpu)
    cuts = torch.full((max(1, n // mn),), -1, dtype=torch.int32, device=gpu)
    n_out = torch.full((2,), -1, dtype=torch.int32, device=gpu)
    ws = torch.full((_lib.lib.ldx_ld_split_workspace_bytes(n),), 0xA5, dtype=torch.uint8, device=gpu)
    ops._split_launch(cd, n, mn, mx, cuts, n_out, ws)
    count, flag = (int(v) for v in n_out.cpu().numpy().view(np.uint32))
    return cuts[:count].cpu().numpy().view(np.uint32).astype(np.int64), count, flag


def profiles(n, seed):
    """Random uint64 profiles (costs up to 2^48), few-valued ones (ties) and zeros."""
    rng = np.random.default_rng(seed)
    return {"random": rng.integers(0, 1 << 63, size=n + 1, dtype=np.int64).astype(np.uint64) << np.uint64(1),
            "ties": rng.integers(0, 3, size=n + 1).astype(np.uint64) << np.uint64(16),
            "zero": np.zeros(n + 1, dtype=np.uint64)}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 5000])
def test_split_kernel_equals_split_host(gpu, n):
    from ld_tools_amd import ops
    ran = flagged = 0
    for mn, mx in ((1, 1), (1, n), (3, 7), (64, 64), (64, 200), (100, 5000)):
        feasible = ops.split_feasible(n, mn, mx)
        for kind, cross in profiles(n, 100 * n + mn).items():
            cuts, count, flag = run_split(gpu, cross, mn, mx)
            if not feasible:   # an infeasible end: the flag, no cuts
                assert (count, flag) == (0, 1), (n, mn, mx, kind)
                flagged += 1
                continue
            want, total = ops.split_host(cross, mn, mx)
            assert flag == 0 and count == want.size and np.array_equal(cuts, want), (n, mn, mx, kind)
            ran += 1
    assert ran >= 3 * 2 and flagged > 0


def test_split_kernel_infeasible_states_ties_and_saturation(gpu):
    from ld_tools_amd import ops
    # interior states infeasible, the end feasible: regions of 64 .. 66 over 130 SNPs (states 67 .. 127 have no predecessor)
    for kind, cross in profiles(130, 7).items():
        want, _ = ops.split_host(cross, 64, 66)
        cuts, count, flag = run_split(gpu, cross, 64, 66)
        assert flag == 0 and want.size == 1 and np.array_equal(cuts, want), kind
    # an infeasible end
    assert run_split(gpu, profiles(129, 1)["random"], 64, 64)[1:] == (0, 1)
    assert run_split(gpu, profiles(5, 1)["zero"], 6, 9)[1:] == (0, 1)
    # max_snps far above n acts as n
    cross = profiles(777, 2)["random"]
    assert np.array_equal(run_split(gpu, cross, 5, 0xFFFFFFFF)[0], ops.split_host(cross, 5, 777)[0])
    # all-zero costs, regions of 2 .. 3: the tie rule takes the latest cut at every step
    cuts, count, flag = run_split(gpu, np.zeros(8, dtype=np.uint64), 2, 3)
    assert cuts.tolist() == [3, 5] and flag == 0
    # every cost 2^48 - 1: with regions of exactly 1 SNP 65 536 cuts stay below 2^64 - 2, 65 537 do not
    top = np.uint64((1 << 64) - 1)
    for n, want_flag in ((65_537, 0), (65_540, 2)):
        cuts, count, flag = run_split(gpu, np.full(n + 1, top, dtype=np.uint64), 1, 1)
        assert flag == want_flag and count == (n - 1 if want_flag == 0 else 0), (n, count, flag)
    with pytest.raises(ops._lib.LdxError):
        ops.split_host(np.full(65_541, top, dtype=np.uint64), 1, 1)


def test_split_kernel_range_minimum_is_amortised(gpu):
    """200 000 states with windows of 4501: a kernel that scanned the window per state would read 9 10^8 words in one
    workgroup; with the block arg-minima every state costs two reads."""
    from ld_tools_amd import ops
    n = 200_000
    cross = profiles(n, 5)["random"]
    t0 = time.perf_counter()
    cuts, count, flag = run_split(gpu, cross, 500, 5000)
    t1 = time.perf_counter()
    want, _ = ops.split_host(cross, 500, 5000)
    print(f"split kernel at n = {n}: {t1 - t0:.3f} s with upload and readback; host mirror {time.perf_counter() - t1:.3f} s")
    assert flag == 0 and np.array_equal(cuts, want)
    sizes = np.diff(np.concatenate([[0], cuts, [n]]))
    assert sizes.min() >= 500 and sizes.max() <= 5000


# ---- 5. end to end -----------------------------------------------------------------------------------------------------
def test_ld_regions_end_to_end(gpu):
    from ld_tools_amd import ops
    codes, ex = rx.panel("lr1000")
    n = ex.n_snps
    p = pack(codes, gpu)
    pos = 1 + 100 * np.arange(n, dtype=np.int64)
    for mn, mx, w in ((20, 150, 12_900), (64, 64 + 40, 300), (1, 1000, 100_000), (100, 101, 2_000)):
        for path in BANDS:
            res = ops.ld_regions(p, pos, window_bp=w, min_snps=mn, max_snps=mx, path=path)
            want, total = ops.split_host(res.cross.cross.cpu().numpy(), mn, mx)
            assert np.array_equal(res.cuts, want), (mn, mx, w, path)
            assert res.n_regions == want.size + 1 and res.starts[0] == 0 and res.ends[-1] == n - 1
            assert np.array_equal(res.starts[1:], res.cuts) and np.array_equal(res.ends[:-1] + 1, res.cuts)
            assert np.array_equal(res.sizes, res.ends - res.starts + 1) and res.sizes.sum() == n
            assert res.sizes.min() >= mn and res.sizes.max() <= mx
            assert np.array_equal(res.region_of, np.searchsorted(res.cuts, np.arange(n), side="right"))
            assert np.array_equal(res.spans_bp, 100 * (res.sizes - 1))
            assert np.array_equal(res.cross_at_cuts, res.cross.cross_r2[res.cuts])
            assert np.isclose(res.total_cross, res.cross_at_cuts.sum()) and int(res.total_cross * 65536) >= total - want.size
    # the cuts avoid the strong LD: the mean cross-LD at the chosen cuts lies below the profile's mean
    res = ops.ld_regions(p, pos, window_bp=12_900, min_snps=20, max_snps=150)
    assert res.cross_at_cuts.mean() < res.cross.cross_r2[20:-20].mean()
    # inadmissible sizes are refused before any launch (a panel that is not on the device would fail later)
    class NoLaunch:
        n_snps, n_hap = 1000, 64
        def __getattr__(self, name):
            raise AssertionError(f"ld_regions touched panel.{name} before refusing its arguments")
    with pytest.raises(ops._lib.LdxError, match="nearest admissible max_snps is 334"):
        ops.ld_regions(NoLaunch(), pos, min_snps=300, max_snps=320)           # 3 x 320 < 1000 < 4 x 300
    with pytest.raises(ops._lib.LdxError, match="nearest admissible max_snps is 500"):
        ops.ld_regions(NoLaunch(), pos, min_snps=400, max_snps=450)
    with pytest.raises(ops._lib.LdxError, match="no max_snps is admissible"):
        ops.ld_regions(NoLaunch(), pos, min_snps=1001, max_snps=2000)
    assert ops.split_feasible(1000, 300, 334) and not ops.split_feasible(1000, 300, 333)


# ---- 6. regions= -------------------------------------------------------------------------------------------------------
def test_regions_keyword_of_score_and_matvec(gpu):
    from ld_tools_amd import ops
    codes, ex = rx.panel("lr700")
    n = ex.n_snps
    p = pack(codes, gpu)
    R = r32_square(p)
    pos = np.cumsum(np.random.default_rng(1).integers(0, 40, size=n)).astype(np.int64) + 7
    regs = ops.ld_regions(p, pos, window_bp=2_000, min_snps=30, max_snps=260)
    assert regs.n_regions >= 3
    region_of = regs.region_of
    same = region_of[:, None] == region_of[None, :]
    x32 = np.random.default_rng(2).uniform(-1, 1, size=(n, 3)).astype(np.float32)
    x32[np.abs(x32).argmax(axis=0), np.arange(3)] = 1.0                       # max |x| = 1: the columns keep their scale
    for w in (150, 2_000, None):
        near = same if w is None else same & (np.abs(pos[:, None] - pos[None, :]) <= w)
        for R_arg in (regs, region_of):
            sc = ops.ld_score(p, pos, window_bp=w, regions=R_arg)
            want = (ops.score_terms(R) * near).sum(axis=1, dtype=np.uint64)
            assert np.array_equal(sc.sums.cpu().numpy()[:, 0], want), w
            assert np.array_equal(sc.m[:, 0], (near & ex.live[None, :]).sum(axis=1)), w
            mv = ops.ld_matvec(p, x32, pos, window_bp=w, regions=R_arg)
            V = np.where(near, R, np.float32(0))
            want = np.stack([ops.prod_terms(V, x32[None, :, k]).sum(axis=1, dtype=np.int64) for k in range(3)], axis=1)
            assert np.array_equal(mv.sums.cpu().numpy(), want), w
    # without regions nothing changes, and whole-region windows need regions
    assert np.array_equal(ops.ld_score(p, pos, window_bp=150, regions=None).sums.cpu().numpy(),
                          ops.ld_score(p, pos, window_bp=150).sums.cpu().numpy())
    for call in (lambda: ops.ld_score(p, pos, window_bp=None), lambda: ops.ld_matvec(p, x32, pos, window_bp=None),
                 lambda: ops.ld_ridge(p, x32, pos, window_bp=None)):
        with pytest.raises(ops._lib.LdxError, match="needs regions"):
            call()
    with pytest.raises(ops._lib.LdxError):
        ops.ld_score(p, pos, window_bp=150, regions=region_of[::-1].copy())


def test_ridge_over_regions_is_never_indefinite(gpu):
    """The existing ridge criteria (tests/test_gpu_ld_matvec.py): recurrence residual <= tol, true residual against the dense
    block-diagonal matrix <= 2 tol, tol = 1e-6 -- the products' term rounding is at most (region size) 2^-41 max |p| each,
    about 1e-10 here.  No missing codes, whole regions, lam = 0.1: no column is indefinite."""
    from ld_tools_amd import PackedPanel, ops, synth
    n, h, tol, lam = 1200, 1008, 1e-6, 0.1
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=77), gpu)
    assert not (np.asarray(synth.synth_codes_host(n, h, seed=77)) > 1).any()
    pos = 1 + 100 * np.arange(n, dtype=np.int64)
    regs = ops.ld_regions(p, pos, window_bp=20_000, min_snps=100, max_snps=400)
    R = r32_square(p).astype(np.float64)
    same = regs.region_of[:, None] == regs.region_of[None, :]
    A = R * same + lam * np.eye(n)
    z = np.random.default_rng(9).standard_normal((n, 4)) * np.array([1.0, 10.0, 0.01, 3.0])
    res = ops.ld_ridge(p, z, pos, window_bp=None, lam=lam, tol=tol, regions=regs)
    beta = res.beta.cpu().numpy()
    true = np.linalg.norm(A @ beta - z, axis=0) / np.linalg.norm(z, axis=0)
    print("regions", regs.n_regions, "iterations", res.iterations, "recurrence", res.residual, "true", true)
    assert not res.indefinite.any() and res.converged.all()
    assert (res.residual <= tol).all()
    assert (true <= 2 * tol).all(), true


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    import torch
    from ld_tools_amd import _lib, ops
    codes, ex = rx.panel((129, 64))
    p = pack(codes, gpu)
    pos = 1 + 100 * np.arange(129, dtype=np.int64)
    with pytest.raises(_lib.LdxError, match="UNSUPPORTED"):
        ops.ld_cross(p, pos, window_bp=1000, path="popcount")
    with pytest.raises(_lib.LdxError, match="non-decreasing"):
        ops.ld_cross(p, pos[::-1].copy(), window_bp=1000)
    with pytest.raises(_lib.LdxError, match="non-decreasing"):
        ops.ld_regions(p, pos[::-1].copy(), window_bp=1000, min_snps=10, max_snps=50)
    small = torch.empty(256, dtype=torch.uint8, device=gpu)
    with pytest.raises(_lib.LdxError, match="workspace too small"):
        ops.ld_cross(p, pos, window_bp=1000, workspace=small)
    for mn, mx in ((0, 5), (6, 5)):
        with pytest.raises(_lib.LdxError, match="min_snps"):
            ops.ld_regions(p, pos, window_bp=1000, min_snps=mn, max_snps=mx)
    # the C entry points: popcount and too many haplotypes are unsupported, a small workspace and bad sizes are argument errors
    ws = torch.empty(_lib.lib.ldx_ld_cross_workspace_bytes(129, 64), dtype=torch.uint8, device=gpu)
    out = torch.zeros(2 * 129 + 130, dtype=torch.int64, device=gpu)
    posd = torch.as_tensor(pos).to(gpu)

    def cross_rc(n_hap=64, path=0, ws_bytes=ws.numel()):
        return _lib.lib.ldx_ld_cross_dev(p.alt.data_ptr(), p.acnt.data_ptr(), p.rcnt.data_ptr(), p.fa.data_ptr(), p.fr.data_ptr(),
                                         129, n_hap, posd.data_ptr(), 1000, path, out.data_ptr(), out[258:].data_ptr(),
                                         ws.data_ptr(), ws_bytes, None)
    assert cross_rc(path=ops.PATHS["popcount"]) == -3
    assert cross_rc(n_hap=_lib.MAX_HAPS + 1) == -3
    assert cross_rc(ws_bytes=ws.numel() - 1) == -1
    assert cross_rc(path=9) == -1
    sws = torch.empty(_lib.lib.ldx_ld_split_workspace_bytes(129), dtype=torch.uint8, device=gpu)
    for mn, mx, nbytes, rc in ((0, 5, sws.numel(), -1), (6, 5, sws.numel(), -1), (1, 5, sws.numel() - 1, -1), (1, 5, sws.numel(), 0)):
        got = _lib.lib.ldx_ld_split_dev(out.data_ptr(), 129, mn, mx, out[140:].data_ptr(), out[300:].data_ptr(), sws.data_ptr(),
                                        nbytes, None)
        assert got == rc, (mn, mx, nbytes)
    torch.cuda.synchronize()
    # one SNP: no pair, no cut
    c1, _ = rx.panel((1, 64))
    one = ops.ld_regions(pack(c1, gpu), np.array([5], dtype=np.int64), window_bp=300, min_snps=1, max_snps=1)
    assert one.n_regions == 1 and one.cuts.size == 0 and one.region_of.tolist() == [0] and one.total_cross == 0.0

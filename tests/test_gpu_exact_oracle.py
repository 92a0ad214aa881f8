"""GPU: the signed-r family against the exact oracle of tests/ld_exact.py -- r32 cells of the three triangle kernels, the
block export, LD scores, neighbour lists, clumping, pruning, ld_matvec and ld_ridge, each against integers computed from
the allele codes on the host (not against another kernel or a host mirror of the product).

Every tolerance follows from include/ldx.h:
  cells        within 4 float32 ulps of num / sqrt(den2); +0.0f iff num == 0; -0.0f iff a SNP is degenerate
  s = r *f32 r within (1 + 4 2^-23)^2 (1 + 2^-24) - 1 < 2^-19 of exact r^2 (tests/ld_exact.py derives the threshold margin)
  LD scores    each term rint(2^32 s): |l2 - sum r^2| <= 2^-19 sum r^2 + P 2^-33, P the in-window pair count
  R x          4 ulps per cell = 2^-21 relative, each term rounded once at 2^-41 of the column's scale
The panels have LD across 128-column tile boundaries (tests/test_ld_exact_host.py pins that, and the ambiguity counts).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_exact as lx  # noqa: E402

pytestmark = pytest.mark.gpu

KERNELS = ("popcount", "mfma", "fp4")
BANDS = ("fp4", "mfma")
NEG_ZERO = np.uint32(0x80000000)


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


def check_cells(got, ex, rows, cols, what):
    """float32 cells of the pairs (rows, cols) against the oracle: zeros by sign, the rest within 4 ulps with num's sign."""
    bits = np.ascontiguousarray(got).view(np.uint32)
    deg = ex.degenerate[rows, cols]
    zero = ex.zero_num[rows, cols]
    assert np.array_equal(bits == NEG_ZERO, deg), what          # -0.0f iff degenerate
    assert np.array_equal(bits == 0, zero), what                # +0.0f iff num == 0
    rest = ~deg & ~zero
    g, e = got[rest], ex.r64[rows, cols][rest]
    err = lx.ulp32_err(g, e)
    worst = float(err.max(initial=0.0))
    assert worst <= 4.0, (what, worst)
    assert np.array_equal(g > 0, ex.num[rows, cols][rest] > 0), what
    return worst


def triangle_cells(p, path, rows, cols):
    from ld_tools_amd import ops
    res = ops.ld_triangle(p, fmt="r32", path=path)
    return res.r32.cpu().numpy()[res.cell_index(rows, cols)] if rows.size else np.zeros(0, dtype=np.float32)


# ---- r32 cells ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hap", lx.EDGE_HAPS)
def test_r32_cells_of_every_kernel_against_exact_counts(gpu, n_hap):
    from ld_tools_amd import ops
    for n in lx.EDGE_SNPS:
        codes = lx.edge_panel(n, n_hap)
        ex = lx.Exact(codes)
        p = pack(codes, gpu)
        rows, cols = np.tril_indices(n, -1)
        worst = 0.0
        for path in KERNELS:
            worst = max(worst, check_cells(triangle_cells(p, path, rows, cols), ex, rows, cols, (n, n_hap, path)))
        print(f"n_hap {n_hap} n {n}: {rows.size} pairs, {int(ex.degenerate[rows, cols].sum())} degenerate, "
              f"{int(ex.zero_num[rows, cols].sum())} with num == 0, worst {worst:.3f} ulp")
        if n_hap == 1:
            assert not ex.live.any()
        d = ops.ld_triangle(p, fmt="r32").r_matrix().cpu().numpy().diagonal()
        check_diagonal(d, ex)


def check_diagonal(d, ex):
    want = ex.diagonal().astype(np.float32)
    want[~ex.live] = -0.0
    assert np.array_equal(np.ascontiguousarray(d).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", list(lx.LONG_RANGE))
def test_long_range_panels_cells_copies_and_square(gpu, name):
    """All three kernels on the panels with LD across tiles (lr2500 is 2500 x 10240 = LDX_MAX_HAPS); exact duplicates and
    complements of complete rows give exactly +-1.0f; the block export is symmetric, within 4 ulps everywhere, and its
    diagonal is float32((n - a) / r) bit for bit."""
    from ld_tools_amd import ops
    codes, plants, ex = lx.long_range_panel(name)
    n = ex.n_snps
    p = pack(codes, gpu)
    rows, cols = np.tril_indices(n, -1)
    src = np.array([s for s, _, _ in plants])
    dst = np.array([d for _, d, _ in plants])
    sign = np.array([sg for _, _, sg in plants], dtype=np.float32)
    for path in KERNELS:
        worst = check_cells(triangle_cells(p, path, rows, cols), ex, rows, cols, (name, path))
        print(f"{name} {path}: {rows.size} pairs, worst {worst:.3f} ulp")
        got = triangle_cells(p, path, dst, src)
        assert np.array_equal(got.view(np.uint32), sign.view(np.uint32)), (name, path, got)   # exactly +1.0f / -1.0f
    R = ops.ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()
    assert R.shape == (n, n) and R.dtype == np.float32
    assert np.array_equal(R.view(np.uint32), R.T.view(np.uint32))
    rr, cc = np.nonzero(~np.eye(n, dtype=bool))
    check_cells(R[rr, cc], ex, rr, cc, (name, "r_matrix"))
    check_diagonal(R.diagonal(), ex)
    # r^2 >= 1 keeps the copies (s = 1.0f exactly), r^2 > 1 drops them
    for path in BANDS:
        keep = ops.ld_neighbors(p, window_snps=n, r2=1.0, path=path)
        drop = ops.ld_neighbors(p, window_snps=n, r2=1.0, strict=True, path=path)
        hk, hd = keep.hits.cpu().numpy(), drop.hits.cpu().numpy()
        kept = set(zip(hk[:, 0].tolist(), hk[:, 1].tolist()))
        dropped = set(zip(hd[:, 0].tolist(), hd[:, 1].tolist()))
        for s, d, _ in plants:
            assert (s, d) in kept and (d, s) in kept and (s, d) not in dropped and (d, s) not in dropped
        # whatever else is listed has r^2 >= 1 by the oracle's margin (|r| > 1 needs missing codes)
        inn, amb, _ = lx.pair_classes(ex, 1.0, np.arange(n), n)
        assert all(inn[i, j] or amb[i, j] for i, j in kept)


# ---- LD scores -------------------------------------------------------------------------------------------------------
SCORE_SHAPES = [(300, 5008), (1000, 1008), (129, 257), (700, 333), (2500, 10240)]
_EXACT = {}


def score_panel(key):
    if isinstance(key, str):
        codes, _, ex = lx.long_range_panel(key)
        return codes, ex
    if key not in _EXACT:
        from ld_tools_amd import synth
        codes = synth.synth_codes_host(key[0], key[1], seed=11 + key[0])
        _EXACT[key] = (codes, lx.Exact(codes))
    return _EXACT[key]


@pytest.mark.parametrize("key", SCORE_SHAPES + list(lx.LONG_RANGE), ids=str)
def test_ld_scores_against_exact_r2_sums(gpu, key):
    from ld_tools_amd import ops
    codes, ex = score_panel(key)
    n = ex.n_snps
    p = pack(codes, gpu)
    ann = np.random.default_rng(n).random((n, 3)) < np.array([0.5, 0.1, 0.9])
    sel = np.concatenate([np.ones((n, 1)), ann.astype(np.float64)], axis=1)
    worst = 0.0
    for pos, w in lx.score_windows(n, n):
        win = lx.window_mask(pos, w)
        L = (ex.r2_64 * win) @ sel                                     # the diagonal is ((n - a) / r)^2: the same formula
        P = win.astype(np.float64) @ sel                               # in-window pairs (self included) per category
        m = (win & ex.live[None, :]).astype(np.int64) @ sel.astype(np.int64)
        bound = 2.0 ** -19 * L + P * 2.0 ** -33
        for path in BANDS:
            for annot, k in ((None, 0), (ann, 3)):
                res = ops.ld_score(p, pos, window_bp=w, annot=annot, path=path)
                assert res.l2.shape == (n, 1 + k)
                err = np.abs(res.l2 - L[:, :1 + k])
                worst = max(worst, float((err / np.maximum(bound[:, :1 + k], 1e-300)).max()))
                assert (err <= bound[:, :1 + k]).all(), (key, w, path, k)
                assert np.array_equal(res.m, m[:, :1 + k]) and np.array_equal(res.live, ex.live)
    print(f"{key}: worst |l2 - exact| / bound = {worst:.3g}")


# ---- neighbour lists ---------------------------------------------------------------------------------------------------
def check_lists(nb, ex, inn, amb, what):
    """decided-in <= reported <= decided-in + ambiguous, both orientations, sorted; r within 4 ulps; s = r *f32 r."""
    n = ex.n_snps
    off = nb.offsets.cpu().numpy().astype(np.int64)
    h = nb.hits.cpu().numpy()
    assert off.shape == (n + 1,) and off[0] == 0 and off[-1] == h.shape[0] and (np.diff(off) >= 0).all(), what
    q, o = h[:, 0].astype(np.int64), h[:, 1].astype(np.int64)
    assert ((q >= 0) & (q < n) & (o >= 0) & (o < n)).all(), what
    assert np.array_equal(q, np.repeat(np.arange(n), np.diff(off))), what
    assert (np.diff(q * n + o) > 0).all(), what                   # rows in order, columns strictly ascending inside a row
    rep = np.zeros((n, n), dtype=bool)
    rep[q, o] = True
    assert np.array_equal(rep, rep.T), what                        # both orientations
    assert not (inn & ~rep).any(), (what, np.argwhere(inn & ~rep)[:5])
    assert not (rep & ~(inn | amb)).any(), (what, np.argwhere(rep & ~(inn | amb))[:5])
    r = np.ascontiguousarray(h[:, 2]).view(np.float32)
    s = np.ascontiguousarray(h[:, 3]).view(np.float32)
    if r.size:
        assert float(lx.ulp32_err(r, ex.r64[q, o]).max()) <= 4.0, what
        assert np.array_equal(r > 0, ex.num[q, o] > 0), what
    assert np.array_equal(s.view(np.uint32), np.multiply(r, r, dtype=np.float32).view(np.uint32)), what
    Rm = np.zeros((n, n), dtype=np.float32)
    Rm[q, o] = r
    assert np.array_equal(Rm.view(np.uint32), Rm.T.view(np.uint32)), what    # one value per pair
    return rep


@pytest.mark.parametrize("path", BANDS)
@pytest.mark.parametrize("name", list(lx.LONG_RANGE))
def test_neighbour_lists_against_exact_decisions(gpu, name, path):
    """`strict` moves the bound b by one float32 ulp; the oracle's margin covers both bounds (tests/ld_exact.py), so the
    same decided sets hold for r^2 >= t and r^2 > t."""
    from ld_tools_amd import ops
    codes, _, ex = lx.long_range_panel(name)
    p = pack(codes, gpu)
    crossing = 0
    for pos, w in lx.neighbour_windows(ex.n_snps):
        for t in lx.NEIGHBOUR_THRESHOLDS:
            inn, amb, win = lx.pair_classes(ex, t, pos, w)
            assert amb.sum() <= lx.AMBIGUOUS_SHARE_MAX * win.sum()         # a condition of the comparison, from the oracle
            for strict in (False, True):
                nb = ops.ld_neighbors(p, pos, window_bp=w, r2=t, strict=strict, path=path)
                rep = check_lists(nb, ex, inn, amb, (name, path, w, t, strict))
                crossing += lx.tile_crossing(rep)
        assert lx.tile_crossing(lx.pair_classes(ex, 0.2, pos, w)[0]) >= 1000
    assert crossing >= 1000
    # the overflow retry, with hits from off-diagonal tiles in the lists
    pos, w = lx.neighbour_windows(ex.n_snps)[1]
    inn, amb, _ = lx.pair_classes(ex, 0.2, pos, w)
    tiny = ops.ld_neighbors(p, pos, window_bp=w, r2=0.2, path=path, hit_capacity=256)
    assert len(tiny) > 256
    check_lists(tiny, ex, inn, amb, (name, path, "hit_capacity=256"))


# ---- clumping and pruning ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lx.CLUMP_CASES))
def test_clump_and_prune_against_the_sequential_rule(gpu, name):
    from ld_tools_amd import ops
    codes, ex = lx.clump_panel(name)
    n = ex.n_snps
    p = pack(codes, gpu)
    pos = lx.clump_positions(n)
    pv = lx.clump_pvalues(n)
    assert np.isnan(pv).sum() > 10 and (pv == 1e-5).sum() > 5 and (pv == 3e-4).sum() > 10        # NaNs and ties
    clumps, prunes = lx.CLUMP_CASES[name]
    spans = 0
    for p1, p2, t, w in clumps:
        inn, amb, _ = lx.pair_classes(ex, t, pos, w)
        assert amb.sum() == 0                                          # the greedy result is unique
        index, owner = lx.clump_exact(inn, pv, p1, p2, ex.live)
        assert len(index) > 1
        for path in BANDS:
            res = ops.ld_clump(p, pos, pv, p1=p1, p2=p2, r2=t, window_bp=w, path=path)
            assert res.index.tolist() == index, (name, p1, p2, t, w, path)
            assert np.array_equal(res.owner, owner), (name, p1, p2, t, w, path)
            assert np.array_equal(res.nan_p, np.flatnonzero(np.isnan(pv)))
            assert np.array_equal(res.degenerate, np.flatnonzero(~ex.live))
        for k in index:
            tiles = set((np.flatnonzero(owner == k) // 128).tolist())
            spans += len(tiles) >= 2
    if name in lx.LONG_RANGE:
        assert spans >= 1                                              # a clump with members in two 128-column tiles
    maf = np.minimum(ex.a, ex.r)                                       # the default priority min(fa, fr), as integers
    tied = np.random.default_rng(3).integers(0, 5, size=n).astype(float)
    for t, w in prunes:
        inn, amb, _ = lx.pair_classes(ex, t, pos, w)
        assert amb.sum() == 0
        for prio, given in ((maf, None), (tied, tied)):
            keep = lx.prune_exact(inn, prio, ex.live)
            assert 1 < keep.sum() < ex.live.sum()
            for path in BANDS:
                res = ops.ld_prune(p, pos, r2=t, window_bp=w, priority=given, path=path)
                assert np.array_equal(res.keep, keep), (name, t, w, path, given is None)
            if name in lx.LONG_RANGE:   # pruning removed SNPs because of a kept one in another tile
                kk = np.flatnonzero(keep)
                gone = np.flatnonzero(~keep & ex.live)
                assert any((kk[inn[j, kk]] // 128 != j // 128).any() for j in gone)


# ---- R x and ridge -----------------------------------------------------------------------------------------------------
def rhs(n, seed):
    """float32 [n, 8]: mixed signs and magnitudes, an all-zero column (5) and a one-hot column (6)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, 8)) * np.exp2(rng.integers(-12, 3, size=(n, 8)))).astype(np.float32)
    x[:, 1] = rng.uniform(-1, 1, n).astype(np.float32)
    x[:, 2] *= np.float32(1e-20)
    x[:, 3] *= np.float32(1e12)
    x[:, 5] = 0
    x[:, 6] = 0
    x[n // 3, 6] = 1
    return x


def column_scale(x):
    """2^e per column, e the smallest integer with max |x| 2^-e <= 1 (include/ldx.h's scaled right-hand sides); 1 for zeros."""
    big = np.abs(x).max(axis=0).astype(np.float64)
    mant, e = np.frexp(big)
    e = np.where(mant == 0.5, e - 1, e)
    return np.where(big > 0, np.ldexp(1.0, e), 1.0)


@pytest.mark.parametrize("name", list(lx.LONG_RANGE))
def test_matvec_against_the_exact_matrix(gpu, name):
    from ld_tools_amd import ops
    codes, _, ex = lx.long_range_panel(name)
    n = ex.n_snps
    p = pack(codes, gpu)
    x = rhs(n, n)
    x64 = x.astype(np.float64)
    scale = column_scale(x)
    worst = {1: 0.0, 2: 0.0}
    for pos, w in lx.neighbour_windows(n):
        win = lx.window_mask(pos, w)
        pop = win.sum(axis=1)[:, None].astype(np.float64)
        for power, M, cell in ((1, ex.r64 * win, 2.0 ** -21), (2, ex.r2_64 * win, 2.0 ** -19)):
            ref = M @ x64
            bound = cell * (np.abs(M) @ np.abs(x64)) + pop * scale * 2.0 ** -41
            for path in BANDS:
                y = ops.ld_matvec(p, x, pos, window_bp=w, power=power, path=path).values().cpu().numpy()
                err = np.abs(y - ref)
                worst[power] = max(worst[power], float((err / np.maximum(bound, 1e-300)).max()))
                assert (err <= bound).all(), (name, w, power, path)
                assert (y[:, 5] == 0).all()
    print(f"{name}: worst |y - exact| / bound: power 1 {worst[1]:.3g}, power 2 {worst[2]:.3g}")


@pytest.mark.parametrize("path", BANDS)
def test_ridge_true_residual_against_the_exact_matrix(gpu, path):
    from ld_tools_amd import ops
    codes, _, ex = lx.long_range_panel("lr1000")
    n = ex.n_snps
    p = pack(codes, gpu)
    reach = 150                                                        # SNPs each side: every window spans a tile boundary
    Rw = ex.r64 * lx.window_mask(np.arange(n), reach)
    lam = 0.5 - min(0.0, float(np.linalg.eigvalsh(Rw).min()))          # positive definite by the ORACLE's matrix: >= 0.5
    A = Rw + lam * np.eye(n)
    z = np.random.default_rng(21).standard_normal((n, 3))
    tol = 1e-6
    res = ops.ld_ridge(p, z, window_snps=reach, lam=lam, tol=tol, path=path)
    assert res.converged.all() and not res.indefinite.any()
    beta = res.beta.cpu().numpy()
    zn = np.linalg.norm(z, axis=0)
    true = np.linalg.norm(A @ beta - z, axis=0) / zn
    bound = 2 * tol + 2.0 ** -21 * np.linalg.norm(np.abs(Rw) @ np.abs(beta), axis=0) / zn
    print(f"ridge {path}: lam {lam:.4g}, iterations {res.iterations.tolist()}, true residual {true}, bound {bound}")
    assert (true <= bound).all()

"""GPU: banded LD matrix-vector products on the matrix-pipe band (ldx_ld_matvec_dev, ops.ld_matvec, ops.ld_ridge).

Contract (include/ldx.h): sums[i][k] = the int64 sum of rint(2^40 * (v_ij x_jk)) over the SNPs j with |pos_i - pos_j| <= w
(j = i included), v the r32 cell of ld_triangle(fmt="r32") bit for bit (the diagonal: r_matrix()'s) or its float32 square.
Checked here as integers against a numpy sum over the r32 square: no floating-point tolerance in the kernel's tests.
"""
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.gpu


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


def r32_square(p):
    from ld_tools_amd import ops
    return ops.ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()


def host_sums(R, pos, w, x32, power):
    """The sums from the r32 square (float32 cells, diagonal included) and the float32 weights: numpy, int64."""
    from ld_tools_amd import ops
    pos = np.asarray(pos, dtype=np.int64)
    V = ops.prod_values(R, power).copy()
    V[np.abs(pos[:, None] - pos[None, :]) > w] = 0
    return np.stack([ops.prod_terms(V, x32[None, :, k]).sum(axis=1, dtype=np.int64) for k in range(x32.shape[1])], axis=1)


def rhs(n, seed):
    """float32 [n, 8]: mixed signs and magnitudes, one all-zero column (5) and one one-hot column (6)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, 8)) * np.exp2(rng.integers(-12, 3, size=(n, 8)))).astype(np.float32)
    x[:, 1] = rng.uniform(-1, 1, n).astype(np.float32)
    x[:, 2] *= np.float32(1e-20)
    x[:, 3] *= np.float32(1e12)
    x[:, 5] = 0
    x[:, 6] = 0
    x[n // 3, 6] = 1
    return x


def windows_for(n, seed):
    """(positions, window) cases: self only, everything, a grid with many |delta| = w pairs, duplicates, ragged."""
    rng = np.random.default_rng(seed)
    grid = 1 + 100 * np.arange(n, dtype=np.int64)
    dup = np.sort(rng.integers(1, max(2, n // 3), size=n)).astype(np.int64)   # many equal positions
    ragged = np.cumsum(rng.integers(0, 40, size=n)).astype(np.int64) + 7
    return [(grid, 0), (grid, int(grid[-1])), (grid, 300), (grid, 100 * 129), (dup, 0), (dup, 2), (ragged, 150)]


def sums_of(res):
    return res.sums.cpu().numpy()


@pytest.mark.parametrize("shape", [(300, 5008), (1000, 1008), (129, 257), (700, 333), (2500, 10240)])
def test_sums_equal_the_r32_square(gpu, shape):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = shape
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=11 + n), gpu)
    R = r32_square(p)
    x = rhs(n, n)
    cases = [(pos, w, None) for pos, w in windows_for(n, n)] + [(np.arange(n), 37, 37)]
    for pos, w, wsnps in cases:
        for power in (1, 2):
            want = None
            for cols in ([1], [4, 5, 6], list(range(8))):   # n_rhs 1, 3 (with the zero and the one-hot column), 8
                kw = dict(window_snps=wsnps) if wsnps is not None else dict(positions=pos, window_bp=w)
                res = ops.ld_matvec(p, x[:, cols], power=power, **kw)
                got = sums_of(res)
                assert got.dtype == np.int64 and got.shape == (n, len(cols))
                if want is None:   # every column has its own scale, so one host sum over all eight serves the subsets
                    full = ops.ld_matvec(p, x, power=power, **kw)
                    want = host_sums(R, pos, w, full.x32.cpu().numpy(), power)
                    assert np.array_equal(sums_of(full), want), (shape, w, power)
                    assert np.array_equal(full.x().cpu().numpy(), x.astype(np.float64))   # float32 in: the scaling is exact
                assert np.array_equal(got, want[:, cols]), (shape, w, power, cols)
                assert (got[:, [c == 5 for c in cols]] == 0).all()
    # values(): the product itself, against float64 numpy on the same cells
    pos, w = windows_for(n, n)[2]
    y = ops.ld_matvec(p, x, pos, window_bp=w).values().cpu().numpy()
    Rw = R.astype(np.float64) * (np.abs(pos[:, None] - pos[None, :]) <= w)
    ref = Rw @ x.astype(np.float64)
    pop = (np.abs(pos[:, None] - pos[None, :]) <= w).sum(axis=1)[:, None]
    scale = np.exp2(np.ceil(np.log2(np.maximum(np.abs(x).max(axis=0).astype(np.float64), 1e-300))))
    assert (np.abs(y - ref) <= pop * scale * 2.0 ** -41 + 1e-12 * np.abs(Rw) @ np.abs(x.astype(np.float64))).all()


@pytest.mark.parametrize("power", [1, 2])
def test_missing_codes_and_degenerate_snps(gpu, power):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = 900, 1008
    codes = synth.synth_codes_host(n, h, seed=23, miss=0.02, mono=0.06, miss_rows=0.5)
    p = PackedPanel.from_codes(codes, gpu)
    a, r = p.alt_counts().astype(np.int64), p.ref_counts().astype(np.int64)
    deg = a * r == 0
    assert deg.sum() > 10 and (a + r < h).sum() > 100
    R = r32_square(p)
    pos = 1 + 50 * np.arange(n, dtype=np.int64)
    x = rhs(n, 5)[:, :3]
    for w in (0, 500, 5000):
        got = {}
        for path in ("fp4", "mfma"):
            res = ops.ld_matvec(p, x, pos, window_bp=w, power=power, path=path)
            got[path] = sums_of(res)
            assert np.array_equal(got[path], host_sums(R, pos, w, res.x32.cpu().numpy(), power)), (w, path)
            assert (got[path][deg] == 0).all()            # a degenerate SNP's row is 0
        assert np.array_equal(got["fp4"], got["mfma"])
    # ... and it adds 0 to every neighbour: the same sums whatever its weight is
    x2 = x.copy()
    x2[deg] = np.float32(0.5) * np.abs(x).max(axis=0)
    assert np.array_equal(sums_of(ops.ld_matvec(p, x2, pos, window_bp=5000, power=power)),
                          sums_of(ops.ld_matvec(p, x, pos, window_bp=5000, power=power)))


def test_power2_of_a_01_column_against_ld_score(gpu):
    """Both terms are the float32 r^2 scaled by a power of two and rounded once, at 2^-40 here and at 2^-32 in ld_score:
    per pair |term - 2^8 score_term| <= 2^7 (each rounding is at most half a unit: 1/2 + 2^8 / 2), and 0 when r^2 >= 2^-9 or
    r^2 = 0 (neither rounds).  So |sums - 2^8 score_sums| <= 2^7 * (the SNP's window population inside the category)."""
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = 1100, 1008
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=5, miss=0.005, mono=0.02), gpu)
    R = r32_square(p)
    r2 = ops.prod_values(R, 2).astype(np.float64)
    pos = 1 + 100 * np.arange(n, dtype=np.int64)
    cat = np.random.default_rng(1).random(n) < 0.4
    n_exact = 0
    for w in (100, 200, 100 * 300):
        mv = ops.ld_matvec(p, cat.astype(np.float32), pos, window_bp=w, power=2)
        assert int(mv.exps[0]) == 0                       # a 0/1 column is multiplied as it is
        got = sums_of(mv)[:, 0]
        sc = ops.ld_score(p, pos, window_bp=w, annot=cat).sums.cpu().numpy()[:, 1].astype(np.int64)
        inwin = (np.abs(pos[:, None] - pos[None, :]) <= w) & cat[None, :]
        popc = inwin.sum(axis=1)
        diff = np.abs(got - (sc << 8))
        print("w", w, "max |diff|", int(diff.max()), "max bound", int((popc << 7).max()))
        assert (diff <= (popc << 7)).all(), w
        exact = (((r2 >= 2.0 ** -9) | (r2 == 0)) | ~inwin).all(axis=1)
        n_exact += int(exact.sum())
        assert (diff[exact] == 0).all(), w
    assert n_exact > 50


def test_one_hot_is_a_column_of_the_r_matrix(gpu):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = 700, 333
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=8, miss=0.01, mono=0.02), gpu)
    R = r32_square(p)
    pos = 1 + 10 * np.arange(n, dtype=np.int64)
    for j in (0, 127, 128, 333, n - 1):
        e = np.zeros(n, dtype=np.float32)
        e[j] = 1
        for w in (0, 640, 10 * n):
            got = sums_of(ops.ld_matvec(p, e, pos, window_bp=w))[:, 0]
            col = R[:, j].copy()
            col[np.abs(pos - pos[j]) > w] = 0
            assert np.array_equal(got, ops.prod_terms(col, np.float32(1))), (j, w)


def test_tile_boundary_shape_at_size(gpu):
    """10 000 x 5008 (a panel that ends inside a tile), +-300 SNPs, eight right-hand sides, every entry against the host
    sum over blocks of r_matrix()."""
    import torch

    from ld_tools_amd import PackedPanel, ops, synth
    n, h, wn = 10_000, 5008, 300
    p = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=gpu), gpu)
    pos = synth.synth_positions(n, step=500)
    x = rhs(n, 77)
    tri = ops.ld_triangle(p, fmt="r32")
    for power in (1, 2):
        res = ops.ld_matvec(p, x, pos, window_bp=500 * wn, power=power)
        got, x32 = sums_of(res), res.x32.cpu().numpy()
        for r0 in range(0, n, 1000):
            r1 = min(n, r0 + 1000)
            c0, c1 = max(0, r0 - wn), min(n, r1 + wn)
            blk = tri.r_matrix(rows=(r0, r1), cols=(c0, c1)).cpu().numpy()
            want = host_sums_block(blk, pos[r0:r1], pos[c0:c1], 500 * wn, x32[c0:c1], power)
            assert np.array_equal(got[r0:r1], want), (power, r0)
    del tri
    torch.cuda.empty_cache()


def host_sums_block(blk, pos_r, pos_c, w, x32, power):
    from ld_tools_amd import ops
    V = ops.prod_values(blk, power).copy()
    V[np.abs(pos_r[:, None] - pos_c[None, :]) > w] = 0
    return np.stack([ops.prod_terms(V, x32[None, :, k]).sum(axis=1, dtype=np.int64) for k in range(x32.shape[1])], axis=1)


def test_run_to_run_graph_and_streams(gpu):
    import torch

    from ld_tools_amd import PackedPanel, _lib, ops, synth
    n, h = 3000, 1008
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=41, miss=0.004), gpu)
    pos = torch.as_tensor(1 + 300 * np.arange(n, dtype=np.int64)).to(gpu)
    x = torch.as_tensor(rhs(n, 2)).to(gpu)
    nbytes = _lib.lib.ldx_ld_matvec_workspace_bytes(n, h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    kw = dict(window_bp=60_000, check_positions=False, check_finite=False)
    a = ops.ld_matvec(p, x, pos, workspace=ws, **kw)
    b = ops.ld_matvec(p, x, pos, workspace=ws, **kw)            # the same call twice into different buffers
    assert a.sums.data_ptr() != b.sums.data_ptr() and torch.equal(a.sums, b.sums)
    assert a.sums.abs().max() > 0
    # captured in a graph and replayed
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = ops.ld_matvec(p, x, pos, workspace=ws, **kw)
    for _ in range(2):
        c.sums.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(a.sums, c.sums)
    # two calls with their own workspaces on two streams
    ws2 = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        d = ops.ld_matvec(p, x, pos, workspace=ws, **kw)
    with torch.cuda.stream(s2):
        e = ops.ld_matvec(p, x, pos, workspace=ws2, path="mfma", **kw)
    s1.synchronize()
    s2.synchronize()
    assert torch.equal(a.sums, d.sums) and torch.equal(a.sums, e.sums)
    # a different window through the same workspace, then the first again
    ops.ld_matvec(p, x[:, :2], pos, window_bp=3_000, workspace=ws, power=2)
    f = ops.ld_matvec(p, x, pos, workspace=ws, **kw)
    assert torch.equal(a.sums, f.sums)


def test_rejections(gpu):
    import torch

    from ld_tools_amd import LdxError, PackedPanel, _lib, ops, synth
    n = 200
    p = PackedPanel.from_codes(synth.synth_codes_host(n, 100, seed=2), gpu)
    pos = 1 + 10 * np.arange(n, dtype=np.int64)
    x = np.ones((n, 2), dtype=np.float32)
    bad = pos.copy()
    bad[50] = 0
    with pytest.raises(LdxError, match="non-decreasing"):
        ops.ld_matvec(p, x, bad)
    with pytest.raises(LdxError, match="window"):
        ops.ld_matvec(p, x, pos, window_bp=-1)
    with pytest.raises(LdxError, match="right-hand sides"):
        ops.ld_matvec(p, np.ones((n, 9), dtype=np.float32), pos)
    with pytest.raises(LdxError, match="finite"):
        ops.ld_matvec(p, np.full((n, 1), np.nan), pos)
    with pytest.raises(LdxError, match="power"):
        ops.ld_matvec(p, x, pos, power=3)
    with pytest.raises(LdxError, match="LDX_E_UNSUPPORTED"):
        ops.ld_matvec(p, x, pos, path="popcount")
    # the C entry point itself
    lib = _lib.lib
    pos_d = torch.as_tensor(pos).to(gpu)
    x_d = torch.as_tensor(x).to(gpu)
    sums = torch.empty((n, 2), dtype=torch.int64, device=gpu)
    ws = torch.empty(lib.ldx_ld_matvec_workspace_bytes(n, 100), dtype=torch.uint8, device=gpu)
    args = [p.alt.data_ptr(), p.acnt.data_ptr(), p.rcnt.data_ptr(), p.fa.data_ptr(), p.fr.data_ptr(), n, 100, pos_d.data_ptr(),
            1000, x_d.data_ptr(), 2, 1, 0, sums.data_ptr(), ws.data_ptr(), ws.numel(), None]
    assert lib.ldx_ld_matvec_dev(*args) == 0
    for k, v, rc in ((8, -1, -1), (9, None, -1), (10, 0, -1), (10, 9, -1), (11, 0, -1), (11, 3, -1), (12, 7, -1),
                     (13, None, -1), (14, ws.data_ptr() + 8, -1), (15, ws.numel() - 1, -1), (6, _lib.MAX_HAPS + 1, -3),
                     (12, 1, -3)):
        bad_args = list(args)
        bad_args[k] = v
        assert lib.ldx_ld_matvec_dev(*bad_args) == rc, (k, v)
    torch.cuda.synchronize()


def test_ridge(gpu):
    """(R_w + lam I) beta = z by conjugate gradients on ld_matvec.  The true residual is asked to be <= 2 tol: the recurrence
    residual is <= tol at convergence and differs from the true one only by the accumulated term rounding of the products,
    at most (window population) 2^-41 max |p| each -- about 1e-9 here, a thousand times below tol = 1e-6."""
    from ld_tools_amd import PackedPanel, ops, synth
    n, h, tol = 2000, 1008, 1e-6
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=77), gpu)
    R = r32_square(p).astype(np.float64)
    idx = np.arange(n)
    rng = np.random.default_rng(9)
    z = rng.standard_normal((n, 4)) * np.array([1.0, 10.0, 0.01, 3.0])
    band = np.abs(idx[:, None] - idx[None, :]) <= 50
    off = np.abs(R * band - np.diag(np.diag(R))).sum(axis=1).max()
    for wn, lam in ((n, 0.1),                # everything: R is a Gram matrix, R + 0.1 I is positive definite
                    (50, 1.0 + off)):        # +-50 SNPs, diagonally dominant, hence positive definite
        A = R * (np.abs(idx[:, None] - idx[None, :]) <= wn) + lam * np.eye(n)
        res = ops.ld_ridge(p, z, window_snps=wn, lam=lam, tol=tol)
        beta = res.beta.cpu().numpy()
        true = np.linalg.norm(A @ beta - z, axis=0) / np.linalg.norm(z, axis=0)
        print("window", wn, "lam", lam, "iterations", res.iterations, "recurrence", res.residual, "true", true)
        assert res.converged.all() and not res.indefinite.any()
        assert (res.residual <= tol).all()
        assert (true <= 2 * tol).all(), true
    # one column, one-dimensional z
    res1 = ops.ld_ridge(p, z[:, 0], window_snps=50, lam=1.0 + off, tol=tol)
    assert res1.beta.shape == (n,) and res1.converged.all()
    assert np.allclose(res1.beta.cpu().numpy(), beta[:, 0], rtol=0, atol=1e-5 * np.abs(beta[:, 0]).max())
    # +-3 SNPs, lam = 0: the truncated band has a negative eigenvalue -- no solution, reported as such
    A3 = R * (np.abs(idx[:, None] - idx[None, :]) <= 3)
    assert np.linalg.eigvalsh(A3).min() < -0.5
    res = ops.ld_ridge(p, z, window_snps=3, lam=0.0, tol=tol)
    assert res.indefinite.all() and not res.converged.any()
    assert np.isnan(res.beta.cpu().numpy()).all()

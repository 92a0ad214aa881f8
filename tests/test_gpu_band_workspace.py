"""GPU: every band operator stays inside a workspace of exactly its *_workspace_bytes() bytes.

The seven operators that run on the band form of the matrix kernel (LD scores, the cross-LD profile, LD decay, the
four-gamete test, R.x, neighbour lists, ld_area) carve one workspace layout.  Each gets the first `need` bytes of a buffer of
need + 4096 bytes filled with 0xA5 -- what a workspace may hold: the operators initialise what they read -- and must give
the result of the same call on a workspace of its own, bit for bit, and leave the 4096 guard bytes as they were.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 4096


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


def host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def run_area(p, pos, ws):
    """One ld_area scan + finish on the FP4 band, every SNP a query; `ws`: the scan's workspace, None = the plan's own."""
    import torch

    from ld_tools_amd import ops
    n = p.n_snps
    plan = ops._AreaPlan(p, n, 1 << 20)
    if ws is not None:
        assert ws.numel() == plan.ws_bytes
        plan.ws = ws
    q = torch.arange(n, dtype=torch.int32, device=p.device)
    old = ops.get_area_path()
    try:
        ops.set_area_path("fp4")
        ops._area_launch(p, pos, q, n, int(pos[-1]), "r_square", 0.01, plan)
    finally:
        ops.set_area_path(old)
    total, reserved = (int(x) for x in plan.summary.tolist())
    assert reserved <= plan.cap
    return host(plan.offsets, plan.hits[:total])


# name -> (the size function, run(panel, positions, window, workspace) -> host arrays)
def operators():
    from ld_tools_amd import ops
    from ld_tools_amd._lib import lib

    def matvec(p, pos, w, ws):
        x = np.random.default_rng(3).standard_normal((p.n_snps, 2)).astype(np.float32)
        return host(ops.ld_matvec(p, x, pos, window_bp=w, path="fp4", workspace=ws).sums)

    def blocks(p, pos, w, ws):
        r = ops.ld_blocks(p, pos, window_bp=w, path="fp4", workspace=ws)
        return host(r.left_dev, r.block_of_dev, r.n_out)

    def decay(p, pos, w, ws):
        r = ops.ld_decay(p, pos, window_bp=w, bin_bp=500, path="fp4", workspace=ws)
        return host(r.sums, r.counts_dev)

    def cross(p, pos, w, ws):
        r = ops.ld_cross(p, pos, window_bp=w, path="fp4", workspace=ws)
        return host(r.sides, r.cross)

    def neighbors(p, pos, w, ws):
        r = ops.ld_neighbors(p, pos, window_bp=w, r2=0.01, path="fp4", workspace=ws)
        return host(r.offsets, r.hits)

    return {
        "score": (lib.ldx_ld_score_workspace_bytes,
                  lambda p, pos, w, ws: host(ops.ld_score(p, pos, window_bp=w, path="fp4", workspace=ws).sums)),
        "cross": (lib.ldx_ld_cross_workspace_bytes, cross),
        "decay": (lib.ldx_ld_decay_workspace_bytes, decay),
        "fgt": (lib.ldx_ld_fgt_workspace_bytes, blocks),
        "matvec": (lib.ldx_ld_matvec_workspace_bytes, matvec),
        "neighbors": (lib.ldx_ld_neighbors_workspace_bytes, neighbors),
        "area": (lambda n, h: lib.ldx_area_workspace_bytes(n, h, n), lambda p, pos, w, ws: run_area(p, pos, ws)),
    }


# 129 SNPs: two tiles, the smallest shape with a cross-tile pass; 1 SNP: no pair (the operators' early return)
CASES = [(op, n) for op in ("score", "cross", "decay", "fgt", "matvec", "neighbors", "area") for n in (129, 1)] + \
        [("neighbors", 300)]


@pytest.mark.parametrize("op,n", CASES)
def test_exact_size_workspace_with_guards(gpu, op, n):
    import torch

    from ld_tools_amd import PackedPanel, synth
    size_fn, run = operators()[op]
    p = PackedPanel.from_codes(synth.synth_codes_host(n, 64, seed=40 + n), gpu)
    pos = torch.as_tensor(1 + 100 * np.arange(n, dtype=np.int64)).to(gpu)
    w = 100 * n                                      # every pair, so the pass across the tile boundary holds pairs
    need = size_fn(n, 64)
    want = run(p, pos, w, None)
    buf = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    got = run(p, pos, w, buf[:need])
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), op
    assert bool((buf[need:] == 0xA5).all()), op
    if n > 1 and op in ("neighbors", "area"):
        assert got[1].shape[0] > 0                   # the comparison is of real lists

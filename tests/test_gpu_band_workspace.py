"""GPU: every band operator stays inside a workspace of exactly its *_workspace_bytes() bytes.

The seven operators that run on the band form of the matrix kernel (LD scores, the cross-LD profile, LD decay, the
four-gamete test, R.x, neighbour lists, ld_area) carve one workspace layout.  Each gets the first `need` bytes of a buffer of
need + 4096 bytes filled with 0xA5 -- what a workspace may hold: the operators initialise what they read -- and must give
the result of the same call on a workspace of its own, bit for bit, and leave the 4096 guard bytes as they were.

The six operators on the plan bands (pairwise-complete and EM: ldx_band_plan.h) carve another: the plan's prefix, then `low`,
each rounded to 256 bytes.  They get the same check at the sizes either side of the prefix part's first step and at the plan
case, whose prefix is written in two trips.
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


# ---- the plan bands (pairwise-complete and EM): prefix [Ti + 1] uint64 rounded to 256 bytes, then low [n] uint32 rounded to 256
def plan_operators():
    """name -> (the size function of n, run(panel, positions, window, workspace) -> host arrays)"""
    from ld_tools_amd import ops
    from ld_tools_amd._lib import lib
    pw, em = lib.ldx_ld_pw_band_workspace_bytes, lib.ldx_ld_em_band_workspace_bytes

    def pw_band(p, pos, w, ws):
        r = ops.ld_band(p, pos, window_bp=w, missing="pairwise", workspace=ws)
        return host(r.values, r.diag, r.lo, r.offsets)

    def pw_neighbors(p, pos, w, ws):
        r = ops.ld_neighbors(p, pos, window_bp=w, r2=0.2, missing="pairwise", workspace=ws)
        return host(r.offsets, r.hits)

    def em_band(p, pos, w, ws):
        r = ops.ld_em_band(p, pos, window_bp=w, missing="pairwise", workspace=ws)
        return host(r.r.values, r.dprime.values, r.r.diag, r.live)

    def em_neighbors(p, pos, w, ws):
        r = ops.ld_neighbors(p, pos, window_bp=w, r2=0.2, em=True, missing="pairwise", workspace=ws)
        return host(r.offsets, r.hits)

    def dprime_ci(p, pos, w, ws):
        r = ops.ld_dprime_ci(p, pos, window_bp=w, missing="pairwise", workspace=ws)
        return host(r.lo, r.hi, r.kept)

    return {
        "pw_band": (pw, pw_band),
        "pw_score": (pw, lambda p, pos, w, ws: host(ops.ld_score(p, pos, window_bp=w, missing="pairwise", workspace=ws).sums)),
        "pw_neighbors": (pw, pw_neighbors),
        "em_band": (em, em_band),
        "em_neighbors": (em, em_neighbors),
        "dprime_ci": (em, dprime_ci),
    }


# rows per I block of the operator's kernel
PLAN_ROWS = {"pw_band": 256, "pw_score": 256, "pw_neighbors": 256, "em_band": 128, "em_neighbors": 128, "dprime_ci": 128}
# 1 SNP: no pair; 129: two slabs; Ti = 31 | 32, where (Ti + 1) * 8 bytes pass 256 and the prefix part grows to 512; "plan": the
# plan case of tests/ld_pwband_cases.py / ld_emband_cases.py, 258 I blocks (the second trip of plan_kernel writes prefix[256 ..])
PLAN_CASES = [(op, n) for op, rows in PLAN_ROWS.items() for n in (1, 129, 31 * rows, 31 * rows + 1, "plan")]


def plan_prefix_bytes(n, rows):
    return ((n + rows - 1) // rows + 1) * 8


@pytest.mark.parametrize("op,n", PLAN_CASES)
def test_plan_band_exact_size_workspace_with_guards(gpu, op, n):
    import torch

    import ld_emband_cases as eb
    import ld_pwband_cases as pb
    from ld_tools_amd import PackedPanel
    size_fn, run = plan_operators()[op]
    rows = PLAN_ROWS[op]
    if n == "plan":
        n, n_hap = (pb if rows == 256 else eb).PLAN_CASE
        pos, w = pb.ragged_positions(n), pb.PLAN_WINDOW
    else:
        n_hap = 62
        pos = 1 + 100 * np.arange(n, dtype=np.int64)
        w = 100 * n if n <= 129 else 100 * 20        # every pair; 20 SNPs each side at the sizes around the step
    p = PackedPanel.from_codes(np.array(pb.mixed_panel(n, n_hap)[0]), gpu)
    pos = torch.as_tensor(pos).to(gpu)
    need = size_fn(n)
    pre = (plan_prefix_bytes(n, rows) + 255) // 256 * 256
    assert need == pre + (4 * n + 255) // 256 * 256
    if n in (31 * rows, 31 * rows + 1):
        assert pre == (256 if n == 31 * rows else 512)   # either side of the step
    want = run(p, pos, w, None)
    buf = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    got = run(p, pos, w, buf[:need])
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), op
    assert bool((buf[need:] == 0xA5).all()), op
    if n > 129 and op.endswith("neighbors"):
        assert got[1].shape[0] > 0                   # the comparison is of real lists

"""GPU: ld_blocks (ldx_ld_fgt_dev + ldx_ld_blocks_dev) -- the four-gamete test on the matrix-pipe band and the block scan.

Every assertion is an integer equality against the exact oracle of tests/ld_blocks_exact.py (counts from the allele codes):
`left` on both paths, fp4 == mfma, keep masks and maf_min, relaunches into pre-filled buffers, window_snps, the device scan
against ops.blocks_host and against the partition computed from the codes, the block invariants on the exact matrix, and
the argument errors.  The conditions that make the panels meaningful are pinned on the CPU (tests/test_ld_blocks_host.py).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_blocks_exact as bx  # noqa: E402

pytestmark = pytest.mark.gpu

BANDS = ("fp4", "mfma")
PHYLO = list(bx.PHYLO)
DENSE = ["lr1000", "lr700"]


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


def check_case(p, g, pos, w, m, keep=None, paths=BANDS, **kw):
    """ld_blocks on every path against the oracle: left, the partition (from the codes and through blocks_host), invariants."""
    from ld_tools_amd import ops
    rec = bx.recombinant(g, pos, w, m, keep)
    want_left = bx.exact_left(rec)
    want_b, want_nb, want_rm, _ = bx.exact_partition(rec, pos, w, keep)
    first = None
    for path in paths:
        res = ops.ld_blocks(p, pos, window_bp=w, min_count=m, keep=keep, path=path, **kw)
        assert res.left.dtype == np.uint32 and np.array_equal(res.left, want_left), (w, m, path)
        first = res.left if first is None else first
        assert np.array_equal(res.left, first)                                   # fp4 == mfma
        host_b, host_nb, host_rm = ops.blocks_host(res.left, pos, w, keep)
        assert np.array_equal(res.block_of, host_b) and (res.n_blocks, res.rm) == (host_nb, host_rm), (w, m, path)
        assert np.array_equal(res.block_of, want_b) and (res.n_blocks, res.rm) == (want_nb, want_rm), (w, m, path)
        if path == paths[0]:
            bx.check_invariants(res.block_of, g, pos, w, m, keep)
        assert res.sizes.sum() == (g.n_snps if keep is None else int(np.asarray(keep).sum())) and len(res.starts) == res.n_blocks
        assert (res.spans_bp <= w).all() and np.array_equal(res.sizes >= 1, np.ones(res.n_blocks, dtype=bool))
    return want_left, want_nb, want_rm


# ---- 1. left and the blocks against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", PHYLO + DENSE, ids=str)
def test_left_and_blocks_equal_the_oracle(gpu, key):
    codes, g = bx.panel(key)
    p = pack(codes, gpu)
    for pos, w in bx.windows(key):
        for m in bx.min_counts(g.n_hap):
            left, nb, rm = check_case(p, g, pos, w, m)
        print(f"{key} w={w}: m={m}: {nb} blocks, rm {rm}, {int((left != 0).sum())} SNPs with a partner")


@pytest.mark.parametrize("key", bx.EDGE_PANELS, ids=str)
def test_edge_panels(gpu, key):
    codes, g = bx.panel(key)
    p = pack(codes, gpu)
    for pos, w in bx.windows(key):
        for m in bx.min_counts(g.n_hap):
            check_case(p, g, pos, w, m)


def test_the_widest_panel_once(gpu):
    """lr2500: 10 240 haplotypes = LDX_MAX_HAPS (80 chunks in the K loop, counts beyond 2^13)."""
    codes, g = bx.panel("lr2500")
    assert g.n_hap == 10240
    p = pack(codes, gpu)
    pos, w = bx.windows("lr2500")[3]                    # more than a tile each side
    check_case(p, g, pos, w, 103)                       # ceil(0.01 n_hap)


# ---- 2. keep masks, maf_min ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PHYLO + ["lr700", (129, 333)], ids=str)
def test_keep_masks_and_maf_min(gpu, key):
    from ld_tools_amd import ops
    codes, g = bx.panel(key)
    n, h = codes.shape
    p = pack(codes, gpu)
    keep = bx.keep_mask(n)
    assert 0.6 < keep.mean() < 0.8
    maf = np.minimum(g.a, h - g.a) >= 0.05 * h
    assert maf.any() and not maf.all()
    for pos, w in bx.windows(key)[1:]:
        for m in (1, 4):
            check_case(p, g, pos, w, m, keep=keep)
            rec = bx.recombinant(g, pos, w, m, maf)
            want_b, want_nb, want_rm, _ = bx.exact_partition(rec, pos, w, maf)
            res = ops.ld_blocks(p, pos, window_bp=w, min_count=m, maf_min=0.05)
            assert np.array_equal(res.left, bx.exact_left(rec)) and np.array_equal(res.block_of, want_b)
            assert (res.n_blocks, res.rm) == (want_nb, want_rm)
            both = ops.ld_blocks(p, pos, window_bp=w, min_count=m, maf_min=0.05, keep=keep, path="mfma")
            assert np.array_equal(both.left, bx.exact_left(bx.recombinant(g, pos, w, m, maf & keep)))
    none = ops.ld_blocks(p, pos, window_bp=w, keep=np.zeros(n, dtype=bool))
    assert not none.left.any() and (none.block_of == bx.NOT_KEPT).all() and (none.n_blocks, none.rm) == (0, 0)


# ---- 3. relaunches, pre-filled buffers, window_snps, min_freq ---------------------------------------------------------------
@pytest.mark.parametrize("key", ["ph700", "lr700", (129, 64)], ids=str)
def test_relaunch_into_prefilled_buffers(gpu, key):
    import torch
    from ld_tools_amd import _lib, ops
    codes, g = bx.panel(key)
    n = g.n_snps
    p = pack(codes, gpu)
    ws = torch.empty(_lib.lib.ldx_ld_fgt_workspace_bytes(n, p.n_hap), dtype=torch.uint8, device=gpu)
    for pos, w in bx.windows(key)[1:4]:
        want = bx.exact_left(bx.recombinant(g, pos, w, 2))
        posd = torch.as_tensor(pos).to(gpu)
        left = torch.full((n,), -1, dtype=torch.int32, device=gpu)         # 0xFFFFFFFF in every word
        block_of = torch.full((n,), 12345, dtype=torch.int32, device=gpu)
        n_out = torch.full((2,), -1, dtype=torch.int32, device=gpu)
        for launch in range(2):
            for path in BANDS:
                if launch:
                    left.fill_(-1)
                ops._fgt_launch(p, posd, w, 2, None, ops.PATHS[path], left, ws)
                assert np.array_equal(left.cpu().numpy().view(np.uint32), want), (key, w, path, launch)
        ops._blocks_launch(left, posd, None, n, w, block_of, n_out)
        hb, hn, hr = ops.blocks_host(want, pos, w)
        assert np.array_equal(block_of.cpu().numpy().view(np.uint32), hb) and n_out.cpu().tolist() == [hn, hr]
        again = ops.ld_blocks(p, pos, window_bp=w, min_count=2, workspace=ws)
        assert np.array_equal(again.left, want)


def test_window_in_snps_and_min_freq(gpu):
    from ld_tools_amd import ops
    codes, g = bx.panel("ph300")
    p = pack(codes, gpu)
    idx = np.arange(300, dtype=np.int64)
    for w in (299, 130, 5, 0):
        rec = bx.recombinant(g, idx, w, 2)
        res = ops.ld_blocks(p, window_snps=w, min_count=2)
        assert np.array_equal(res.left, bx.exact_left(rec))
        assert np.array_equal(res.block_of, bx.exact_partition(rec, idx, w)[0])
    codes, g = bx.panel("ph1000")
    p = pack(codes, gpu)
    pos, w = bx.windows("ph1000")[1]
    res = ops.ld_blocks(p, pos, window_bp=w, min_freq=0.01)             # Haploview's rule: ceil(10.08) = 11
    assert res.min_count == 11 and np.array_equal(res.left, bx.exact_left(bx.recombinant(g, pos, w, 11)))
    assert ops.ld_blocks(p, pos, window_bp=w, min_freq=0.0).min_count == 1


# ---- 4. no recombinant pair at all, window 0 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["ph700", "lr1000", (300, 64)], ids=str)
def test_min_count_n_hap_leaves_the_window_alone(gpu, key):
    from ld_tools_amd import ops
    codes, g = bx.panel(key)
    p = pack(codes, gpu)
    assert int(g.min_gamete.max()) < g.n_hap
    for pos, w in bx.windows(key):
        for path in BANDS:
            res = ops.ld_blocks(p, pos, window_bp=w, min_count=g.n_hap, path=path)
            assert not res.left.any() and res.rm == 0
            want_b, want_nb, _ = ops.blocks_host(np.zeros(g.n_snps, dtype=np.uint32), pos, w)
            assert np.array_equal(res.block_of, want_b) and res.n_blocks == want_nb


def test_window_0_with_duplicate_positions(gpu):
    from ld_tools_amd import ops
    codes, g = bx.panel("lr700")
    p = pack(codes, gpu)
    pos, w = bx.windows("lr700")[4]
    assert w == 0 and (np.diff(pos) == 0).sum() > 200
    left, nb, rm = check_case(p, g, pos, 0, 1)
    assert left.any() and rm > 0 and nb > len(np.unique(pos))              # pairs at d = 0 are tested, and some break blocks


# ---- 5. errors, the single-SNP panel -------------------------------------------------------------------------------------------
def test_errors_and_the_single_snp_panel(gpu):
    import torch
    from ld_tools_amd import _lib, ops
    codes, g = bx.panel((129, 64))
    p = pack(codes, gpu)
    pos = 1 + 100 * np.arange(129, dtype=np.int64)
    for bad in (0, 65):
        with pytest.raises(_lib.LdxError):
            ops.ld_blocks(p, pos, window_bp=1000, min_count=bad)
    with pytest.raises(_lib.LdxError, match="UNSUPPORTED"):
        ops.ld_blocks(p, pos, window_bp=1000, path="popcount")
    with pytest.raises(_lib.LdxError):
        ops.ld_blocks(p, pos[::-1].copy(), window_bp=1000)              # unsorted positions
    with pytest.raises(_lib.LdxError):
        ops.ld_blocks(p, pos, window_bp=1000, keep=np.ones(5, dtype=bool))
    with pytest.raises(_lib.LdxError):
        ops.ld_blocks(p, pos, window_bp=-1)
    # the C entry point: min_count 0 and > n_hap are LDX_E_ARG (-1), n_hap > LDX_MAX_HAPS and the popcount path unsupported
    ws = torch.empty(_lib.lib.ldx_ld_fgt_workspace_bytes(129, 64), dtype=torch.uint8, device=gpu)
    out = torch.zeros(129, dtype=torch.int32, device=gpu)
    posd = torch.as_tensor(pos).to(gpu)

    def call(n_hap, m, path):
        return _lib.lib.ldx_ld_fgt_dev(p.alt.data_ptr(), p.acnt.data_ptr(), 129, n_hap, posd.data_ptr(), 1000, m, None, path,
                                       out.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert call(64, 0, 0) == -1 and call(64, 65, 0) == -1
    unsupported = call(64, 1, ops.PATHS["popcount"])
    assert unsupported not in (0, -1) and call(_lib.MAX_HAPS + 1, 1, 0) == unsupported
    assert call(64, 1, 0) == 0
    torch.cuda.synchronize()
    # one SNP: one block, rm = 0
    c1, _ = bx.panel((1, 64))
    one = ops.ld_blocks(pack(c1, gpu), np.array([5], dtype=np.int64), window_bp=300)
    assert one.left.tolist() == [0] and one.block_of.tolist() == [0] and (one.n_blocks, one.rm) == (1, 0)
    assert one.starts.tolist() == [0] and one.ends.tolist() == [0] and one.spans_bp.tolist() == [0]

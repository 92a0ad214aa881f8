"""GPU: the weighted sample products and the genetic relationship matrix (include/ldx.h, "weighted sample products") against their
numpy mirrors, bit for bit: over shapes that take one tile, a ragged slab, an off-diagonal tile with its mirror write and three
slabs; one SNP, just under a K-block, past a K-block; several stores; forced K slices; weights on every edge of the base-256
digits; panels without, with 3 % and with 50 % missing calls; the invariances; the special weights; the refusals."""
import numpy as np
import pytest

from ld_grm_exact import HOLES, MAX_W, N_IND, N_SLICES, N_SNPS, edge_weights, panel_codes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_CASES = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


def case(n_ind, n_snps, holes):
    """(codes, q, host S) of a case, computed once."""
    from ld_tools_amd import sample_wprod_host

    key = (n_ind, n_snps, holes)
    if key not in _CASES:
        codes = panel_codes(n_ind, n_snps, seed=1000 * n_ind + n_snps, holes=holes)
        q = edge_weights(n_snps, seed=n_ind + n_snps)
        want = sample_wprod_host(codes, q)
        want.setflags(write=False)
        _CASES[key] = (codes, q, want)
    return _CASES[key]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("holes", HOLES)
@pytest.mark.parametrize("n_ind", N_IND)
def test_sums_exact(gpu, n_ind, holes):
    from ld_tools_amd import PackedPanel, sample_wprod

    for n_snps in N_SNPS:
        codes, q, want = case(n_ind, n_snps, holes)
        panel = PackedPanel.from_codes(codes, gpu)
        for n_slices in N_SLICES:
            S = sample_wprod(panel, q, n_slices=n_slices)
            assert S.dtype == torch.int64 and tuple(S.shape) == (n_ind, n_ind)
            assert torch.equal(S, S.T), (n_snps, n_slices)
            assert np.array_equal(S.cpu().numpy(), want), (n_snps, n_slices)


@pytest.mark.parametrize("holes", ["none", "3%"])
def test_three_stores_and_two_halves(gpu, holes):
    """1300 SNPs in stores of 512: three stores, the last one ragged, on the accumulate path; out= over two halves of the SNPs."""
    from ld_tools_amd import LdxError, PackedPanel, sample_wprod

    codes, q, want = case(130, 1300, holes)
    panel = PackedPanel.from_codes(codes, gpu)
    assert np.array_equal(sample_wprod(panel, q, store_snps=512).cpu().numpy(), want)
    assert np.array_equal(sample_wprod(panel, torch.from_numpy(q).to(gpu), store_snps=512, n_slices=3).cpu().numpy(), want)
    first = np.arange(1300) < 601
    part = sample_wprod(panel, q, keep=first)
    both = sample_wprod(panel, q, keep=~first, out=part)
    assert both is part and np.array_equal(both.cpu().numpy(), want)
    part = sample_wprod(panel.select(snps=first), q[first])
    assert np.array_equal(sample_wprod(panel.select(snps=~first), q[~first], out=part).cpu().numpy(), want)
    # a bad out, weights out of range or of the wrong shape: refused before any launch, out untouched
    before = part.clone()
    for bad_out in (part.to(torch.int32), part[:, :-1], part[:-1, :-1].contiguous(), part.cpu()):
        with pytest.raises(LdxError):
            sample_wprod(panel, q, out=bad_out)
    for bad_q in (q.astype(np.int64), q[:-1], q[:, :2]):
        with pytest.raises(LdxError):
            sample_wprod(panel, bad_q, out=part)
    for value in (MAX_W + 1, -MAX_W - 1):
        bad = q.copy()
        bad[777, 1] = value
        for w in (bad, torch.from_numpy(bad).to(gpu)):
            with pytest.raises(LdxError):
                sample_wprod(panel, w, out=part)
    assert torch.equal(part, before)


def test_invariances(gpu):
    from ld_tools_amd import PackedPanel, sample_wprod, sample_wprod_host

    n_ind, n_snps = 130, 700
    codes, q, want = case(n_ind, n_snps, "3%")
    base = sample_wprod(PackedPanel.from_codes(codes, gpu), q)
    rng = np.random.default_rng(4)
    perm = rng.permutation(n_snps)                                                       # permuted SNPs, weights alike
    assert torch.equal(sample_wprod(PackedPanel.from_codes(codes[perm], gpu), q[perm]), base)
    swap = np.arange(2 * n_ind).reshape(n_ind, 2)
    flip = rng.random(n_ind) < 0.5
    swap[flip] = swap[flip][:, ::-1]
    assert torch.equal(sample_wprod(PackedPanel.from_codes(codes[:, swap.reshape(-1)], gpu), q), base)   # rephased genotypes
    mask = rng.random(n_snps) < 0.6                                                      # a keep mask
    kept = sample_wprod(PackedPanel.from_codes(codes, gpu), q, keep=mask)
    assert np.array_equal(kept.cpu().numpy(), sample_wprod_host(codes, q, keep=mask)) and not torch.equal(kept, base)
    assert torch.equal(kept, sample_wprod(PackedPanel.from_codes(codes[mask], gpu), q[mask]))


def test_special_weights(gpu):
    from ld_tools_amd import PackedPanel, sample_wprod
    from ld_tools_amd.ops import geno_planes_host

    n_ind, n_snps = 130, 700
    codes, _, _ = case(n_ind, n_snps, "none")
    panel = PackedPanel.from_codes(codes, gpu)
    mask = np.arange(n_snps) % 3 != 1
    ones = np.tile(np.array([[0, 0, 1]], dtype=np.int32), (n_snps, 1))
    S = sample_wprod(panel, ones, keep=mask).cpu().numpy()
    assert (S == int(mask.sum())).all()                                                  # q = (0, 0, 1): the kept SNPs, everywhere
    g, _ = geno_planes_host(codes)
    gg = np.tile(np.array([[1, 0, 0]], dtype=np.int32), (n_snps, 1))
    assert np.array_equal(sample_wprod(panel, gg).cpu().numpy(), g.T @ g)               # q = (1, 0, 0): G G^T
    # with missing calls q = (0, 0, 1) is N, and q = (0, 1, 0) the dosage sums over the jointly called
    codes, _, _ = case(n_ind, n_snps, "50%")
    panel = PackedPanel.from_codes(codes, gpu)
    g, c = geno_planes_host(codes)
    assert np.array_equal(sample_wprod(panel, ones).cpu().numpy(), c.T @ c)
    mid = np.tile(np.array([[0, 1, 0]], dtype=np.int32), (n_snps, 1))
    assert np.array_equal(sample_wprod(panel, mid).cpu().numpy(), g.T @ c + c.T @ g)


@pytest.mark.parametrize("holes", HOLES)
def test_grm_equals_the_host_mirror(gpu, holes):
    from ld_tools_amd import PackedPanel, ld_grm, ld_grm_from_sums, ld_grm_host, sample_counts

    n_ind, n_snps = 130, 700
    codes = panel_codes(n_ind, n_snps, seed=9, holes=holes)
    codes[5] = 0                                                                         # a monomorphic SNP
    panel = PackedPanel.from_codes(codes, gpu)
    keep = np.random.default_rng(2).random(n_snps) < 0.9
    minus0 = bits(np.float32(-0.0))
    for k, maf in ((None, None), (keep, 0.1)):
        want = ld_grm_host(codes, keep=k, maf_min=maf)
        res = ld_grm(panel, keep=k, maf_min=maf)
        assert res.exp == want.exp and res.n_live == want.n_live and 0 < res.n_live < n_snps
        assert np.array_equal(res.S.cpu().numpy(), want.S)
        N = res.N.cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(N, want.N)
        grm = res.grm().cpu().numpy()
        assert grm.dtype == np.float32 and np.array_equal(bits(grm), bits(want.grm()))
        assert np.array_equal(bits(grm), bits(grm.T))
        if holes == "none":
            assert (N == res.n_live).all()
        else:                                                                            # individual 1 has no call at all
            assert (N[1] == 0).all() and (bits(grm[1]) == minus0).all() and (bits(grm[:, 1]) == minus0).all()
    # N is sample_counts over the live SNPs
    from ld_tools_amd import geno_snp_counts, grm_weights

    live = grm_weights(geno_snp_counts(panel, keep=keep), None, 0.1)[2]
    assert torch.equal(res.counts.counts, sample_counts(panel, keep=live).counts)
    # two halves of the SNPs with the whole panel's exponent: the same integers, the same cells
    whole = ld_grm(panel)
    first = np.arange(n_snps) < 300
    part = ld_grm(panel.select(snps=first), exp=whole.exp)
    both = ld_grm(panel.select(snps=~first), out=part)
    assert both.exp == whole.exp and both.n_live == whole.n_live
    assert torch.equal(both.S, whole.S) and torch.equal(both.counts.counts, whole.counts.counts)
    assert torch.equal(both.grm().view(torch.int32), whole.grm().view(torch.int32))
    assert torch.equal(ld_grm_from_sums(both.S.cpu().numpy(), whole.N.cpu().numpy().astype(np.int64), whole.exp,
                                        device=gpu).view(torch.int32), whole.grm().view(torch.int32))


def test_cells_on_given_integers(gpu):
    from ld_tools_amd import grm_cell_host, ld_grm_from_sums

    rng = np.random.default_rng(11)
    S = rng.integers(-(1 << 58), 1 << 58, size=(33, 33))
    S[0, :4] = [0, (1 << 58) + 1, -(1 << 58) - 1, (1 << 53) + 1]
    N = rng.integers(0, 1 << 32, size=(33, 33))
    N[1, :3] = [0, 1, (1 << 32) - 1]
    for e in (-3, 0, 4, 17):
        got = ld_grm_from_sums(S, N, e, device=gpu).cpu().numpy()
        assert np.array_equal(bits(got), bits(grm_cell_host(S, N, e)))
    assert bits(got)[1, 0] == bits(np.float32(-0.0))


def test_argument_rules(gpu):
    """The documented codes, returned before any HIP call: the pointers are never followed."""
    from ld_tools_amd import _lib

    lib, ptr = _lib.lib, 0x1000
    E_ARG, E_UNSUPPORTED = -1, -3
    ws = lib.ldx_sample_wprod_workspace_bytes(100)
    assert ws == 384 * 16 and lib.ldx_sample_wprod_workspace_bytes(257) == 2 * ws
    wprod = lambda **kw: lib.ldx_sample_wprod_dev(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("store", ptr), ("tables", ptr), ("n_ind", 4), ("n_snps", 100), ("q", ptr), ("S", ptr), ("ld", 4), ("accumulate", 0),
        ("n_slices", 0), ("workspace", ptr), ("workspace_bytes", ws), ("stream", None))])
    big = _lib.WPROD_MAX_SLICE_SNPS
    for bad in (dict(store=None), dict(tables=None), dict(q=None), dict(S=None), dict(workspace=None), dict(n_ind=0), dict(n_snps=0),
                dict(ld=3), dict(workspace_bytes=ws - 1), dict(workspace=ptr + 8), dict(n_snps=257),
                dict(n_snps=big + 1, n_slices=1, workspace_bytes=1 << 40), dict(n_snps=2 * big + 1, n_slices=2, workspace_bytes=1 << 40),
                dict(n_snps=_lib.KING_MAX_STORE_SNPS + 1, workspace_bytes=1 << 40)):
        assert wprod(**bad) == E_ARG, bad
        assert b"ldx_sample_wprod_dev" in lib.ldx_last_error()
    assert wprod(n_ind=_lib.MAX_HAPS // 2 + 1, ld=_lib.MAX_HAPS) == E_UNSUPPORTED
    cells = lambda **kw: lib.ldx_grm_cells_dev(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("S", ptr), ("ld_s", 4), ("N", ptr), ("ld_n", 4), ("n_ind", 4), ("exp", 3), ("grm", ptr), ("ld_out", 4), ("stream", None))])
    for bad in (dict(S=None), dict(N=None), dict(grm=None), dict(n_ind=0), dict(ld_s=3), dict(ld_n=3), dict(ld_out=3),
                dict(exp=_lib.GRM_MAX_EXP + 1), dict(exp=-_lib.GRM_MAX_EXP - 1)):
        assert cells(**bad) == E_ARG, bad
        assert b"ldx_grm_cells_dev" in lib.ldx_last_error()

"""GPU: unphased LD by EM (ops.ld_em, ld_em_hits, ld_em_counts, ld_em_from_counts; include/ldx.h, "unphased LD by EM").

The kernel is checked in two halves that meet at the integers (S, H): ld_em_counts against integer GEMMs of the dosages
(every cell, across the kernel's edges), and the epilogue -- alone on lists through ld_em_from_counts, and inside the kernel,
which must give the list's cells bit for bit -- against the 60-digit oracle of tests/ld_em_exact.py:

    |cell - v| <= 2 ulp32(v) + 2^-40 at a near-best x (ties of two local maxima are accepted either way),
    -0.0f in both cells of a degenerate pair, NaN for a tuple that is no genotype table.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import fakevcf  # noqa: E402
import ld_em_exact as emx  # noqa: E402
import ld_rect_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

NEG0 = np.uint32(0x80000000)
SAMPLED_CELLS = 2000


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    from ld_tools_amd import _lib

    buf = C.create_string_buffer(64)
    _lib.check(_lib.lib.ldx_device_arch(0, buf, 64))
    assert buf.value.decode().startswith("gfx950"), buf.value
    return torch.device("cuda", 0)


def bits(t) -> np.ndarray:
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


_CASES = {}


def case(shape, n_hap, extremes=False):
    """(codes_i, codes_j, where, panel_i, panel_j, (N, a_i, a_j, S, H)) of one case, built once and left unchanged."""
    from ld_tools_amd import PackedPanel
    key = (shape, n_hap, extremes)
    if key not in _CASES:
        ci, cj, where = emx.panel(shape, n_hap, extremes=extremes)
        _CASES[key] = (ci, cj, where, PackedPanel.from_codes(ci), PackedPanel.from_codes(cj), emx.pair_counts(ci, cj))
    return _CASES[key]


def list_cells(n_ind, a_i, a_j, S, H):
    """ld_em_from_counts over a whole rectangle of oracle integers: (r bits, D' bits, x) as [n_i, n_j] host arrays."""
    from ld_tools_amd import ops
    A = np.broadcast_to(a_i[:, None], S.shape)
    B = np.broadcast_to(a_j[None, :], S.shape)
    r, d, x = ops.ld_em_from_counts(n_ind, A, B, S, H)
    return bits(r).reshape(S.shape), bits(d).reshape(S.shape), x.cpu().numpy().reshape(S.shape)


# ---- 1. the K loop: both counts, every cell --------------------------------------------------------------------------------
def test_count_cases_cover_what_they_must():
    assert sorted({h for _, h in emx.COUNT_CASES}) == [2, 254, 256, 258, 1008, 5008]
    assert {s for s, _ in emx.COUNT_CASES} == set(rc.SHAPES) | {s for s, _ in emx.TILE_CASES}
    # the workgroup tile is 128 x 128: one row / column past it in each direction
    assert any(s[0] == emx.TILE + 1 for s, _ in emx.COUNT_CASES) and any(s[1] == emx.TILE + 1 for s, _ in emx.COUNT_CASES)
    assert emx.WALK_CASE[0][0] == 32 * emx.TILE + 1


COUNTS = emx.COUNT_CASES + (emx.WALK_CASE, emx.BIG_CASE)


@pytest.mark.parametrize("shape,n_hap", COUNTS, ids=[f"{s[0]}x{s[1]}x{h}" for s, h in COUNTS])
def test_counts_equal_the_integer_oracle(gpu, shape, n_hap):
    from ld_tools_amd import ops
    big = (shape, n_hap) == emx.BIG_CASE
    _, _, where, pi, pj, (n_ind, a_i, a_j, S, H) = case(shape, n_hap, extremes=big)
    gs, gh = ops.ld_em_counts(pi, pj)
    assert gs.shape == shape and gh.shape == shape
    assert np.array_equal(gs.cpu().numpy().astype(np.int64), S)
    assert np.array_equal(gh.cpu().numpy().astype(np.int64), H)
    assert np.array_equal(pi.acnt.cpu().numpy()[:shape[0]].astype(np.int64), a_i)
    if big:
        assert int(S.max()) == 4 * n_ind == 20480 and int(H.max()) == n_ind == 5120
        assert S[3, where["all_alt"][0]] == 20480 and H[2, where["all_het"][0]] == 5120


# ---- 2. the epilogue alone -------------------------------------------------------------------------------------------------
def test_epilogue_on_the_exhaustive_tables(gpu):
    from ld_tools_amd import ops
    worst = 0
    for n in range(1, 6):
        tables = sorted(set(emx.live_tables(n)))
        cols = np.array(tables, dtype=np.int64)
        r, d, x = (t.cpu().numpy() for t in ops.ld_em_from_counts(n, cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3]))
        assert r.dtype == np.float32 and d.dtype == np.float32 and x.dtype == np.float64
        for k, t in enumerate(tables):
            sol = emx.solve(n, *t)
            assert 0.0 <= x[k] <= t[3]
            assert emx.cells_ok(sol, r[k], d[k]), (n, t, float(r[k]), float(d[k]), float(x[k]), [float(v) for v in sol.near_best])
        worst += len(tables)
    assert worst == 873            # the distinct tuples of the 1801 tables (tests/test_ld_em_host.py counts both)


def test_epilogue_degenerate_and_malformed_tuples(gpu):
    from ld_tools_amd import ops
    n = 3   # T = 6
    degenerate = [(0, 2, 0, 0), (6, 2, 4, 0), (2, 0, 0, 0), (3, 6, 6, 0), (0, 0, 0, 0), (6, 6, 12, 0), (0, 6, 0, 0)]
    malformed = [(2, 2, 2, 1), (7, 2, 0, 0), (2, 7, 0, 0), (2, 2, 4, 4), (1, 1, 3, 1), (2, 2, 0, 1), (5, 5, 2, 0), (1, 1, 4, 0)]
    for t in degenerate:
        assert emx.table(n, *t) is not None, t
    for t in malformed:
        assert emx.table(n, *t) is None, t
    cols = np.array(degenerate + malformed, dtype=np.int64)
    r, d, x = (t.cpu().numpy() for t in ops.ld_em_from_counts(n, cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3]))
    k = len(degenerate)
    assert (bits(r[:k]) == NEG0).all() and (bits(d[:k]) == NEG0).all() and (x[:k] == 0.0).all()   # the sign bit too
    assert np.isnan(r[k:]).all() and np.isnan(d[k:]).all() and np.isnan(x[k:]).all()


# ---- 3. dense cells --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n_hap", emx.DENSE_CASES, ids=[f"{s[0]}x{s[1]}x{h}" for s, h in emx.DENSE_CASES])
def test_dense_cells(gpu, shape, n_hap):
    from ld_tools_amd import ops
    _, _, where, pi, pj, (n_ind, a_i, a_j, S, H) = case(shape, n_hap)
    T = 2 * n_ind
    out = ops.ld_em(pi, pj)
    assert out.r.shape == shape and out.dprime.shape == shape
    rb, db = bits(out.r), bits(out.dprime)
    # the kernel's epilogue is the list's: every cell, bit for bit, from the oracle's integers
    lr, ld_, _ = list_cells(n_ind, a_i, a_j, S, H)
    assert np.array_equal(rb, lr) and np.array_equal(db, ld_)
    # degenerate pairs: -0.0f in both, and nowhere else
    deg = ((a_i == 0) | (a_i == T))[:, None] | ((a_j == 0) | (a_j == T))[None, :]
    assert deg.any() and np.array_equal(rb == NEG0, deg) and np.array_equal(db == NEG0, deg)
    r, d = out.r.cpu().numpy(), out.dprime.cpu().numpy()
    assert not np.isnan(r).any() and not np.isnan(d).any() and (d[~deg] >= 0.0).all()
    # H = 0: r is +0.0f iff T n1 = a_i a_j
    phased = (H == 0) & ~deg
    zero = T * (S // 2) == np.multiply.outer(a_i, a_j)
    assert np.array_equal((rb == 0)[phased], zero[phased])
    # sampled cells against the oracle
    ii, jj = emx.sample_live(n_ind, a_i, a_j, S, H, SAMPLED_CELLS, seed=shape[1] + n_hap)
    assert ii.size == min(SAMPLED_CELLS, int((~deg).sum()))
    bad = [(int(i), int(j)) for i, j in zip(ii, jj)
           if not emx.cells_ok(emx.solve(n_ind, a_i[i], a_j[j], S[i, j], H[i, j]), r[i, j], d[i, j])]
    assert not bad, f"{len(bad)} of {ii.size} sampled cells off the oracle, the first at {bad[:3]}"
    # the planted pairs (side I's row 0 is side J's source row)
    dup, comp, het = where["duplicate"][0], where["complement"][0], where["all_het"][0]
    if n_hap > 2:   # (one individual: a heterozygous source ties with its copy, and the kernel may take either end)
        assert r[0, dup] == 1.0 and d[0, dup] == 1.0
        assert r[0, comp] == -1.0
    for kind in ("mono", "all_alt"):
        col = where[kind][0]
        assert (rb[:, col] == NEG0).all() and (db[:, col] == NEG0).all()
    live_rows = (a_i > 0) & (a_i < T)
    assert live_rows.any() and (rb[live_rows, het] != NEG0).all()          # all-het x ordinary: live


# ---- 4. invariances, bit for bit ----------------------------------------------------------------------------------------------
def test_rephased_panels_give_identical_cells(gpu):
    from ld_tools_amd import PackedPanel, ops
    shape, n_hap = (300, 130), 1008
    ci, cj, _, pi, pj, _ = case(shape, n_hap)
    qi, qj = emx.rephased(shape, n_hap)
    assert not np.array_equal(qi, ci) and not np.array_equal(qj, cj)
    a, b = ops.ld_em(pi, pj), ops.ld_em(PackedPanel.from_codes(qi), PackedPanel.from_codes(qj))
    assert np.array_equal(bits(a.r), bits(b.r)) and np.array_equal(bits(a.dprime), bits(b.dprime))


def test_swapped_sides_are_bit_transposes_and_self_is_the_square(gpu):
    from ld_tools_amd import ops
    _, _, _, A, B, _ = case((129, 257), 256)
    ab, ba = ops.ld_em(A, B), ops.ld_em(B, A)
    assert np.array_equal(bits(ab.r), bits(ba.r).T) and np.array_equal(bits(ab.dprime), bits(ba.dprime).T)
    sq, same = ops.ld_em(B), ops.ld_em(B, B)
    assert sq.r.shape == (257, 257)
    assert np.array_equal(bits(sq.r), bits(same.r)) and np.array_equal(bits(sq.dprime), bits(same.dprime))
    assert np.array_equal(bits(sq.r), bits(sq.r).T) and np.array_equal(bits(sq.dprime), bits(sq.dprime).T)


# ---- 5. a homozygous panel: fully phased ----------------------------------------------------------------------------------
def test_homozygous_panel_matches_the_haplotype_rectangle(gpu):
    """Haplotype 2k + 1 copies haplotype 2k, no missing codes: H = 0 everywhere, the EM has nothing to resolve, and r is the
    haplotype r of the same panel -- within 6 float32 ulps of ld_rect's cell (its 4 plus this contract's 2)."""
    from ld_tools_amd import PackedPanel, ops
    ci, cj = emx.homozygous_codes(150, 300, seed=5), emx.homozygous_codes(131, 300, seed=6)
    ci[7], cj[9] = 0, 1                     # a monomorphic row, an all-ALT column
    cj[10] = ci[0]                          # a duplicate pair
    n_ind, a_i, a_j, S, H = emx.pair_counts(ci, cj)
    assert not H.any()
    pi, pj = PackedPanel.from_codes(ci), PackedPanel.from_codes(cj)
    out = ops.ld_em(pi, pj)
    r, d = out.r.cpu().numpy(), out.dprime.cpu().numpy()
    ref = ops.ld_rect(pi, pj, dosage=False).cpu().numpy()
    assert np.array_equal(bits(r) == NEG0, bits(ref) == NEG0)
    live = bits(ref) != NEG0
    assert np.array_equal(r[live] == 0.0, ref[live] == 0.0)
    nz = live & (ref != 0.0)
    err = np.abs(r[nz].astype(np.float64) - ref[nz].astype(np.float64)) / np.spacing(np.abs(ref[nz])).astype(np.float64)
    print(f"homozygous panel: {int(nz.sum())} cells, max distance from ld_rect {float(err.max()):.3f} float32 ulps")
    assert float(err.max()) <= 6.0
    assert r[0, 10] == 1.0 and d[0, 10] == 1.0
    # D' against the oracle's closed form (x* = 0)
    ii, jj = emx.sample_live(n_ind, a_i, a_j, S, H, 1500, seed=11)
    for i, j in zip(ii, jj):
        sol = emx.solve(n_ind, a_i[i], a_j[j], S[i, j], 0)
        assert sol.roots == [0] and emx.cells_ok(sol, r[i, j], d[i, j]), (i, j)


# ---- 6. hits -----------------------------------------------------------------------------------------------------------------
def test_hits_are_the_host_mirror_of_the_dense_cells(gpu):
    from ld_tools_amd import PackedPanel, ops
    shape, n_hap = rc.HITS_CASE
    ci, cj = rc.pair_codes(shape[0], shape[1], n_hap, seed=rc.pair_seed(shape, n_hap), family=rc.FAMILY)
    pi, pj = PackedPanel.from_codes(ci), PackedPanel.from_codes(cj)
    dense = ops.ld_em(pi, pj)
    r, d = dense.r.cpu().numpy(), dense.dprime.cpu().numpy()
    bound = ops.r2_bound(0.2)
    i, j = ops.rect_hits_host(r, bound)
    assert 256 < i.size <= r.size // 2

    def check(h, what):
        assert h.em and not h.dosage and len(h) == i.size and np.float32(h.bound) == np.float32(bound), what
        gi, gj, gr = h.pairs()
        assert np.array_equal(gi, i) and np.array_equal(gj, j), what
        assert np.array_equal(gr.view(np.uint32), bits(r[i, j])), what           # the dense r cell, bit for bit
        assert np.array_equal(bits(h.dprime), bits(d[i, j])), what               # ... and the dense D' cell
        offsets = np.zeros(shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(i, minlength=shape[0]), out=offsets[1:])
        assert np.array_equal(h.offsets.cpu().numpy().astype(np.int64), offsets), what

    check(ops.ld_em_hits(pi, pj, r2=0.2), "r2 >= 0.2")
    # a buffer of one batch: the first run reserves more than it holds, the re-run gives the same CSR
    check(ops.ld_em_hits(pi, pj, r2=0.2, hit_capacity=256), "r2 >= 0.2 from a 256-slot buffer")


# ---- 6b. panels WITH missing codes: the plain form counts a missing call as REF -----------------------------------------------
# The plain and the pairwise entries run one kernel template, so comparing them no longer guards the plain form where codes
# are missing.  By definition the plain cells of such a panel are those of the panel with every missing code replaced by REF
# on the host: same bytes from ld_em, ld_em_hits, ld_em_counts and ld_em_band.  A plain form that consulted the hole test, ref
# or rcnt would fail here.  Shapes: ragged rows and columns, more than one tile per side, a K tail.
REF_CASES = tuple((kind, shape, n_hap) for kind in ("holed", "mixed") for shape, n_hap in (((129, 257), 254), ((300, 130), 1008)))
_REF_PANELS = {}


def ref_case(kind, shape, n_hap):
    """(panel_i, panel_j) of the codes as they are and of the codes with every missing code set to REF, built once."""
    import ld_em_pairwise_exact as epx
    from ld_tools_amd import PackedPanel
    key = (kind, shape, n_hap)
    if key not in _REF_PANELS:
        ci, cj, _ = epx.panel(kind, shape, n_hap)
        assert ((ci > 1).any() or (ci < 0).any()) and ((cj > 1).any() or (cj < 0).any()), "the panel holds missing codes"
        as_ref = [np.where((c == 0) | (c == 1), c, 0).astype(c.dtype) for c in (ci, cj)]
        _REF_PANELS[key] = tuple(PackedPanel.from_codes(c) for c in (ci, cj, *as_ref))
    return _REF_PANELS[key]


def sorted_hits(h):
    i, j, r = h.pairs()
    order = np.lexsort((j, i))
    return i[order], j[order], np.asarray(r).view(np.uint32)[order], bits(h.dprime)[order]


@pytest.mark.parametrize("kind,shape,n_hap", REF_CASES, ids=[f"{k}-{s[0]}x{s[1]}x{h}" for k, s, h in REF_CASES])
def test_plain_forms_count_a_missing_code_as_ref(gpu, kind, shape, n_hap):
    from ld_tools_amd import ops
    pi, pj, qi, qj = ref_case(kind, shape, n_hap)
    got, want = ops.ld_em(pi, pj), ops.ld_em(qi, qj)
    assert got.r.shape == shape
    assert np.array_equal(bits(got.r), bits(want.r)) and np.array_equal(bits(got.dprime), bits(want.dprime))
    for g, w in zip(ops.ld_em_counts(pi, pj), ops.ld_em_counts(qi, qj)):
        assert g.shape == shape and np.array_equal(g.cpu().numpy(), w.cpu().numpy())
    hg, hw = ops.ld_em_hits(pi, pj, r2=0.2), ops.ld_em_hits(qi, qj, r2=0.2)
    assert len(hw) > 0 and len(hg) == len(hw)
    assert np.array_equal(hg.offsets.cpu().numpy(), hw.offsets.cpu().numpy())
    for g, w in zip(sorted_hits(hg), sorted_hits(hw)):
        assert np.array_equal(g, w)


def test_plain_band_counts_a_missing_code_as_ref(gpu):
    from ld_tools_amd import ops
    p, _, q, _ = ref_case("mixed", (300, 130), 1008)
    got, want = ops.ld_em_band(p, window_snps=40), ops.ld_em_band(q, window_snps=40)
    assert got.n_cells == want.n_cells > 0
    for g, w in ((got.r, want.r), (got.dprime, want.dprime)):
        assert np.array_equal(g.lo.cpu().numpy(), w.lo.cpu().numpy())
        assert np.array_equal(g.offsets.cpu().numpy(), w.offsets.cpu().numpy())
        assert np.array_equal(bits(g.values), bits(w.values)) and np.array_equal(bits(g.diag), bits(w.diag))
    assert np.array_equal(got.live.cpu().numpy(), want.live.cpu().numpy())


# ---- 7. outputs ------------------------------------------------------------------------------------------------------------
def test_outputs_keep_their_surroundings_and_one_may_be_left_out(gpu):
    import torch
    from ld_tools_amd import ops
    shape, n_hap = (300, 130), 1008
    _, _, _, pi, pj, _ = case(shape, n_hap)
    n_i, n_j = shape
    want = ops.ld_em(pi, pj)
    fill = 0x7FC12345   # a quiet NaN with a payload no kernel produces
    bufs = [torch.full((n_i + 3, n_j + 5), fill, dtype=torch.int32, device=gpu).view(torch.float32) for _ in range(2)]
    got = ops.ld_em(pi, pj, out_r=bufs[0][:n_i], out_dprime=bufs[1][:n_i])
    assert got.r.data_ptr() == bufs[0].data_ptr() and got.dprime.data_ptr() == bufs[1].data_ptr()
    for buf, ref in zip(bufs, (want.r, want.dprime)):
        b = bits(buf)
        assert (b[:, n_j:] == fill).all() and (b[n_i:] == fill).all()
        assert np.array_equal(b[:n_i, :n_j], bits(ref))
    only_r = ops.ld_em(pi, pj, want_dprime=False)
    only_d = ops.ld_em(pi, pj, want_r=False)
    assert only_r.dprime is None and only_d.r is None
    assert np.array_equal(bits(only_r.r), bits(want.r)) and np.array_equal(bits(only_d.dprime), bits(want.dprime))


# ---- 8. argument rules -----------------------------------------------------------------------------------------------------
def test_argument_rules(gpu):
    import torch
    from ld_tools_amd import _lib
    lib = _lib.lib
    _, _, _, pi, pj, _ = case((129, 257), 256)
    n_i, n_j, h = 129, 257, 256
    out = torch.empty((n_i, n_j), dtype=torch.float32, device=gpu)
    words = torch.empty((n_i, n_j), dtype=torch.int32, device=gpu)
    hits = torch.empty((256, 4), dtype=torch.int32, device=gpu)
    n_hits = torch.zeros(1, dtype=torch.int64, device=gpu)
    ai, ci_, aj, cj_ = pi.alt.data_ptr(), pi.acnt.data_ptr(), pj.alt.data_ptr(), pj.acnt.data_ptr()
    o, w, hp, nh = out.data_ptr(), words.data_ptr(), hits.data_ptr(), n_hits.data_ptr()

    who = ""

    def refused(rc_, code, message):
        """the code and the WHOLE message, word for word (callers match on the words)"""
        assert rc_ == code, (rc_, code, message)
        assert lib.ldx_last_error().decode() == f"{who}: {message}"

    E_ARG, E_UNSUPPORTED = -1, -3
    assert _lib.E_NAMES[E_ARG] == "LDX_E_ARG" and _lib.E_NAMES[E_UNSUPPORTED] == "LDX_E_UNSUPPORTED"
    null, odd = "{} is a null pointer", "n_hap 255 is odd (haplotypes 2k and 2k + 1 are the two alleles of individual k)"
    plane = "{} is a bit plane of 4 GiB or more (4194304 SNPs x 10240 haplotypes)"
    bound = "r2_bound must be a float32 > 0 (got {})"
    dense, who = lib.ldx_ld_em_rect_dev, "ldx_ld_em_rect_dev"
    refused(dense(None, ci_, n_i, aj, cj_, n_j, h, o, o, n_j, None), E_ARG, null.format("alt_i"))
    refused(dense(ai, None, n_i, aj, cj_, n_j, h, o, o, n_j, None), E_ARG, null.format("acnt_i"))
    refused(dense(ai, ci_, n_i, None, cj_, n_j, h, o, o, n_j, None), E_ARG, null.format("alt_j"))
    refused(dense(ai, ci_, n_i, aj, None, n_j, h, o, o, n_j, None), E_ARG, null.format("acnt_j"))
    refused(dense(ai, ci_, n_i, aj, cj_, n_j, h, None, None, n_j, None), E_ARG, "out_r and out_dprime are both null pointers")
    refused(dense(ai, ci_, 0, aj, cj_, n_j, h, o, o, n_j, None), E_ARG, "n_i is 0")
    refused(dense(ai, ci_, n_i, aj, cj_, 0, h, o, o, n_j, None), E_ARG, "n_j is 0")
    refused(dense(ai, ci_, n_i, aj, cj_, n_j, h, o, o, n_j - 1, None), E_ARG, "ld_out 256 < n_j 257")
    refused(dense(ai, ci_, n_i, aj, cj_, n_j, 255, o, o, n_j, None), E_ARG, odd)
    refused(dense(ai, ci_, n_i, aj, cj_, n_j, 10242, o, o, n_j, None), E_UNSUPPORTED, "n_hap 10242 > LDX_MAX_HAPS 10240")
    refused(dense(ai, ci_, 1 << 22, aj, cj_, n_j, 10240, o, o, n_j, None), E_UNSUPPORTED, plane.format("alt_i"))   # a 5 GiB plane
    refused(dense(ai, ci_, n_i, aj, cj_, 1 << 22, 10240, o, o, 1 << 22, None), E_UNSUPPORTED, plane.format("alt_j"))
    refused(dense(ai, ci_, 1 << 26, aj, cj_, 1 << 26, 64, o, o, 1 << 26, None), E_UNSUPPORTED,
            "n_i x n_j = 67108864 x 67108864 needs 2^31 or more tiles of 128 x 128")
    refused(dense(ai, ci_, 0, aj, cj_, 0, 255, o, o, n_j, None), E_ARG, "n_i is 0")   # the first broken rule speaks
    hit, who = lib.ldx_ld_em_rect_hits_dev, "ldx_ld_em_rect_hits_dev"
    refused(hit(ai, ci_, n_i, aj, cj_, n_j, h, 0.0, hp, 256, nh, None), E_ARG, bound.format("0"))
    refused(hit(ai, ci_, n_i, aj, cj_, n_j, h, float("nan"), hp, 256, nh, None), E_ARG, bound.format("nan"))
    refused(hit(ai, ci_, n_i, aj, cj_, n_j, h, 0.2, None, 256, nh, None), E_ARG, "hits is a null pointer but hit_cap is 256")
    refused(hit(ai, ci_, n_i, aj, cj_, n_j, h, 0.2, hp, 256, None, None), E_ARG, null.format("n_hits"))
    refused(hit(ai, ci_, n_i, aj, cj_, n_j, 255, 0.2, hp, 256, nh, None), E_ARG, odd)
    refused(hit(ai, ci_, n_i, aj, cj_, n_j, 255, 0.0, None, 256, None, None), E_ARG, null.format("n_hits"))
    cnt, who = lib.ldx_ld_em_counts_dev, "ldx_ld_em_counts_dev"
    refused(cnt(None, n_i, aj, n_j, h, w, w, n_j, None), E_ARG, null.format("alt_i"))
    refused(cnt(ai, n_i, aj, n_j, h, None, w, n_j, None), E_ARG, null.format("S"))
    refused(cnt(ai, n_i, aj, n_j, h, w, None, n_j, None), E_ARG, null.format("H"))
    refused(cnt(ai, n_i, aj, n_j, h, w, w, n_j - 1, None), E_ARG, "ld 256 < n_j 257")
    refused(cnt(ai, n_i, aj, n_j, 10242, w, w, n_j, None), E_UNSUPPORTED, "n_hap 10242 > LDX_MAX_HAPS 10240")
    lst, who = lib.ldx_ld_em_from_counts_dev, "ldx_ld_em_from_counts_dev"
    refused(lst(3, 4, None, w, w, w, o, o, None, None), E_ARG, null.format("a1"))
    refused(lst(3, 0, w, w, w, w, o, o, None, None), E_ARG, "m is 0")
    refused(lst(0, 4, w, w, w, w, o, o, None, None), E_ARG, "n_ind is 0")
    refused(lst(5121, 4, w, w, w, w, o, o, None, None), E_UNSUPPORTED, "n_ind 5121 > LDX_MAX_HAPS / 2 = 5120")
    # the Python layer's own rules
    from ld_tools_amd import PackedPanel, ops
    odd = PackedPanel.from_codes(rc.random_codes(4, 255, np.random.default_rng(1)))
    with pytest.raises(_lib.LdxError, match="even"):
        ops.ld_em(odd)
    with pytest.raises(_lib.LdxError, match="haplotype count"):
        ops.ld_em(pi, odd)
    with pytest.raises(_lib.LdxError, match="neither"):
        ops.ld_em(pi, pj, want_r=False, want_dprime=False)


# ---- 9. driver -------------------------------------------------------------------------------------------------------------
def test_em_driver(gpu, tmp_path):
    from ld_tools_amd import PackedPanel, ops
    from ld_tools_amd.drivers import em_hits, em_matrix, write_em_matrix, write_ld_table
    from ld_tools_amd.drivers.em import LD_HEADER
    from ld_tools_amd.drivers.rmatrix import VARIANTS_HEADER
    a, names = fakevcf.make_chromosome(chrom="6", n_variants=48, seed=11)
    b, _ = fakevcf.make_chromosome(chrom="7", n_variants=37, seed=23, first_pos=5000, step=211)
    vcf = fakevcf.FakeVcf(a.records + b.records)

    def rs_rows(chrom):
        seen, rows = set(), []
        for rec in vcf.records:
            if rec.chrom == chrom and rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
                seen.add(rec.id)
                rows.append([rec.pos, rec.id])
        return rows

    rows_i, rows_j = rs_rows("6"), rs_rows("7")
    m = em_matrix(vcf, "6", rows_i, "7", rows_j, names)
    assert (m.rows.n, m.cols.n) == (len(rows_i), len(rows_j))
    want = ops.ld_em(PackedPanel.from_codes(m.rows.codes), PackedPanel.from_codes(m.cols.codes))
    assert np.array_equal(bits(m.r), bits(want.r)) and np.array_equal(bits(m.dprime), bits(want.dprime))
    base = str(tmp_path / "chr6_chr7_em")
    paths = write_em_matrix(base, m, rows_per_block=7)
    assert paths == [base + ".r.npy", base + ".dprime.npy", base + ".rows.tsv", base + ".cols.tsv"]
    for path, ref in zip(paths[:2], (m.r, m.dprime)):
        got = np.load(path)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), bits(ref))
    for path, side in zip(paths[2:], (m.rows, m.cols)):
        lines = Path(path).read_text().splitlines(keepends=True)
        assert lines[0] == VARIANTS_HEADER and len(lines) == side.n + 1
        assert [ln.split("\t")[1] for ln in lines[1:]] == side.rs_ids
    # the .ld table: the hits of the dense cells, in (row, column) order
    side_i, side_j, hits = em_hits(vcf, "6", rows_i, "7", rows_j, names, r2=0.05)
    r, d = m.r.cpu().numpy(), m.dprime.cpu().numpy()
    i, j = ops.rect_hits_host(r, ops.r2_bound(0.05))
    assert i.size and len(hits) == i.size
    table = str(tmp_path / "chr6_chr7.ld")
    assert write_ld_table(table, side_i, side_j, hits) == i.size
    lines = Path(table).read_text().splitlines(keepends=True)
    assert lines[0] == LD_HEADER == "SNP_A\tSNP_B\tR2\tDP\n" and len(lines) == i.size + 1
    for ln, a_, b_ in zip(lines[1:], i.tolist(), j.tolist()):
        rv = float(r[a_, b_])
        assert ln == f"{side_i.rs_ids[a_]}\t{side_j.rs_ids[b_]}\t{rv * rv:.6f}\t{float(d[a_, b_]):.6f}\n"

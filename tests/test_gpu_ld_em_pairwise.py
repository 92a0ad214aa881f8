"""GPU: pairwise-complete EM (ops.ld_em / ld_em_hits / ld_em_counts with missing="pairwise", ld_em_from_counts with a per-tuple
N; include/ldx.h, "pairwise-complete EM").

As for ld_em, the kernel is checked in two halves that meet at the integers: ld_em_counts(missing="pairwise") against the
integer oracle of tests/ld_em_pairwise_exact.py (every cell, across the kernel's edges and both of its paths), and the
epilogue -- alone on lists through ld_em_from_counts, and inside the kernel, which must give the list's cells bit for bit --
against the 60-digit oracle of tests/ld_em_exact.py on the pair's own (N, A, B, S, H):

    |cell - v| <= 2 ulp32(v) + 2^-40 at a near-best x, -0.0f in both cells of a degenerate pair (N = 0 included).
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
import ld_em_pairwise_exact as epx  # noqa: E402
import ld_pairwise_exact as px  # noqa: E402
import ld_rect_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

PW = "pairwise"
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


def case(key, build):
    """(codes_i, codes_j, planted, panel_i, panel_j, counts) of one panel, built once and left unchanged."""
    from ld_tools_amd import PackedPanel
    if key not in _CASES:
        ci, cj, planted = build()
        _CASES[key] = (ci, cj, planted, PackedPanel.from_codes(ci), PackedPanel.from_codes(cj), epx.pair_counts(ci, cj))
    return _CASES[key]


def mixed_case(shape, n_hap, family=0):
    return case(("mixed", shape, n_hap, family), lambda: epx.mixed(shape, n_hap, family=family))


def dense_case(kind, shape, n_hap):
    return mixed_case(shape, n_hap) if kind == "mixed" else case((kind, shape, n_hap), lambda: epx.panel(kind, shape, n_hap))


def list_cells(counts):
    """ld_em_from_counts with a per-tuple N over a whole rectangle of oracle integers: (r bits, D' bits) [n_i, n_j]."""
    from ld_tools_amd import ops
    shape = counts.shape[1:]
    r, d, _ = ops.ld_em_from_counts(*(k.reshape(-1) for k in counts))
    return bits(r).reshape(shape), bits(d).reshape(shape)


def em_bits(pi, pj, **kw):
    from ld_tools_amd import ops
    out = ops.ld_em(pi, pj, **kw)
    return bits(out.r), bits(out.dprime)


def assert_cells_are_the_lists(pi, pj, counts, what):
    rb, db = em_bits(pi, pj, missing=PW)
    lr, ld_ = list_cells(counts)
    for name, got, want in (("r", rb, lr), ("D'", db, ld_)):
        off = np.argwhere(got != want)
        assert off.size == 0, f"{what}: {len(off)} {name} cells differ from the list epilogue, the first at {off[0].tolist()}"
    return rb, db


# ---- 1. the K loops: five integers, every cell ------------------------------------------------------------------------------
COUNTS = epx.COUNT_CASES + (epx.BIG_CASE,)


@pytest.mark.parametrize("shape,n_hap", COUNTS, ids=[f"{s[0]}x{s[1]}x{h}" for s, h in COUNTS])
def test_counts_equal_the_integer_oracle(gpu, shape, n_hap):
    from ld_tools_amd import ops
    big = (shape, n_hap) == epx.BIG_CASE
    _, _, _, pi, pj, want = case(("big",), epx.big) if big else mixed_case(shape, n_hap)
    got = ops.ld_em_counts(pi, pj, missing=PW)
    assert got.shape == (5,) + shape and str(got.dtype) == "torch.int32"
    got = got.cpu().numpy().astype(np.int64)
    for s, name in enumerate(epx.SETS):
        off = np.argwhere(got[s] != want[s])
        assert off.size == 0, f"{name}: {len(off)} cells differ, the first at {off[0].tolist()}"
    if big:
        N, A, B, S, H = want
        assert N.max() == 5120 and S[epx.ROW_ALT, epx.ROW_ALT] == 20480 and H[epx.ROW_HET, epx.ROW_HET] == 5120
        assert A[epx.ROW_ALT].max() == 10240 and B[:, epx.ROW_ALT].max() == 10240


# ---- 2. the epilogue alone ------------------------------------------------------------------------------------------------
def test_epilogue_with_a_per_tuple_n_is_the_scalar_form(gpu):
    from ld_tools_amd import ops
    rng = np.random.default_rng(5)
    for n in (1, 3, 5):
        cols = np.array(sorted(set(emx.live_tables(n))), dtype=np.int64)
        # degenerate and malformed tuples ride along (T = 2 n)
        extra = np.array([(0, 1, 0, 0), (2 * n, 1, 2, 0), (1, 0, 0, 0), (2 * n, 2 * n, 4 * n, 0),     # degenerate
                          (2 * n + 1, 1, 0, 0), (1, 1, 3, 1), (1, 1, 4, 0), (1, 1, 0, 1)], dtype=np.int64)   # no table
        cols = np.concatenate([cols, extra])[rng.permutation(len(cols) + len(extra))]
        want = ops.ld_em_from_counts(n, cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3])
        got = ops.ld_em_from_counts(np.full(len(cols), n), cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3])
        for g, w in zip(got, want):
            g, w = g.cpu().numpy(), w.cpu().numpy()
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8))
        assert np.isnan(want[0].cpu().numpy()).sum() == 4
    # one list with many N: each tuple is the scalar form at its own N
    tuples = [(n,) + t for n in (1, 2, 4) for t in sorted(set(emx.live_tables(n)))[:40]]
    cols = np.array(tuples, dtype=np.int64)
    r, d, x = (t.cpu().numpy() for t in ops.ld_em_from_counts(cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3], cols[:, 4]))
    for n in (1, 2, 4):
        sel = cols[:, 0] == n
        wr, wd, wx = (t.cpu().numpy() for t in ops.ld_em_from_counts(n, cols[sel, 1], cols[sel, 2], cols[sel, 3], cols[sel, 4]))
        assert np.array_equal(bits(r[sel]), bits(wr)) and np.array_equal(bits(d[sel]), bits(wd)) and np.array_equal(x[sel], wx)


def test_epilogue_degenerate_and_malformed_tuples(gpu):
    from ld_tools_amd import ops
    degenerate = [(0, 0, 0, 0, 0), (3, 0, 2, 0, 0), (3, 6, 2, 4, 0), (3, 2, 0, 0, 0), (3, 3, 6, 6, 0), (1, 2, 2, 4, 0), (5120, 10240, 7, 14, 0)]
    malformed = [(0, 1, 0, 0, 0), (0, 0, 0, 1, 1), (3, 2, 2, 2, 1), (3, 7, 2, 0, 0), (3, 2, 2, 4, 4), (3, 1, 1, 3, 1), (2, 5, 5, 2, 0),
                 (5121, 2, 2, 0, 0), (0xFFFFFFFF, 2, 2, 0, 0)]
    for t in degenerate:
        assert emx.table(*t) is not None, t
    for t in malformed[:-2]:
        assert emx.table(*t) is None, t
    cols = np.array(degenerate + malformed, dtype=np.int64)
    r, d, x = (t.cpu().numpy() for t in ops.ld_em_from_counts(*(cols[:, k] for k in range(5))))
    k = len(degenerate)
    assert (bits(r[:k]) == NEG0).all() and (bits(d[:k]) == NEG0).all() and (x[:k] == 0.0).all()   # the sign bit too
    assert np.isnan(r[k:]).all() and np.isnan(d[k:]).all() and np.isnan(x[k:]).all()


# ---- 3. dense cells ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,n_hap", epx.DENSE_CASES, ids=[f"{k}-{s[0]}x{s[1]}x{h}" for k, s, h in epx.DENSE_CASES])
def test_dense_cells(gpu, kind, shape, n_hap):
    from ld_tools_amd import ops
    _, _, planted, pi, pj, counts = dense_case(kind, shape, n_hap)
    out = ops.ld_em(pi, pj, missing=PW)
    assert out.r.shape == shape and out.dprime.shape == shape
    # the kernel's epilogue is the list's: every cell, bit for bit, from the oracle's integers
    rb, db = assert_cells_are_the_lists(pi, pj, counts, f"{kind} {shape} x {n_hap}")
    # degenerate pairs: -0.0f in both, and nowhere else
    deg = epx.degenerate(counts)
    assert deg.any() and np.array_equal(rb == NEG0, deg) and np.array_equal(db == NEG0, deg)
    r, d = out.r.cpu().numpy(), out.dprime.cpu().numpy()
    assert not np.isnan(r).any() and not np.isnan(d).any() and (d[~deg] >= 0.0).all()
    if "disjoint" in planted:
        k = planted["disjoint"]
        assert counts[0][k, k] == 0 and deg[k, k]
    if "mono" in planted:
        k = planted["mono"]
        assert counts[0][k, k] > 0 and deg[k, k] and not deg[k].all()
    if "all_missing" in planted:
        row, col = planted["all_missing"]
        assert deg[row].all() and deg[:, col].all()
    if kind == "holed":     # side I's row 0 and the planted columns keep every call: the pair is the plain one
        dup, comp, het = planted["duplicate"][0], planted["complement"][0], planted["all_het"][0]
        assert r[0, dup] == 1.0 and d[0, dup] == 1.0 and r[0, comp] == -1.0
        assert not deg[~deg[:, dup], het].any()                 # all-het x a live row: live
    # sampled live cells against the oracle, each at its own N
    ii, jj = epx.sample_live(counts, SAMPLED_CELLS, seed=shape[1] + n_hap)
    assert ii.size == min(SAMPLED_CELLS, int((~deg).sum())) and ii.size > 0
    bad = [(int(i), int(j)) for i, j in zip(ii, jj)
           if not emx.cells_ok(emx.solve(*(int(v) for v in counts[:, i, j])), r[i, j], d[i, j])]
    assert not bad, f"{len(bad)} of {ii.size} sampled cells off the oracle, the first at {bad[:3]}"


# ---- 4. a panel without holes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n_hap", [((300, 130), 1008), ((129, 257), 254)])
def test_without_holes_the_cells_are_ld_ems(gpu, shape, n_hap):
    from ld_tools_amd import PackedPanel, ops
    ci, cj = px.complete_pair(shape, n_hap)
    assert px.complete_rows(ci).all() and px.complete_rows(cj).all()
    pi, pj = PackedPanel.from_codes(ci), PackedPanel.from_codes(cj)
    (r0, d0), (r1, d1) = em_bits(pi, pj), em_bits(pi, pj, missing=PW)
    assert np.array_equal(r0, r1) and np.array_equal(d0, d1)
    counts = ops.ld_em_counts(pi, pj, missing=PW).cpu().numpy().astype(np.int64)
    assert np.array_equal(counts, epx.pair_counts(ci, cj))     # the shortcut's N, A, B come from the tables


# ---- 5. four tile kinds in one launch ------------------------------------------------------------------------------------------
def test_tiles_with_and_without_holes_in_one_launch(gpu):
    from ld_tools_amd import ops
    ci, cj, _, pi, pj, counts = case(("tiles",), epx.tiles)
    shape, _ = epx.TILES_CASE
    clean_i, clean_j = px.complete_rows(ci), px.complete_rows(cj)
    # 128 x 128 tiles: rows [128, 256) of each side hold every hole
    assert clean_i[:128].all() and clean_i[256:].all() and not clean_i[128:256].all()
    assert clean_j[:128].all() and clean_j[256:].all() and not clean_j[128:256].all()
    got = ops.ld_em_counts(pi, pj, missing=PW).cpu().numpy().astype(np.int64)
    assert np.array_equal(got, counts)
    rb, db = assert_cells_are_the_lists(pi, pj, counts, "tiles")
    r0, d0 = em_bits(pi, pj)
    both = np.ix_(clean_i, clean_j)
    assert np.array_equal(rb[both], r0[both]) and np.array_equal(db[both], d0[both])
    assert not np.array_equal(rb, r0)                                # (elsewhere a hole counted as REF shows)


# ---- 6. invariances, bit for bit ----------------------------------------------------------------------------------------------
def test_swapped_sides_give_the_bit_transpose(gpu):
    _, _, _, pi, pj, _ = mixed_case((129, 257), 256)
    (rab, dab), (rba, dba) = em_bits(pi, pj, missing=PW), em_bits(pj, pi, missing=PW)
    assert np.array_equal(rab, rba.T) and np.array_equal(dab, dba.T)


def test_permuted_individuals_and_rephased_genotypes_give_identical_bits(gpu):
    from ld_tools_amd import PackedPanel
    shape, n_hap = (300, 130), 258
    ci, cj, _, pi, pj, _ = mixed_case(shape, n_hap)
    want = em_bits(pi, pj, missing=PW)
    both = np.concatenate([ci, cj])
    for what, other in (("permuted", px.permute_individuals(both, seed=31)), ("rephased", px.rephase(both, seed=32))):
        assert not np.array_equal(other, both), what
        qi, qj = np.ascontiguousarray(other[:shape[0]]), np.ascontiguousarray(other[shape[0]:])
        got = em_bits(PackedPanel.from_codes(qi), PackedPanel.from_codes(qj), missing=PW)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


# ---- 7. hits -----------------------------------------------------------------------------------------------------------------
def test_hits_are_the_host_mirror_of_the_dense_cells(gpu):
    from ld_tools_amd import ops
    shape, n_hap = rc.HITS_CASE
    _, _, _, pi, pj, _ = mixed_case(shape, n_hap, family=rc.FAMILY)
    dense = ops.ld_em(pi, pj, missing=PW)
    r, d = dense.r.cpu().numpy(), dense.dprime.cpu().numpy()
    bound = ops.r2_bound(0.2)
    i, j = ops.rect_hits_host(r, bound)            # ONE float32 multiply against the bound; -0.0f is never a hit
    assert 256 < i.size <= r.size // 2

    def check(h, what):
        assert h.em and not h.dosage and h.missing == PW and len(h) == i.size and np.float32(h.bound) == np.float32(bound), what
        gi, gj, gr = h.pairs()
        assert np.array_equal(gi, i) and np.array_equal(gj, j), what
        assert np.array_equal(gr.view(np.uint32), bits(r[i, j])), what           # the dense r cell, bit for bit
        assert np.array_equal(bits(h.dprime), bits(d[i, j])), what               # ... and the dense D' cell
        offsets = np.zeros(shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(i, minlength=shape[0]), out=offsets[1:])
        assert np.array_equal(h.offsets.cpu().numpy().astype(np.int64), offsets), what

    check(ops.ld_em_hits(pi, pj, r2=0.2, missing=PW), "r2 >= 0.2")
    # a buffer of one batch: the first run reserves more than it holds, the re-run gives the same CSR
    check(ops.ld_em_hits(pi, pj, r2=0.2, missing=PW, hit_capacity=256), "r2 >= 0.2 from a 256-slot buffer")


# ---- 8. the walk ----------------------------------------------------------------------------------------------------------------
def test_walk_past_one_band_against_the_list_epilogue(gpu):
    ci, cj, planted, pi, pj, counts = case(("walk",), epx.walk)
    assert (ci.shape[0], cj.shape[0]) == epx.WALK_CASE[0] and planted == {"rows": [4096], "cols": [77]}
    clean_i, clean_j = px.complete_rows(ci), px.complete_rows(cj)
    assert clean_i[:-1].all() and not clean_i[-1] and clean_j.sum() == cj.shape[0] - 1 and not clean_j[77]
    assert_cells_are_the_lists(pi, pj, counts, "walk")


# ---- 9. outputs ------------------------------------------------------------------------------------------------------------
def test_outputs_keep_their_surroundings_and_one_may_be_left_out(gpu):
    import torch
    from ld_tools_amd import ops
    shape, n_hap = (300, 130), 258
    _, _, _, pi, pj, _ = mixed_case(shape, n_hap)
    n_i, n_j = shape
    want = ops.ld_em(pi, pj, missing=PW)
    fill = 0x7FC12345   # a quiet NaN with a payload no kernel produces
    bufs = [torch.full((n_i + 3, n_j + 5), fill, dtype=torch.int32, device=gpu).view(torch.float32) for _ in range(2)]
    got = ops.ld_em(pi, pj, out_r=bufs[0][:n_i], out_dprime=bufs[1][:n_i], missing=PW)
    assert got.r.data_ptr() == bufs[0].data_ptr() and got.dprime.data_ptr() == bufs[1].data_ptr()
    for buf, ref in zip(bufs, (want.r, want.dprime)):
        b = bits(buf)
        assert (b[:, n_j:] == fill).all() and (b[n_i:] == fill).all()
        assert np.array_equal(b[:n_i, :n_j], bits(ref))
    only_r = ops.ld_em(pi, pj, want_dprime=False, missing=PW)
    only_d = ops.ld_em(pi, pj, want_r=False, missing=PW)
    assert only_r.dprime is None and only_d.r is None
    assert np.array_equal(bits(only_r.r), bits(want.r)) and np.array_equal(bits(only_d.dprime), bits(want.dprime))


# ---- 10. argument rules ------------------------------------------------------------------------------------------------------
def test_argument_rules(gpu):
    import torch
    from ld_tools_amd import PackedPanel, _lib, ops
    lib = _lib.lib
    _, _, _, pi, pj, _ = mixed_case((129, 257), 256)
    n_i, n_j, h = 129, 257, 256
    out = torch.empty((n_i, n_j), dtype=torch.float32, device=gpu)
    words = torch.empty((5, n_i, n_j), dtype=torch.int32, device=gpu)
    hits = torch.empty((256, 4), dtype=torch.int32, device=gpu)
    n_hits = torch.zeros(1, dtype=torch.int64, device=gpu)
    si = [pi.alt.data_ptr(), pi.ref.data_ptr(), pi.acnt.data_ptr(), pi.rcnt.data_ptr()]
    sj = [pj.alt.data_ptr(), pj.ref.data_ptr(), pj.acnt.data_ptr(), pj.rcnt.data_ptr()]
    o, w, hp, nh = out.data_ptr(), words.data_ptr(), hits.data_ptr(), n_hits.data_ptr()
    names = ("alt", "ref", "acnt", "rcnt")
    who = ""

    def refused(rc_, code, message):
        """the code and the WHOLE message, word for word (callers match on the words)"""
        assert rc_ == code, (rc_, code, message)
        assert lib.ldx_last_error().decode() == f"{who}: {message}"

    def without(side, k):
        return side[:k] + [None] + side[k + 1:]

    E_ARG, E_UNSUPPORTED = -1, -3
    assert _lib.E_NAMES[E_ARG] == "LDX_E_ARG" and _lib.E_NAMES[E_UNSUPPORTED] == "LDX_E_UNSUPPORTED"
    null, odd = "{} is a null pointer", "n_hap 255 is odd (haplotypes 2k and 2k + 1 are the two alleles of individual k)"
    plane = "{} is a bit plane of 4 GiB or more (4194304 SNPs x 10240 haplotypes)"
    bound = "r2_bound must be a float32 > 0 (got {})"
    dense, who = lib.ldx_ld_em_rect_pw_dev, "ldx_ld_em_rect_pw_dev"
    for k, name in enumerate(names):
        refused(dense(*without(si, k), n_i, *sj, n_j, h, o, o, n_j, None), E_ARG, null.format(name + "_i"))
        refused(dense(*si, n_i, *without(sj, k), n_j, h, o, o, n_j, None), E_ARG, null.format(name + "_j"))
    refused(dense(*si, n_i, *sj, n_j, h, None, None, n_j, None), E_ARG, "out_r and out_dprime are both null pointers")
    refused(dense(*si, 0, *sj, n_j, h, o, o, n_j, None), E_ARG, "n_i is 0")
    refused(dense(*si, n_i, *sj, 0, h, o, o, n_j, None), E_ARG, "n_j is 0")
    refused(dense(*si, n_i, *sj, n_j, h, o, o, n_j - 1, None), E_ARG, "ld_out 256 < n_j 257")
    refused(dense(*si, n_i, *sj, n_j, 255, o, o, n_j, None), E_ARG, odd)
    refused(dense(*si, n_i, *sj, n_j, 10242, o, o, n_j, None), E_UNSUPPORTED, "n_hap 10242 > LDX_MAX_HAPS 10240")
    refused(dense(*si, 1 << 22, *sj, n_j, 10240, o, o, n_j, None), E_UNSUPPORTED, plane.format("alt_i"))   # a 5 GiB plane
    refused(dense(*si, n_i, *sj, 1 << 22, 10240, o, o, 1 << 22, None), E_UNSUPPORTED, plane.format("alt_j"))
    refused(dense(*si, 1 << 26, *sj, 1 << 26, 64, o, o, 1 << 26, None), E_UNSUPPORTED,
            "n_i x n_j = 67108864 x 67108864 needs 2^31 or more tiles of 128 x 128")
    hit, who = lib.ldx_ld_em_rect_pw_hits_dev, "ldx_ld_em_rect_pw_hits_dev"
    refused(hit(*si, n_i, *sj, n_j, h, 0.0, hp, 256, nh, None), E_ARG, bound.format("0"))
    refused(hit(*si, n_i, *sj, n_j, h, float("nan"), hp, 256, nh, None), E_ARG, bound.format("nan"))
    refused(hit(*si, n_i, *sj, n_j, h, 0.2, None, 256, nh, None), E_ARG, "hits is a null pointer but hit_cap is 256")
    refused(hit(*si, n_i, *sj, n_j, h, 0.2, hp, 256, None, None), E_ARG, null.format("n_hits"))
    refused(hit(*without(si, 1), n_i, *sj, n_j, h, 0.2, hp, 256, nh, None), E_ARG, null.format("ref_i"))
    refused(hit(*si, n_i, *sj, n_j, 255, 0.2, hp, 256, nh, None), E_ARG, odd)
    cnt, who = lib.ldx_ld_em_pw_counts_dev, "ldx_ld_em_pw_counts_dev"
    refused(cnt(*without(si, 3), n_i, *sj, n_j, h, w, n_j, None), E_ARG, null.format("rcnt_i"))
    refused(cnt(*si, n_i, *sj, n_j, h, None, n_j, None), E_ARG, null.format("counts"))
    refused(cnt(*si, n_i, *sj, n_j, h, w, n_j - 1, None), E_ARG, "ld 256 < n_j 257")
    refused(cnt(*si, n_i, *sj, n_j, 255, w, n_j, None), E_ARG, odd)
    refused(cnt(*si, n_i, *sj, n_j, 10242, w, n_j, None), E_UNSUPPORTED, "n_hap 10242 > LDX_MAX_HAPS 10240")
    lst, who = lib.ldx_ld_em_from_counts_pw_dev, "ldx_ld_em_from_counts_pw_dev"
    refused(lst(4, None, w, w, w, w, o, o, None, None), E_ARG, null.format("N"))
    refused(lst(4, w, w, w, w, None, o, o, None, None), E_ARG, null.format("H"))
    refused(lst(0, w, w, w, w, w, o, o, None, None), E_ARG, "m is 0")
    # the Python layer's own rules, before the device is touched
    odd_panel = PackedPanel.from_codes(rc.random_codes(4, 255, np.random.default_rng(1)))
    for fn in (ops.ld_em, ops.ld_em_hits, ops.ld_em_counts):
        with pytest.raises(_lib.LdxError, match="even"):
            fn(odd_panel, missing=PW)
        with pytest.raises(_lib.LdxError, match='missing must be None or "pairwise"'):
            fn(pi, pj, missing="complete")
        with pytest.raises(_lib.LdxError, match="haplotype count"):
            fn(pi, odd_panel, missing=PW)
    with pytest.raises(_lib.LdxError, match="differ in length"):
        ops.ld_em_from_counts(np.array([3, 3]), [2], [2], [2], [0])


# ---- 11. driver ------------------------------------------------------------------------------------------------------------
def test_em_driver_with_missing_calls(gpu):
    from ld_tools_amd import ops
    from ld_tools_amd.drivers import em_hits, em_matrix
    a, names = fakevcf.make_chromosome(chrom="6", n_variants=48, seed=11)
    b, _ = fakevcf.make_chromosome(chrom="7", n_variants=37, seed=23, first_pos=5000, step=211)
    vcf = fakevcf.FakeVcf(a.records + b.records)
    carried = [n for n in names if n in vcf.records[0].samples]
    for k, rec in enumerate(vcf.records):          # ./. calls, and one half-missing call
        if k % 3 == 1:
            rec.samples[carried[k % len(carried)]] = {"GT": (None, None)}
    vcf.records[2].samples[carried[3]] = {"GT": (None, 1)}

    def rs_rows(chrom):
        seen, rows = set(), []
        for rec in vcf.records:
            if rec.chrom == chrom and rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
                seen.add(rec.id)
                rows.append([rec.pos, rec.id])
        return rows

    rows_i, rows_j = rs_rows("6"), rs_rows("7")
    m = em_matrix(vcf, "6", rows_i, "7", rows_j, names, missing=PW)
    ci, cj = m.rows.codes, m.cols.codes
    assert (m.rows.n, m.cols.n) == (len(rows_i), len(rows_j))
    called_i = np.isin(ci, (0, 1))
    assert (~called_i[:, 0::2] & ~called_i[:, 1::2]).any() and (called_i[:, 0::2] != called_i[:, 1::2]).any()
    assert not px.complete_rows(cj).all()
    counts = epx.pair_counts(ci, cj)
    lr, ld_ = list_cells(counts)
    assert np.array_equal(bits(m.r), lr) and np.array_equal(bits(m.dprime), ld_)
    r, d = m.r.cpu().numpy(), m.dprime.cpu().numpy()
    ii, jj = epx.sample_live(counts, 400, seed=3)
    assert ii.size == 400
    for i, j in zip(ii, jj):
        assert emx.cells_ok(emx.solve(*(int(v) for v in counts[:, i, j])), r[i, j], d[i, j]), (i, j)
    plain = em_matrix(vcf, "6", rows_i, "7", rows_j, names)
    assert not np.array_equal(bits(plain.r), bits(m.r))                       # a missing call counted as REF shows
    side_i, side_j, hits = em_hits(vcf, "6", rows_i, "7", rows_j, names, r2=0.05, missing=PW)
    i, j = ops.rect_hits_host(r, ops.r2_bound(0.05))
    gi, gj, gr = hits.pairs()
    assert i.size and hits.missing == PW and np.array_equal(gi, i) and np.array_equal(gj, j)
    assert np.array_equal(gr.view(np.uint32), bits(r[i, j])) and np.array_equal(bits(hits.dprime), bits(d[i, j]))

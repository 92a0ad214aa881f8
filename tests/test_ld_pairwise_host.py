"""CPU: pairwise-complete LD -- hand-computed cases of the definitions (include/ldx.h, "pairwise-complete LD"), the oracle
(tests/ld_pairwise_exact.py) against the plain oracles where no call is missing, the numpy mirrors (ops.pairwise_counts_host,
ops.pairwise_cell_host) against the oracle, the ABI of the three new entries, the argument rules that come before the device,
and the properties of the GPU tests' panels.  No kernel is launched here."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_dosage_exact as dx  # noqa: E402
import ld_exact as lx  # noqa: E402
import ld_pairwise_exact as px  # noqa: E402
import ld_rect_cases as rc  # noqa: E402

NEW_SYMBOLS = ["ldx_ld_rect_pw_dev", "ldx_ld_rect_pw_hits_dev", "ldx_ld_rect_pw_counts_dev"]
E_ARG, E_UNSUPPORTED = -1, -3
NEG0, POS0 = np.uint32(0x80000000), np.uint32(0)
M = 2   # a missing code


def codes(*rows):
    return np.array(rows, dtype=np.int8)


# ---- 1. the definitions, by hand ------------------------------------------------------------------------------------------
def test_haplotype_counts_and_cell_by_hand():
    from ld_tools_amd import ops
    #          h: 0  1  2  3  4  5  6  7
    x = codes([1, 1, 0, 0, 1, M, 0, 1])
    y = codes([1, 0, 0, M, 1, 1, M, 1])
    # jointly called: h = 0, 1, 2, 4, 7 -> n = 5; x = 1 there: 0, 1, 4, 7 -> a = 4; y = 1 there: 0, 4, 7 -> b = 3; both: 0, 4, 7
    k = ops.pairwise_counts_host(x, y)
    assert k.shape == (4, 1, 1) and k[:, 0, 0].tolist() == [5, 4, 3, 3]
    ex = px.PairwiseExactBlock(x, y)
    assert np.array_equal(ex.counts, k) and ex.names == ("n", "a", "b", "c")
    # num = 3 * 5 - 4 * 3 = 3, v_x = 4 * 1, v_y = 3 * 2, r = 3 / sqrt(24)
    assert int(ex.num[0, 0]) == 3 and int(ex.den2[0, 0]) == 24
    cell = ops.pairwise_cell_host(k)
    assert cell.dtype == np.float32 and cell.shape == (1, 1) and cell[0, 0] == np.float32(3.0 / np.sqrt(24.0))
    # the plain rectangle's r of the same two rows differs: n = 8, a = 4, b = 4, n11 = 3, rcnt 3 and 2
    plain = lx.ExactBlock(x, y)
    assert int(plain.num[0, 0]) == 8 and plain.r64[0, 0] != ex.r64[0, 0]


def test_dosage_counts_and_cell_by_hand():
    from ld_tools_amd import ops
    #   individual:  0     1     2     3     4     5
    x = codes([1, 1, 0, 1, M, 1, 0, 0, 1, 1, 1, 0])    # g = 2, 1, -(half-missing), 0, 2, 1
    y = codes([1, 0, 1, 1, 1, 1, M, M, 1, 1, 0, 0])    # g = 1, 2, 2, -, 2, 0
    # called at both: individuals 0, 1, 4, 5 -> N = 4; g_x = 2, 1, 2, 1 -> A = 6, HA = 2; g_y = 1, 2, 2, 0 -> B = 5, HB = 2
    # S = 2 + 2 + 4 + 0 = 8
    k = ops.pairwise_counts_host(x, y, dosage=True)
    assert k.shape == (6, 1, 1) and k[:, 0, 0].tolist() == [4, 6, 5, 2, 2, 8]
    ex = px.PairwiseExactBlock(x, y, dosage=True)
    assert np.array_equal(ex.counts, k) and ex.names == ("N", "A", "B", "HA", "HB", "S")
    # num = 8 * 4 - 6 * 5 = 2; v_x = 4 * (6 + 4) - 36 = 4; v_y = 4 * (5 + 4) - 25 = 11
    assert int(ex.num[0, 0]) == 2 and int(ex.v_x[0, 0]) == 4 and int(ex.v_y[0, 0]) == 11
    cell = ops.pairwise_cell_host(k, dosage=True)
    assert cell[0, 0] == np.float32(2.0 / np.sqrt(44.0))
    # missing = REF would count the half-missing individual's ALT allele: not this rule
    assert int(dx.DosageExactBlock(x, y).a_i[0]) == 7


def test_signed_zero_cells_by_hand():
    from ld_tools_amd import ops
    left, right = codes([1, 0, 1, 0, M, M, M, M]), codes([M, M, M, M, 1, 0, 0, 1])
    for dosage in (False, True):
        k = ops.pairwise_counts_host(left, right, dosage=dosage)
        assert int(k[0, 0, 0]) == 0 and not k.any()                                # disjoint called sets: n = 0 / N = 0
        assert ops.pairwise_cell_host(k, dosage).view(np.uint32)[0, 0] == NEG0
    # monomorphic within the partner's called set only
    x, y = codes([1, 1, 0, 0, 0, 0, 0, 0]), codes([M, M, 1, 0, 0, 1, 1, 0])
    assert ops.pairwise_cell_host(ops.pairwise_counts_host(x, y)).view(np.uint32)[0, 0] == NEG0
    assert ops.pairwise_cell_host(ops.pairwise_counts_host(x, x)).view(np.uint32)[0, 0] == np.float32(1.0).view(np.uint32)
    # num = 0 exactly: independent rows
    x, y = codes([1, 1, 0, 0, M, 1]), codes([1, 0, 1, 0, 1, M])
    assert ops.pairwise_cell_host(ops.pairwise_counts_host(x, y)).view(np.uint32)[0, 0] == POS0
    with pytest.raises(ops._lib.LdxError, match="even n_hap"):
        ops.pairwise_counts_host(codes([1, 0, 1]), codes([1, 0, 1]), dosage=True)
    with pytest.raises(ops._lib.LdxError, match="same haplotypes"):
        ops.pairwise_counts_host(codes([1, 0, 1, 0]), codes([1, 0, 1]))
    with pytest.raises(ops._lib.LdxError, match="count sets"):
        ops.pairwise_cell_host(np.zeros((4, 1, 1)), dosage=True)


# ---- 2. the oracle against the plain oracles, the mirrors against the oracle ------------------------------------------------
@pytest.mark.parametrize("shape,n_hap", [((129, 257), 256), ((300, 130), 254), ((5, 700), 1008)])
def test_oracle_without_holes_is_the_plain_oracle(shape, n_hap):
    ci, cj = px.complete_pair(shape, n_hap)
    for dosage, plain in ((False, lx.ExactBlock(ci, cj)), (True, dx.DosageExactBlock(ci, cj))):
        ex = px.PairwiseExactBlock(ci, cj, dosage)
        for name in ("num", "den2", "num2", "degenerate", "zero_num", "r64", "r2_64"):
            assert np.array_equal(getattr(ex, name), getattr(plain, name)), (dosage, name)
        assert (ex.counts[0] == (n_hap // 2 if dosage else n_hap)).all()


@pytest.mark.parametrize("shape,n_hap", [((129, 257), 2), ((300, 130), 258), ((5, 700), 1008), ((129, 257), 5008)])
def test_host_mirrors_equal_the_oracle(shape, n_hap):
    from ld_tools_amd import ops
    ci, cj, _ = px.mixed_pair(shape, n_hap)
    for dosage in (False, True):
        ex = px.PairwiseExactBlock(ci, cj, dosage)
        k = ops.pairwise_counts_host(ci, cj, dosage=dosage)
        assert k.dtype == np.int64 and np.array_equal(k, ex.counts)
        cell = ops.pairwise_cell_host(k, dosage)
        b = cell.view(np.uint32)
        assert np.array_equal(b == NEG0, ex.degenerate) and np.array_equal(b == POS0, ex.zero_num)
        rest = ~ex.degenerate & ~ex.zero_num
        if rest.any():
            assert float(lx.ulp32_err(cell[rest], ex.r64[rest]).max()) <= 0.5 + 2.0 ** -20   # fp64 throughout, one float32 rounding
        one = (ex.num2 == ex.den2) & ~ex.degenerate
        assert np.array_equal(cell[one], np.sign(ex.num[one]).astype(np.float32))


# ---- 3. the ABI and the argument rules --------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    from ld_tools_amd import _lib
    text = (ROOT / "include" / "ldx.h").read_text()
    assert "pairwise-complete LD" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ldx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/ldx.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libldx.so"
    assert _lib.version() == 102                                           # new symbols only: no version bump
    assert "#define LDX_VERSION 102" in (ROOT / "include" / "ldx.h").read_text().replace("  ", " ")
    import ld_tools_amd
    for name in ("ld_rect_counts", "pairwise_counts_host", "pairwise_cell_host"):
        assert name in ld_tools_amd.__all__ and hasattr(ld_tools_amd, name)


def test_entries_refuse_bad_arguments_before_any_launch():
    from ld_tools_amd import _lib
    lib = _lib.lib
    big = C.create_string_buffer(4096 + 256)
    ptr = (C.addressof(big) + 255) // 256 * 256   # a non-null stand-in for every pointer (never read)
    sides = ("alt_i", "ref_i", "acnt_i", "rcnt_i", "alt_j", "ref_j", "acnt_j", "rcnt_j")

    def call(entry, tail, **kw):
        a = {name: ptr for name in sides}
        a.update(n_i=100, n_j=50, n_hap=64, dosage=0)
        a.update(tail)
        a.update(kw)
        head = [a["alt_i"], a["ref_i"], a["acnt_i"], a["rcnt_i"], a["n_i"], a["alt_j"], a["ref_j"], a["acnt_j"], a["rcnt_j"],
                a["n_j"], a["n_hap"], a["dosage"]]
        return getattr(lib, entry)(*head, *[a[name] for name in tail], None)

    def dense(**kw):
        return call("ldx_ld_rect_pw_dev", dict(out=ptr, ld_out=50), **kw)

    def hits(**kw):
        return call("ldx_ld_rect_pw_hits_dev", dict(r2_bound=0.2, hits=ptr, hit_cap=256, n_hits=ptr), **kw)

    def counts(**kw):
        return call("ldx_ld_rect_pw_counts_dev", dict(counts=ptr, ld=50), **kw)

    who = {dense: "ldx_ld_rect_pw_dev", hits: "ldx_ld_rect_pw_hits_dev", counts: "ldx_ld_rect_pw_counts_dev"}

    def said(fn, message):
        return lib.ldx_last_error().decode() == f"{who[fn]}: {message}"

    for fn, extra in ((dense, ("out",)), (hits, ("n_hits",)), (counts, ("counts",))):
        for name in sides + extra:
            assert fn(**{name: None}) == E_ARG and said(fn, f"{name} is a null pointer"), lib.ldx_last_error()
        assert fn(n_i=0) == E_ARG and said(fn, "n_i is 0")
        assert fn(n_j=0) == E_ARG and said(fn, "n_j is 0")
        assert fn(n_hap=0) == E_ARG and said(fn, "n_hap is 0")
        for n_hap in (63, _lib.MAX_HAPS + 1):                                    # parity speaks before the limit
            assert fn(n_hap=n_hap, dosage=1) == E_ARG
            assert said(fn, f"n_hap {n_hap} is odd (dosage pairs haplotypes 2k and 2k + 1 into individuals)")
        assert fn(n_hap=63, n_i=0) == E_ARG and said(fn, "n_i is 0")             # an odd n_hap is fine for haplotype r
        assert fn(n_hap=_lib.MAX_HAPS + 2) == E_UNSUPPORTED and said(fn, "n_hap 10242 > LDX_MAX_HAPS 10240")
        assert fn(n_i=1 << 24, n_hap=10240) == E_UNSUPPORTED
        assert said(fn, "alt_i is a bit plane of 4 GiB or more (16777216 SNPs x 10240 haplotypes)")
    assert dense(ld_out=49) == E_ARG and said(dense, "ld_out 49 < n_j 50")
    assert counts(ld=49) == E_ARG and said(counts, "ld 49 < n_j 50")
    assert hits(hits=None) == E_ARG and said(hits, "hits is a null pointer but hit_cap is 256")
    for bad, shown in ((0.0, "0"), (-0.5, "-0.5"), (float("nan"), "nan")):
        assert hits(r2_bound=bad) == E_ARG and said(hits, f"r2_bound must be a float32 > 0 (got {shown})")


def test_python_argument_rules_come_before_the_device():
    import torch
    from ld_tools_amd import LdxError, PackedPanel, ops
    from ld_tools_amd.drivers import rect_matrix

    def host_panel(n_snps, n_hap):
        z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731
        return PackedPanel(n_snps, n_hap, z(1, torch.uint8), z(1, torch.uint8), z(128, torch.int32), z(128, torch.int32),
                           z(128, torch.float64), z(128, torch.float64), z(128, torch.float64))

    a, b, odd = host_panel(10, 64), host_panel(7, 62), host_panel(10, 63)
    for fn in (ops.ld_rect, ops.ld_rect_hits):
        for bad in ("ref", "complete", "Pairwise", 1, True, ""):
            with pytest.raises(LdxError, match="missing must be"):
                fn(a, a, missing=bad)
        with pytest.raises(LdxError, match="haplotype count"):
            fn(a, b, missing="pairwise")
        with pytest.raises(LdxError, match="even n_hap"):
            fn(odd, odd, dosage=True, missing="pairwise")
    with pytest.raises(LdxError, match="haplotype count"):
        ops.ld_rect_counts(a, b)
    with pytest.raises(LdxError, match="even n_hap"):
        ops.ld_rect_counts(odd, dosage=True)
    with pytest.raises(LdxError, match="missing must be"):
        rect_matrix(None, "6", [], "7", [], [], missing="ref")
    if not torch.cuda.is_available():                                       # valid arguments: only now the device is asked for
        for call in (lambda: ops.ld_rect(a, a, missing="pairwise"), lambda: ops.ld_rect_hits(a, a, missing="pairwise"),
                     lambda: ops.ld_rect_counts(a, a)):
            with pytest.raises(LdxError, match="HIP device"):
                call()
    h = ops.LDRectHits(None, None, 1, 1, np.float32(0.2))
    assert h.missing is None and h.dosage is False and h.em is False        # the new field has a default


# ---- 4. the GPU tests' panels -----------------------------------------------------------------------------------------------
def test_hits_panel_is_decided_by_the_oracle():
    """At r^2 = 0.2 the oracle leaves at most AMBIGUOUS_SHARE_MAX of the hits panel's pairs open (the planted rows sit near
    r^2 = 1 and 0.6, the rest near 0) and decides at least MIN_DECIDED_IN pairs in, in both forms."""
    shape, n_hap = rc.HITS_CASE
    ci, cj, _ = px.mixed_pair(shape, n_hap, family=rc.FAMILY)
    for dosage in (False, True):
        cls = px.PairwiseExactBlock(ci, cj, dosage).classes(px.HITS_R2)
        amb, n_in = int((cls == px.AMBIGUOUS).sum()), int((cls == px.IN).sum())
        print(f"dosage={dosage}: {n_in} in, {amb} ambiguous of {cls.size}")
        assert amb <= px.AMBIGUOUS_SHARE_MAX * cls.size and n_in >= px.MIN_DECIDED_IN
        assert n_in > 256                                                   # more than one batch of slots


def test_the_panels_hold_what_the_gpu_tests_rely_on():
    shape, n_hap = (300, 130), 1008
    ci, cj, done = px.mixed_pair(shape, n_hap)
    assert set(done) == {"individual", "half", "disjoint", "mono"}
    comp_i, comp_j = px.complete_rows(ci), px.complete_rows(cj)
    assert comp_i[0::3].all() and comp_j.any() and not comp_j.all()         # side I's rows % 3 == 0 stay complete (side J holds copies)
    assert (~comp_i[np.arange(shape[0]) % 3 != 0]).mean() > 0.95            # ... the others (but the monomorphic row) do not
    miss = float(np.mean(ci[~comp_i][:-1] == 2))                            # (the last row of a side is the all-missing one)
    assert 0.04 < miss < 0.08, miss                                         # the raised rate
    assert (ci[-1] == 2).all() and (cj[-1] == 2).all()                      # an all-missing row
    slab = [r for r in done["individual"] if r not in (1, shape[1] // 2)]    # (the monomorphic and the all-ALT row stay complete)
    assert len(slab) > 80 and max(slab) < 128 and (cj[slab, 2:4] == 2).all()   # a whole individual missing across a slab
    r = ci[px.ROW_HALF]
    assert ((r[0::2] == 2) & (r[1::2] == 1)).sum() >= n_hap // 8            # half-missing genotypes, the other allele ALT
    for dosage in (False, True):
        ex = px.PairwiseExactBlock(ci, cj, dosage)
        assert int(ex.counts[0][px.ROW_DISJOINT, px.ROW_DISJOINT]) == 0 and ex.degenerate[px.ROW_DISJOINT, px.ROW_DISJOINT]
        assert ex.degenerate[px.ROW_MONO, px.ROW_MONO] and int(ex.counts[1][px.ROW_MONO, px.ROW_MONO]) == 0
        assert not ex.degenerate[px.ROW_MONO, 0]                            # ... while the row itself is polymorphic
        assert int(ex.counts[0].min()) == 0 and int(ex.counts[0].max()) == (n_hap // 2 if dosage else n_hap)
    # the half-missing individuals are missing in the dosage form and ALT under missing = REF
    k = px.PairwiseExactBlock(ci, cj, True)
    assert int(k.N[px.ROW_HALF, 0]) <= n_hap // 2 - n_hap // 8
    # the largest counts
    bi, bj, _ = px.mixed_pair(*px.BIG_CASE)
    n = px.BIG_CASE[1]
    assert (bi[65] == 1).all() and (bj[65] == 1).all()
    assert int(px.PairwiseExactBlock(bi[60:70], bj[60:70]).c.max()) == n
    assert int(px.PairwiseExactBlock(bi[60:70], bj[60:70], True).S.max()) == 2 * n
    # the edge cases: the K-block boundary from both sides, the chunk tail, n_hap % 4 == 2
    assert sorted({h for _, h in rc.EDGE_CASES}) == [2, 254, 256, 258, 1008, 5008]
    # the walk: one I block more than a band of 4096 rows in either form, one row in it, two J slabs with a partial last one
    (wi, wj), wh = px.WALK_CASE
    assert wi == 4096 + 1 and 128 < wj < 256 and wh == 254
    # the tiles case: holes in rows [128, 256) of each side only
    ti, tj = px.tiles_pair()
    for c in (ti, tj):
        holes = ~px.complete_rows(c)
        assert holes[128:256].any() and not holes[:128].any() and not holes[256:].any()


def test_permutation_and_rephasing_keep_the_counts():
    shape, n_hap = (129, 257), 258
    ci, cj, _ = px.mixed_pair(shape, n_hap)
    base = [px.PairwiseExactBlock(ci, cj, d).counts for d in (False, True)]
    pi, pj = px.permute_individuals(ci, 5), px.permute_individuals(cj, 5)
    assert not np.array_equal(pi, ci)
    for d in (False, True):
        assert np.array_equal(px.PairwiseExactBlock(pi, pj, d).counts, base[d])
    ri, rj = px.rephase(ci, 8), px.rephase(cj, 9)
    assert not np.array_equal(ri, ci)
    assert np.array_equal(px.PairwiseExactBlock(ri, rj, True).counts, base[1])
    assert not np.array_equal(px.PairwiseExactBlock(ri, rj, False).counts, base[0])   # the haplotype form sees the phase

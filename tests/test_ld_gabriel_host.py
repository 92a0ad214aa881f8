"""CPU: the Gabriel block definition (include/ldx.h, "Gabriel blocks") -- the fp64 host mirror of the D' confidence bounds
against the 60-digit oracle (tests/ld_ci_exact.py), the planted panel's properties, the candidate and pick mirrors against
plain loops (tests/ld_gabriel_cases.py), and the entries' argument rules, which are checked before any HIP call.

Fragile tuples (ld_ci_exact: a cumulative sum within 2^-30 W of the 5 % line, |Dn*| < 10^-6, or two maxima within 10^-9) are
excluded from the comparison and their share is capped at 0.5 % on the SAMPLED sets.  The small exhaustive tables are reported
separately: about one in twelve of them is fragile, nearly all because Dn* is exactly 0 -- a table symmetric in its two phases --
so their share says nothing about the arithmetic (measured here: 147 of 1819 distinct tuples for n <= 6).
"""
import ctypes as C

import numpy as np
import pytest

import ld_ci_exact as cx
import ld_em_exact as emx
import ld_gabriel_cases as gc
import ld_gabriel_kernel_cases as kc
from ld_tools_amd import _lib, ops

FRAGILE_CAP = 0.005
HAND = (
    (127, 100, 100, 200, 0),      # perfect positive LD, fully phased
    (127, 100, 154, 0, 0),        # complete negative: no individual carries both ALT alleles
    (127, 127, 127, 127, 127),    # H = N: both SNPs all-heterozygous
    (127, 127, 90, 90, 40),       # an all-heterozygous SNP against an ordinary one
    (127, 120, 120, 210, 30),     # perfect LD with heterozygotes
    (127, 120, 134, 30, 30),      # its complement
    (504, 300, 300, 420, 180),
)
NO_TABLE = ((127, 300, 10, 0, 0), (127, 10, 10, 3, 0), (127, 10, 10, 40, 0), (0, 0, 0, 0, 0))
DEGENERATE = ((127, 0, 100, 0, 0), (127, 254, 100, 200, 0), (127, 100, 254, 200, 0))


def sampled_tuples(n_ind: int, count: int, seed: int):
    """Seeded count tuples of n_ind individuals: two SNPs with random allele frequencies and a random share of Dmax on either
    side, haplotypes drawn from the four frequencies and paired in order."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        p, q = rng.uniform(0.04, 0.96, size=2)
        share = rng.choice([0.0, 0.3, 0.7, 0.95, 1.0]) * rng.choice([-1.0, 1.0])
        d = share * (min(p * (1 - q), (1 - p) * q) if share >= 0 else min(p * q, (1 - p) * (1 - q)))
        f = np.clip([p * q + d, p * (1 - q) - d, (1 - p) * q - d, (1 - p) * (1 - q) + d], 0.0, 1.0)
        hap = rng.choice(4, size=2 * n_ind, p=f / f.sum())
        gi = (hap < 2).astype(np.int64).reshape(-1, 2).sum(axis=1)
        gj = ((hap == 0) | (hap == 2)).astype(np.int64).reshape(-1, 2).sum(axis=1)
        t = (n_ind, int(gi.sum()), int(gj.sum()), int((gi * gj).sum()), int(((gi == 1) & (gj == 1)).sum()))
        if cx.usable(*t):
            out.append(t)
    return out


def compare(tuples):
    """(tested, fragile, mismatches) of the host mirror against the oracle over the distinct tuples."""
    tuples = sorted(set(tuples))
    cols = np.array(tuples, dtype=np.int64).T
    lo, hi = ops.dprime_ci_host(*cols)
    fragile, bad = 0, []
    for k, t in enumerate(tuples):
        want_lo, want_hi, frag = cx.bounds(*t)
        assert cx.bounds_fast(*t) == (want_lo, want_hi, frag), t       # the fixed-point oracle of the GPU tests
        if frag:
            fragile += 1
        elif (int(lo[k]), int(hi[k])) != (want_lo, want_hi):
            bad.append((t, (int(lo[k]), int(hi[k])), (want_lo, want_hi)))
    return len(tuples), fragile, bad


def test_the_fixed_point_oracle_has_decimal_logarithms_and_exponentials():
    from decimal import Decimal, localcontext

    rng = np.random.default_rng(3)
    one = Decimal(cx.FixedMath.ONE)
    with localcontext() as ctx:
        ctx.prec = 90
        for v in [1, 2, 3, 255, 256, 257, 10 ** 13 + 7] + [int(x) for x in rng.integers(1, 1 << 62, size=40)]:
            assert abs(Decimal(cx.FixedMath.ln_int(v)) / one - Decimal(v).ln()) < Decimal(2) ** -225, v
        for x in [0.0, 1e-30, 0.5, 0.6931471805599453, 1.0, 37.5, 150.0, 166.3, 400.0] + rng.uniform(0, 60, size=40).tolist():
            d = Decimal(x)
            got = Decimal(cx.FixedMath.exp(-int(d * one))) / one
            assert abs(got - (-d).exp()) < Decimal(2) ** -215, x


def test_the_definition_on_hand_tuples():
    assert ops.dprime_ci_host(127, 100, 100, 200, 0) == (97, 100)     # the prototype's perfect-LD pair
    for t in HAND:
        lo, hi, frag = cx.bounds(*t)
        assert 0 <= lo <= hi <= 100
        if not frag:
            assert ops.dprime_ci_host(*t) == (lo, hi), t
    for t in NO_TABLE + DEGENERATE:
        assert ops.dprime_ci_host(*t) == (ops.NO_CI, ops.NO_CI) and cx.bounds(*t)[:2] == (cx.NO_CI, cx.NO_CI), t
    # the bounds do not depend on which SNP comes first
    for n_ind, a, b, s, h in HAND:
        assert ops.dprime_ci_host(n_ind, b, a, s, h) == ops.dprime_ci_host(n_ind, a, b, s, h)
    lo, hi = ops.dprime_ci_host(127, [100, 0], [100, 100], [200, 0], [0, 0])
    assert lo.dtype == np.uint8 and lo.tolist() == [97, ops.NO_CI] and hi.tolist() == [100, ops.NO_CI]


def test_host_bounds_equal_the_oracle_on_every_small_table():
    tuples = [(n,) + t for n in range(1, 7) for t in emx.live_tables(n)]
    tested, fragile, bad = compare(tuples)
    print(f"exhaustive n <= 6: {tested} distinct tuples, {fragile} fragile ({100.0 * fragile / tested:.2f} %), {len(bad)} mismatches")
    assert tested > 1500 and not bad, bad[:5]
    assert fragile < tested // 5          # reported separately (module docstring): exact symmetries, not arithmetic


@pytest.mark.parametrize("n_ind,count,seed", [(127, 400, 11), (504, 300, 12)])
def test_host_bounds_equal_the_oracle_on_sampled_tuples(n_ind, count, seed):
    tested, fragile, bad = compare(sampled_tuples(n_ind, count, seed) + [t for t in HAND if t[0] == n_ind])
    print(f"N = {n_ind}: {tested} tuples, {fragile} fragile, {len(bad)} mismatches")
    assert not bad, bad[:5]
    assert fragile <= FRAGILE_CAP * tested, (fragile, tested)


@pytest.fixture(scope="module")
def planted():
    """The host definition on gabriel_panel(254), plain form: bounds, brute-force candidates and pick."""
    codes, pos, where = gc.gabriel_panel(254)
    lo, hi, kept, band_lo, off, rows, cols = gc.host_bounds(codes, pos, gc.WINDOW, False)
    n = pos.shape[0]
    lo_d, hi_d = gc.dense_from_band(lo, band_lo, off, n), gc.dense_from_band(hi, band_lo, off, n)
    valid, lost = gc.brute_candidates(lo_d, hi_d, pos, kept, gc.WINDOW)
    block_of, accepted, overlapped = gc.brute_pick(valid, n, kept)
    return dict(codes=codes, pos=pos, where=where, lo=lo, hi=hi, kept=kept, valid=valid, lost=lost, block_of=block_of,
                accepted=accepted, overlapped=overlapped, n=n)


def test_the_planted_panel_is_not_trivial(planted):
    p = planted
    kept, pos = p["kept"], p["pos"]
    sizes = [int(kept[f:l + 1].sum()) for f, l in p["accepted"]]
    assert {2, 3, 4} <= set(sizes) and max(sizes) >= 5, sizes
    assert p["lost"]["span"] and p["lost"]["informative"] and p["lost"]["share"] and p["overlapped"]
    assert tuple(p["where"]["gap"][0]) in p["lost"]["span"]               # the pair 25 kb apart
    assert tuple(p["where"]["sandwich"][0]) in p["lost"]["share"]         # A, X, A'
    rare = p["where"]["rare_snp"][0]
    assert not kept[rare] and p["block_of"][rare] == gc.NOT_KEPT
    assert p["block_of"][rare - 1] == p["block_of"][rare + 1] < gc.NO_BLOCK   # between a block's ends, no member
    dup = p["where"]["dup_snp"][0]
    assert pos[dup] == pos[dup - 1] and (np.diff(pos) >= 0).all()
    assert (p["block_of"][kept] == gc.NO_BLOCK).any()                    # and kept SNPs outside every block
    assert (p["codes"] == 2).any()                                       # holes for the pairwise form


def test_candidates_and_pick_equal_the_plain_loops(planted):
    p = planted
    cands = ops.gabriel_candidates_host(p["lo"], p["hi"], p["pos"], p["kept"], gc.WINDOW)
    assert [tuple(c) for c in cands.tolist()] == p["valid"] and len(p["valid"]) > 100
    block_of, n_blocks = ops.gabriel_pick_host(cands, p["n"], p["kept"])
    assert np.array_equal(block_of, p["block_of"]) and n_blocks == len(p["accepted"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mirrors_on_random_bounds_and_other_parameters(seed):
    """Integer logic only: random bytes for the bounds (strong, recombinant, uninformative and missing pairs in every mix),
    duplicate positions, SNPs not kept, and parameters away from the defaults."""
    n, window = 40, 9000
    c = kc.random_bounds(n, window, seed)                  # (the generator of the kernel cases, at its defaults)
    pos, kept, lo, hi, band_lo, off = (c[k] for k in ("pos", "kept", "lo", "hi", "band_lo", "off"))
    assert (np.diff(pos) == 0).any() and not kept.all() and (lo == ops.NO_CI).any()
    for params in ({}, kc.OTHER):
        lo_d, hi_d = gc.dense_from_band(lo, band_lo, off, n), gc.dense_from_band(hi, band_lo, off, n)
        valid, _ = gc.brute_candidates(lo_d, hi_d, pos, kept, window, **params)
        cands = ops.gabriel_candidates_host(lo, hi, pos, kept, window, **params)
        assert [tuple(c) for c in cands.tolist()] == valid
        want, accepted, _ = gc.brute_pick(valid, n, kept)
        block_of, n_blocks = ops.gabriel_pick_host(cands, n, kept)
        assert np.array_equal(block_of, want) and n_blocks == len(accepted)
    assert len(valid) > 3


def test_tie_order_of_the_pick():
    """Equal spans: the smaller first wins, then the smaller last -- pinned with duplicate positions, where a candidate can
    hold another of the same span."""
    # positions 0 0 5 5: (0, 3), (0, 2), (1, 3), (1, 2) all span 5
    cands = [(1, 2, 5), (0, 3, 5), (1, 3, 5), (0, 2, 5)]
    block_of, n_blocks = ops.gabriel_pick_host(cands, 4)
    assert block_of.tolist() == [0, 0, 0, ops.NO_BLOCK] and n_blocks == 1          # (0, 2) first: first 0, the smaller last
    block_of, n_blocks = ops.gabriel_pick_host([(1, 2, 5), (1, 3, 5), (4, 5, 5), (0, 1, 4)], 6)
    assert block_of.tolist() == [ops.NO_BLOCK, 0, 0, ops.NO_BLOCK, 1, 1] and n_blocks == 2
    # a larger span goes first whatever its place in the list; a SNP not kept inside a block is no member
    block_of, n_blocks = ops.gabriel_pick_host([(0, 1, 3), (1, 4, 9)], 5, kept=[True, True, False, True, True])
    assert block_of.tolist() == [ops.NO_BLOCK, 0, ops.NOT_KEPT, 0, 0] and n_blocks == 1
    assert gc.brute_pick(cands, 4, [True] * 4)[0].tolist() == [0, 0, 0, ops.NO_BLOCK]


def test_parameters_are_checked():
    assert ops.gabriel_params()["cuts"] == (80, 50, 50, 70) and ops.gabriel_params()["max_spans"] == (20000, 30000, -1, -1)
    for bad in (dict(cuts=(1, 2, 3)), dict(strong_share=(21, 20)), dict(no_such=1), dict(cand_cut=-1)):
        with pytest.raises(_lib.LdxError):
            ops.gabriel_params(**bad)
    d = _lib.GabrielParams()
    _lib.lib.ldx_gabriel_default_params(C.addressof(d))
    s = ops._gabriel_struct(ops.gabriel_params())
    assert bytes(d) == bytes(s) and list(d.cut) == [80, 50, 50, 70] and list(d.max_span) == [20000, 30000, -1, -1]
    assert (d.cand_cut, d.strong_hi, d.recomb_hi, d.frac_num, d.frac_den) == (70, 98, 90, 19, 20)


def test_argument_rules_hold_before_any_hip_call():
    """No GPU is needed: every rule returns before the first HIP call, with the argument named."""
    lib = _lib.lib
    buf = C.create_string_buffer(4096)
    ptr = C.addressof(buf)

    def band(**kw):
        a = dict(alt=ptr, ref=ptr, acnt=ptr, rcnt=ptr, n_snps=4, n_hap=8, pairwise=1, positions=ptr, window=10, keep=None, lo=ptr,
                 offsets=ptr, ci_lo=ptr, ci_hi=ptr, n_cells=6, workspace=ptr, workspace_bytes=4096)
        a.update(kw)
        return lib.ldx_ld_em_ci_band_dev(a["alt"], a["ref"], a["acnt"], a["rcnt"], a["n_snps"], a["n_hap"], a["pairwise"],
                                         a["positions"], a["window"], a["keep"], a["lo"], a["offsets"], a["ci_lo"], a["ci_hi"],
                                         a["n_cells"], a["workspace"], a["workspace_bytes"], None)

    for kw, word in ((dict(alt=None), "alt"), (dict(ref=None), "ref"), (dict(rcnt=None), "rcnt"), (dict(lo=None), "lo"),
                     (dict(offsets=None), "offsets"), (dict(ci_lo=None), "ci_lo"), (dict(ci_hi=None), "ci_lo"),
                     (dict(positions=None), "positions"), (dict(workspace=None), "workspace"), (dict(n_snps=0), "n_snps"),
                     (dict(n_hap=7), "odd"), (dict(window=-1), "window"), (dict(workspace_bytes=8), "workspace_bytes")):
        assert band(**kw) == -1 and word in lib.ldx_last_error().decode(), (kw, lib.ldx_last_error())
    assert band(n_hap=_lib.MAX_HAPS + 2) == -3
    assert band(n_cells=0, ci_lo=None, ci_hi=None) == 0          # no pair in any window: nothing is launched

    assert lib.ldx_ld_ci_from_counts_dev(0, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None) == -1
    assert lib.ldx_ld_ci_from_counts_dev(4, ptr, ptr, ptr, ptr, ptr, None, ptr, None) == -1 and b"lo" in lib.ldx_last_error()

    def cand(**kw):
        a = dict(ci_lo=ptr, ci_hi=ptr, lo=ptr, offsets=ptr, n_cells=6, positions=ptr, keep=None, n_snps=4, window=10, params=None,
                 span=ptr, first=ptr, last=ptr, workspace=ptr, workspace_bytes=4096)
        a.update(kw)
        return lib.ldx_gabriel_candidates_dev(a["ci_lo"], a["ci_hi"], a["lo"], a["offsets"], a["n_cells"], a["positions"], a["keep"],
                                              a["n_snps"], a["window"], a["params"], a["span"], a["first"], a["last"],
                                              a["workspace"], a["workspace_bytes"], None)

    for kw, word in ((dict(lo=None), "lo"), (dict(offsets=None), "offsets"), (dict(positions=None), "positions"),
                     (dict(workspace=None), "workspace"), (dict(n_snps=0), "n_snps"), (dict(window=-2), "window"),
                     (dict(ci_hi=None), "ci_hi"), (dict(span=None), "cand_span"), (dict(workspace_bytes=16), "workspace_bytes")):
        assert cand(**kw) == -1 and word in lib.ldx_last_error().decode(), (kw, lib.ldx_last_error())
    wrong = ops._gabriel_struct(ops.gabriel_params())
    wrong.frac_den = 0
    assert cand(params=C.addressof(wrong)) == -1 and b"fraction" in lib.ldx_last_error()
    assert lib.ldx_gabriel_candidates_workspace_bytes(4, 6) >= 6 * 16 + 5 * 8 + 4 * 4
    assert lib.ldx_gabriel_candidates_workspace_bytes(4, 6) % 256 == 0 and lib.ldx_gabriel_pick_workspace_bytes(300) == 1024

    def pick(**kw):
        a = dict(span=ptr, order=ptr, first=ptr, last=ptr, n_cells=6, keep=None, n_snps=4, block_of=ptr, n_out=ptr, workspace=ptr,
                 workspace_bytes=4096)
        a.update(kw)
        return lib.ldx_gabriel_pick_dev(a["span"], a["order"], a["first"], a["last"], a["n_cells"], a["keep"], a["n_snps"],
                                        a["block_of"], a["n_out"], a["workspace"], a["workspace_bytes"], None)

    for kw, word in ((dict(block_of=None), "block_of"), (dict(n_out=None), "n_out"), (dict(workspace=None), "workspace"),
                     (dict(n_snps=0), "n_snps"), (dict(order=None), "order"), (dict(workspace_bytes=16), "workspace_bytes")):
        assert pick(**kw) == -1 and word in lib.ldx_last_error().decode(), (kw, lib.ldx_last_error())


def test_the_operators_refuse_what_the_em_refuses():
    """dosage=True, a haplotype path and an odd n_hap are refused before anything touches the device."""
    class Panel:
        n_snps, n_hap, device = 4, 8, None

    for kw in (dict(dosage=True), dict(path="mfma"), dict(missing="mean")):
        with pytest.raises(_lib.LdxError):
            ops.ld_gabriel_blocks(Panel(), window_snps=2, **kw)
    odd = Panel()
    odd.n_hap = 7
    for fn in (ops.ld_gabriel_blocks, ops.ld_dprime_ci):
        with pytest.raises(_lib.LdxError):
            fn(odd, window_snps=2)
    with pytest.raises(_lib.LdxError):
        ops.ld_dprime_ci(Panel(), window_snps=2, maf_min=0.7)
    with pytest.raises(_lib.LdxError):
        ops.ld_dprime_ci(Panel(), window_snps=2, keep=[1, 0])


# ---- the inputs of the direct kernel tests (tests/ld_gabriel_kernel_cases.py): each must stay in the regime it is there for ------
def test_settle_profile_on_hand_worked_chunks():
    """Rounds are counted as the kernel runs them: everybody reads the states of the round before."""
    # a chain: (0, 1) is accepted in round 1, (1, 2) sees that in round 2 and dies, (2, 3) sees THAT in round 3 ...
    assert kc.settle_profile([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1)], 5) == (1, 4)
    # round 1: (0, 5) and (6, 7) have nobody in front that overlaps them; round 2: (1, 2) and (7, 8) die with them
    assert kc.settle_profile([(0, 5, 9), (1, 2, 3), (6, 7, 3), (7, 8, 3)], 9) == (1, 2)
    assert kc.settle_profile([(2 * k, 2 * k + 1, 1) for k in range(257)], 514) == (2, 1)
    assert kc.settle_profile([], 3) == (0, 0)
    # two chunks: a wide block and the chain (k, k + 1), k < 255, then k = 255, 256, 257.  Chunk 1: the chain's k is settled in
    # round k + 1, 255 rounds.  Chunk 2: (255, 256) is dead on entry -- (254, 255) was accepted --, (256, 257) is accepted in
    # round 1 and (257, 258) dies in round 2.
    cands = [(500, 503, 5)] + [(k, k + 1, 1) for k in range(258)]
    assert kc.settle_profile(cands, 504) == (2, 255)
    assert kc.late_rejections(cands, 504) == [(256, 255, 256, 0)]
    assert kc.pick_order([(1, 2, 5), (0, 3, 5), (4, 9, 7), (0, 2, 5)]).tolist() == [[4, 9, 7], [0, 2, 5], [0, 3, 5], [1, 2, 5]]
    first, last, cell = kc.column_major(*ops.band_layout_host([0, 1, 2, 3], 2))       # rows 1: (0); 2: (0, 1); 3: (1, 2)
    assert (first.tolist(), last.tolist(), cell.tolist()) == ([0, 0, 1, 1, 2], [1, 2, 2, 3, 3], [0, 1, 2, 3, 4])


@pytest.mark.parametrize("name", ["random257", "random513"])
def test_the_random_kernel_cases_reach_every_rule(name):
    c = kc.case(name)
    assert (np.diff(c["pos"]) == 0).sum() > 20 and 0.75 < c["kept"].mean() < 0.95
    reasons = set()
    for params in (None, kc.OTHER):
        valid, lost, block_of, accepted, overlapped = kc.brute(name, params)
        cands, mirror_blocks, n_blocks = kc.mirrors(name, params)
        assert [tuple(v) for v in cands.tolist()] == valid and np.array_equal(mirror_blocks, block_of) and n_blocks == len(accepted)
        rows = [min(int(c["kept"][f:l + 1].sum()), 5) for f, l, _ in valid]
        print(f"{name}, {'other' if params else 'default'} parameters: {c['n_cells']} cells, {len(valid)} valid candidates "
              f"(m = 2, 3, 4, >= 5: {[rows.count(m) for m in (2, 3, 4, 5)]}), {len(accepted)} blocks, {len(overlapped)} overlapped, "
              f"lost {({k: len(v) for k, v in lost.items()})}")
        assert set(rows) == {2, 3, 4, 5} and len(valid) >= 100 and len(accepted) >= 15 and overlapped
        reasons |= {k for k, v in lost.items() if v}
    assert reasons == {"span", "informative", "share"}
    if name == "random257":                                 # the window passes 20 kb: the default cap of a two-SNP block bites
        assert kc.brute(name)[1]["span"] and c["window"] > 20_000


def test_the_many_chunk_cases_carry_blocks_from_chunk_to_chunk():
    for name, least in (("long3000", 10), ("wide600", 20)):
        c = kc.case(name)
        cands, _, n_blocks = kc.mirrors(name)
        order = kc.pick_order(cands)
        chunks, rounds = kc.settle_profile(order, c["n"])
        late = kc.late_rejections(order, c["n"])
        print(f"{name}: {c['n_cells']} cells, {len(cands)} valid candidates in {chunks} chunks, at most {rounds} rounds, "
              f"{n_blocks} blocks, {len(late)} candidates lost to a block of an earlier chunk")
        assert chunks >= least and chunks == -(-len(cands) // kc.CHUNK) and n_blocks >= 10
        assert late and max(rank // kc.CHUNK - was for rank, _, _, was in late) >= least // 2    # ... of many chunks earlier
    assert kc.case("long3000")["n"] > 11 * kc.CHUNK and kc.case("wide600")["n_cells"] > 30_000


@pytest.mark.parametrize("n,window,rounds", [(600, 1, 256), (600, 2, 150), (1500, 3, 100), (601, 1, 256)])
def test_the_chains_need_deep_settles(n, window, rounds):
    c = kc.case(f"chain{n}w{window}")
    cands, block_of, n_blocks = kc.mirrors(f"chain{n}w{window}")
    assert cands.shape[0] == c["n_cells"] and np.unique(cands[:, 2]).size == window     # every slot valid, spans tie
    chunks, deepest = kc.settle_profile(kc.pick_order(cands), n)
    print(f"chain n = {n}, window {window}: {chunks} chunks, {deepest} rounds in the deepest")
    assert (deepest == 256 if rounds == 256 else rounds <= deepest <= 256) and chunks >= 3
    if window == 1:                                           # written out without any mirror: the pairs (0, 1), (2, 3), ...
        want = np.arange(n) // 2
        assert n_blocks == n // 2 and np.array_equal(block_of[:n - n % 2], want[:n - n % 2])
        assert n % 2 == 0 or block_of[n - 1] == ops.NO_BLOCK


def test_the_trip_cases_sit_on_the_boundaries():
    assert kc.TRIP_SIZES == (1, 2, 255, 256, 257, 512, 513) and kc.CHUNK == 256
    for n in kc.TRIP_SIZES:
        c = kc.case(f"trip{n}")
        cands, block_of, n_blocks = kc.mirrors(f"trip{n}")
        assert c["n_cells"] == n - 1 and cands.shape[0] == int((c["kept"][1:] & c["kept"][:-1]).sum())
        assert n < 255 or (not c["kept"].all() and n_blocks > 50 and (block_of == ops.NO_BLOCK).any())
    for name, n_cells, n_valid in (("valid256of512", 512, 256), ("valid512of699", 699, 512), ("full256", 256, 256), ("full512", 512, 512)):
        assert kc.case(name)["n_cells"] == n_cells and kc.mirrors(name)[0].shape[0] == n_valid and kc.case(name)["kept"].all()
    empty = kc.case("empty700")
    assert empty["n_cells"] == 0 and (np.diff(empty["pos"]) > 0).all() and not empty["kept"].all() and kc.mirrors("empty700")[2] == 0


def test_the_scaled_case_has_spans_above_32_bits():
    base, scaled = kc.case("random513"), kc.case("scaled513")
    assert np.array_equal(scaled["band_lo"], base["band_lo"]) and np.array_equal(scaled["off"], base["off"])
    assert scaled["window"] == base["window"] << 33 < ops.BAND_WINDOW_MAX
    cands, block_of, n_blocks = kc.mirrors("scaled513", kc.SCALED)
    want, want_blocks, want_n = kc.mirrors("random513")
    assert np.array_equal(cands[:, :2], want[:, :2]) and np.array_equal(cands[:, 2], want[:, 2] << 33)
    assert np.array_equal(block_of, want_blocks) and n_blocks == want_n
    assert cands[:, 2].max() > 1 << 32 and (cands[:, 2] % (1 << 32) == 0).all()    # the low word says nothing about a span
    assert (want[:, 2] == 0).any() and np.unique(want[:, 2]).size > 20


def test_the_nested_list_needs_the_scan_inside_a_candidate():
    span, first, last, block_of, n_out = kc.nested_list()
    live = span >= 0
    cands = np.stack([first[live], last[live], span[live]], axis=1).astype(np.int64)
    got, n_blocks = ops.gabriel_pick_host(cands, 600)
    assert np.array_equal(got, block_of) and [n_blocks, cands.shape[0]] == n_out == [258, 259]
    order = kc.pick_order(cands)
    assert kc.late_rejections(order, 600) == [(256, 1, 514, 0)] and kc.settle_profile(order, 600) == (2, 1)
    assert block_of[1] == 0 and block_of[514] == 257            # both ends of (1, 514) are free when its chunk begins
    assert live.sum() < live.size and not live[:3].all() and kc.case("chain600w1")["n_cells"] == live.size

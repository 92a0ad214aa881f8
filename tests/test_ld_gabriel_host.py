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
    rng = np.random.default_rng(seed)
    n, window = 40, 9000
    pos = np.cumsum(rng.choice([0, 300, 700, 2500], size=n)).astype(np.int64)
    kept = rng.random(n) > 0.15
    band_lo, off = ops.band_layout_host(pos, window)
    m = int(off[-1])
    kind = rng.choice(4, size=m, p=[0.55, 0.15, 0.2, 0.1])
    lo = np.select([kind == 0, kind == 1, kind == 2], [rng.integers(45, 100, m), rng.integers(0, 40, m), rng.integers(0, 70, m)],
                   ops.NO_CI).astype(np.uint8)
    hi = np.select([kind == 0, kind == 1, kind == 2], [rng.integers(96, 101, m), rng.integers(40, 90, m), rng.integers(90, 101, m)],
                   ops.NO_CI).astype(np.uint8)
    for params in ({}, dict(cuts=(75, 60, 55, 65), max_spans=(1500, 4000, 6000, None), min_informative=(1, 2, 4, 5),
                            strong_share=(3, 4), cand_cut=60, strong_hi=97, recomb_hi=85)):
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

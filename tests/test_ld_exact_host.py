"""CPU: the exact oracle of tests/ld_exact.py against other independent statements of the same quantities, and the
conditions tests/test_gpu_exact_oracle.py relies on -- pairs in LD across 128-column tile boundaries, planted duplicate and
complement rows, and how many pairs lie too close to a threshold to be decided (every (panel, threshold, window) the GPU
file uses is counted and printed here).
"""
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_exact as lx  # noqa: E402


def synth_panel(n, h, **kw):
    from ld_tools_amd import synth
    return synth.synth_codes_host(n, h, **kw)


@pytest.mark.parametrize("shape", [(300, 5008), (200, 1008), (257, 37), (64, 2)])
def test_oracle_equals_corrcoef_without_missing_codes(shape):
    n, h = shape
    codes = synth_panel(n, h, seed=3 + n)
    codes[7] = 0
    codes[n - 2] = 1
    ex = lx.Exact(codes)
    x = codes.astype(np.float64)
    poly = x.min(axis=1) != x.max(axis=1)
    assert np.array_equal(ex.live, poly) and (~poly).sum() >= 2
    ok = np.outer(poly, poly)
    assert np.array_equal(ex.degenerate, ~ok)
    with np.errstate(invalid="ignore", divide="ignore"):
        cc = np.corrcoef(x)
    # np.corrcoef centres in float64: ~1e-16 per element, far above the oracle's two roundings
    assert np.abs(ex.r64[ok] - cc[ok]).max() <= 1e-12
    assert np.abs(ex.r2_64[ok] - cc[ok] ** 2).max() <= 1e-12
    assert (ex.r64[~ok] == 0).all()
    assert np.array_equal(ex.diagonal(), poly.astype(np.float64))


def ulp64(x):
    _, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(1.0, e - 53)


@pytest.mark.parametrize("shape,seed", [((96, 37), 7), ((64, 1008), 11)])
def test_oracle_equals_fractions_and_the_reference_restatement(shape, seed):
    from oracle import ld_oracle as orc
    n, h = shape
    codes = synth_panel(n, h, seed=seed, miss=0.05, mono=0.04)
    codes[5] = 0                                        # degenerate rows: no ALT, no REF
    codes[9] = np.where(codes[9] == 0, 2, codes[9])
    ex = lx.Exact(codes)
    assert (ex.a + ex.r < h).sum() > n // 2 and (~ex.live).sum() > 0
    rows = [row.tolist() for row in codes]
    gate_open, worst, beyond = 0, 0.0, 0
    for i in range(n):
        for j in range(n):
            cnt = orc.pair_counts_lists(rows[i], rows[j])
            assert cnt == (h, int(ex.n11[i, j]), int(ex.a[i]), int(ex.r[i]), int(ex.a[j]), int(ex.r[j]))
            num = h * cnt[1] - cnt[2] * cnt[4]
            den2 = cnt[2] * cnt[3] * cnt[4] * cnt[5]
            assert num == ex.num[i, j] and den2 == ex.den2[i, j]
            assert bool(ex.degenerate[i, j]) == (den2 == 0) and bool(ex.zero_num[i, j]) == (den2 != 0 and num == 0)
            if den2 == 0:
                assert ex.r64[i, j] == 0 and ex.r2_64[i, j] == 0
                continue
            want = Fraction(num * num, den2)
            assert abs(Fraction(float(ex.r2_64[i, j])) - want) <= 2 * Fraction(float(ulp64(float(want))))
            # r: its square against the same fraction (sqrt, division, and the squaring here: a few ulps)
            assert abs(Fraction(float(ex.r64[i, j])) ** 2 - want) <= 8 * Fraction(float(ulp64(float(want))))
            assert (ex.r64[i, j] > 0) == (num > 0) and (ex.r64[i, j] == 0) == (num == 0)
            rsq, _, _, _, flags = orc.ld_raw_from_counts(*cnt)
            if not flags & orc.FLAG_RSQ_INT0 and num != 0:
                gate_open += 1
                # 1e-12 relative is what oracle/ld_oracle.py documents for its float64 op order.  That order forms
                # d = f11 - fa1 fa2 from rounded frequencies (three roundings of values below 1: |error of d| <= 2^-52), so
                # where d cancels its r^2 = d^2 / den carries 2 |d| 2^-52 / den = 2 sqrt(r^2 / den) 2^-52 of its own -- the
                # restatement's error, not the oracle's (the Fraction comparison above holds to 2 ulps for the same pair).
                den = (cnt[2] / h) * (cnt[3] / h) * (cnt[4] / h) * (cnt[5] / h)
                own = 2.0 * np.sqrt(ex.r2_64[i, j] / den) * 2.0 ** -52
                rel = abs(rsq - ex.r2_64[i, j]) / ex.r2_64[i, j]
                worst = max(worst, rel)
                beyond += rel > 1e-12
                assert abs(rsq - ex.r2_64[i, j]) <= 1e-12 * ex.r2_64[i, j] + own, (cnt, rsq, ex.r2_64[i, j])
    print(f"{shape}: {gate_open} pairs with the D' gate open, worst relative difference {worst:.3g} "
          f"({beyond} pairs beyond 1e-12, all within the restatement's own cancellation error)")
    assert gate_open > n * n // 2
    d = ex.diagonal()
    for i in range(n):
        if ex.live[i]:
            assert Fraction(float(d[i])) == Fraction(float(Fraction(h - int(ex.a[i]), int(ex.r[i]))))
            assert abs(ex.r64[i, i] - d[i]) <= 4 * ulp64(d[i])


def test_threshold_classes_are_exact_at_the_edges():
    """Pairs built to sit exactly on, just inside and just outside the two edges of a threshold."""
    h = 1 << 10
    # rows with a = r = 512 and n11 = 256 + k: num = 1024 k, den2 = 2^36, r^2 = k^2 / 2^16 (exact in float64)
    base = (np.arange(h) < 512).astype(np.int8)
    ks = [0, 1, 64, 128, 181, 182, 255, 256]
    rows = [base]
    for k in ks:
        row = np.zeros(h, dtype=np.int8)
        row[:256 + k] = 1
        row[512:512 + 256 - k] = 1
        rows.append(row)
    ex = lx.Exact(np.stack(rows))
    for idx, k in enumerate(ks, start=1):
        assert ex.num[idx, 0] == 1024 * k and ex.r2_64[idx, 0] == k * k / 65536.0
    q = 128 * 128 / 65536.0                     # 0.25, the exact r^2 of k = 128
    m = float(lx.MARGIN)
    cell = (1 + ks.index(128), 0)
    for t in (q, q / (1 + m), np.nextafter(q / (1 + m), 1.0), np.nextafter(q / (1 + m), 0.0), q / (1 - m),
              np.nextafter(q / (1 - m), 0.0), np.nextafter(q / (1 - m), 1.0), 0.2, 0.3):
        # the edges in exact arithmetic, independent of the float64 shortcut in classes(): these t lie within 2^-52 of one
        ft = Fraction(float(t))
        exact = lx.IN if Fraction(q) >= ft * (1 + lx.MARGIN) else lx.OUT if Fraction(q) <= ft * (1 - lx.MARGIN) else lx.AMBIGUOUS
        assert ex.classes(t)[cell] == exact, (t, exact)
    assert ex.classes(q)[cell] == lx.AMBIGUOUS and ex.classes(0.2)[cell] == lx.IN and ex.classes(0.3)[cell] == lx.OUT
    assert ex.classes(np.nextafter(q / (1 + m), 0.0))[cell] == lx.IN and ex.classes(np.nextafter(q / (1 + m), 1.0))[cell] == lx.AMBIGUOUS
    assert ex.classes(np.nextafter(q / (1 - m), 1.0))[cell] == lx.OUT and ex.classes(np.nextafter(q / (1 - m), 0.0))[cell] == lx.AMBIGUOUS
    c = ex.classes(1.0)
    assert c[1 + ks.index(256), 0] == lx.AMBIGUOUS and c[1 + ks.index(255), 0] == lx.OUT   # r^2 = 1 against t = 1
    assert ex.classes(0.5)[1 + ks.index(0), 0] == lx.OUT


def test_greedy_selection_on_a_hand_made_graph():
    #   0 - 1 - 2 - 3     4 (NaN p)    5 (degenerate)   6 - 7
    nbr = np.zeros((8, 8), dtype=bool)
    for i, j in [(0, 1), (1, 2), (2, 3), (6, 7), (4, 0), (5, 1)]:
        nbr[i, j] = nbr[j, i] = True
    live = np.array([1, 1, 1, 1, 1, 0, 1, 1], dtype=bool)
    p = np.array([1e-3, 1e-5, 1e-5, 0.5, np.nan, 1e-9, 0.2, 0.2])
    index, owner = lx.clump_exact(nbr, p, 1e-2, 0.3, live)
    assert index == [1]                          # 1 takes 0 and 2 (its tie with 2: the lower row goes first)
    assert owner.tolist() == [1, 1, 1, -1, -1, -1, -1, -1]
    index, owner = lx.clump_exact(nbr, p, 0.3, 0.3, live)
    assert index == [1, 6] and owner.tolist() == [1, 1, 1, -1, -1, -1, 6, 6]
    index, owner = lx.clump_exact(nbr, p, 1.0, 1.0, live)
    assert index == [1, 6, 3] and owner.tolist() == [1, 1, 1, 3, -1, -1, 6, 6]
    keep = lx.prune_exact(nbr, np.array([1, 2, 2, 0, 5, 9, 3, 3], dtype=float), live)
    assert keep.tolist() == [False, True, False, True, True, False, True, False]


# ---- the panels of the GPU file -------------------------------------------------------------------------------------
def test_default_panels_have_no_ld_across_tiles():
    """Why the long-range panels exist: synth's 32-SNP blocks put no pair with r^2 >= 0.2 across a tile boundary."""
    for n, h in [(1000, 1008), (700, 333), (129, 257)]:
        ex = lx.Exact(synth_panel(n, h, seed=11 + n))
        m = ex.r2_64 >= 0.2
        np.fill_diagonal(m, False)
        assert lx.tile_crossing(m) == 0 and lx.far_apart(m) == 0


def test_long_range_panels_reach_across_tiles():
    ex = lx.Exact(lx.long_range_codes("lr1000"))
    m = ex.r2_64 >= 0.2
    np.fill_diagonal(m, False)
    assert (lx.tile_crossing(m), lx.far_apart(m)) == (10310, 13734)   # counted with exact integers when the panel was chosen
    for name in lx.LONG_RANGE:
        codes, plants, ex = lx.long_range_panel(name)
        inn = ex.classes(0.2) == lx.IN
        np.fill_diagonal(inn, False)
        cross, far = lx.tile_crossing(inn), lx.far_apart(inn)
        print(f"{name}: {int(inn.sum())} ordered pairs decided in at 0.2, {cross} across a tile boundary, {far} at 32+ SNPs")
        assert cross >= 1000 and far >= 1000
        assert (~ex.live).sum() > 0 and (ex.a + ex.r < ex.n_hap).sum() > ex.n_snps // 2
        # planted rows: exact duplicates / complements of complete rows, at 128 k + delta
        assert {(d - s) % 128 for s, d, _ in plants} == set(lx.PLANT_DELTAS) and {sg for _, _, sg in plants} == {1, -1}
        assert len({(d - s) // 128 for s, d, _ in plants}) >= 3
        for s, d, sg in plants:
            assert ex.a[s] + ex.r[s] == ex.n_hap and ex.live[s]
            assert np.array_equal(codes[d], codes[s] if sg > 0 else 1 - codes[s])
            assert ex.num2[d, s] == ex.den2[d, s] and np.sign(ex.num[d, s]) == sg and ex.r64[d, s] == float(sg)
            assert s // 128 != d // 128


def test_count_targeted_pairs_are_in_the_edge_panels():
    """The near-cancellation pairs the cell test relies on are really there (host arithmetic only)."""
    ex = lx.Exact(lx.edge_panel(1000, 10240))
    off = ~np.eye(1000, dtype=bool)
    big = ex.zero_num & off & (10240 * ex.n11 > (1 << 24))      # n n11 == a_i a_j with both products above 2^24
    assert big.any()
    i, j = np.argwhere(big & (ex.a[:, None] == 5120) & (ex.a[None, :] == 5120))[0]
    assert ex.n11[i, j] == 2560
    assert ((np.abs(ex.num) == 10240) & (ex.a[:, None] == 5120) & (ex.a[None, :] == 5120) & off).any()   # n11 = 2560 +- 1
    assert ((ex.a == 1) & (ex.r == 10239)).any() and ((ex.a == 10239) & (ex.r == 1)).any()
    assert ((ex.r == 1) & (ex.a > 1) & (ex.a + ex.r < 10240)).any() and ((ex.a == 1) & (ex.r == 1)).any()
    ex = lx.Exact(lx.edge_panel(1000, 10239))
    assert (ex.zero_num & ~np.eye(1000, dtype=bool) & (10239 * ex.n11 > (1 << 24))).any()


def test_ambiguity_of_the_neighbour_cases():
    """Pairs too close to a threshold to be decided are rare in every neighbour-list case, as the GPU tests require."""
    for name in lx.LONG_RANGE:
        _, _, ex = lx.long_range_panel(name)
        for pos, w in lx.neighbour_windows(ex.n_snps):
            for t in lx.NEIGHBOUR_THRESHOLDS:
                inn, amb, win = lx.pair_classes(ex, t, pos, w)
                print(f"{name} t={t} w={w}: in-window {int(win.sum())}, decided in {int(inn.sum())} "
                      f"({lx.tile_crossing(inn)} across tiles), ambiguous {int(amb.sum())}")
                assert amb.sum() <= lx.AMBIGUOUS_SHARE_MAX * win.sum()
                assert np.array_equal(inn, inn.T) and np.array_equal(amb, amb.T)
            assert lx.tile_crossing(lx.pair_classes(ex, 0.2, pos, w)[0]) >= 1000


def test_no_ambiguity_in_the_clump_and_prune_cases():
    """The greedy result is unique only if no in-window pair is ambiguous: zero in every case the GPU tests compare."""
    for name, (clumps, prunes) in lx.CLUMP_CASES.items():
        _, ex = lx.clump_panel(name)
        pos = lx.clump_positions(ex.n_snps)
        for t, w in [(c[2], c[3]) for c in clumps] + list(prunes):
            inn, amb, win = lx.pair_classes(ex, t, pos, w)
            print(f"{name} t={t} w={w}: in-window {int(win.sum())}, decided in {int(inn.sum())} "
                  f"({lx.tile_crossing(inn)} across tiles), ambiguous {int(amb.sum())}")
            assert amb.sum() == 0
    # at 0.3 the long-range panel does have ambiguous pairs: that threshold is not among its cases
    _, ex = lx.clump_panel("lr1000")
    assert (ex.classes(0.3) == lx.AMBIGUOUS).sum() == 2
    assert all(c[2] != 0.3 for c in lx.CLUMP_CASES["lr1000"][0]) and all(c[0] != 0.3 for c in lx.CLUMP_CASES["lr1000"][1])

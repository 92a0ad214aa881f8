"""CPU: the host side of the max(T) permutation test (include/ldx.h, "permutation tests") -- the labels' definition against an
independent rank count, the statistic's mirror against model_tests_host bit for bit and against exact rationals within a derived
bound, ld_mperm_host against per-individual loops, the SNP flags and the invalid cells.  No kernel is launched here."""
from fractions import Fraction

import numpy as np
import pytest

import ld_mperm_exact as X


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- labels ----------------------------------------------------------------------------------------------------------------------
# the cases of three permutations, from synth.key64 by X.rank_labels: an O(n^2) count of the pairs (key, k') < (key, k)
KNOWN = [
    ((1, 0, 12, 5), [2, 5, 8, 10, 11]),
    ((20261003, 7, 40, 13), [2, 5, 6, 7, 9, 13, 14, 18, 22, 28, 29, 37, 39]),
    ((2 ** 63 + 5, 123456789, 129, 37),
     [11, 12, 13, 16, 17, 20, 21, 26, 28, 29, 33, 34, 43, 46, 47, 49, 53, 54, 55, 56, 58, 61, 74, 77, 80, 82, 85, 96, 98, 102, 104,
      106, 110, 120, 123, 126, 127]),
]


@pytest.mark.parametrize("args,cases", KNOWN)
def test_labels_known_answers(args, cases):
    from ld_tools_amd import perm_labels_host

    seed, p, n, n_case = args
    want = np.zeros(n, dtype=bool)
    want[cases] = True
    assert np.array_equal(X.rank_labels(seed, p, n, n_case), want)          # the pin is the definition's
    assert np.array_equal(perm_labels_host(n, n_case, 1, seed, first=p)[0], want)


def test_labels_have_n_case_cases_and_do_not_depend_on_the_chunking():
    from ld_tools_amd import perm_labels_host

    n, n_case, seed = 187, 37, 9
    whole = perm_labels_host(n, n_case, 200, seed)
    assert whole.shape == (200, n) and whole.dtype == bool
    assert (whole.sum(axis=1) == n_case).all()
    assert len({r.tobytes() for r in whole}) == 200                          # 200 different permutations
    assert np.array_equal(perm_labels_host(n, n_case, 50, seed, first=150), whole[150:])
    parts = [perm_labels_host(n, n_case, r, seed, first=f) for f, r in ((0, 128), (128, 72))]
    assert np.array_equal(np.concatenate(parts), whole)
    for p in (0, 77, 199):
        assert np.array_equal(whole[p], X.rank_labels(seed, p, n, n_case))
    assert not np.array_equal(perm_labels_host(n, n_case, 1, seed + 1)[0], whole[0])
    assert not np.array_equal(perm_labels_host(n, n_case + 1, 1, seed)[0], whole[0])


def test_labels_argument_rules():
    from ld_tools_amd import LdxError, perm_labels_host

    for n, n_case, n_perm in ((10, 0, 1), (10, 10, 1), (1, 1, 1), (10, 3, 0), (5121, 3, 1)):
        with pytest.raises(LdxError):
            perm_labels_host(n, n_case, n_perm, 1)
    with pytest.raises(LdxError):
        perm_labels_host(10, 3, 1, 1, first=-1)


# ---- the statistic ---------------------------------------------------------------------------------------------------------------
def tuples_of(t):
    cn, ch, cm, un, uh, um = t
    return cn + un, ch + uh, cm + um, cn, ch + 2 * cm


@pytest.mark.parametrize("n_max", [40, 700, 2560])
def test_stat_mirror_is_the_model_tests_bit_for_bit(n_max):
    from ld_tools_amd import mperm_stat_host, model_tests_host

    t = X.random_tables(np.random.default_rng(n_max), 400, n_max)
    chisq, _, _, _, flags = model_tests_host(*t)
    for k, test in enumerate(("allelic", "trend")):
        x, f = mperm_stat_host(*tuples_of(t), test=test)
        assert np.array_equal(f, flags[:, k])
        assert np.array_equal(bits(x), bits(chisq[:, k]))
        assert (f == 0).sum() > 250 and (f == 1).any() and (f == 2).any()


def test_stat_against_exact_rationals():
    """Two roundings of at most 2^-53 each (the product and the quotient; the integers and their conversions are exact):
    |chisq - exact| <= 2^-51 exact leaves a factor of almost two."""
    from ld_tools_amd import mperm_stat_host

    t = tuples_of(X.random_tables(np.random.default_rng(3), 300, 2560))
    worst = Fraction(0)
    for test in ("allelic", "trend"):
        x, f = mperm_stat_host(*t, test=test)
        for k in range(x.size):
            want = X.stat_fraction(test, *(c[k] for c in t))
            if f[k] == 0:
                assert want is not None
                err = abs(Fraction(float(x[k])) - want)
                assert err <= Fraction(1, 2 ** 51) * want
                if want:
                    worst = max(worst, err / want)
            else:
                assert np.isnan(x[k]) and want is None
    assert worst > 0


def test_invalid_cells_and_refused_tuples():
    from ld_tools_amd import LdxError, mperm_stat_host

    #            N   het hom  R   a
    rows = [(100, 40, 10, 0, 0),       # R = 0
            (100, 40, 10, 100, 60),    # R = N
            (100, 0, 0, 30, 0),        # monomorphic REF: den = 0
            (100, 0, 100, 30, 60),     # monomorphic ALT
            (100, 40, 10, 30, 20)]     # a table
    cols = [np.array(c) for c in zip(*rows)]
    for test in ("allelic", "trend"):
        x, f = mperm_stat_host(*cols, test=test)
        assert f.tolist() == [1, 1, 2, 2, 0]
        assert np.isnan(x[:4]).all() and x[4] > 0
        assert float(x[4]) == float(X.stat_fraction(test, *rows[4]))
    for bad in ((100, 40, 70, 30, 20), (100, 40, 10, 101, 20), (100, 40, 10, 30, 61), (100, 40, 10, 5, 11),
                (100, 40, 10, 95, 20), (5121, 40, 10, 30, 20)):
        with pytest.raises(LdxError):
            mperm_stat_host(*(np.array([v]) for v in bad))
    with pytest.raises(LdxError):
        mperm_stat_host(*cols, test="genotypic")


# ---- the whole scan on the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    case = X.case_vector(60, 17, 36, seed=2)
    codes = X.mperm_codes(40, 60, seed=4, miss=0.05, miss_from=10)
    case_of = np.nonzero(case == 1.0)[0]
    codes[3] = 0                                     # monomorphic: flag 2
    codes[5] = 2                                     # nobody called: flag 1
    codes[7] = 1
    codes[7, np.repeat(2 * case_of, 2) + np.tile([0, 1], case_of.size)] = 2      # no called case: flag 1
    return codes, case


@pytest.mark.parametrize("test", ["allelic", "trend"])
def test_scan_mirror_against_the_loops(small, test):
    from ld_tools_amd import ld_mperm_host, perm_labels_host

    codes, case = small
    keep = np.ones(40, dtype=bool)
    keep[[11, 12]] = False
    P = 64
    res = ld_mperm_host(codes, case, test=test, n_perm=P, seed=5, keep=keep)
    assert (res.n_perm, res.n_case, res.n_ctrl) == (P, 17, 36)
    flags = res.flags.numpy()
    assert flags[[3, 5, 7, 11, 12]].tolist() == [2, 1, 1, 3, 3] and (np.delete(flags, [3, 5, 7, 11, 12]) == 0).all()
    labels = perm_labels_host(53, 17, P, 5)
    ar = X.counts_brute(codes, case, labels)
    N, n1, n2, R, a = X.snp_margins(codes, case)
    stat = res.stat.numpy()
    n_ge, maxima = np.zeros(40, dtype=np.int64), [Fraction(0)] * P
    for i in range(40):
        obs = X.stat_fraction(test, N[i], n1[i], n2[i], R[i], a[i])
        if flags[i]:
            assert np.isnan(stat[i])
            continue
        assert float(obs) == stat[i]
        for p in range(P):
            x = X.stat_fraction(test, N[i], n1[i], n2[i], ar[1, i, p], ar[0, i, p])
            if x is not None:
                # 53 individuals: the product T det^2 < 2^30 is exact, so a cell IS the correctly rounded rational and the
                # mirror's fp64 compare is this one
                n_ge[i] += float(x) >= stat[i]
                maxima[p] = max(maxima[p], x)
    assert np.array_equal(res.n_ge.numpy(), n_ge)
    assert np.array_equal(res.maxima.numpy(), np.array([float(m) for m in maxima]))
    assert (res.n_ge.numpy()[flags != 0] == 0).all()
    emp1, emp2 = res.emp1.numpy(), res.emp2.numpy()
    ok = flags == 0
    assert np.isnan(emp1[~ok]).all() and np.isnan(emp2[~ok]).all()
    assert np.array_equal(emp1[ok], (n_ge[ok] + 1) / (P + 1))
    mx = res.maxima.numpy()
    assert np.array_equal(emp2[ok], np.array([((mx >= s).sum() + 1) / (P + 1) for s in stat[ok]]))
    assert (emp2[ok] >= emp1[ok]).all()


def test_scan_mirror_takes_a_label_matrix_and_refuses_a_wrong_one(small):
    from ld_tools_amd import LdxError, ld_mperm_host, perm_labels_host

    codes, case = small
    labels = perm_labels_host(53, 17, 16, 8)
    a = ld_mperm_host(codes, case, n_perm=16, seed=8)
    b = ld_mperm_host(codes, case, labels=labels)
    assert np.array_equal(a.n_ge.numpy(), b.n_ge.numpy()) and np.array_equal(bits(a.maxima.numpy()), bits(b.maxima.numpy()))
    with pytest.raises(LdxError):
        ld_mperm_host(codes, case, labels=labels[:, :52])
    with pytest.raises(LdxError):
        ld_mperm_host(codes, case, labels=~labels)
    with pytest.raises(LdxError):
        ld_mperm_host(codes, case)
    with pytest.raises(LdxError):
        ld_mperm_host(codes, case, test="boost", n_perm=4)

"""CPU: pairwise-complete EM (include/ldx.h, "pairwise-complete EM") -- the integer oracle of tests/ld_em_pairwise_exact.py against
a plain loop over the individuals, the pairs the GPU test's panels must hold, the fp64 restatement ops.em_host on the pair's
own integers against the 60-digit oracle of tests/ld_em_exact.py, and the reduction to ld_em's integers on a panel without holes.
"""
import math
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_em_exact as emx  # noqa: E402
import ld_em_pairwise_exact as epx  # noqa: E402
import ld_pairwise_exact as px  # noqa: E402
import ld_rect_cases as rc  # noqa: E402

NEW_SYMBOLS = ("ldx_ld_em_rect_pw_dev", "ldx_ld_em_rect_pw_hits_dev", "ldx_ld_em_pw_counts_dev", "ldx_ld_em_from_counts_pw_dev")
SMALL = ((40, 30), 64)
SAMPLES = 1500
HOLED_N = epx.HOLED_CASE[1] // 2


def test_new_symbols_are_declared_bound_and_exported():
    import inspect

    import ld_tools_amd
    from ld_tools_amd import _lib, drivers, ops
    text = (ROOT / "include" / "ldx.h").read_text()
    assert "pairwise-complete EM" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ldx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/ldx.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libldx.so"
    for fn in (ld_tools_amd.ld_em, ld_tools_amd.ld_em_hits, ld_tools_amd.ld_em_counts, drivers.em_matrix, drivers.em_hits):
        assert inspect.signature(fn).parameters["missing"].default is None, fn.__name__
    assert ops.EM_PAIRWISE_COUNTS == epx.SETS


def test_matrix_product_counts_equal_a_plain_loop():
    shape, n_hap = SMALL
    ci, cj, planted = epx.mixed(shape, n_hap)
    assert {"individual", "half", "disjoint", "mono", "all_missing"} <= set(planted)
    counts = epx.pair_counts(ci, cj)
    assert counts.shape == (5,) + shape and np.array_equal(counts, epx.loop_counts(ci, cj))
    # the haplotype-level joint mask would count half-missing genotypes: the oracle must not
    half = ci[px.ROW_HALF]
    assert ((half[0::2] == 2) != (half[1::2] == 2)).any()


def test_the_planted_pairs_are_present():
    shape, n_hap = (300, 130), 258
    ci, cj, planted = epx.mixed(shape, n_hap)
    N, A, B, S, H = epx.pair_counts(ci, cj)
    deg = epx.degenerate(np.stack((N, A, B, S, H)))
    # a row missing everywhere: N = 0 against everything
    row, col = planted["all_missing"]
    assert not N[row].any() and not N[:, col].any() and deg[row].all() and deg[:, col].all()
    # a pair whose called sets are disjoint, both rows polymorphic and called elsewhere
    k = planted["disjoint"]
    assert N[k, k] == 0 and N[k].max() > 0 and N[:, k].max() > 0
    # polymorphic overall, monomorphic on its joint set with one partner
    k = planted["mono"]
    own = px.ind_planes(ci[k:k + 1])
    assert 0 < int(own[1].sum()) < 2 * int(own[0].sum())
    assert N[k, k] > 0 and A[k, k] == 0 and deg[k, k] and not deg[k].all()
    # an individual half-missing at one SNP is missing there
    k = planted["half"]
    assert N[k].max() < n_hap // 2 and N[k].max() == int(px.ind_planes(ci[k:k + 1])[0].sum())
    # the duplicate, complement and all-het rows of ld_em_exact.panel, with every call kept
    hi, hj, where = epx.holed()
    assert not px.complete_rows(hi).all() and not px.complete_rows(hj).all()
    for kind in ("duplicate", "complement", "all_het"):
        assert px.complete_rows(hj[where[kind]]).all(), kind
    assert np.array_equal(hi[0], hj[where["duplicate"][0]]) and np.array_equal(1 - hi[0], hj[where["complement"][0]])
    hN, _, _, _, hH = epx.pair_counts(hi, hj)
    assert hN[0, where["all_het"][0]] == HOLED_N and hN.min() < HOLED_N
    # the largest counts
    bi, bj, _ = epx.big()
    bN, bA, bB, bS, bH = epx.pair_counts(bi, bj)
    assert bN.max() == 5120 and bS[epx.ROW_ALT, epx.ROW_ALT] == 20480 and bH[epx.ROW_HET, epx.ROW_HET] == 5120
    assert bA.max() == 10240 and bB.max() == 10240


def test_em_host_on_the_pairs_own_integers_is_within_the_bound():
    from ld_tools_amd import em_host
    worst, worst_key, sizes = 0.0, None, set()
    for ci, cj, _ in (epx.mixed((129, 257), 254), epx.holed()):
        counts = epx.pair_counts(ci, cj)
        ii, jj = epx.sample_live(counts, SAMPLES, seed=ci.shape[0])
        assert ii.size == SAMPLES
        for key in sorted({tuple(int(v) for v in counts[:, i, j]) for i, j in zip(ii, jj)}):
            sizes.add(key[0])
            sol = emx.solve(*key)
            x, r, d = em_host(*key)
            assert 0.0 <= x <= key[4]
            err = emx.host_error(sol, r, d)
            if err > worst:
                worst, worst_key = err, key
    print(f"em_host on pairwise-complete tuples: {len(sizes)} distinct N, max error {worst:.3e} at {worst_key}")
    assert len(sizes) > 20 and worst <= emx.ABS_TOL
    # N = 0 and a SNP monomorphic within the joint set: the degenerate pair
    for key in ((0, 0, 0, 0, 0), (7, 0, 5, 0, 0), (7, 14, 5, 10, 0)):
        x, r, d = em_host(*key)
        assert x == 0.0 and r == 0.0 and d == 0.0 and math.copysign(1.0, r) < 0 and math.copysign(1.0, d) < 0, key


def test_a_panel_without_holes_reduces_to_the_plain_integers():
    shape, n_hap = (129, 257), 254
    ci, cj = px.complete_pair(shape, n_hap)
    N, A, B, S, H = epx.pair_counts(ci, cj)
    n_ind, a_i, a_j, S0, H0 = emx.pair_counts(ci, cj)
    assert (N == n_ind).all() and np.array_equal(S, S0) and np.array_equal(H, H0)
    assert np.array_equal(A, np.broadcast_to(a_i[:, None], shape)) and np.array_equal(B, np.broadcast_to(a_j[None, :], shape))


def test_case_lists_cover_what_the_gpu_tests_must():
    assert sorted({h for _, h in epx.COUNT_CASES}) == [2, 254, 256, 258, 1008, 5008]
    assert {s for s, _ in epx.COUNT_CASES} == set(rc.SHAPES) | {(257, 129)}
    assert all(h % 2 == 0 for _, h in rc.EDGE_CASES)                      # every edge case takes part
    assert epx.WALK_CASE[0][0] == 32 * epx.TILE + 1 and epx.BIG_CASE[1] == 10240

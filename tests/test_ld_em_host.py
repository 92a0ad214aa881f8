"""CPU: unphased LD by EM -- the fp64 restatement of the kernel's epilogue (ops.em_host) against the 60-digit oracle
(tests/ld_em_exact.py), the conditions the GPU test's panels must meet, and the oracle against its own definitions.

em_host must stay within 2^-40 of the oracle in r and in D' (at a near-best x: ties are accepted, not excluded) on
  * every live 3 x 3 genotype table of N = 1 .. 5 individuals (1801 tables),
  * 4000 seeded live pairs each of (129, 257) x 254 and (300, 130) x 1008,
  * the live pairs of (5, 130) x 10240.
The measured maximum is printed; DESIGN.md, "Unphased LD by EM", records it.
"""
import math
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_em_exact as emx  # noqa: E402

SAMPLED = (((129, 257), 254), ((300, 130), 1008))
SAMPLES = 4000


def tuples_of(shape, n_hap, count):
    ci, cj, _ = emx.panel(shape, n_hap)
    n_ind, a_i, a_j, S, H = emx.pair_counts(ci, cj)
    ii, jj = emx.sample_live(n_ind, a_i, a_j, S, H, count, seed=shape[0] + n_hap)
    return [(n_ind, int(a_i[i]), int(a_j[j]), int(S[i, j]), int(H[i, j])) for i, j in zip(ii, jj)]


def host_max_error(tuples):
    from ld_tools_amd import em_host
    worst, worst_key = 0.0, None
    for key in tuples:
        sol = emx.solve(*key)
        x, r, d = em_host(*key)
        assert 0.0 <= x <= key[4]
        err = emx.host_error(sol, r, d)
        if err > worst:
            worst, worst_key = err, key
    return worst, worst_key


def test_exhaustive_tables_count_and_host_error():
    tables = [(n,) + t for n in range(1, 6) for t in emx.live_tables(n)]
    assert len(tables) == 1801
    ties = sum(1 for key in tables if emx.solve(*key).ambiguous)
    print(f"exhaustive tables: {len(tables)}, {len(set(tables))} distinct tuples, {ties} tables are ties")
    assert all(emx.solve(*key).ambiguous for key in tables if key[0] == 1 and key[4] == 1)   # one individual, both het: a tie
    worst, key = host_max_error(sorted(set(tables)))
    print(f"em_host on the exhaustive tables: max error {worst:.3e} at {key}")
    assert worst <= emx.ABS_TOL


@pytest.mark.parametrize("shape,n_hap", SAMPLED + (emx.BIG_CASE,), ids=lambda v: str(v).replace(" ", ""))
def test_host_error_and_panel_conditions(shape, n_hap):
    tuples = tuples_of(shape, n_hap, SAMPLES)
    if (shape, n_hap) in SAMPLED:
        assert len(tuples) == SAMPLES
    else:
        assert 100 <= len(tuples) <= shape[0] * shape[1]     # (three of side I's five rows are degenerate)
    sols = [emx.solve(*key) for key in tuples]
    worst, key = host_max_error(tuples)
    print(f"em_host on {shape} x {n_hap}: {len(tuples)} live pairs, max error {worst:.3e} at {key}")
    assert worst <= emx.ABS_TOL
    # conditions on the oracle alone: few ties; where it is asked, enough pairs whose likelihood comparison is exercised
    ambiguous = sum(s.ambiguous for s in sols)
    three = sum(s.three_real for s in sols)
    two_maxima = sum(len(s.roots) > 1 for s in sols)
    print(f"  ambiguous {ambiguous}, three real roots {three} ({three / len(sols):.1%}), more than one root in [0, H] {two_maxima}")
    assert ambiguous <= 0.01 * len(sols)
    if (shape, n_hap) == ((129, 257), 254):
        assert three >= 0.05 * len(sols)


def test_oracle_self_checks():
    keys = [(n,) + t for n in range(1, 6) for t in sorted(set(emx.live_tables(n)))]
    for shape, n_hap in SAMPLED + (emx.BIG_CASE,):
        keys += tuples_of(shape, n_hap, SAMPLES)[::10]
    for key in keys:
        assert emx.table(*key) is not None
        emx.self_check(emx.solve(*key))
    assert len(keys) > 1000


def test_panels_carry_the_special_pairs():
    """What tests/test_gpu_ld_em.py relies on: the planted pairs are what their names say, on the integer counts."""
    for shape, n_hap in emx.DENSE_CASES:
        ci, cj, where = emx.panel(shape, n_hap)
        n_ind, a_i, a_j, S, H = emx.pair_counts(ci, cj)
        T = 2 * n_ind
        dup, comp = where["duplicate"][0], where["complement"][0]
        assert a_i[0] == a_j[dup] and S[0, dup] == a_i[0] + 2 * int((emx.dx.dosages(ci[:1]) == 2).sum())   # S = Q
        assert a_i[0] + a_j[comp] == T
        assert a_j[where["mono"][0]] == 0 and a_j[where["all_alt"][0]] == T
        het = where["all_het"][0]
        assert a_j[het] == n_ind and H[:, het].max() <= n_ind
    ci, cj, where = emx.panel(*emx.BIG_CASE, extremes=True)
    n_ind, a_i, a_j, S, H = emx.pair_counts(ci, cj)
    assert S[3, where["all_alt"][0]] == 4 * n_ind == 20480 and H[2, where["all_het"][0]] == n_ind == 5120


def test_em_host_degenerate_and_malformed():
    from ld_tools_amd import em_host
    x, r, d = em_host(3, 0, 2, 0, 0)
    assert x == 0.0 and math.copysign(1.0, r) < 0 and r == 0.0 and math.copysign(1.0, d) < 0 and d == 0.0
    for bad in ((3, 2, 2, 2, 1), (3, 7, 2, 0, 0), (3, 2, 2, 4, 4), (3, 1, 1, 3, 1), (3, 2, 2, 0, 1)):
        assert emx.table(*bad) is None
        assert all(math.isnan(v) for v in em_host(*bad)), bad
    # H = 0: the closed form; r = +0.0 iff T n1 = a_i a_j
    x, r, d = em_host(2, 2, 2, 2, 0)    # genotypes (2, 0) and (0, 2) ... n1 = 1, T n1 - a_i a_j = 0
    assert x == 0.0 and r == 0.0 and math.copysign(1.0, r) > 0

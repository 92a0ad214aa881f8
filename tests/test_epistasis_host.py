"""CPU: the epistasis scan (include/ldx.h, "epistasis scan") on the host mirrors and the exact oracle (tests/ld_epistasis_exact.py)
-- the counts against a per-individual loop, the fitted table against the observed margins, the cycle cap, the accuracy of both
statistics, their symmetry, the flags, the tails, the writers' text and the refusals.

The accuracy contract of the header is |chisq - exact| <= BOUND max(exact, 1) with BOUND = 8 x the worst error the numpy mirror
shows on the oracle's tuples (the factor allows for the device's own log).  This file measures that worst error and checks that the
written bounds (_lib.EPI_REL_BOUND: 2^-46 allelic, 4.17e-12 boost) are what it gives: no smaller than the mirror's error, no larger
than 8 x it.  Measured here: allelic 1.78e-15, boost 5.22e-13 (a table of 3290 individuals with G2 = 1.17: the stop rule's
residue and the cancellation in the sum of n ln(n / mu), which is why the boost bound is looser than 2^-40)."""
import math
from decimal import Decimal

import numpy as np
import pytest

import ld_epistasis_exact as X

from ld_tools_amd import (LdxError, _lib, epi_allelic_host, epi_boost_host, epi_chisq_bound, epi_counts_host,  # noqa: I100
                          epi_tail_host)

TR = [(k // 9) * 9 + (k % 3) * 3 + (k % 9) // 3 for k in range(18)]


@pytest.fixture(scope="module")
def mirrors():
    """The tuples, the oracle and both mirrors, computed once and left unchanged."""
    t = X.tuples()
    return t, X.oracle(), epi_allelic_host(t.T), epi_boost_host(t.T)


def test_counts_against_brute_force():
    n_ind = 61
    case = X.case_vector(n_ind, 23, 31, seed=3)
    ci = X.epi_codes(7, n_ind, seed=1, miss=0.08)
    cj = X.epi_codes(5, n_ind, seed=2, miss=0.08)
    ci[0, 4] = 3   # a second-ALT code: missing
    got, want = epi_counts_host(ci, cj, case), X.tables_brute(ci, cj, case)
    assert got.shape == (18, 7, 5) and got.dtype == np.int64 and np.array_equal(got, want)
    assert got[:9].sum(axis=0).max() <= 23 and got[9:].sum(axis=0).max() <= 31
    assert np.array_equal(epi_counts_host(cj, ci, case), want.transpose(0, 2, 1)[TR])


def test_tuple_kinds(mirrors):
    """The generator covers what the header's statements are made on."""
    t, _, _, (_, cycles, _, flags) = mirrors
    sums = np.stack([t[:, :9].sum(axis=1), t[:, 9:].sum(axis=1)], axis=1)
    assert (sums == 0).any(axis=0).all()                    # an empty group, either one
    assert (sums == 1).any(axis=0).all()                    # single-individual groups
    assert (sums == X.MAX_GROUP).all(axis=1).any()          # totals at the limit
    assert sums.max() <= X.MAX_GROUP
    assert ((t == 0).sum(axis=1) >= 4).sum() >= 20          # sampling zeros
    assert (flags & 8).any() and not (flags & 8).all()
    ab = t[:, :9] + t[:, 9:]
    assert ((ab == 0).any(axis=1) & (sums > 0).all(axis=1)).any()
    xor = np.array([((k // 3) == 1) != ((k % 3) == 1) for k in range(9)])
    assert ((t[:, :9][:, ~xor] == 0).all(axis=1) & (t[:, 9:][:, xor] == 0).all(axis=1) & (sums >= 150).all(axis=1)).sum() >= 3


def test_mu_margins_and_cycle_cap(mirrors):
    """The fitted table reproduces the three two-way margins to the stop rule, and no tuple without flag 8 reaches the cap.  A
    cell moves by at most 2^-40 N in the last cycle, so after it a margin of up to six cells is within 6 x 2^-40 N of the
    observed one (the last step fits the SNP j x group margins exactly up to rounding; the other two moved by at most that)."""
    t, _, _, (mu, cycles, _, flags) = mirrors
    mu = mu.T
    cap = _lib.EPI_MAX_CYCLES
    fitted = (flags & (1 | 4)) == 0
    assert fitted.sum() >= 80
    free = (flags & (1 | 8)) == 0
    assert cycles[free].max() == cap and not (flags[free] & 4).any()   # the cap is the smallest that holds
    assert (cycles <= cap).all() and (cycles[(flags & 1) != 0] == 0).all()
    assert ((flags & 4) != 0).sum() >= 1 and (flags[(flags & 4) != 0] & 8).all()
    for k in np.nonzero(fitted)[0]:
        n, m = t[k].astype(np.float64).reshape(2, 3, 3), mu[k].reshape(2, 3, 3)
        tol = 6.0 * 2.0 ** -40 * n.sum()
        for axis in (0, 1, 2):
            assert np.abs(n.sum(axis=axis) - m.sum(axis=axis)).max() <= tol, (k, axis)
        assert (m[n > 0] > 0).all()


def test_accuracy_against_oracle(mirrors):
    t, oracle, (x2, d, fa), (_, _, g2, fb) = mirrors
    worst = {"allelic": 0.0, "boost": 0.0}
    for k, ((ac, ad, af), (bg, bf, _)) in enumerate(oracle):
        assert fa[k] == af and (fb[k] & 2) == af
        if ac is None:
            assert math.isnan(x2[k]) and math.isnan(d[k])
        else:
            worst["allelic"] = max(worst["allelic"], X.rel_error(x2[k], ac))
            assert abs(Decimal(float(d[k])) - ad) <= Decimal(2.0 ** -46) * max(abs(ad), Decimal(1))
        assert (fb[k] & 1) == (bf & 1) and (fb[k] & 8) == (bf & 8)
        if fb[k] & 1:
            assert math.isnan(g2[k])
        elif not fb[k] & 4:
            assert bg is not None, "a fit the mirror finished must be one the oracle finishes"
            worst["boost"] = max(worst["boost"], X.rel_error(g2[k], bg))
    print("worst relative error of the numpy mirror:", worst)
    for test, w in worst.items():
        bound = _lib.EPI_REL_BOUND[test]
        assert w <= bound <= 8.0 * w, (test, w, bound)
    assert _lib.EPI_REL_BOUND["allelic"] <= 2.0 ** -40


def test_header_states_the_measured_numbers():
    import re
    from pathlib import Path

    text = (Path(__file__).resolve().parents[1] / "include" / "ldx.h").read_text()
    assert re.search(rf"#define LDX_EPI_MAX_CYCLES {_lib.EPI_MAX_CYCLES}u\b", text)
    assert float.fromhex(re.search(r"#define LDX_EPI_REL_BOUND_ALLELIC (\S+)", text).group(1)) == _lib.EPI_REL_BOUND["allelic"]
    assert float(re.search(r"#define LDX_EPI_REL_BOUND_BOOST (\S+)", text).group(1)) == _lib.EPI_REL_BOUND["boost"]
    assert "NOT validated against PLINK" in text[text.index("epistasis scan"):]
    assert _lib.EPI_TESTS == {"allelic": 0, "boost": 1} and _lib.MAX_HAPS // 2 == X.MAX_GROUP
    for name in ("ldx_epi_counts_dev", "ldx_epi_rect_dev", "ldx_epi_hits_dev", "ldx_epi_from_counts_dev"):
        assert re.search(rf"\bint {name}\(", text) and name in _lib.SIGNATURES and hasattr(_lib.lib, name)


def test_symmetry_under_snp_swap(mirrors):
    t, _, (x2, d, fa), (mu, cycles, g2, fb) = mirrors
    s = t[:, TR]
    assert not np.array_equal(s, t)
    x2s, ds, fas = epi_allelic_host(s.T)
    mus, cycs, g2s, fbs = epi_boost_host(s.T)
    same = lambda a, b: np.array_equal(a.view(np.int64), b.view(np.int64))  # noqa: E731
    assert same(x2, x2s) and same(d, ds) and np.array_equal(fa, fas)
    assert same(g2, g2s) and np.array_equal(cycles, cycs) and np.array_equal(fb, fbs)
    assert same(np.ascontiguousarray(mu[TR]), np.ascontiguousarray(mus))


def test_flags_by_hand():
    base = np.array([5, 6, 7, 8, 9, 10, 11, 12, 13, 3, 4, 5, 6, 7, 8, 9, 10, 11])
    assert epi_allelic_host(base)[2] == 0 and epi_boost_host(base)[3] == 0
    t = base.copy()
    t[:9] = 0
    x2, d, f = epi_allelic_host(t)
    mu, cyc, g2, fb = epi_boost_host(t)
    assert f == 2 and math.isnan(x2) and math.isnan(d) and fb == 3 and math.isnan(g2) and cyc == 0 and np.isnan(mu).all()
    t = base.copy()
    t[[6, 7, 8]] = 0          # no case with g_i = 2: a zero in the SNP i x group margin
    mu, cyc, g2, fb = epi_boost_host(t)
    assert fb & 8 and not fb & 1 and g2 >= 0.0 and (mu[[6, 7, 8]] == 0.0).all()
    assert epi_allelic_host(t)[2] == 0
    t = np.zeros(18, dtype=np.int64)
    t[0], t[9] = 4, 7         # everybody homozygous REF at both: three allele cells of each group are 0
    assert epi_allelic_host(t)[2] == 2 and epi_boost_host(t)[3] == (2 | 8)
    assert epi_boost_host(t)[2] == 0.0
    capped = epi_boost_host(base, max_cycles=2)
    assert capped[3] == 4 and capped[1] == 2 and capped[2] > 0.0
    # a product table has no interaction at all: G2 is 0 up to rounding, and never negative
    prod = np.outer([2, 3, 5], [1, 4, 2]).reshape(-1)
    assert 0.0 <= epi_boost_host(np.concatenate([prod, 3 * prod]))[2] < 1e-9


def test_tails_against_decimal():
    xs = np.array([0.0, 1e-9, 0.3, 1.0, 3.84, 15.13, 23.5, 49.9, 50.1, 200.0, 1500.0, 4e4])
    for test in ("allelic", "boost"):
        ln_p, p, nlp = epi_tail_host(xs, test)
        assert ln_p[0] == 0.0 and p[0] == 1.0 and nlp[0] == 0.0
        for x, got in zip(xs[1:], ln_p[1:]):
            want = X.ln_tail_exact(Decimal(float(x)), test)
            assert abs(Decimal(float(got)) - want) <= Decimal(2.0 ** -30) * max(Decimal(1), abs(want)), (test, x)
        assert np.isfinite(nlp).all() and p[-1] == 0.0 and nlp[-1] > 4000
        assert math.isnan(epi_tail_host(np.nan, test)[0])
    for test, df_bound in (("allelic", 15.1367), ("boost", 23.5127)):
        b = epi_chisq_bound(1e-4, test)
        assert isinstance(b, np.float32) and b == pytest.approx(df_bound, rel=1e-5)
        below = np.nextafter(b, np.float32(0))
        assert epi_tail_host(float(b), test)[0] <= math.log(1e-4) < epi_tail_host(float(below), test)[0]


def _tiny_table():
    import torch

    from ld_tools_amd import EpiHits, EpiSummary
    from ld_tools_amd.drivers.epistasis import EpiTable

    x = np.array([30.5, 24.0, 3000.0], dtype=np.float32)
    d = np.array([0.75, np.nan, -2.5], dtype=np.float32)
    hits = np.stack([np.array([1, 2, 2]), np.array([0, 0, 1]), x.view(np.int32), d.view(np.int32)], axis=1).astype(np.int32)
    summary = EpiSummary(torch.tensor([2, 2, 2, 0], dtype=torch.int32), torch.tensor([2, 2, 2, 0], dtype=torch.int32),
                         torch.tensor([30.5, 3000.0, 3000.0, np.nan], dtype=torch.float32), torch.tensor([1, 2, 1, -1]),
                         np.float32(13.28))
    res = EpiHits(torch.tensor([0, 0, 1, 3, 3], dtype=torch.int32), torch.from_numpy(hits), 4, 4, np.float32(23.51), "boost", True,
                  summary)
    return EpiTable(["1", "1", "2", "2"], ["rsA", "rsB", "rsC", "rsD"], ["1", "1", "2", "2"], ["rsA", "rsB", "rsC", "rsD"], res)


def test_writers_text(tmp_path):
    from ld_tools_amd.drivers import epistasis as W

    table = _tiny_table()
    assert W.write_epi_cc(str(tmp_path / "x.epi.cc"), table) == 3
    lines = [ln.split("\t") for ln in (tmp_path / "x.epi.cc").read_text().splitlines()]
    assert tuple(lines[0]) == W.EPI_CC_COLUMNS == ("CHR1", "SNP1", "CHR2", "SNP2", "STAT", "DIR", "P")
    assert lines[1][:6] == ["1", "rsB", "1", "rsA", "30.5", "0.75"]
    assert float(lines[1][6]) == pytest.approx(math.exp(-15.25) * 16.25, rel=1e-12)
    assert lines[2][:6] == ["2", "rsC", "1", "rsA", "24.0", "NA"]
    # p = e^-1500 1501 is below the float64 range: written with its exponent, as .glm.linear does
    assert lines[3][:6] == ["2", "rsC", "1", "rsB", "3000.0", "-2.5"]
    m = lines[3][6].split("e")
    want = (-1500.0 + math.log(1501.0)) / math.log(10.0)
    assert int(m[1]) == math.floor(want) and float(m[0]) == pytest.approx(10.0 ** (want - math.floor(want)), rel=1e-5)
    assert W.write_epi_summary(str(tmp_path / "x.epi.cc.summary"), table) == 4
    lines = [ln.split("\t") for ln in (tmp_path / "x.epi.cc.summary").read_text().splitlines()]
    assert tuple(lines[0]) == W.EPI_SUMMARY_COLUMNS == ("CHR", "SNP", "N_SIG", "N_TOT", "PROP", "BEST_CHISQ", "BEST_CHR", "BEST_SNP")
    assert lines[1] == ["1", "rsA", "2", "2", "1.0", "30.5", "1", "rsB"]
    assert lines[3] == ["2", "rsC", "2", "2", "1.0", "3000.0", "1", "rsB"]
    assert lines[4] == ["2", "rsD", "0", "0", "NA", "NA", "NA", "NA"]


def test_refusals():
    from ld_tools_amd import ld_epistasis, ld_epistasis_counts, ld_epistasis_from_counts, ld_epistasis_hits
    from ld_tools_amd.drivers.plink import Bfile, bfile_epistasis

    with pytest.raises(LdxError, match="test must be one of"):
        ld_epistasis(None, np.zeros(4), test="joint-effects")
    with pytest.raises(LdxError, match="test must be one of"):
        ld_epistasis_hits(None, np.zeros(4), test="case-only")
    with pytest.raises(LdxError, match="pairwise-complete"):
        ld_epistasis(None, np.zeros(4), missing="ref")
    with pytest.raises(LdxError, match="pairwise-complete"):
        ld_epistasis_counts(None, np.zeros(4), missing="mean")
    with pytest.raises(LdxError, match="bound must be > 0"):
        ld_epistasis_hits(None, np.zeros(4), chisq=0.0)
    with pytest.raises(LdxError, match=r"\(0, 1\)"):
        ld_epistasis_hits(None, np.zeros(4), p=0.0)
    with pytest.raises(LdxError, match=r"\[18, \.\.\.\]"):
        ld_epistasis_from_counts(np.zeros((17, 3), dtype=np.int64))
    with pytest.raises(LdxError, match="negative"):
        ld_epistasis_from_counts(-np.ones((18, 3), dtype=np.int64))
    big = np.zeros((18, 1), dtype=np.int64)
    big[4] = X.MAX_GROUP + 1
    with pytest.raises(LdxError, match="LDX_MAX_HAPS / 2"):
        ld_epistasis_from_counts(big)
    with pytest.raises(LdxError, match="even number of haplotypes"):
        epi_counts_host(np.zeros((2, 7), dtype=np.int8), np.zeros((2, 7), dtype=np.int8), np.zeros(3))
    with pytest.raises(LdxError, match="case must be a vector"):
        epi_counts_host(np.zeros((2, 8), dtype=np.int8), np.zeros((2, 8), dtype=np.int8), np.array([0, 1, 2, 0.0]))

    iid = [f"i{k}" for k in range(6)]
    bf = Bfile("x", None, "a1", ["1"] * 3, ["rs1", "rs2", "rs3"], np.zeros(3), np.arange(3), ["A"] * 3, ["G"] * 3, iid, iid,
               ["0"] * 6, ["0"] * 6, ["1"] * 6, ["-9"] * 6)
    quantitative = (iid, iid, ["height"], np.array([1.5, 1.7, 1.6, 1.8, 1.4, 1.9])[:, None])
    with pytest.raises(LdxError, match="bfile_epistasis.*quantitative trait belongs to bfile_glm"):
        bfile_epistasis(bf, quantitative)
    with pytest.raises(LdxError, match="bfile_epistasis.*no value"):
        bfile_epistasis(bf)       # the .fam's column is all -9
    cc = (iid, iid, ["cc"], np.array([1, 2, 1, 2, 1, 2.0])[:, None])
    with pytest.raises(LdxError, match="unknown variant"):
        bfile_epistasis(bf, cc, set_i=["rs1", "rs9"])
    with pytest.raises(LdxError, match="lists of variant IDs"):
        bfile_epistasis(bf, cc, set_j=[])

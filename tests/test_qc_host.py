"""CPU: genotype QC and table tests (include/ldx.h, "genotype QC and table tests") on the oracle and the host mirrors -- pinned
values, the HWE distribution against brute-force enumeration, Fisher against math.comb (and scipy where it imports), the mirrors
against the exact oracle (tests/ld_qc_exact.py), the group counts against loops, the writers' columns and the refusals.

Bounds: ln p is held to the definition's 2^-30 max(1, |ln p|).  The chi-square mirror is compared with the exact rational at
CHISQ_REL = 2^-49: a statistic is three or, for the genotypic test, seventeen fp64 operations on exactly converted integers, each
within 2^-53 relatively and all terms of the genotypic sum positive, so 17 x 2^-53 < 2^-48.9 bounds it."""
import ctypes as C
import math
from fractions import Fraction
from math import comb

import numpy as np
import pytest

import ld_qc_exact as X

CHISQ_REL = 2.0 ** -48.9


def test_pinned_values():
    p, flag = X.hwe_exact(100, 13, 4)
    assert flag == 0 and p == Fraction(236998165861271, 23024209048998807)
    assert float(p) == pytest.approx(0.0102934, rel=1e-5)
    assert float(X.hwe_exact(100, 13, 4, midp=True)[0]) == pytest.approx(0.00560615, rel=1e-5)
    assert float(X.hwe_exact(100, 5, 8)[0]) == pytest.approx(2.13070431e-8, rel=1e-8)
    assert X.hwe_exact(6, 2, 1) == (Fraction(1), 0) and X.hwe_exact(6, 4, 0) == (Fraction(1), 0)      # the tie: 4 ALT alleles
    assert X.fisher_exact(3, 1, 1, 3) == (Fraction(17, 35), 0)
    assert float(X.fisher_exact(10, 30, 30, 10)[0]) == pytest.approx(1.48748e-5, rel=1e-5)
    assert float(X.ln_fraction(X.hwe_exact(2560, 2560, 0)[0]) / X.LN10) == pytest.approx(-768.68, abs=0.01)
    assert float(X.ln_fraction(X.hwe_exact(5120, 0, 2560)[0]) / X.LN10) == pytest.approx(-1541.12, abs=0.01)


def test_hwe_distribution_against_enumeration():
    for n in range(1, 6):
        for nA in range(1, 2 * n):
            brute = X.hwe_brute(n, nA)
            total = sum(brute.values())
            k0 = nA & 1
            hom = (nA - k0) // 2
            w, io = X.hwe_weights(n, k0, hom)
            assert io == 0
            ks = list(range(k0, min(nA, 2 * n - nA) + 1, 2))
            assert sorted(brute) == ks
            for k, wk in zip(ks, w):
                assert Fraction(wk, sum(w)) == Fraction(brute[k], total), (n, nA, k)


def test_fisher_against_comb_and_scipy():
    tables = [(3, 1, 1, 3), (10, 30, 30, 10), (0, 5, 7, 2), (12, 3, 4, 9), (7, 7, 7, 7), (1, 0, 0, 1), (20, 1, 2, 30), (5, 0, 0, 9)]
    for a, b, c, d in tables:
        r1, r2, c1, n = a + b, c + d, a + c, a + b + c + d
        lo, hi = max(0, c1 - r2), min(r1, c1)
        probs = {x: Fraction(comb(r1, x) * comb(r2, c1 - x), comb(n, c1)) for x in range(lo, hi + 1)}
        assert sum(probs.values()) == 1
        want = sum(q for q in probs.values() if q <= probs[a] * X.TIE)
        assert X.fisher_exact(a, b, c, d)[0] == want
        assert X.fisher_exact(a, b, c, d, midp=True)[0] == want - probs[a] / 2
    stats = pytest.importorskip("scipy.stats")
    for a, b, c, d in tables:
        assert float(X.fisher_exact(a, b, c, d)[0]) == pytest.approx(stats.fisher_exact([[a, b], [c, d]])[1], rel=1e-12)


def test_small_configurations_are_admissible_and_hold_ties():
    closest, ties = Fraction(1), 0
    for n, het, hom in X.small_hwe_tuples(30):
        if 0 < het + 2 * hom < 2 * n:
            w, io = X.hwe_weights(n, het, hom)
            assert X.admissible(w, io)
            closest = min(closest, X.closest_non_tie(w, io))
            ties += sum(1 for x in w if x == w[io]) - 1
    for t in X.balanced_tables(40):
        if min(t[0] + t[1], t[2] + t[3], t[0] + t[2], t[1] + t[3]) > 0:
            w, io = X.fisher_weights(*t)
            assert X.admissible(w, io)
            closest = min(closest, X.closest_non_tie(w, io))
            ties += sum(1 for x in w if x == w[io]) - 1
    print(f"closest non-tie ratio is {float(closest):.3g} from 1; {ties} exact ties")
    assert closest > Fraction(1, 1 << 20) and ties > 100


@pytest.mark.parametrize("midp", (False, True))
def test_exact_mirrors_against_the_oracle(midp):
    from ld_tools_amd import fisher_exact_host, hwe_exact_host

    hw = X.small_hwe_tuples(12) + [(0, 0, 0), (100, 13, 4), (100, 5, 8), (700, 300, 10), (2560, 2560, 0), (5120, 0, 2560), (5120, 2496, 1200)]
    p, nlp, flags = hwe_exact_host(*(np.array(c) for c in zip(*hw)), midp=midp)
    worst = X.check_exact("hwe", hw, midp, p, nlp, flags)
    fi = X.balanced_tables(16) + [(0, 0, 0, 0), (3, 0, 5, 0), (5120, 5120, 0, 10240), (10, 30, 30, 10), (2000, 3000, 2500, 2740)]
    p, nlp, flags = fisher_exact_host(*(np.array(c) for c in zip(*fi)), midp=midp)
    worst = max(worst, X.check_exact("fisher", fi, midp, p, nlp, flags))
    print(f"midp={midp}: largest ln p error / bound = {worst:.3g}")


def test_model_mirror_against_the_oracle():
    from ld_tools_amd import model_tests_host

    tuples = X.model_tuples()
    seen = set()
    for min_cell in (4, 5, 6):
        outs = model_tests_host(*(np.array(c) for c in zip(*tuples)), min_cell=min_cell)
        s, worst = X.check_model(tuples, min_cell, *outs, rel=CHISQ_REL)
        seen |= s
        print(f"min_cell={min_cell}: largest tail error / bound = {worst:.3g}")
    assert seen == {0, 1, 2, 3}
    cell5 = tuples.index((40, 20, 5, 50, 25, 5))
    assert [int(model_tests_host(*(np.array([c]) for c in tuples[cell5]), min_cell=m)[4][0, 2]) for m in (4, 5, 6)] == [0, 0, 3]


def test_group_counts_host_against_loops():
    from ld_tools_amd import geno_group_counts_host

    codes = X.qc_codes(37, 20, seed=2, miss=0.1)
    keep = np.arange(20) % 4 != 1
    for name, groups in X.group_sets(37, seed=5).items():
        got, sizes = geno_group_counts_host(codes, groups, keep)
        assert got.dtype == np.uint32 and got.shape == (20, groups.shape[0], 4)
        assert np.array_equal(sizes, groups.sum(axis=1))
        want = np.zeros(got.shape, dtype=np.int64)
        for s in range(20):
            if not keep[s]:
                continue
            for a in range(37):
                h0, h1 = int(codes[s, 2 * a]), int(codes[s, 2 * a + 1])
                if h0 in (0, 1) and h1 in (0, 1):
                    for g in np.flatnonzero(groups[:, a]):
                        want[s, g, 0] += 1
                        want[s, g, 1] += h0 + h1 == 1
                        want[s, g, 2] += h0 + h1 == 2
        assert np.array_equal(got, want), name
    labels = np.array([0, 2, 2, 5] * 9 + [5], dtype=np.float64)
    labels[3] = np.nan
    got, sizes = geno_group_counts_host(codes, labels)
    assert sizes.tolist() == [9, 18, 9] and got.shape == (20, 3, 4)
    by_matrix, _ = geno_group_counts_host(codes, np.stack([labels == 0, labels == 2, labels == 5]))
    assert np.array_equal(got, by_matrix)


def test_sample_qc_host():
    from ld_tools_amd import geno_matmul_host, sample_qc_host
    from ld_tools_amd.ops import het_weights
    from ld_tools_amd import geno_counts_host

    codes = X.qc_codes(37, 50, seed=4, miss=0.05)
    keep = np.arange(50) % 7 != 2
    qc = sample_qc_host(codes, keep)
    h0, h1 = codes[keep][:, 0::2], codes[keep][:, 1::2]
    called = (h0 != 2) & (h1 != 2)
    assert np.array_equal(qc.called, called.sum(axis=0)) and qc.n_kept == int(keep.sum())
    assert np.array_equal(qc.het, (called & (h0 != h1)).sum(axis=0))
    assert np.array_equal(qc.hom, (called & (h0 == 1) & (h1 == 1)).sum(axis=0))
    q, exps = het_weights(geno_counts_host(codes, keep))
    y = geno_matmul_host(codes, np.zeros_like(q), q, keep)[:, 0]
    e_hom = y.astype(np.float64) * 2.0 ** float(exps[0] - 30)
    assert np.array_equal(qc.e_hom, e_hom)
    assert np.array_equal(qc.f, ((qc.called - qc.het) - e_hom) / (qc.called - e_hom))
    # against a float sum of the definition, to the quantisation of the weights (2^-30 per SNP)
    c = geno_counts_host(codes, keep).astype(np.int64)
    n, a = c[:, 0], c[:, 1] + 2 * c[:, 2]
    e = np.where(n > 0, 1.0 - a * (2 * n - a) / np.maximum(n * (2 * n - 1), 1), 0.0)
    full = np.zeros((50, 37))
    full[keep] = called
    assert np.abs(qc.e_hom - (full * e[:, None]).sum(axis=0)).max() <= 50 * 2.0 ** -30
    assert np.isfinite(qc.f).all() and np.abs(qc.f).max() < 1.0


def test_writers_columns(tmp_path):
    from ld_tools_amd import (HardyResult, MissingResult, ModelResult, fisher_exact_host, geno_group_counts_host, hwe_exact_host,
                              model_tests_host, sample_qc_host)
    from ld_tools_amd.drivers import qc as W

    n_ind, n_snps = 30, 9
    codes = X.qc_codes(n_ind, n_snps, seed=6, miss=0.1)
    case = X.case_vector(n_ind, seed=1)
    counts, sizes = geno_group_counts_host(codes, np.stack([np.ones(n_ind, dtype=bool), case == 1, case == 0]))
    variants = W.QcVariants(["6"] * n_snps, [100 + 10 * k for k in range(n_snps)], [f"rs{k}" for k in range(n_snps)], ["G"] * n_snps,
                            ["A"] * n_snps)
    c64 = counts.astype(np.int64)
    flat = c64.reshape(-1, 4)
    p, nlp, flags = hwe_exact_host(flat[:, 0], flat[:, 1], flat[:, 2])
    with np.errstate(all="ignore"):
        o = flat[:, 1] / flat[:, 0]
        a = flat[:, 1] + 2 * flat[:, 2]
        e = a * (2 * flat[:, 0] - a) / (2.0 * flat[:, 0] ** 2)
    shape = (n_snps, 3)
    hardy = HardyResult(counts, sizes, [0, 1, 2], o.reshape(shape), e.reshape(shape), p.reshape(shape), nlp.reshape(shape),
                        flags.reshape(shape))
    assert W.write_hardy(str(tmp_path / "x.hardy"), variants, hardy, 1) == n_snps
    lines = [ln.split("\t") for ln in (tmp_path / "x.hardy").read_text().splitlines()]
    assert tuple(lines[0]) == W.HARDY_COLUMNS
    for k, ln in enumerate(lines[1:]):
        assert ln[:4] == ["6", f"rs{k}", "G", "A"]
        assert [int(v) for v in ln[4:7]] == [c64[k, 1, 2], c64[k, 1, 1], c64[k, 1, 0] - c64[k, 1, 1] - c64[k, 1, 2]]
        if c64[k, 1, 0]:
            assert float(ln[7]) == o.reshape(shape)[k, 1] and float(ln[8]) == e.reshape(shape)[k, 1] and float(ln[9]) == p.reshape(shape)[k, 1]
        else:
            assert ln[7:] == ["NA", "NA", "NA"]
    assert lines[8][7:] == ["NA", "NA", "NA"]                    # SNP 7 has no call

    outs = model_tests_host(c64[:, 1, 0], c64[:, 1, 1], c64[:, 1, 2], c64[:, 2, 0], c64[:, 2, 1], c64[:, 2, 2], min_cell=2)
    alt_c, alt_u = c64[:, 1, 1] + 2 * c64[:, 1, 2], c64[:, 2, 1] + 2 * c64[:, 2, 2]
    fp = fisher_exact_host(alt_c, 2 * c64[:, 1, 0] - alt_c, alt_u, 2 * c64[:, 2, 0] - alt_u)
    model = ModelResult(*outs, *fp, counts[:, 1], counts[:, 2], int(sizes[1]), int(sizes[2]))
    assert W.write_model(str(tmp_path / "x.model"), variants, model) == 5 * n_snps
    lines = [ln.split("\t") for ln in (tmp_path / "x.model").read_text().splitlines()]
    assert tuple(lines[0]) == W.MODEL_COLUMNS and [ln[4] for ln in lines[1:6]] == list(W.MODEL_ORDER)
    from ld_tools_amd import MODEL_TESTS
    for k in range(n_snps):
        for j, test in enumerate(W.MODEL_ORDER):
            ln, t = lines[1 + 5 * k + j], MODEL_TESTS.index(test)
            assert ln[:5] == ["6", f"rs{k}", "G", "A", test]
            if outs[4][k, t]:
                assert ln[7:] == ["NA", "NA", "NA"]
            else:
                assert float(ln[7]) == outs[0][k, t] and int(ln[8]) == (2 if test == "GENO" else 1) and float(ln[9]) == outs[1][k, t]
        geno = lines[1 + 5 * k]
        assert [int(v) for v in geno[5].split("/")] == [c64[k, 1, 2], c64[k, 1, 1], c64[k, 1, 0] - c64[k, 1, 1] - c64[k, 1, 2]]
        assert [int(v) for v in lines[3 + 5 * k][6].split("/")] == [alt_u[k], 2 * c64[k, 2, 0] - alt_u[k]]
    assert W.write_assoc_fisher(str(tmp_path / "x.assoc.fisher"), variants, model) == n_snps
    lines = [ln.split() for ln in (tmp_path / "x.assoc.fisher").read_text().splitlines()]
    assert tuple(lines[0]) == W.FISHER_COLUMNS
    for k, ln in enumerate(lines[1:]):
        assert ln[1] == f"rs{k}" and int(ln[2]) == 100 + 10 * k
        assert ln[7] == "NA" if np.isnan(fp[0][k]) else float(ln[7]) == fp[0][k]
    from ld_tools_amd.drivers.plink import _read_pvalues
    got = _read_pvalues(str(tmp_path / "x.assoc.fisher"), variants.ids, "SNP", "P")
    assert np.array_equal(got, fp[0], equal_nan=True)

    miss = MissingResult(1.0 - c64[:, 1, 0] / sizes[1], 1.0 - c64[:, 2, 0] / sizes[2],
                         *fisher_exact_host(sizes[1] - c64[:, 1, 0], c64[:, 1, 0], sizes[2] - c64[:, 2, 0], c64[:, 2, 0]),
                         counts[:, 1:, 0], int(sizes[1]), int(sizes[2]))
    assert W.write_test_missing(str(tmp_path / "x.missing"), variants, miss) == n_snps
    lines = [ln.split("\t") for ln in (tmp_path / "x.missing").read_text().splitlines()]
    assert tuple(lines[0]) == W.TEST_MISSING_COLUMNS and float(lines[2][2]) == miss.f_miss_case[1]

    assert W.write_vmiss(str(tmp_path / "x.vmiss"), variants, counts[:, 0, 0], n_ind) == n_snps
    lines = [ln.split("\t") for ln in (tmp_path / "x.vmiss").read_text().splitlines()]
    assert tuple(lines[0]) == W.VMISS_COLUMNS
    assert [int(ln[2]) for ln in lines[1:]] == (n_ind - c64[:, 0, 0]).tolist() and lines[8][4] == "1.0"
    qc = sample_qc_host(codes)
    fid, iid = [f"F{k}" for k in range(n_ind)], [f"I{k}" for k in range(n_ind)]
    assert W.write_smiss(str(tmp_path / "x.smiss"), fid, iid, qc) == n_ind
    assert W.write_het(str(tmp_path / "x.het"), fid, iid, qc) == n_ind
    lines = [ln.split("\t") for ln in (tmp_path / "x.smiss").read_text().splitlines()]
    assert tuple(lines[0]) == W.SMISS_COLUMNS and [int(ln[2]) for ln in lines[1:]] == (n_snps - qc.called).tolist()
    lines = [ln.split("\t") for ln in (tmp_path / "x.het").read_text().splitlines()]
    assert tuple(lines[0]) == W.HET_COLUMNS
    assert [float(ln[5]) for ln in lines[1:]] == qc.f.tolist() and [int(ln[2]) for ln in lines[1:]] == (qc.called - qc.het).tolist()


def test_refusals():
    from ld_tools_amd import (LdxError, _lib, fisher_exact_host, geno_group_counts_host, hwe_exact_host, ld_hardy, ld_model,
                              ld_test_missing, model_tests_host, sample_qc)

    lib, E_ARG, E_UNSUPPORTED = _lib.lib, -1, -3
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    ptr = C.c_void_p(base)

    def refused(rc, code, word):
        assert rc == code and word in lib.ldx_last_error().decode(), lib.ldx_last_error()

    gc = lib.ldx_geno_group_counts_dev
    for k, name in ((0, "alt"), (1, "ref"), (5, "member"), (7, "counts")):
        args = [ptr, ptr, 4, 8, None, ptr, 3, ptr, None]
        args[k] = None
        refused(gc(*args), E_ARG, name)
    refused(gc(ptr, ptr, 4, 7, None, ptr, 3, ptr, None), E_ARG, "even")
    refused(gc(ptr, ptr, 4, 0, None, ptr, 3, ptr, None), E_ARG, "non-zero")
    refused(gc(ptr, ptr, 0, 8, None, ptr, 3, ptr, None), E_ARG, "n_snps")
    refused(gc(ptr, ptr, 4, 8, None, ptr, 0, ptr, None), E_ARG, "n_groups")
    refused(gc(ptr, ptr, 4, 8, None, ptr, 33, ptr, None), E_ARG, "n_groups")
    refused(gc(ptr, ptr, 4, 8, None, ptr, 3, C.c_void_p(base + 4), None), E_ARG, "aligned")
    refused(gc(ptr, ptr, 4, _lib.MAX_HAPS + 2, None, ptr, 3, ptr, None), E_UNSUPPORTED, "LDX_MAX_HAPS")
    refused(lib.ldx_hwe_exact_dev(4, ptr, None, ptr, 0, ptr, ptr, ptr, None), E_ARG, "het")
    refused(lib.ldx_hwe_exact_dev(0, ptr, ptr, ptr, 0, ptr, ptr, ptr, None), E_ARG, "m 0")
    refused(lib.ldx_hwe_exact_dev(4, ptr, ptr, ptr, 2, ptr, ptr, ptr, None), E_ARG, "midp")
    refused(lib.ldx_fisher_exact_dev(4, ptr, ptr, ptr, None, 0, ptr, ptr, ptr, None), E_ARG, "d is")
    refused(lib.ldx_fisher_exact_dev(4, ptr, ptr, ptr, ptr, 0, ptr, ptr, None, None), E_ARG, "flags")
    refused(lib.ldx_model_tests_dev(4, ptr, ptr, ptr, ptr, ptr, ptr, 5, ptr, ptr, ptr, None, ptr, None), E_ARG, "odds")
    refused(lib.ldx_model_tests_dev(0, ptr, ptr, ptr, ptr, ptr, ptr, 5, ptr, ptr, ptr, ptr, ptr, None), E_ARG, "m 0")

    with pytest.raises(LdxError, match="het \\+ hom > n"):
        hwe_exact_host([5], [3], [3])
    with pytest.raises(LdxError, match="LDX_QC_MAX_N"):
        hwe_exact_host([70000], [3], [3])
    with pytest.raises(LdxError, match="uint32"):
        hwe_exact_host([5], [-1], [3])
    with pytest.raises(LdxError, match="length"):
        fisher_exact_host([1, 2], [1], [1], [1])
    with pytest.raises(LdxError, match="LDX_QC_MAX_N"):
        fisher_exact_host([100000], [100000], [1], [1])
    with pytest.raises(LdxError, match="cases and controls"):
        model_tests_host([5000], [1], [1], [5000], [1], [1])
    with pytest.raises(LdxError, match="het \\+ hom > n"):
        model_tests_host([5], [4], [4], [5], [1], [1])
    with pytest.raises(LdxError, match="min_cell"):
        model_tests_host([5], [1], [1], [5], [1], [1], min_cell=-1)
    codes = X.qc_codes(8, 4, seed=1)
    with pytest.raises(LdxError, match="groups"):
        geno_group_counts_host(codes, np.ones((33, 8), dtype=bool))
    with pytest.raises(LdxError, match="groups"):
        geno_group_counts_host(codes, np.full((2, 8), 2))
    with pytest.raises(LdxError, match="label vector"):
        geno_group_counts_host(codes, np.zeros(7))
    for fn, args in ((ld_hardy, (None,)), (ld_model, (None, np.zeros(8))), (ld_test_missing, (None, np.zeros(8))), (sample_qc, (None,))):
        with pytest.raises(LdxError, match="missing"):
            fn(*args, missing="pairwise")


def test_tail_rule_is_what_the_text_says():
    """P(k) / P(obs) <= 1 + 2^-30 includes a term 2^-31 above the observed one and excludes one 2^-29 above it."""
    from ld_tools_amd.ops import _tail_ints

    big = 1 << 40
    assert _tail_ints([big, big + (big >> 31), 5 * big], 0, False)[0] == pytest.approx((2 * big + (big >> 31)) / (7 * big + (big >> 31)))
    assert _tail_ints([big, big + (big >> 29), 5 * big], 0, False)[0] == pytest.approx(big / (7 * big + (big >> 29)))
    assert math.isclose(_tail_ints([big, big, 5 * big], 0, True)[0], 1.5 / 7)

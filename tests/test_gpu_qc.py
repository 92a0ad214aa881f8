"""GPU: genotype QC and table tests (include/ldx.h, "genotype QC and table tests") -- the group counts kernel against the host
mirror, the exact tests and the chi-square tests against the exact oracle (tests/ld_qc_exact.py) and the numpy mirror, the
panel-level operators against their compositions.

Shapes: 37, 64, 130 and 200 individuals are a partial 64-individual chunk, exactly one, an odd and an even number of chunks for
the kernel's two halves; 1, 130 and 300 SNPs a slab's tail and more than two slabs.  Bounds are the definition's: counts,
chisq, odds and flags exact, |ln p - exact| <= 2^-30 max(1, |ln p|)."""
import numpy as np
import pytest

import ld_qc_exact as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (n_ind, n_snps, missing rate, with a keep mask)
CASES = ((37, 300, 0.05, True), (37, 1, 0.0, False), (64, 130, 0.0, False), (64, 300, 0.05, True), (130, 130, 0.05, True),
         (130, 1, 0.05, False), (200, 300, 0.05, False), (200, 130, 0.0, True))
SETS = ("all", "cc", "g32")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


def u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


@pytest.fixture(scope="module")
def panels(gpu):
    """case -> (codes, keep, panel, {set: (groups, device counts as int64 numpy, sizes)}): made and counted once."""
    from ld_tools_amd import PackedPanel, geno_group_counts

    out = {}
    for case in CASES:
        n_ind, n_snps, miss, masked = case
        codes = X.qc_codes(n_ind, n_snps, seed=n_ind + n_snps, miss=miss)
        keep = (np.arange(n_snps) % 5 != 3) if masked else None
        panel = PackedPanel.from_codes(codes, device=gpu)
        sets = {}
        for name, groups in X.group_sets(n_ind, seed=n_snps).items():
            counts, sizes = geno_group_counts(panel, groups, keep)
            assert counts.dtype == torch.int32 and tuple(counts.shape) == (n_snps, groups.shape[0], 4)
            sets[name] = (groups, u32(counts), sizes)
        out[case] = (codes, keep, panel, sets)
    return out


@pytest.mark.parametrize("case", CASES)
def test_group_counts_equal_the_host_mirror(panels, case):
    from ld_tools_amd import geno_group_counts_host, geno_snp_counts

    codes, keep, panel, sets = panels[case]
    for name in SETS:
        groups, got, sizes = sets[name]
        want, want_sizes = geno_group_counts_host(codes, groups, keep)
        assert np.array_equal(got, want.astype(np.int64)), name
        assert np.array_equal(sizes, want_sizes)
        if keep is not None:
            assert not got[~keep].any() and got[keep].any()
    assert np.array_equal(sets["all"][1][:, 0], u32(geno_snp_counts(panel, keep)))        # one group of everybody
    assert np.array_equal(sets["cc"][1][:, 0], sets["all"][1][:, 0]) and np.array_equal(sets["g32"][1][:, 0], sets["all"][1][:, 0])
    assert not sets["g32"][1][:, 5].any()                                                   # the empty group
    assert np.array_equal(sets["g32"][1][:, 6], sets["g32"][1][:, 4])                      # the overlapping pair


def test_group_counts_equal_counts_of_selected_panels(panels):
    from ld_tools_amd import geno_snp_counts

    case = (130, 130, 0.05, True)
    _, keep, panel, sets = panels[case]
    groups, got, _ = sets["g32"]
    for g in (1, 4, 17, 31):
        rows = np.flatnonzero(groups[g])
        sub = panel.select(haplotypes=np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1))
        assert np.array_equal(got[:, g], u32(geno_snp_counts(sub, keep))), g


def test_labels_and_refusals(gpu, panels):
    from ld_tools_amd import LdxError, geno_group_counts

    _, _, panel, sets = panels[(64, 130, 0.0, False)]
    groups, got, _ = sets["cc"]
    labels = np.where(groups[1], 1.0, np.where(groups[2], 0.0, np.nan))
    by_label, sizes = geno_group_counts(panel, labels)
    assert np.array_equal(u32(by_label), got[:, [2, 1]]) and sizes.tolist() == [int(groups[2].sum()), int(groups[1].sum())]
    with pytest.raises(LdxError, match="groups"):
        geno_group_counts(panel, np.ones((33, 64), dtype=bool))


@pytest.fixture(scope="module")
def panel_tuples(panels):
    """The distinct (n, het, hom) of every panel and group set, and the distinct allelic and missingness 2 x 2 tables of the
    case/control sets."""
    hw, fi = set(), set()
    for case, (_, _, _, sets) in panels.items():
        for name in SETS:
            hw |= {tuple(r) for r in sets[name][1].reshape(-1, 4)[:, :3].tolist()}
        groups, c, sizes = sets["cc"]
        a, u = c[:, 1, 1] + 2 * c[:, 1, 2], c[:, 2, 1] + 2 * c[:, 2, 2]
        fi |= set(zip(a.tolist(), (2 * c[:, 1, 0] - a).tolist(), u.tolist(), (2 * c[:, 2, 0] - u).tolist()))
        fi |= set(zip((sizes[1] - c[:, 1, 0]).tolist(), c[:, 1, 0].tolist(), (sizes[2] - c[:, 2, 0]).tolist(), c[:, 2, 0].tolist()))
    return sorted(hw), sorted(fi)


HAND_HWE = [(5120, 2560, 1280), (5120, 2562, 1279), (2560, 2560, 0), (5120, 0, 2560), (0, 0, 0), (50, 0, 0), (50, 0, 50), (1, 1, 0),
            (100, 13, 4), (100, 5, 8), (6, 2, 1), (6, 4, 0), (4000, 100, 1900)]
HAND_FISHER = [(5120, 5120, 0, 10240), (10240, 0, 5120, 5120), (0, 0, 0, 0), (3, 0, 5, 0), (0, 0, 2, 3), (0, 4, 0, 6), (3, 1, 1, 3),
               (10, 30, 30, 10), (2000, 3000, 2500, 2740), (5120, 5120, 5120, 5120), (1, 0, 0, 1)]


def run_exact(kind, tuples, midp):
    from ld_tools_amd import ld_fisher_from_counts, ld_hwe_from_counts

    fn = ld_hwe_from_counts if kind == "hwe" else ld_fisher_from_counts
    p, nlp, flags = fn(*(np.array(c, dtype=np.int64) for c in zip(*tuples)), midp=midp)
    assert p.dtype == torch.float64 and nlp.dtype == torch.float64 and flags.dtype == torch.uint8
    return p.cpu().numpy(), nlp.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("midp", (False, True))
def test_exact_tests_on_the_panels_tuples(gpu, panel_tuples, midp):
    hw, fi = panel_tuples
    assert len(hw) > 1000 and len(fi) > 500
    worst = X.check_exact("hwe", hw, midp, *run_exact("hwe", hw, midp))
    worst = max(worst, X.check_exact("fisher", fi, midp, *run_exact("fisher", fi, midp)))
    print(f"midp={midp}: {len(hw)} HWE and {len(fi)} Fisher tuples, largest ln p error / bound = {worst:.3g}")


@pytest.mark.parametrize("midp", (False, True))
def test_exact_tests_on_hand_made_tuples(gpu, midp):
    hw = X.small_hwe_tuples(30) + HAND_HWE                     # every (n <= 30, n_A, het): all the small exact ties
    p, nlp, flags = run_exact("hwe", hw, midp)
    worst = X.check_exact("hwe", hw, midp, p, nlp, flags)
    at = len(hw) - len(HAND_HWE)
    assert p[at + 3] == 0.0 and 1541.0 < nlp[at + 3] < 1541.5                         # n = 5120, 2560 hom ALT, no het
    assert 768.0 < nlp[at + 2] < 769.5
    assert flags[at + 4] == 1 and flags[at + 5] == 2 and flags[at + 6] == 2
    fi = [(a, m - a, c, m - c) for m in range(1, 41) for a in range(m + 1) for c in range(a, m + 1)] + HAND_FISHER
    p, nlp, flags = run_exact("fisher", fi, midp)
    worst = max(worst, X.check_exact("fisher", fi, midp, p, nlp, flags))
    at = len(fi) - len(HAND_FISHER)
    assert flags[at:at + 6].tolist() == [0, 0, 1, 2, 2, 2]
    assert (p[at] == 0.0 or nlp[at] > 300.0) and np.isfinite(nlp[at])
    print(f"midp={midp}: {len(hw)} HWE and {len(fi)} Fisher tuples, largest ln p error / bound = {worst:.3g}")


def test_exact_refusals(gpu):
    from ld_tools_amd import LdxError, ld_fisher_from_counts, ld_hwe_from_counts, ld_model_from_counts

    with pytest.raises(LdxError, match="LDX_E_ARG"):
        ld_hwe_from_counts([5, 5], [1, 3], [1, 3])
    with pytest.raises(LdxError, match="LDX_E_ARG"):
        ld_fisher_from_counts([100000], [100000], [1], [1])
    with pytest.raises(LdxError, match="LDX_E_ARG"):
        ld_model_from_counts([5000], [1], [1], [5000], [1], [1])


def test_model_against_the_mirror_and_the_oracle(gpu, panels):
    from ld_tools_amd import ld_model_from_counts, model_tests_host

    tuples = X.model_tuples()
    for _, (_, _, _, sets) in panels.items():
        c = sets["cc"][1]
        tuples += [tuple(r) for r in np.concatenate([c[:, 1, :3], c[:, 2, :3]], axis=1)[::7].tolist()]
    cols = [np.array(c, dtype=np.int64) for c in zip(*tuples)]
    seen = set()
    for min_cell in (4, 5, 6):
        got = [t.cpu().numpy() for t in ld_model_from_counts(*cols, min_cell=min_cell)]
        want = model_tests_host(*cols, min_cell=min_cell)
        assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))        # chisq, bit for bit (NaN included)
        assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))        # odds
        assert np.array_equal(got[4], want[4])
        s, worst = X.check_model(tuples, min_cell, *got, rel=2.0 ** -48.9)
        seen |= s
        print(f"min_cell={min_cell}: {len(tuples)} tuples, largest tail error / bound = {worst:.3g}")
    assert seen == {0, 1, 2, 3}
    at = tuples.index((40, 20, 5, 50, 25, 5))
    flags = [int(ld_model_from_counts(*(c[at:at + 1] for c in cols), min_cell=m)[4][0, 2]) for m in (4, 5, 6)]
    assert flags == [0, 0, 3]


def same(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("case", ((200, 300, 0.05, False), (37, 300, 0.05, True)))
def test_operators_equal_their_compositions(gpu, panels, case):
    from ld_tools_amd import (geno_group_counts, ld_fisher_from_counts, ld_hardy, ld_hwe_from_counts, ld_model,
                              ld_model_from_counts, ld_test_missing)

    codes, keep, panel, sets = panels[case]
    n_ind, n_snps = case[:2]
    groups, counts, sizes = sets["cc"]
    for midp in (False, True):
        res = ld_hardy(panel, groups, midp=midp, keep=keep)
        assert np.array_equal(u32(res.counts), counts) and np.array_equal(res.sizes, sizes)
        flat = counts.reshape(-1, 4)
        p, nlp, flags = ld_hwe_from_counts(flat[:, 0], flat[:, 1], flat[:, 2], midp=midp)
        assert same(res.p.reshape(-1), p) and same(res.neglog10_p.reshape(-1), nlp) and same(res.flags.reshape(-1), flags)
        with np.errstate(all="ignore"):
            a = flat[:, 1] + 2 * flat[:, 2]
            assert np.array_equal(res.o_het.cpu().numpy().reshape(-1), flat[:, 1] / flat[:, 0], equal_nan=True)
            assert np.array_equal(res.e_het.cpu().numpy().reshape(-1), (a * (2.0 * flat[:, 0] - a)) / (2.0 * flat[:, 0] * flat[:, 0]),
                                  equal_nan=True)
    alone = ld_hardy(panel, groups[1:2], keep=keep)                    # a group's bits do not depend on the groups beside it
    beside = ld_hardy(panel, groups, keep=keep)
    assert tuple(beside.p.shape) == (n_snps, 3) and same(alone.p[:, 0], beside.p[:, 1])
    assert same(alone.neglog10_p[:, 0], beside.neglog10_p[:, 1]) and same(alone.counts[:, 0], beside.counts[:, 1])
    everybody = ld_hardy(panel, keep=keep)
    assert everybody.labels == [0] and same(everybody.p[:, 0], beside.p[:, 0])

    case_v = np.where(groups[1], 1.0, np.where(groups[2], 0.0, np.nan))
    res = ld_model(panel, case_v, midp=True, min_cell=3, keep=keep)
    cc, uc = counts[:, 1], counts[:, 2]
    assert np.array_equal(u32(res.case_counts), cc) and np.array_equal(u32(res.ctrl_counts), uc)
    assert (res.n_case, res.n_ctrl) == (int(sizes[1]), int(sizes[2]))
    outs = ld_model_from_counts(cc[:, 0], cc[:, 1], cc[:, 2], uc[:, 0], uc[:, 1], uc[:, 2], min_cell=3)
    for got, want in zip((res.chisq, res.p, res.neglog10_p, res.odds, res.flags), outs):
        assert same(got, want)
    a, u = cc[:, 1] + 2 * cc[:, 2], uc[:, 1] + 2 * uc[:, 2]
    fp = ld_fisher_from_counts(a, 2 * cc[:, 0] - a, u, 2 * uc[:, 0] - u, midp=True)
    assert same(res.fisher_p, fp[0]) and same(res.fisher_neglog10_p, fp[1]) and same(res.fisher_flags, fp[2])
    assert ld_model(panel, case_v, fisher=False).fisher_p is None

    tm = ld_test_missing(panel, case_v)
    full, _ = geno_group_counts(panel, groups)
    called = u32(full)[:, :, 0]
    fp = ld_fisher_from_counts(sizes[1] - called[:, 1], called[:, 1], sizes[2] - called[:, 2], called[:, 2])
    assert same(tm.p, fp[0]) and same(tm.flags, fp[2])
    assert np.array_equal(tm.f_miss_case.cpu().numpy(), (sizes[1] - called[:, 1]) / float(sizes[1]))
    assert np.array_equal(tm.f_miss_ctrl.cpu().numpy(), (sizes[2] - called[:, 2]) / float(sizes[2]))


def test_bits_do_not_depend_on_the_slab(gpu):
    from ld_tools_amd import PackedPanel, ld_hardy, ld_model

    codes = X.qc_codes(130, 300, seed=9, miss=0.05)
    codes[290], codes[131] = codes[2], codes[2]                  # SNP 2 again in the second and in the third slab
    case_v = X.case_vector(130, seed=2)
    panel = PackedPanel.from_codes(codes, device=gpu)
    res = ld_hardy(panel, np.stack([case_v == 1, case_v == 0]))
    for field in (res.counts, res.p, res.neglog10_p, res.flags, res.o_het, res.e_het):
        f = field.cpu().numpy()
        assert np.array_equal(f[2], f[131], equal_nan=True) and np.array_equal(f[2], f[290], equal_nan=True)
    mod = ld_model(panel, case_v)
    for field in (mod.chisq, mod.p, mod.odds, mod.fisher_p, mod.fisher_neglog10_p):
        f = field.cpu().numpy()
        assert np.array_equal(f[2], f[131], equal_nan=True) and np.array_equal(f[2], f[290], equal_nan=True)


@pytest.mark.parametrize("case", ((130, 130, 0.05, True), (64, 300, 0.05, True), (37, 1, 0.0, False)))
def test_sample_qc(gpu, panels, case):
    from ld_tools_amd import sample_qc, sample_qc_host, sample_qc_mask, snp_qc_mask

    codes, keep, panel, sets = panels[case]
    got, want = sample_qc(panel, keep), sample_qc_host(codes, keep)
    rows = codes if keep is None else codes[keep]
    h0, h1 = rows[:, 0::2], rows[:, 1::2]
    called = (h0 != 2) & (h1 != 2)
    assert np.array_equal(got.called, called.sum(axis=0)) and np.array_equal(got.het, (called & (h0 != h1)).sum(axis=0))
    assert np.array_equal(got.hom, (called & (h0 == 1) & (h1 == 1)).sum(axis=0)) and got.n_kept == rows.shape[0]
    assert np.array_equal(got.e_hom, want.e_hom) and np.array_equal(got.f, want.f, equal_nan=True)      # the host product mirror
    if case[1] > 1:
        ok = sample_qc_mask(panel, mind_max=0.06, het_sd=3.0, keep=keep)
        fin = np.isfinite(want.f)
        mean, sd = want.f[fin].mean(), want.f[fin].std(ddof=1)
        assert np.array_equal(ok, (want.f_miss <= 0.06) & fin & (np.abs(want.f - mean) <= 3.0 * sd))
        c_all = sets["all"][1] if keep is None else None
        mask = snp_qc_mask(panel, maf_min=0.2, geno_max=0.05, hwe_min=0.01, hwe_group=sets["cc"][0][2])
        assert mask.dtype == torch.uint8 and mask.device.type == "cuda"
        from ld_tools_amd import geno_group_counts_host, hwe_exact_host
        c, _ = geno_group_counts_host(codes, np.stack([np.ones(case[0], dtype=bool), sets["cc"][0][2]]))
        c = c.astype(np.int64)
        n, a = c[:, 0, 0], c[:, 0, 1] + 2 * c[:, 0, 2]
        p, _, flags = hwe_exact_host(c[:, 1, 0], c[:, 1, 1], c[:, 1, 2])
        want_mask = (n > 0) & (np.minimum(a, 2 * n - a) >= 0.2 * (2 * n)) & ((case[0] - n) <= 0.05 * case[0]) & (flags != 1)
        near = np.abs(np.nan_to_num(p, nan=1.0) - 0.01) < 1e-9          # the mirror's p is not the device's bit for bit
        got_mask = mask.cpu().numpy().astype(bool)
        assert not near.any() and np.array_equal(got_mask, want_mask & (np.nan_to_num(p, nan=0.0) >= 0.01))
        assert 0 < got_mask.sum() < got_mask.size
        assert c_all is None or np.array_equal(c_all[:, 0], c[:, 0])
        from ld_tools_amd import geno_snp_counts
        assert not u32(geno_snp_counts(panel, mask))[~got_mask].any()      # an operator takes the mask as keep= as it stands

"""GPU: the max(T) permutation test (include/ldx.h, "permutation tests"; csrc/ldx_perm.hip) -- the label plane against the numpy
mirror, the two integers of every cell against per-individual loops and against the pairwise-complete EM kernel on every path,
the epilogue alone against the mirror and the --model tests, the scan's counters and maxima against the host reduction of the
epilogue over the counts, the invariances, a planted causal SNP from the panel to the .assoc.mperm line, and the argument rules.

Shapes: 300 SNPs (three I tiles, the last one ragged) x 200 permutations (two J slabs, 128 + 72); 200 individuals of whom 187
have a phenotype, 37 of them cases -- more than one K-block of 128 individuals and no multiple of it."""
import ctypes as C

import numpy as np
import pytest

import ld_mperm_exact as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_IND, N_CASE, N_CTRL, N_SNPS, R, SEED = 200, 37, 150, 300, 200, 20261021
N = N_CASE + N_CTRL
KINDS = {"clean": (0.0, 0), "holes": (0.03, 0), "mixed": (0.03, 128)}   # miss, the first SNP with holes


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case():
    return X.case_vector(N_IND, N_CASE, N_CTRL, seed=5)


@pytest.fixture(scope="module")
def labels():
    from ld_tools_amd import perm_labels_host

    return perm_labels_host(N, N_CASE, R, SEED)


@pytest.fixture(scope="module")
def scans(gpu, case, labels):
    """Per path of the kernel: the codes, the panel, the device's counts and the loops' -- made once and left unchanged."""
    from ld_tools_amd import PackedPanel, ld_mperm_counts

    out = {}
    for kind, (miss, miss_from) in KINDS.items():
        codes = X.mperm_codes(N_SNPS, N_IND, seed=11, miss=miss, miss_from=miss_from)
        panel = PackedPanel.from_codes(codes, device=gpu)
        out[kind] = (codes, panel, ld_mperm_counts(panel, case, n_perm=R, seed=SEED), X.counts_brute(codes, case, labels))
    return out


def bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


# ---- 1. labels -------------------------------------------------------------------------------------------------------------------
def test_label_plane_is_the_mirror_bit_for_bit(gpu, labels):
    from ld_tools_amd import PermLabels, perm_labels, perm_labels_host

    dev = perm_labels(N, N_CASE, R, SEED, device=gpu)
    assert np.array_equal(dev.to_array(), labels)
    # the whole plane, pad rows and pad haplotypes included, is what the panels' own packing makes of the matrix
    assert torch.equal(dev.plane, PermLabels.from_array(labels, device=gpu).plane)
    assert np.array_equal(perm_labels(N, N_CASE, 50, SEED, first=150, device=gpu).to_array(), labels[150:])
    for n, n_case, r in ((129, 37, 3), (5120, 1000, 2), (2, 1, 130)):   # one past a K-block edge; the largest n; the smallest
        got = perm_labels(n, n_case, r, SEED + n, device=gpu)
        want = perm_labels_host(n, n_case, r, SEED + n)
        assert np.array_equal(got.to_array(), want)
        assert torch.equal(got.plane, PermLabels.from_array(want, device=gpu).plane)


# ---- 2. counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_counts_against_the_loops_and_the_em_kernel(scans, case, labels, gpu, kind):
    from ld_tools_amd import PackedPanel, ld_em_counts

    codes, panel, counts, want = scans[kind]
    got = counts.cpu().numpy()
    assert got.shape == (2, N_SNPS, R) and got.dtype == np.int32
    assert np.array_equal(got.astype(np.int64), want)
    if kind == "clean":
        assert (want[1] == N_CASE).all()
    else:
        first = KINDS[kind][1]
        assert (want[1][:first] == N_CASE).all() and (want[1][first:] < N_CASE).any()
    # an independent route through an existing kernel: against a panel whose cases are hom REF and whose controls are missing,
    # the pairwise-complete EM counts N and A are R and a
    ind = np.nonzero(~np.isnan(case))[0]
    sub = panel.select(haplotypes=np.stack([2 * ind, 2 * ind + 1], axis=1).reshape(-1))
    lab = PackedPanel.from_codes(np.repeat(np.where(labels, 0, 2).astype(np.int8), 2, axis=1), device=gpu)
    em = ld_em_counts(sub, lab, missing="pairwise").cpu().numpy()
    assert np.array_equal(em[1], got[0]) and np.array_equal(em[0], got[1])


# ---- 3. the epilogue alone -------------------------------------------------------------------------------------------------------
def test_epilogue_is_the_mirror_and_the_model_tests(scans, gpu):
    from ld_tools_amd import ld_model_from_counts, ld_mperm_from_counts, mperm_stat_host

    t = X.random_tables(np.random.default_rng(8), 2000, 2560)
    cn, ch, cm, un, uh, um = t
    tup = (cn + un, ch + uh, cm + um, cn, ch + 2 * cm)
    model = ld_model_from_counts(*t, device=gpu)
    for k, test in enumerate(("allelic", "trend")):
        chisq, flags = ld_mperm_from_counts(*tup, test=test, device=gpu)
        x, f = mperm_stat_host(*tup, test=test)
        assert np.array_equal(bits(chisq), bits(x)) and np.array_equal(flags.cpu().numpy(), f)
        assert np.array_equal(bits(chisq), bits(model[0][:, k])) and np.array_equal(flags.cpu().numpy(), model[4][:, k].cpu().numpy())
        assert (f == 0).sum() > 1200 and (f == 1).any() and (f == 2).any()   # (the tables' own mix: most are usable)


def cells_of(codes, case, counts, test):
    """The epilogue entry over the device's counts: chisq float64 [n_snps, R] (NaN: invalid)."""
    from ld_tools_amd import ld_mperm_from_counts

    Nn, n1, n2, _, _ = X.snp_margins(codes, case)
    c = counts.cpu().numpy().astype(np.int64)
    rep = lambda v: np.repeat(v, c.shape[2])  # noqa: E731
    chisq, _ = ld_mperm_from_counts(rep(Nn), rep(n1), rep(n2), c[1].reshape(-1), c[0].reshape(-1), test=test, device=counts.device)
    return chisq.cpu().numpy().reshape(c.shape[1:])


# ---- 4. the scan -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("test", ["allelic", "trend"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_scan_against_the_host_reduction_and_the_mirror(scans, case, kind, test):
    from ld_tools_amd import ld_mperm, ld_mperm_host

    codes, panel, counts, _ = scans[kind]
    res = ld_mperm(panel, case, test=test, n_perm=R, seed=SEED)
    assert (res.n_perm, res.n_perm_total, res.n_case, res.n_ctrl) == (R, R, N_CASE, N_CTRL)
    stat, flags = res.stat.cpu().numpy(), res.flags.cpu().numpy()
    x = cells_of(codes, case, counts, test)
    valid = ~np.isnan(x) & (flags == 0)[:, None]
    n_ge = (valid & (x >= np.where(flags == 0, stat, np.inf)[:, None])).sum(axis=1)
    maxima = np.where(valid, x, 0.0).max(axis=0)
    assert np.array_equal(res.n_ge.cpu().numpy(), n_ge)
    assert np.array_equal(bits(res.maxima), bits(maxima))
    # the conditions under which this says something
    assert (flags == 0).mean() >= 0.9
    assert 0 < n_ge.max() and n_ge.min() < R and len(set(n_ge.tolist())) > 20
    assert (valid & (x == stat[:, None])).any()                      # an exact tie, counted by >=
    host = ld_mperm_host(codes, case, test=test, n_perm=R, seed=SEED)
    for name in ("stat", "flags", "n_ge", "maxima", "emp1", "emp2"):
        assert np.array_equal(bits(getattr(res, name)), bits(getattr(host, name))), name


def test_flags_and_keep(gpu, case):
    from ld_tools_amd import PackedPanel, ld_mperm, ld_mperm_host

    codes = X.mperm_codes(140, N_IND, seed=21, miss=0.02)
    cases = np.nonzero(case == 1.0)[0]
    codes[3], codes[5] = 0, 2                                         # monomorphic: flag 2; nobody called: flag 1
    codes[130] = 1
    codes[130, np.concatenate([2 * cases, 2 * cases + 1])] = 2        # no called case: flag 1
    keep = np.ones(140, dtype=bool)
    keep[[7, 129]] = False
    panel = PackedPanel.from_codes(codes, device=gpu)
    res = ld_mperm(panel, case, n_perm=R, seed=SEED, keep=keep)
    flags = res.flags.cpu().numpy()
    bad = [3, 5, 7, 129, 130]
    assert flags[bad].tolist() == [2, 1, 3, 3, 1] and (np.delete(flags, bad) == 0).all()
    assert np.isnan(res.stat.cpu().numpy()[bad]).all() and (res.n_ge.cpu().numpy()[bad] == 0).all()
    assert np.isnan(res.emp1.cpu().numpy()[bad]).all() and np.isnan(res.emp2.cpu().numpy()[bad]).all()
    host = ld_mperm_host(codes, case, n_perm=R, seed=SEED, keep=keep)
    for name in ("stat", "flags", "n_ge", "maxima", "emp1", "emp2"):
        assert np.array_equal(bits(getattr(res, name)), bits(getattr(host, name))), name
    # keep equals the sub-panel
    sub = ld_mperm(panel.select(snps=keep), case, n_perm=R, seed=SEED)
    assert np.array_equal(bits(sub.maxima), bits(res.maxima))
    assert np.array_equal(bits(sub.stat), bits(res.stat)[keep]) and np.array_equal(bits(sub.n_ge), bits(res.n_ge)[keep])
    assert np.array_equal(sub.flags.cpu().numpy(), flags[keep])


# ---- 5. invariances --------------------------------------------------------------------------------------------------------------
def same(a, b):
    return all(np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in ("stat", "flags", "n_ge", "maxima"))


@pytest.mark.parametrize("test", ["allelic", "trend"])
def test_invariances(scans, case, labels, gpu, test):
    from ld_tools_amd import PackedPanel, PermLabels, ld_mperm

    codes, panel, _, _ = scans["mixed"]
    ref = ld_mperm(panel, case, test=test, n_perm=R, seed=SEED)
    assert same(ref, ld_mperm(panel, case, test=test, labels=PermLabels.from_array(labels, device=gpu)))
    rng = np.random.default_rng(77)
    # the individuals in another order, the labels with them
    perm = rng.permutation(N_IND)
    rank = np.cumsum(~np.isnan(case)) - 1                            # an individual's place among those with a phenotype
    case2 = case[perm]
    labels2 = labels[:, rank[perm[~np.isnan(case2)]]]
    codes2 = codes.reshape(N_SNPS, N_IND, 2)[:, perm].reshape(N_SNPS, -1)
    assert same(ref, ld_mperm(PackedPanel.from_codes(codes2, device=gpu), case2, test=test, labels=labels2))
    # another phase
    flip = rng.random((N_SNPS, N_IND)) < 0.5
    c3 = codes.reshape(N_SNPS, N_IND, 2)
    codes3 = np.where(flip[:, :, None], c3[:, :, ::-1], c3).reshape(N_SNPS, -1)
    assert same(ref, ld_mperm(PackedPanel.from_codes(codes3, device=gpu), case, test=test, n_perm=R, seed=SEED))
    # 128 + 72 permutations on a shared n_ge
    one = ld_mperm(panel, case, test=test, n_perm=128, seed=SEED)
    two = ld_mperm(panel, case, test=test, n_perm=72, seed=SEED, first=128, n_ge=one.n_ge, n_perm_before=128)
    assert two.n_ge is one.n_ge and two.n_perm_total == R
    assert np.array_equal(bits(two.n_ge), bits(ref.n_ge)) and np.array_equal(bits(two.emp1), bits(ref.emp1))
    assert np.array_equal(bits(torch.cat([one.maxima, two.maxima])), bits(ref.maxima))
    # two SNP halves on a shared maxima
    lo = ld_mperm(panel.select(snps=np.arange(150)), case, test=test, n_perm=R, seed=SEED)
    assert not np.array_equal(bits(lo.maxima), bits(ref.maxima))
    hi = ld_mperm(panel.select(snps=np.arange(150, N_SNPS)), case, test=test, n_perm=R, seed=SEED, maxima=lo.maxima)
    assert hi.maxima is lo.maxima and np.array_equal(bits(hi.maxima), bits(ref.maxima))
    assert np.array_equal(bits(torch.cat([lo.n_ge, hi.n_ge])), bits(ref.n_ge))
    assert np.array_equal(bits(hi.emp2), bits(ref.emp2)[150:])


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def test_planted_snp_null_panel_and_the_driver(gpu, tmp_path):
    from ld_tools_amd import PackedPanel, ld_mperm
    from ld_tools_amd.drivers import plink as shell
    from ld_tools_amd.drivers.mperm import mperm_table, write_assoc_mperm

    n, n_ind, at, P = 150, 300, 41, 999
    rng = np.random.default_rng(41)
    codes = X.mperm_codes(n, n_ind, seed=40)
    case = (rng.random(n_ind) < 0.4).astype(np.float64)
    null = ld_mperm(PackedPanel.from_codes(codes, device=gpu), case, n_perm=P, seed=3)
    e1 = null.emp1.cpu().numpy()
    assert e1.min() < 0.1 and e1.max() > 0.9 and 0.3 < np.median(e1) < 0.7            # not degenerate
    assert null.emp2.cpu().numpy().min() > 0.01                                        # and nothing study-wide
    codes[at] = rng.random(2 * n_ind) < np.repeat(np.where(case == 1.0, 0.6, 0.25), 2)   # the cases enriched for ALT
    gone = np.repeat(rng.random((n, n_ind)) < 0.01, 2, axis=1)                         # whole genotypes missing, as a .bed holds them
    codes[gone] = 2
    panel = PackedPanel.from_codes(codes, device=gpu)
    for test in ("allelic", "trend"):
        res = ld_mperm(panel, case, test=test, n_perm=P, seed=3)
        e2 = res.emp2.cpu().numpy()
        assert int(np.argmin(e2)) == at and e2[at] == 1.0 / (P + 1) and np.delete(e2, at).min() > 5.0 / (P + 1)
        assert res.emp1.cpu().numpy()[at] == 1.0 / (P + 1)

    ids = [f"rs{1000 + k}" for k in range(n)]
    chrom = ["3" if k < 100 else "9" for k in range(n)]
    direct = tmp_path / "direct.assoc.mperm"
    write_assoc_mperm(str(direct), mperm_table(panel, case, chrom, ids, n_perm=P, seed=3))
    prefix = str(tmp_path / "study")
    bim = {"chrom": chrom, "ids": ids, "pos": [500 + 11 * k for k in range(n)], "a1": ["T"] * n, "a2": ["C"] * n}
    fam = {"fid": [f"F{k}" for k in range(n_ind)], "iid": [f"I{k}" for k in range(n_ind)]}
    shell.make_bed(prefix, panel, bim=bim, fam=fam)
    pheno = tmp_path / "study.pheno"
    pheno.write_text("#FID IID CC QT\n" + "".join(f"F{k} I{k} {int(c) + 1} {0.5 * k}\n" for k, c in enumerate(case)))
    out = str(tmp_path / "o")
    assert shell.main(["mperm", "--bfile", prefix, "--out", out, "--pheno", str(pheno), "--mperm", str(P), "--seed", "3"]) == 0
    lines = open(out + ".assoc.mperm").read().splitlines()
    assert lines[0].split("\t") == ["CHR", "SNP", "EMP1", "EMP2", "CHISQ"] and len(lines) == n + 1
    hit = lines[1 + at].split("\t")
    assert hit[:4] == ["3", ids[at], repr(1.0 / (P + 1)), repr(1.0 / (P + 1))] and float(hit[4]) > 30.0
    assert "\n".join(lines) + "\n" == direct.read_text()
    with pytest.raises(shell.LdxError):
        shell.bfile_mperm(prefix, str(pheno), pheno_name="QT", n_perm=4)               # a quantitative trait
    table = shell.bfile_mperm(prefix, str(pheno), test="trend", n_perm=64, seed=3, out=out)   # 0 / 1 and 1 / 2 both read
    assert len(open(out + ".model.trend.mperm").read().splitlines()) == n + 1 and table.result.n_perm == 64


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_operator_refusals(gpu, case, labels):
    from ld_tools_amd import (LdxError, PackedPanel, PermLabels, ld_mperm, ld_mperm_counts, ld_mperm_from_counts, perm_labels,
                              perm_labels_host)

    panel = PackedPanel.from_codes(X.mperm_codes(4, N_IND, seed=1), device=gpu)
    with pytest.raises(LdxError, match="missing must be None"):
        ld_mperm(panel, case, n_perm=4, missing="pairwise")
    with pytest.raises(LdxError, match="both groups must hold an individual"):
        ld_mperm(panel, np.where(case == 1.0, np.nan, case), n_perm=4)
    with pytest.raises(LdxError, match="case must be a vector"):
        ld_mperm_counts(panel, case[:-1], n_perm=4)
    with pytest.raises(LdxError, match="test must be one of"):
        ld_mperm(panel, case, test="genotypic", n_perm=4)
    with pytest.raises(LdxError, match="give n_perm"):
        ld_mperm(panel, case)
    with pytest.raises(LdxError, match="labels of"):
        ld_mperm(panel, case, labels=perm_labels_host(N - 1, N_CASE, 4, 1))
    with pytest.raises(LdxError, match="labels of"):
        ld_mperm(panel, case, labels=perm_labels(N, N_CASE + 1, 4, 1, device=gpu))
    with pytest.raises(LdxError, match="same number of cases"):
        PermLabels.from_array(np.eye(5, dtype=bool) | np.eye(5, k=1, dtype=bool), device=gpu)
    with pytest.raises(LdxError, match="maxima must be"):
        ld_mperm(panel, case, n_perm=4, maxima=torch.zeros(5, dtype=torch.float64, device=gpu))
    with pytest.raises(LdxError, match="n_ge must be"):
        ld_mperm(panel, case, n_perm=4, n_ge=torch.zeros(4, dtype=torch.int64, device=gpu))
    with pytest.raises(LdxError, match="LDX_E_ARG"):
        ld_mperm_from_counts([100], [40], [10], [30], [61], device=gpu)
    with pytest.raises(LdxError, match="n_hap must be even"):
        ld_mperm(PackedPanel.from_codes(X.mperm_codes(4, N_IND, seed=1)[:, :-1], device=gpu), case, n_perm=4)


def test_argument_rules():
    """Each returns its code before any HIP call: the pointers are host memory that a launch would fault on."""
    from ld_tools_amd import _lib

    lib, E_ARG, E_UNSUPPORTED = _lib.lib, -1, -3
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    ptr = C.c_void_p(base)

    def refused(rc, code, word):
        assert rc == code and word in lib.ldx_last_error().decode(), lib.ldx_last_error()

    lab = lib.ldx_perm_labels_dev
    refused(lab(1, 0, 4, 20, 3, None, None), E_ARG, "labels is a null pointer")
    refused(lab(1, 0, 0, 20, 3, ptr, None), E_ARG, "n_perm is 0")
    refused(lab(1, 0, 4, 21, 3, ptr, None), E_ARG, "must be even")
    refused(lab(1, 0, 4, 0, 3, ptr, None), E_ARG, "must be even")
    refused(lab(1, 0, 4, 20, 0, ptr, None), E_ARG, "n_case 0 outside")
    refused(lab(1, 0, 4, 20, 10, ptr, None), E_ARG, "n_case 10 outside")
    refused(lab(1, 0, 4, 10242, 3, ptr, None), E_UNSUPPORTED, "LDX_MAX_HAPS")
    refused(lab(1, 0, 1 << 22, 10240, 3, ptr, None), E_UNSUPPORTED, "4 GiB")

    def scan(alt=ptr, ref=ptr, cnt=ptr, n_snps=4, n_hap=20, labels=ptr, n_perm=4, n_case=3, test=0, stat=ptr, n_ge=ptr, mx=ptr):
        return lib.ldx_perm_scan_dev(alt, ref, cnt, n_snps, n_hap, labels, n_perm, n_case, test, stat, n_ge, mx, None)

    for name in ("alt", "ref", "cnt", "labels", "stat", "n_ge"):
        refused(scan(**{name: None}), E_ARG, f"{name} is a null pointer")
    refused(scan(mx=None), E_ARG, "max is a null pointer")
    refused(scan(cnt=C.c_void_p(base + 4)), E_ARG, "16-byte aligned")
    refused(scan(test=2), E_ARG, "test 2")
    refused(scan(n_snps=0), E_ARG, "n_snps is 0")
    refused(scan(n_perm=0), E_ARG, "n_perm is 0")
    refused(scan(n_hap=19), E_ARG, "must be even")
    refused(scan(n_case=0), E_ARG, "outside 1 .. n - 1")
    refused(scan(n_case=10), E_ARG, "outside 1 .. n - 1")
    refused(scan(n_hap=10242), E_UNSUPPORTED, "LDX_MAX_HAPS")
    refused(scan(n_hap=10240, n_perm=1 << 22), E_UNSUPPORTED, "labels is a bit plane of 4 GiB")
    refused(scan(n_hap=10240, n_snps=1 << 22), E_UNSUPPORTED, "alt is a bit plane of 4 GiB")

    cnts = lambda **o: lib.ldx_perm_counts_dev(*[o.get(k, v) for k, v in (  # noqa: E731
        ("alt", ptr), ("ref", ptr), ("cnt", ptr), ("n_snps", 4), ("n_hap", 20), ("labels", ptr), ("n_perm", 4), ("n_case", 3),
        ("counts", ptr), ("ld", 4))], None)
    refused(cnts(counts=None), E_ARG, "counts is a null pointer")
    refused(cnts(ld=3), E_ARG, "ld 3 < n_perm 4")
    refused(cnts(n_hap=19), E_ARG, "must be even")
    refused(cnts(n_hap=10242), E_UNSUPPORTED, "LDX_MAX_HAPS")

    fc = lib.ldx_perm_from_counts_dev
    refused(fc(0, 0, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None), E_ARG, "m 0")
    refused(fc(4, 2, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None), E_ARG, "test 2")
    refused(fc(4, 0, ptr, ptr, None, ptr, ptr, ptr, ptr, None), E_ARG, "hom is a null pointer")
    refused(fc(4, 0, ptr, ptr, ptr, ptr, ptr, None, ptr, None), E_ARG, "chisq is a null pointer")

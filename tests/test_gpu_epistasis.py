"""GPU: the epistasis scan (include/ldx.h, "epistasis scan"; csrc/ldx_epi.hip) -- the 18 integers of every pair against a
per-individual loop on every path of the kernel, the dense cells against the epilogue alone, the epilogue against the numpy
mirror (mu and cycles bit for bit) and the exact oracle (chisq within the header's bound), the invariances, the self scan with
its hit list and per-SNP summary, a planted XOR pair from the panel to the .epi.cc line, and the argument rules.

Shapes: 130 x 200 SNPs, so both tile edges are ragged and the rectangle has 2 x 2 tiles; 37 cases and 150 controls of 200
individuals.  A K-block of the loops is 256 haplotypes = 128 individuals: the controls are more than one block and no multiple of
it, the cases less than one.  The self scan has 300 SNPs: three tile rows, six tiles, three of them on the diagonal."""
import ctypes as C

import numpy as np
import pytest

import ld_epistasis_exact as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_IND, N_CASE, N_CTRL, N_I, N_J = 200, 37, 150, 130, 200
TR = [(k // 9) * 9 + (k % 3) * 3 + (k % 9) // 3 for k in range(18)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case():
    return X.case_vector(N_IND, N_CASE, N_CTRL, seed=5)


def codes_of(kind, case):
    """The two code matrices of one path of the kernel: no holes (the shortcut in both groups), 3 % holes (the nine-set loop
    in both) or holes among the controls only (the paths mix per group)."""
    miss, who = {"clean": (0.0, None), "holes": (0.03, None), "ctrl_holes": (0.03, case == 0.0)}[kind]
    return X.epi_codes(N_I, N_IND, seed=11, miss=miss, miss_ind=who), X.epi_codes(N_J, N_IND, seed=12, miss=miss, miss_ind=who)


@pytest.fixture(scope="module")
def rect(gpu, case):
    """Per path: the codes, the two panels and the device's counts, made once and left unchanged."""
    from ld_tools_amd import PackedPanel, ld_epistasis_counts

    out = {}
    for kind in ("clean", "holes", "ctrl_holes"):
        ci, cj = codes_of(kind, case)
        pi, pj = PackedPanel.from_codes(ci, device=gpu), PackedPanel.from_codes(cj, device=gpu)
        out[kind] = (ci, cj, pi, pj, ld_epistasis_counts(pi, case, pj))
    return out


def bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


@pytest.mark.parametrize("kind", ["clean", "holes", "ctrl_holes"])
def test_counts_against_brute_force(rect, case, kind):
    ci, cj, _, _, counts = rect[kind]
    got = counts.cpu().numpy()
    assert got.shape == (18, N_I, N_J) and got.dtype == np.int32
    want = X.tables_brute(ci, cj, case)
    assert np.array_equal(got.astype(np.int64), want)
    called = want[:9].sum(axis=0), want[9:].sum(axis=0)
    if kind == "clean":
        assert (called[0] == N_CASE).all() and (called[1] == N_CTRL).all()
    elif kind == "holes":
        assert (called[0] < N_CASE).any() and (called[1] < N_CTRL).any()
    else:
        assert (called[0] == N_CASE).all() and (called[1] < N_CTRL).any()


@pytest.mark.parametrize("test", ["allelic", "boost"])
def test_dense_equals_the_epilogue_on_the_counts(rect, case, test):
    from ld_tools_amd import ld_epistasis, ld_epistasis_from_counts

    for kind in ("clean", "holes", "ctrl_holes"):
        _, _, pi, pj, counts = rect[kind]
        res = ld_epistasis(pi, case, pj, test=test)
        cells = ld_epistasis_from_counts(counts, test=test)
        assert res.chisq.shape == (N_I, N_J) and res.n_case == N_CASE and res.n_ctrl == N_CTRL
        assert np.array_equal(bits(res.chisq), bits(cells.chisq32))
        assert np.array_equal(bits(res.dir), bits(cells.dir.to(torch.float32)))
        assert np.array_equal(bits(res.flags), bits(cells.flags))
        x = res.chisq.cpu().numpy()
        assert np.isfinite(x).mean() > 0.9 and (x[np.isfinite(x)] >= 0.0).all()
        ln_p = res.ln_p.cpu().numpy()
        fin = np.isfinite(x)
        assert np.allclose(ln_p[fin], cells.ln_p.cpu().numpy()[fin], rtol=1e-6, atol=1e-6)   # float32 cell against the fp64 statistic
        assert np.allclose(res.neglog10_p.cpu().numpy()[fin], -ln_p[fin] / np.log(10.0))


def test_epilogue_against_mirror_and_oracle(rect, gpu):
    """mu and the cycle count are numpy's bit for bit, on the oracle's tuples and on the tables of a rectangle with holes; chisq
    is within the header's bound of the exact value wherever a fit came to rest."""
    from ld_tools_amd import _lib, epi_allelic_host, epi_boost_host, ld_epistasis_from_counts

    t = X.tuples().T
    both = np.concatenate([t, rect["holes"][4].cpu().numpy().reshape(18, -1).astype(np.int64)], axis=1)
    dev_b = ld_epistasis_from_counts(both, test="boost", device=gpu)
    mu, cycles, g2, flags = epi_boost_host(both)
    assert np.array_equal(bits(dev_b.mu), bits(mu))
    assert np.array_equal(dev_b.cycles.cpu().numpy(), cycles)
    assert np.array_equal(dev_b.flags.cpu().numpy(), flags)
    dev_a = ld_epistasis_from_counts(both, test="allelic", device=gpu)
    x2, d, fa = epi_allelic_host(both)
    assert np.array_equal(dev_a.flags.cpu().numpy(), fa) and np.isnan(dev_a.mu.cpu().numpy()).all()
    assert np.array_equal(np.isnan(dev_a.chisq.cpu().numpy()), np.isnan(x2))
    assert np.array_equal(bits(dev_a.dir), bits(dev_b.dir))
    xa, xb = dev_a.chisq.cpu().numpy(), dev_b.chisq.cpu().numpy()
    assert np.array_equal(bits(dev_a.chisq32), bits(xa.astype(np.float32))) and np.array_equal(bits(dev_b.chisq32), bits(xb.astype(np.float32)))
    worst = {"allelic": 0.0, "boost": 0.0}
    for k, ((ac, _, _), (bg, _, _)) in enumerate(X.oracle()):
        if ac is not None:
            worst["allelic"] = max(worst["allelic"], X.rel_error(xa[k], ac))
        if not flags[k] & (1 | 4):
            worst["boost"] = max(worst["boost"], X.rel_error(xb[k], bg))
    print("worst relative error of the device:", worst, "bounds:", _lib.EPI_REL_BOUND)
    assert worst["allelic"] <= _lib.EPI_REL_BOUND["allelic"] and worst["boost"] <= _lib.EPI_REL_BOUND["boost"]
    # the tails, from chisq alone
    from ld_tools_amd import epi_tail_host
    for dev, test in ((dev_a, "allelic"), (dev_b, "boost")):
        x = dev.chisq.cpu().numpy()
        fin = np.isfinite(x)
        want = epi_tail_host(x, test)[0]
        got = dev.ln_p.cpu().numpy()
        assert np.array_equal(np.isnan(got), ~fin)
        assert (np.abs(got[fin] - want[fin]) <= 2.0 ** -30 * np.maximum(1.0, np.abs(want[fin]))).all()


@pytest.mark.parametrize("test", ["allelic", "boost"])
def test_invariances(rect, case, gpu, test):
    """The transpose under swapped sides, permuted individuals and rephasing give identical bits."""
    from ld_tools_amd import PackedPanel, ld_epistasis

    ci, cj, pi, pj, _ = rect["holes"]
    ref = ld_epistasis(pi, case, pj, test=test)
    want = [bits(ref.chisq), bits(ref.dir), bits(ref.flags)]
    swapped = ld_epistasis(pj, case, pi, test=test)
    for w, g in zip(want, (swapped.chisq, swapped.dir, swapped.flags)):
        assert np.array_equal(w.T, bits(g))
    rng = np.random.default_rng(9)
    perm = rng.permutation(N_IND)
    hap = np.stack([2 * perm, 2 * perm + 1], axis=1)
    flip = rng.random(N_IND) < 0.5          # rephase: the two haplotypes of an individual change places
    hap[flip] = hap[flip][:, ::-1]
    hap = hap.reshape(-1)
    moved = ld_epistasis(PackedPanel.from_codes(ci[:, hap], device=gpu), case[perm], PackedPanel.from_codes(cj[:, hap], device=gpu),
                         test=test)
    for w, g in zip(want, (moved.chisq, moved.dir, moved.flags)):
        assert np.array_equal(w, bits(g))


@pytest.fixture(scope="module")
def self_scan(gpu):
    """300 SNPs with 2 % holes; SNP 7 interacts with SNP 150 (XOR penetrance) and SNP 231 is a copy of SNP 150, so SNP 7 has two
    equal best partners."""
    from ld_tools_amd import PackedPanel

    n, n_ind = 300, 240
    codes = X.epi_codes(n, n_ind, seed=21, miss=0.02)
    g = X.genotypes(codes)
    rng = np.random.default_rng(22)
    xor = (g[7] == 1) != (g[150] == 1)
    case = np.where(rng.random(n_ind) < np.where(xor, 0.85, 0.15), 1.0, 0.0)
    case[rng.random(n_ind) < 0.05] = np.nan
    codes[231] = codes[150]
    return codes, case, PackedPanel.from_codes(codes, device=gpu)


@pytest.mark.parametrize("test", ["allelic", "boost"])
def test_self_scan_hits_and_summary(self_scan, test):
    from ld_tools_amd import epi_chisq_bound, ld_epistasis, ld_epistasis_hits

    codes, case, panel = self_scan
    n = panel.n_snps
    dense = ld_epistasis(panel, case, test=test)
    x, d = dense.chisq.cpu().numpy(), dense.dir.cpu().numpy()
    assert np.array_equal(bits(dense.chisq), bits(dense.chisq).T)
    lower = np.tril(np.ones((n, n), dtype=bool), -1)
    res = ld_epistasis_hits(panel, case, test=test, p=0.05, p_sig=0.2)
    assert res.self_scan and res.bound == epi_chisq_bound(0.05, test) and res.summary.bound_sig == epi_chisq_bound(0.2, test)
    with np.errstate(invalid="ignore"):
        keep = lower & (x >= res.bound)          # the same float32 compare; a NaN is never a hit
    wi, wj = np.nonzero(keep)
    assert 200 < wi.size < lower.sum() // 2
    i, j, hx, hd = res.pairs()
    assert np.array_equal(i, wi) and np.array_equal(j, wj)
    assert np.array_equal(bits(hx), bits(x[wi, wj])) and np.array_equal(bits(hd), bits(d[wi, wj]))
    off = res.offsets.cpu().numpy()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(keep.sum(axis=1))]))
    # the summary: every SNP against all others, from the dense matrix
    valid = ~np.isnan(x) & ~np.eye(n, dtype=bool)
    s = res.summary
    assert np.array_equal(s.n_tot.cpu().numpy(), valid.sum(axis=1))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(s.n_sig.cpu().numpy(), (valid & (x >= s.bound_sig)).sum(axis=1))
    masked = np.where(valid, x, -1.0)
    partner = masked.argmax(axis=1)              # the first maximum: the smallest partner index on ties
    assert (valid.sum(axis=1) > 0).all()
    assert np.array_equal(s.best_partner.cpu().numpy(), partner)
    assert np.array_equal(bits(s.best_chisq), bits(masked.max(axis=1).astype(np.float32)))
    assert bits(dense.chisq)[7, 150] == bits(dense.chisq)[7, 231] and partner[7] == 150   # the planted tie
    # overflow and retry: a buffer of one batch; the result and the summary do not depend on it
    small = ld_epistasis_hits(panel, case, test=test, p=0.05, p_sig=0.2, hit_capacity=256)
    assert np.array_equal(small.hits.cpu().numpy(), res.hits.cpu().numpy()) and np.array_equal(small.offsets.cpu().numpy(), off)
    for a, b in ((small.summary.n_tot, s.n_tot), (small.summary.n_sig, s.n_sig), (small.summary.best_partner, s.best_partner)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_rect_hits_and_summary(rect, case):
    """The set-by-set form: the summary is over the rows of I, the partner a row of J."""
    from ld_tools_amd import ld_epistasis, ld_epistasis_hits

    _, _, pi, pj, _ = rect["ctrl_holes"]
    x = ld_epistasis(pi, case, pj, test="boost").chisq.cpu().numpy()
    res = ld_epistasis_hits(pi, case, pj, test="boost", chisq=9.0, p_sig=0.3)
    assert not res.self_scan and res.bound == np.float32(9.0)
    wi, wj = np.nonzero(x >= np.float32(9.0))
    i, j, hx, _ = res.pairs()
    assert wi.size > 50 and np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(bits(hx), bits(x[wi, wj]))
    assert np.array_equal(res.summary.n_tot.cpu().numpy(), (~np.isnan(x)).sum(axis=1))
    assert np.array_equal(res.summary.best_partner.cpu().numpy(), np.where(np.isnan(x), -1.0, x).argmax(axis=1))


def test_planted_pair_end_to_end(gpu, tmp_path):
    """An XOR-penetrance pair without marginal effect in 300 SNPs: the numpy mirror says it is the strongest pair of the panel
    for this seed; the scan must name each of the two as the other's best partner, and the subcommand must write the same line
    from the fileset."""
    from ld_tools_amd import PackedPanel, epi_boost_host, epi_counts_host, ld_epistasis_hits
    from ld_tools_amd.drivers import plink as shell
    from ld_tools_amd.drivers.epistasis import epistasis_table, write_epi_cc

    n, n_ind, a, b = 300, 400, 41, 222
    codes = X.epi_codes(n, n_ind, seed=31)
    rng = np.random.default_rng(32)
    gone = np.repeat(rng.random((n, n_ind)) < 0.01, 2, axis=1)   # whole genotypes missing, as a .bed holds them
    for k in (a, b):                                             # ALT frequency 1/2: half of the genotypes are heterozygous,
        codes[k] = rng.random(2 * n_ind) < 0.5                   # so neither SNP has an effect of its own
    codes[gone] = 2
    g = X.genotypes(codes)
    xor = (g[a] == 1) != (g[b] == 1)
    case = (rng.random(n_ind) < np.where(xor, 0.9, 0.1)).astype(np.float64)
    # first, on the CPU: the planted pair's chi-square exceeds every other pair's
    chisq = epi_boost_host(epi_counts_host(codes, codes, case))[2]
    chisq[np.triu_indices(n)] = -1.0
    assert np.unravel_index(np.nanargmax(chisq), chisq.shape) == (b, a)
    others = chisq.copy()
    others[b, a] = -1.0
    assert chisq[b, a] > 1.5 * np.nanmax(others)

    panel = PackedPanel.from_codes(codes, device=gpu)
    res = ld_epistasis_hits(panel, case, test="boost", p=1e-6)
    partner = res.summary.best_partner.cpu().numpy()
    assert partner[a] == b and partner[b] == a
    i, j, x, _ = res.pairs()
    at = np.nonzero((i == b) & (j == a))[0]
    assert at.size == 1 and x[at[0]] == res.summary.best_chisq.cpu().numpy()[a] == res.summary.best_chisq.cpu().numpy()[b]
    assert x[at[0]] == pytest.approx(chisq[b, a], rel=1e-6)

    ids = [f"rs{1000 + k}" for k in range(n)]
    chrom = ["3" if k < 150 else "9" for k in range(n)]
    write_epi_cc(str(tmp_path / "direct.epi.cc"), epistasis_table(panel, case, chrom, ids, p=1e-6))
    prefix = str(tmp_path / "study")
    bim = {"chrom": chrom, "ids": ids, "pos": [500 + 11 * k for k in range(n)], "a1": ["T"] * n, "a2": ["C"] * n}
    fam = {"fid": [f"F{k}" for k in range(n_ind)], "iid": [f"I{k}" for k in range(n_ind)]}
    shell.make_bed(prefix, panel, bim=bim, fam=fam)
    pheno = tmp_path / "study.pheno"
    pheno.write_text("#FID IID CC\n" + "".join(f"F{k} I{k} {int(c) + 1}\n" for k, c in enumerate(case)))
    out = str(tmp_path / "o")
    assert shell.main(["epistasis", "--bfile", prefix, "--out", out, "--pheno", str(pheno), "--epi1", "1e-6"]) == 0
    want = [ln for ln in (tmp_path / "direct.epi.cc").read_text().splitlines() if ln.split("\t")[1:4:2] == [ids[b], ids[a]]]
    got = [ln for ln in open(out + ".epi.cc").read().splitlines() if ln.split("\t")[1:4:2] == [ids[b], ids[a]]]
    assert len(want) == 1 and got == want and want[0].split("\t")[:4] == ["9", ids[b], "3", ids[a]]
    assert open(out + ".epi.cc").read() == (tmp_path / "direct.epi.cc").read_text()
    summary = [ln.split("\t") for ln in open(out + ".epi.cc.summary").read().splitlines()]
    assert len(summary) == n + 1 and summary[1 + a][6:] == ["9", ids[b]] and summary[1 + b][6:] == ["3", ids[a]]
    # a set-by-set scan through the same door
    table = shell.bfile_epistasis(prefix, str(pheno), p=1e-6, set_i=[ids[a], ids[5]], set_j=[ids[b], ids[6], ids[7]])
    i, j, x2, _ = table.result.pairs()
    assert (i[0], j[0]) == (0, 0) and x2[0] == x[at[0]] and table.ids_i == [ids[a], ids[5]]


def test_operator_refusals(gpu, case):
    from ld_tools_amd import LdxError, PackedPanel, ld_epistasis, ld_epistasis_counts

    panel = PackedPanel.from_codes(X.epi_codes(4, N_IND, seed=1), device=gpu)
    with pytest.raises(LdxError, match="both groups must hold an individual"):
        ld_epistasis(panel, np.where(case == 1.0, np.nan, case))
    with pytest.raises(LdxError, match="case must be a vector"):
        ld_epistasis_counts(panel, case[:-1])
    with pytest.raises(LdxError, match="haplotype count"):
        ld_epistasis(panel, case, PackedPanel.from_codes(X.epi_codes(4, N_IND - 1, seed=1), device=gpu))
    assert ld_epistasis(panel, case, missing="pairwise").chisq.shape == (4, 4)


def test_argument_rules():
    """Each returns its code before any HIP call: the pointers are host memory that a launch would fault on."""
    from ld_tools_amd import _lib

    lib, E_ARG, E_UNSUPPORTED = _lib.lib, -1, -3
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    ptr = C.c_void_p(base)

    def side(n=4, **over):
        f = dict(alt_case=base, ref_case=base, cnt_case=base, alt_ctrl=base, ref_ctrl=base, cnt_ctrl=base, n_snps=n)
        f.update(over)
        return C.byref(_lib.EpiSide(**f))

    def refused(rc, code, word):
        assert rc == code and word in lib.ldx_last_error().decode(), lib.ldx_last_error()

    s = side()
    rect = lambda *a: lib.ldx_epi_rect_dev(*a)  # noqa: E731
    refused(rect(None, s, 8, 8, 1, ptr, None, None, 4, None), E_ARG, "side_i")
    refused(rect(s, None, 8, 8, 1, ptr, None, None, 4, None), E_ARG, "side_j")
    refused(rect(side(ref_ctrl=None), s, 8, 8, 1, ptr, None, None, 4, None), E_ARG, "side_i holds a null pointer")
    refused(rect(s, side(cnt_case=base + 4), 8, 8, 1, ptr, None, None, 4, None), E_ARG, "16-byte aligned")
    refused(rect(s, s, 8, 8, 2, ptr, None, None, 4, None), E_ARG, "test 2")
    refused(rect(s, s, 8, 8, 1, None, None, None, 4, None), E_ARG, "chisq")
    refused(rect(s, s, 8, 8, 1, ptr, None, None, 3, None), E_ARG, "ld 3 < n_j 4")
    refused(rect(s, s, 7, 8, 1, ptr, None, None, 4, None), E_ARG, "odd")
    refused(rect(s, s, 8, 0, 1, ptr, None, None, 4, None), E_ARG, "n_hap is 0")
    refused(rect(side(0), s, 8, 8, 1, ptr, None, None, 4, None), E_ARG, "n_i")
    refused(rect(s, s, 8, _lib.MAX_HAPS + 2, 1, ptr, None, None, 4, None), E_UNSUPPORTED, "LDX_MAX_HAPS")
    refused(lib.ldx_epi_counts_dev(s, s, 8, 8, None, 4, None), E_ARG, "counts")
    refused(lib.ldx_epi_counts_dev(s, s, 8, 8, ptr, 2, None), E_ARG, "ld 2 < n_j 4")
    hits = lambda *a: lib.ldx_epi_hits_dev(*a)  # noqa: E731
    refused(hits(s, s, 8, 8, 1, 2, 1.0, ptr, 4, ptr, 1.0, None, None, None, None), E_ARG, "self must be 0 or 1")
    refused(hits(s, side(5), 8, 8, 1, 1, 1.0, ptr, 4, ptr, 1.0, None, None, None, None), E_ARG, "self = 1")
    refused(hits(s, s, 8, 8, 1, 0, 0.0, ptr, 4, ptr, 1.0, None, None, None, None), E_ARG, "> 0")
    refused(hits(s, s, 8, 8, 1, 0, float("nan"), ptr, 4, ptr, 1.0, None, None, None, None), E_ARG, "> 0")
    refused(hits(s, s, 8, 8, 1, 0, 1.0, None, 4, ptr, 1.0, None, None, None, None), E_ARG, "hits")
    refused(hits(s, s, 8, 8, 1, 0, 1.0, ptr, 4, None, 1.0, None, None, None, None), E_ARG, "n_hits")
    refused(hits(s, s, 8, 8, 1, 0, 1.0, ptr, 4, ptr, 1.0, ptr, None, ptr, None), E_ARG, "together")
    refused(hits(s, s, 8, 8, 1, 0, 1.0, ptr, 4, ptr, 0.0, ptr, ptr, ptr, None), E_ARG, "bound_sig")
    fc = lambda *a: lib.ldx_epi_from_counts_dev(*a)  # noqa: E731
    refused(fc(4, 1, None, ptr, None, None, None, None, None, None, None), E_ARG, "tuples")
    refused(fc(0, 1, ptr, ptr, None, None, None, None, None, None, None), E_ARG, "m is 0")
    refused(fc(4, 7, ptr, ptr, None, None, None, None, None, None, None), E_ARG, "test 7")
    refused(fc(1 << 40, 1, ptr, ptr, None, None, None, None, None, None, None), E_UNSUPPORTED, "workgroups")

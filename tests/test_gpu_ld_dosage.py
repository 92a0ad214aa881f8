"""GPU: genotype-dosage LD (ldx_dosage_stats_dev, ldx_triangle_dosage_dev, ldx_ld_score_dosage_dev,
ldx_ld_neighbors_dosage_dev; ops' ``dosage=True``) against the exact integer oracle of tests/ld_dosage_exact.py.

Contract (include/ldx.h): a cell is within 4 float32 ulps of exact r, -0.0f exactly on a degenerate pair (v_i v_j == 0), +0.0f
exactly when num == 0; the LD-score sums equal the host sum of score_terms over the dosage r32 matrix bit for bit; the
neighbour lists hold every decided-in pair and no decided-out pair (ld_exact's 2^-19 margin) with the r32 cell as r.  The
panels, their special SNPs and the share of ambiguous pairs are pinned on the CPU by tests/test_ld_dosage_host.py.
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import fakevcf  # noqa: E402
import ld_dosage_exact as dx  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = [s for s in dx.SHAPES if s[0] > 128]
PHASE_SHAPES = [(5, 6), (129, 258), (300, 1008), (130, 10240)]


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    from ld_tools_amd import _lib

    buf = __import__("ctypes").create_string_buffer(64)
    _lib.check(_lib.lib.ldx_device_arch(0, buf, 64))
    assert buf.value.decode().startswith("gfx950"), buf.value
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def device_case(shape):
    """(panel, dosage r32 result, its square matrix on the host) of one shape: computed once, shared by the tests."""
    from ld_tools_amd import PackedPanel, ld_triangle
    p = PackedPanel.from_codes(dx.panel(shape)[0])
    tri = ld_triangle(p, fmt="r32", dosage=True)
    R = tri.r_matrix().cpu().numpy()
    R.setflags(write=False)
    return p, tri, R


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def host_sums(R, pos, w, annot_bits=None, k=0):
    """uint64 [n, 1 + k]: the sums from the r32 square (diagonal included), in numpy."""
    from ld_tools_amd import ops
    pos = np.asarray(pos, dtype=np.int64)
    T = ops.score_terms(R)
    T[np.abs(pos[:, None] - pos[None, :]) > w] = 0
    cols = [T.sum(axis=1, dtype=np.uint64)]
    for c in range(k):
        cols.append(T[:, ((np.asarray(annot_bits) >> c) & 1).astype(bool)].sum(axis=1, dtype=np.uint64))
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("shape", dx.SHAPES, ids=str)
def test_stats_and_r32_cells(gpu, shape):
    codes, where, ex = dx.panel(shape)
    p, tri, R = device_case(shape)
    n, h = shape
    hom, gstat = p.dosage_stats()
    assert p.n_ind == h // 2 and p.dosage_stats()[1] is gstat                       # cached
    hom, gstat = hom.cpu().numpy().view(np.uint32), gstat.cpu().numpy()
    assert np.array_equal(hom[:n], ex.hom) and not hom[n:].any() and not gstat[n:].any()
    assert np.array_equal(gstat[:n, 0], ex.a.astype(np.float64))
    assert np.array_equal(gstat[:n, 1] > 0, ex.live)
    assert np.array_equal(gstat[:n, 1][ex.live], 1.0 / np.sqrt(ex.v[ex.live].astype(np.float64)))
    assert np.array_equal(p.dosage_live(), ex.live)
    # the square: symmetric, the dosage diagonal, every cell below it against the oracle
    assert tri.dosage and R.shape == (n, n) and np.array_equal(bits(R), bits(R.T))
    want_diag = np.where(ex.live, np.float32(1.0), np.float32(-0.0)).astype(np.float32)
    assert np.array_equal(bits(np.diagonal(R)), bits(want_diag))
    off = ~np.eye(n, dtype=bool)
    neg0, pos0 = np.uint32(0x80000000), np.uint32(0)
    assert (bits(R)[ex.degenerate & off] == neg0).all()
    assert (bits(R)[ex.zero_num & off] == pos0).all()
    rest = off & ~ex.degenerate & ~ex.zero_num
    if rest.any():
        err = dx.ulp32_err(R[rest], ex.r64[rest])
        print(f"{shape}: {int(rest.sum())} cells, max error {err.max():.3f} float32 ulps")
        assert err.max() <= 4.0
        assert (R[rest] != 0).all()
    live = np.flatnonzero(ex.live)
    if live.size >= 2:
        c = np.corrcoef(ex.g[live].astype(np.float64))
        d = np.abs(R[np.ix_(live, live)].astype(np.float64) - c)
        np.fill_diagonal(d, 0.0)
        assert d.max() <= 5e-7
    for s_, d_ in zip(where.get("source", []), where.get("duplicate", [])):
        assert R[d_, s_] == 1.0
    for s_, d_ in zip(where.get("source", []), where.get("complement", [])):
        assert R[d_, s_] == -1.0
    # the strip cells themselves (what r_matrix reads), and zero cells outside the triangle
    if n > 1:
        rows, cols = np.tril_indices(n, -1)
        cells = tri.r32.cpu().numpy()
        assert np.array_equal(bits(cells[tri.cell_index(rows, cols)]), bits(R[rows, cols]))
        assert int(np.count_nonzero(bits(cells))) <= rows.size


@pytest.mark.parametrize("shape", PHASE_SHAPES, ids=str)
def test_phase_invariance(gpu, shape):
    """Another phase inside every call and another order of the individuals: the kernel sees the same integers, so cells,
    sums and lists are bit-identical -- while the haplotype r of the two panels differs (the test is not vacuous)."""
    from ld_tools_amd import PackedPanel, ld_neighbors, ld_score, ld_triangle
    p, _, R = device_case(shape)
    q = PackedPanel.from_codes(dx.rephased(shape))
    n = shape[0]
    Rq = ld_triangle(q, fmt="r32", dosage=True).r_matrix().cpu().numpy()
    assert np.array_equal(bits(Rq), bits(R))
    pos = dx.positions(n)
    ann = np.random.default_rng(1).random((n, 3)) < 0.5
    for kw in (dict(window_bp=100 * 129), dict(window_bp=100 * 129, annot=ann)):
        assert np.array_equal(ld_score(q, pos, dosage=True, **kw).sums.cpu().numpy(),
                              ld_score(p, pos, dosage=True, **kw).sums.cpu().numpy())
    a, b = (ld_neighbors(x, pos, window_bp=int(pos[-1]), r2=dx.NEIGHBOUR_R2, dosage=True) for x in (p, q))
    assert np.array_equal(a.offsets.cpu().numpy(), b.offsets.cpu().numpy())
    assert np.array_equal(a.hits.cpu().numpy(), b.hits.cpu().numpy())
    Hp = ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()
    Hq = ld_triangle(q, fmt="r32").r_matrix().cpu().numpy()
    assert not np.array_equal(bits(Hp), bits(Hq))
    assert not np.array_equal(bits(Hp), bits(R))


@pytest.mark.parametrize("shape", [(1, 2), (5, 6), (130, 130), (129, 256), (300, 1008), (130, 10240)], ids=str)
def test_ld_scores(gpu, shape):
    from ld_tools_amd import ld_score, ops
    _, _, ex = dx.panel(shape)
    p, _, R = device_case(shape)
    n, h = shape
    ann = np.random.default_rng(n + h).random((n, 3)) < 0.4
    ab, k = ops.pack_annot(ann, n)
    cases = [dict(positions=pos, window_bp=w) for pos, w in dx.score_windows(n, seed=n)]
    cases += [dict(window_snps=0), dict(window_snps=129), dict(window_snps=n)]
    for kw in cases:
        pos = kw.get("positions", np.arange(n, dtype=np.int64))
        w = kw["window_bp"] if "positions" in kw else kw["window_snps"]
        res = ld_score(p, dosage=True, **kw)
        assert res.dosage and np.array_equal(res.sums.cpu().numpy(), host_sums(R, pos, w))
        resa = ld_score(p, annot=ann, dosage=True, **kw)
        got = resa.sums.cpu().numpy()
        assert np.array_equal(got, host_sums(R, pos, w, ab, k)) and np.array_equal(got[:, 0], res.sums.cpu().numpy()[:, 0])
        assert np.array_equal(ld_score(p, annot=ann, dosage=True, **kw).sums.cpu().numpy(), got)    # run to run
        assert np.array_equal(resa.live, ex.live)
        assert np.array_equal(resa.m, ops.window_counts(pos, w, ex.live, ab, k))
        if h // 2 > 2:
            assert np.array_equal(resa.adjusted(), ops.adjust_l2(resa.l2, resa.m, h // 2))
        else:
            with pytest.raises(ops._lib.LdxError):
                resa.adjusted()


@pytest.mark.parametrize("shape", dx.SHAPES, ids=str)
def test_neighbour_lists_and_pruning(gpu, shape):
    from ld_tools_amd import ld_neighbors, ld_prune, ops
    _, _, ex = dx.panel(shape)
    p, _, R = device_case(shape)
    n = shape[0]
    for pos, w in dx.neighbour_windows(n):
        din, amb, inw = dx.pair_classes(ex, dx.NEIGHBOUR_R2, pos, w)
        nb = ld_neighbors(p, pos, window_bp=w, r2=dx.NEIGHBOUR_R2, dosage=True)
        hits = nb.hits.cpu().numpy()
        got = np.zeros((n, n), dtype=bool)
        got[hits[:, 0], hits[:, 1]] = True
        assert nb.dosage and got.sum() == len(nb) and np.array_equal(got, got.T)
        assert not (din & ~got).any(), "a decided-in pair is missing"
        assert not (got & ~(din | amb)).any(), "a decided-out pair (or one outside the window) is listed"
        assert np.array_equal(hits[:, 2].view(np.uint32), bits(R[hits[:, 0], hits[:, 1]]))
        off = nb.offsets.cpu().numpy()
        assert np.array_equal(np.diff(off), got.sum(axis=1))
        # pruning: the device's selection over the strict lists equals the sequential rule on those very lists
        pr = ld_prune(p, pos, r2=dx.NEIGHBOUR_R2, window_bp=w, dosage=True)
        f = ex.a / (2.0 * ex.n_ind)
        assert np.array_equal(pr.rank, ops.priority_ranks(np.minimum(f, 1.0 - f), ex.live))
        state, _ = ops.select_host(pr.neighbors.offsets.cpu().numpy(), pr.neighbors.nbr.cpu().numpy(), pr.rank,
                                   ex.live.astype(np.uint8))
        assert np.array_equal(pr.keep, state == ops.SEL_INDEX) and not pr.keep[~ex.live].any()
        assert pr.neighbors.dosage and len(pr.neighbors) <= len(nb)     # r^2 > t is a subset of r^2 >= t


def test_clump_takes_the_dosage_lists(gpu):
    from ld_tools_amd import ld_clump, ops
    shape = (300, 1008)
    _, _, ex = dx.panel(shape)
    p, _, _ = device_case(shape)
    pos = dx.positions(300)
    pv = 10.0 ** -np.random.default_rng(3).uniform(0, 8, size=300)
    cl = ld_clump(p, pos, pv, p1=1e-3, p2=0.05, r2=0.2, window_bp=100 * 129, dosage=True)
    rank, ok = ops.clump_ranks(pv, 1e-3, 0.05, ex.live)
    state, owner = ops.select_host(cl.neighbors.offsets.cpu().numpy(), cl.neighbors.nbr.cpu().numpy(), rank, ok)
    assert cl.neighbors.dosage and np.array_equal(cl.owner, owner)
    assert np.array_equal(np.sort(cl.index), np.flatnonzero(state == ops.SEL_INDEX))
    assert np.array_equal(cl.degenerate, np.flatnonzero(~ex.live))


def test_default_unchanged_and_paths(gpu):
    """dosage=False is the call without the argument, bit for bit; the dosage entries refuse every kernel but the FP4 one."""
    from ld_tools_amd import LdxError, ld_neighbors, ld_prune, ld_score, ld_triangle
    shape = (300, 1008)
    p, _, R = device_case(shape)
    pos = dx.positions(300)
    same = lambda x, y: np.array_equal(x.cpu().numpy(), y.cpu().numpy())   # noqa: E731
    assert same(ld_triangle(p, fmt="r32", dosage=False).r32, ld_triangle(p, fmt="r32").r32)
    assert same(ld_triangle(p, dosage=False).ld32.view(__import__("torch").int32), ld_triangle(p).ld32.view(__import__("torch").int32))
    assert same(ld_score(p, pos, window_bp=5000, dosage=False).sums, ld_score(p, pos, window_bp=5000).sums)
    a, b = ld_neighbors(p, pos, window_bp=5000, dosage=False), ld_neighbors(p, pos, window_bp=5000)
    assert same(a.hits, b.hits) and same(a.offsets, b.offsets) and not a.dosage
    assert np.array_equal(ld_prune(p, pos, dosage=False).keep, ld_prune(p, pos).keep)
    assert not np.array_equal(bits(ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()), bits(R))
    for path in ("mfma", "popcount"):
        for call in (lambda: ld_triangle(p, fmt="r32", dosage=True, path=path),
                     lambda: ld_score(p, pos, dosage=True, path=path),
                     lambda: ld_neighbors(p, pos, dosage=True, path=path)):
            with pytest.raises(LdxError, match="LDX_E_UNSUPPORTED"):
                call()
    assert np.array_equal(bits(ld_triangle(p, fmt="r32", dosage=True, path="fp4").r_matrix().cpu().numpy()), bits(R))


def test_driver(gpu, tmp_path):
    """drivers/ldscore.py in dosage mode: the table is the op's on the packed codes, n_obs = N, M_5_50 from a / (2 N); a panel
    with a missing call is refused unless missing='ref'."""
    import gzip
    from ld_tools_amd import LdxError, PackedPanel, ld_score
    from ld_tools_amd.drivers.ingest import codes_matrix
    from ld_tools_amd.drivers.ldscore import ld_scores, ld_scores_by_group, write_ldscore
    vcf, names = fakevcf.make_chromosome()
    seen, rows = set(), []
    for rec in vcf.records:
        if rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
            seen.add(rec.id)
            rows.append([rec.pos, rec.id])
    with pytest.raises(LdxError, match="missing='ref'"):
        ld_scores(vcf, "6", rows, names, window_bp=2_000, dosage=True)
    tab = ld_scores(vcf, "6", rows, names, window_bp=2_000, dosage=True, missing="ref")
    carried = [nm for nm in names if nm in vcf.records[0].samples]
    by_id = {rec.id: rec for rec in reversed(vcf.records)}              # the first record of an id, as the driver finds it
    codes = codes_matrix([[a for nm in carried for a in by_id[r].samples[nm]["GT"]] for r in tab.rs_ids])
    ex = dx.DosageExact(np.asarray(codes, dtype=np.int8))
    p = PackedPanel.from_codes(np.asarray(codes, dtype=np.int8))
    want = ld_score(p, np.asarray(tab.poss, dtype=np.int64), window_bp=2_000, dosage=True)
    assert tab.scores.dosage and np.array_equal(tab.scores.sums.cpu().numpy(), want.sums.cpu().numpy())
    assert np.array_equal(tab.scores.live, ex.live)
    n_ind = len(carried)
    assert np.array_equal(tab.values(), tab.scores.adjusted(n_ind)[:, :1])
    assert np.array_equal(tab.alt_freqs_exact, ex.a / (2.0 * n_ind))
    paths = write_ldscore(str(tmp_path / "d"), tab)
    with gzip.open(paths[0], "rt") as f:
        lines = f.read().splitlines()
    keep = np.flatnonzero(ex.live)
    assert [ln.split("\t")[1] for ln in lines[1:]] == [tab.rs_ids[k] for k in keep]
    assert [ln.split("\t")[3] for ln in lines[1:]] == ["%.3f" % x for x in tab.values()[keep, 0]]
    maf = np.minimum(tab.alt_freqs_exact, 1.0 - tab.alt_freqs_exact)
    assert Path(paths[2]).read_text().split() == [str(int((ex.live & (maf > 0.05)).sum()))]
    # one pass for several groups: each table is ld_scores on the group alone
    groups = {"a": carried[:20], "b": carried[10:]}
    tabs = ld_scores_by_group(vcf, "6", rows, groups, window_bp=2_000, dosage=True, missing="ref")
    for label, members in groups.items():
        alone = ld_scores(vcf, "6", rows, members, window_bp=2_000, dosage=True, missing="ref")
        assert np.array_equal(tabs[label].scores.sums.cpu().numpy(), alone.scores.sums.cpu().numpy())
        assert np.array_equal(tabs[label].values(), alone.values())
    with pytest.raises(LdxError, match="missing='ref'"):
        ld_scores_by_group(vcf, "6", rows, groups, window_bp=2_000, dosage=True)

"""GPU: LD scores on the matrix-pipe band (ldx_ld_score_dev, ops.ld_score, drivers/ldscore.py).

Contract (include/ldx.h): sums[i][c] = the uint64 sum of rint(2^32 * (r *f32 r)) over the SNPs j with |pos_i - pos_j| <= w
(j = i included), r the r32 cell of ld_triangle(fmt="r32") bit for bit (the diagonal: r_matrix()'s), column 1 + k only over
the j whose annotation carries bit k.  Checked here as integers against a numpy sum of the r32 triangle's own cells.
"""
import gzip
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import fakevcf  # noqa: E402

pytestmark = pytest.mark.gpu


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


def r32_square(p):
    from ld_tools_amd import ops
    return ops.ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()


def host_sums(R, pos, w, bits=None, k=0):
    """The sums from the r32 square (float32 cells, diagonal included): numpy, uint64."""
    from ld_tools_amd import ops
    pos = np.asarray(pos, dtype=np.int64)
    T = ops.score_terms(R)
    T[np.abs(pos[:, None] - pos[None, :]) > w] = 0
    cols = [T.sum(axis=1, dtype=np.uint64)]
    for c in range(k):
        sel = ((np.asarray(bits) >> c) & 1).astype(bool)
        cols.append(T[:, sel].sum(axis=1, dtype=np.uint64))
    return np.stack(cols, axis=1)


def sums_of(res):
    return res.sums.cpu().numpy()


def windows_for(n, seed):
    """(positions, window) cases: self only, everything, a grid with many |delta| = w pairs, duplicates."""
    rng = np.random.default_rng(seed)
    grid = 1 + 100 * np.arange(n, dtype=np.int64)
    dup = np.sort(rng.integers(1, max(2, n // 3), size=n)).astype(np.int64)   # many equal positions
    ragged = np.cumsum(rng.integers(0, 40, size=n)).astype(np.int64) + 7
    return [(grid, 0), (grid, int(grid[-1])), (grid, 300), (grid, 100 * 129), (dup, 0), (dup, 2), (ragged, 150)]


@pytest.mark.parametrize("shape", [(300, 5008), (1000, 1008), (129, 257), (700, 333), (2500, 10240)])
def test_sums_equal_the_r32_triangle(gpu, shape):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = shape
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=11 + n), gpu)
    R = r32_square(p)
    for pos, w in windows_for(n, n):
        got = sums_of(ops.ld_score(p, pos, window_bp=w))
        assert got.dtype == np.uint64 and got.shape == (n, 1)
        assert np.array_equal(got, host_sums(R, pos, w)), (shape, w)
    # the everything-window: the row sums of the square r^2 matrix
    pos, w = windows_for(n, n)[1]
    assert np.array_equal(sums_of(ops.ld_score(p, pos, window_bp=w))[:, 0], ops.score_terms(R).sum(axis=1, dtype=np.uint64))
    # a window of SNP counts: positions 0 .. n-1
    assert np.array_equal(sums_of(ops.ld_score(p, window_snps=37)), host_sums(R, np.arange(n), 37))


@pytest.mark.parametrize("path", ["fp4", "mfma"])
def test_missing_codes_and_degenerate_snps(gpu, path):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = 900, 1008
    codes = synth.synth_codes_host(n, h, seed=23, miss=0.02, mono=0.06, miss_rows=0.5)
    p = PackedPanel.from_codes(codes, gpu)
    a, r = p.alt_counts().astype(np.int64), p.ref_counts().astype(np.int64)
    deg = a * r == 0
    assert deg.sum() > 10 and (a + r < h).sum() > 100
    R = r32_square(p)
    pos = 1 + 50 * np.arange(n, dtype=np.int64)
    for w in (0, 500, 5000):
        res = ops.ld_score(p, pos, window_bp=w, path=path)
        got = sums_of(res)
        assert np.array_equal(got, host_sums(R, pos, w)), w
        assert (got[deg] == 0).all()
        assert (res.m[deg, 0] >= 0).all()
    # a degenerate SNP adds 0 to every neighbour: the same sums with its codes replaced by another degenerate pattern
    codes2 = codes.copy()
    codes2[deg] = 0
    p2 = PackedPanel.from_codes(codes2, gpu)
    assert np.array_equal(sums_of(ops.ld_score(p2, pos, window_bp=5000, path=path)),
                          sums_of(ops.ld_score(p, pos, window_bp=5000, path=path)))


def test_categories(gpu):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = 1100, 1008
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=5, miss=0.005, mono=0.02), gpu)
    R = r32_square(p)
    pos = 1 + 100 * np.arange(n, dtype=np.int64)
    w = 100 * 300
    rng = np.random.default_rng(1)
    base = sums_of(ops.ld_score(p, pos, window_bp=w))
    for k in range(1, 9):
        ann = rng.random((n, k)) < rng.uniform(0.05, 0.7, size=k)
        for path in ("fp4", "mfma"):
            res = ops.ld_score(p, pos, window_bp=w, annot=ann, path=path)
            got = sums_of(res)
            assert got.shape == (n, 1 + k)
            bits = (ann.astype(np.uint8) << np.arange(k, dtype=np.uint8)).sum(axis=1).astype(np.uint8)
            assert np.array_equal(got, host_sums(R, pos, w, bits, k)), (k, path)
            assert np.array_equal(got[:, 0], base[:, 0])
    ones = np.ones((n, 8), dtype=bool)
    ones[:, 3] = rng.random(n) < 0.5
    got = sums_of(ops.ld_score(p, pos, window_bp=w, annot=ones))
    for c in (1, 2, 3 + 2, 8):
        assert np.array_equal(got[:, c], got[:, 0])
    assert np.array_equal(got[:, 0], base[:, 0])


def test_float64_ground_truth(gpu):
    """l2 against r^2 computed in float64 from the codes with numpy, independently of the r32 code."""
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = 400, 333
    codes = synth.synth_codes_host(n, h, seed=31, miss=0.03, mono=0.03, miss_rows=0.6)
    p = PackedPanel.from_codes(codes, gpu)
    A = (codes == 1).astype(np.float64)
    a = A.sum(axis=1)
    r = (codes == 0).sum(axis=1).astype(np.float64)
    num = h * (A @ A.T) - np.outer(a, a)
    den = np.outer(a * r, a * r)
    r2 = np.where(den > 0, num * num / np.where(den > 0, den, 1.0), 0.0)
    live = a * r > 0
    np.fill_diagonal(r2, np.where(live, ((h - a) / np.where(live, r, 1.0)) ** 2, 0.0))
    pos = 1 + 10 * np.arange(n, dtype=np.int64)
    for w in (0, 200, 10 * n):
        res = ops.ld_score(p, pos, window_bp=w)
        mask = np.abs(pos[:, None] - pos[None, :]) <= w
        L = (r2 * mask).sum(axis=1)
        m = (mask & live[None, :]).sum(axis=1)
        assert np.array_equal(res.m[:, 0], m)
        assert (np.abs(res.l2[:, 0] - L) <= 2e-6 * L + m * 2.0 ** -32).all(), w


@pytest.fixture(scope="module")
def big(gpu):
    from ld_tools_amd import PackedPanel, synth
    n, h = 100_000, 5008
    codes = synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=gpu)
    return codes, PackedPanel.from_codes(codes, gpu), synth.synth_positions(n, step=500)


def test_full_size_configs2(gpu, big):
    import torch

    from ld_tools_amd import PackedPanel, ops
    codes, p, pos = big
    n, w = p.n_snps, 500_000
    res = ops.ld_score(p, pos, window_bp=w)
    got = sums_of(res)
    # closed-form window population: 1 000 neighbours each side, clipped at the ends -- SNP j lies in the windows of pop[j]
    # SNPs, so sum(m) = sum over the non-degenerate j of pop[j]
    idx = np.arange(n)
    pop = np.minimum(idx, 1000) + np.minimum(n - 1 - idx, 1000) + 1
    live = res.live
    assert live.mean() > 0.99
    assert int(res.m[:, 0].sum()) == int(pop[live].sum())
    # five slices, both ends included: SNPs whose whole window lies inside slice +- 1 000 SNPs against the r32 triangle
    for c0 in (0, 25_000, 50_000, 77_777, n - 300):
        c1 = min(n, c0 + 300)
        lo, hi = max(0, c0 - 1000), min(n, c1 + 1000)
        sub = PackedPanel.from_codes(codes[lo:hi], gpu)
        ref = host_sums(r32_square(sub), pos[lo:hi], w)
        assert np.array_equal(got[c0:c1], ref[c0 - lo:c1 - lo]), c0
        del sub
        torch.cuda.empty_cache()
    # the int8 band gives the same sums over the whole panel
    assert np.array_equal(sums_of(ops.ld_score(p, pos, window_bp=w, path="mfma")), got)


def test_reuse_and_streams(gpu):
    import torch

    from ld_tools_amd import PackedPanel, _lib, ops, synth
    n, h = 3000, 1008
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=41, miss=0.004), gpu)
    pos = 1 + 300 * np.arange(n, dtype=np.int64)
    ann = np.random.default_rng(3).random((n, 3)) < 0.3
    ws = torch.empty(_lib.lib.ldx_ld_score_workspace_bytes(n, h), dtype=torch.uint8, device=gpu)
    a = ops.ld_score(p, pos, window_bp=60_000, annot=ann, workspace=ws)
    b = ops.ld_score(p, pos, window_bp=60_000, annot=ann, workspace=ws)
    assert torch.equal(a.sums, b.sums)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = ops.ld_score(p, pos, window_bp=60_000, annot=ann)
    s.synchronize()
    assert torch.equal(a.sums, c.sums)
    # a different window through the same workspace, then the first again
    ops.ld_score(p, pos, window_bp=3_000, workspace=ws)
    d = ops.ld_score(p, pos, window_bp=60_000, annot=ann, workspace=ws)
    assert torch.equal(a.sums, d.sums)


def test_rejections(gpu):
    from types import SimpleNamespace

    from ld_tools_amd import LdxError, PackedPanel, _lib, ops, synth
    n = 200
    p = PackedPanel.from_codes(synth.synth_codes_host(n, 100, seed=2), gpu)
    pos = 1 + 10 * np.arange(n, dtype=np.int64)
    bad = pos.copy()
    bad[50] = 0
    with pytest.raises(LdxError, match="non-decreasing"):
        ops.ld_score(p, bad)
    import torch
    with pytest.raises(LdxError, match="non-decreasing"):
        ops.ld_score(p, torch.as_tensor(bad).to(gpu))
    with pytest.raises(LdxError, match="window"):
        ops.ld_score(p, pos, window_bp=-1)
    with pytest.raises(LdxError, match="at most 8"):
        ops.ld_score(p, pos, annot=np.zeros((n, 9), dtype=bool))
    with pytest.raises(LdxError, match="0/1"):
        ops.ld_score(p, pos, annot=np.full((n, 2), 2))
    with pytest.raises(LdxError, match="one entry per SNP"):
        ops.ld_score(p, pos[:-1])
    with pytest.raises(LdxError, match="LDX_MAX_HAPS"):
        ops.ld_score(SimpleNamespace(n_snps=n, n_hap=_lib.MAX_HAPS + 1, device=gpu), pos)
    with pytest.raises(LdxError, match="LDX_E_UNSUPPORTED"):
        ops.ld_score(p, pos, path="popcount")
    # the C entry point itself
    lib = _lib.lib
    pos_d = torch.as_tensor(pos).to(gpu)
    sums = torch.empty((n, 1), dtype=torch.uint64, device=gpu)
    ws = torch.empty(lib.ldx_ld_score_workspace_bytes(n, 100), dtype=torch.uint8, device=gpu)
    args = [p.alt.data_ptr(), p.acnt.data_ptr(), p.rcnt.data_ptr(), p.fa.data_ptr(), p.fr.data_ptr(), n, 100, pos_d.data_ptr(),
            1000, None, 0, 0, sums.data_ptr(), ws.data_ptr(), ws.numel(), None]
    assert lib.ldx_ld_score_dev(*args) == 0
    for k, v, rc in ((8, -1, -1), (10, 9, -1), (14, ws.numel() - 1, -1), (6, _lib.MAX_HAPS + 1, -3), (11, 1, -3)):
        bad_args = list(args)
        bad_args[k] = v
        if k == 10:
            bad_args[9] = pos_d.data_ptr()   # a non-null mask with 9 categories
        assert lib.ldx_ld_score_dev(*bad_args) == rc, (k, v)
    torch.cuda.synchronize()


def test_driver_and_writer(gpu, tmp_path):
    from ld_tools_amd import LdxError
    from ld_tools_amd.drivers.ldscore import ld_scores, write_ldscore
    vcf, names = fakevcf.make_chromosome()
    seen, rows = set(), []
    for rec in vcf.records:
        if rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
            seen.add(rec.id)
            rows.append([rec.pos, rec.id])
    n_rows = len(rows)
    rng = np.random.default_rng(4)
    ann = rng.random((n_rows, 2)) < 0.5
    rows_in = rows[::-1]
    ann_in = ann[::-1]
    tab = ld_scores(vcf, "6", rows_in + [[12, "rs1"]], names, window_bp=2_000, annot=np.concatenate([ann_in, [[True, True]]]),
                    annot_names=["coding", "enh"])
    assert len(tab.rs_ids) == n_rows
    adj = tab.scores.adjusted()
    base = str(tmp_path / "chr6")
    paths = write_ldscore(base, tab)
    assert paths == [base + ".l2.ldscore.gz", base + ".l2.M", base + ".l2.M_5_50"]
    with gzip.open(paths[0], "rt") as f:
        lines = f.read().splitlines()
    assert lines[0] == "CHR\tSNP\tBP\tcodingL2\tenhL2"
    live = tab.scores.live
    body = [ln.split("\t") for ln in lines[1:]]
    assert len(body) == int(live.sum())
    keep = np.flatnonzero(live)
    assert [b[1] for b in body] == [tab.rs_ids[k] for k in keep]
    assert [int(b[2]) for b in body] == [tab.poss[k] for k in keep]
    assert all(b[0] == "6" for b in body)
    for b, k in zip(body, keep):
        assert b[3:] == ["%.3f" % x for x in adj[k, 1:]]
    m_cols = [int(x) for x in Path(paths[1]).read_text().split()]
    assert m_cols == [int(tab.annot[keep][:, c].sum()) for c in range(2)]
    maf = np.minimum(np.asarray(tab.alt_freqs_exact), 1 - np.asarray(tab.alt_freqs_exact))
    m550 = [int((tab.annot[keep][:, c] & (maf[keep] > 0.05)).sum()) for c in range(2)]
    assert [int(x) for x in Path(paths[2]).read_text().split()] == m550
    # no annotation: one L2 column and the counts of every written SNP
    tab0 = ld_scores(vcf, "6", rows, names, window_bp=2_000, adjust=False)
    write_ldscore(base + "_0", tab0)
    with gzip.open(base + "_0.l2.ldscore.gz", "rt") as f:
        lines0 = f.read().splitlines()
    assert lines0[0] == "CHR\tSNP\tBP\tL2"
    l2 = tab0.scores.l2
    assert [ln.split("\t")[3] for ln in lines0[1:]] == ["%.3f" % x for x in l2[tab0.scores.live, 0]]
    assert Path(base + "_0.l2.M").read_text().split() == [str(int(tab0.scores.live.sum()))]
    # mixed ploidy is refused
    vcf2, names2 = fakevcf.make_chromosome(haploid_from=30)
    rows2 = [[rec.pos, rec.id] for rec in vcf2.records if rec.id.startswith("rs") and ";" not in rec.id][:40]
    with pytest.raises(LdxError, match="mixed ploidy"):
        ld_scores(vcf2, "6", rows2, names2)

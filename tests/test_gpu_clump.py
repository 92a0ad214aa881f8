"""GPU: neighbour lists on the matrix-pipe band (ldx_ld_neighbors_dev), the greedy selection (ldx_ld_select_dev) and
clumping / pruning on top of them (ops.ld_neighbors, ld_clump, ld_prune, drivers/clump.py, drivers/prune.py).

Ground truth: the square r matrix of ld_triangle(fmt="r32").r_matrix(); a pair (i, j), i != j, is a neighbour pair iff
|pos_i - pos_j| <= w and s = r *f32 r >= b (b = the float32 bound of the threshold).  The greedy results are compared with a
plain sequential loop over the host neighbour sets.
"""
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


def host_mask(R, pos, w, b, row0=0, col0=0):
    """bool block: the neighbour pairs of rows row0.. x columns col0.. of the square R (a block of it)."""
    pos = np.asarray(pos, dtype=np.int64)
    nr, nc = R.shape
    S = np.multiply(R, R, dtype=np.float32)
    M = (np.abs(pos[row0:row0 + nr, None] - pos[None, col0:col0 + nc]) <= w) & (S >= b)
    rr, cc = np.nonzero(np.arange(row0, row0 + nr)[:, None] == np.arange(col0, col0 + nc)[None, :])
    M[rr, cc] = False
    return M


def csr_of(nb):
    return nb.offsets.cpu().numpy().astype(np.int64), nb.hits.cpu().numpy()


def check_csr(nb, R, pos, w, b):
    """Every row's sorted neighbour rows equal the host set; r and s equal the square's cells bit for bit."""
    n = R.shape[0]
    off, h = csr_of(nb)
    assert off.shape == (n + 1,) and off[0] == 0 and off[-1] == h.shape[0]
    M = host_mask(R, pos, w, b)
    ii, jj = np.nonzero(M)   # row-major: sorted by (row, neighbour), both orientations (M is symmetric)
    assert np.array_equal(np.diff(off), M.sum(axis=1))
    assert np.array_equal(h[:, 0].astype(np.int64), ii) and np.array_equal(h[:, 1].astype(np.int64), jj)
    assert np.array_equal(h[:, 2].view(np.uint32), R[ii, jj].view(np.uint32))
    S = np.multiply(R, R, dtype=np.float32)
    assert np.array_equal(h[:, 3].view(np.uint32), S[ii, jj].view(np.uint32))
    return M


def windows_for(n, seed):
    """(positions, window) cases: self only, everything, a grid with many |delta| = w pairs, duplicates, ragged spacing."""
    rng = np.random.default_rng(seed)
    grid = 1 + 100 * np.arange(n, dtype=np.int64)
    dup = np.sort(rng.integers(1, max(2, n // 3), size=n)).astype(np.int64)
    ragged = np.cumsum(rng.integers(0, 40, size=n)).astype(np.int64) + 7
    return [(grid, 0), (grid, int(grid[-1])), (grid, 300), (grid, 100 * 129), (dup, 0), (dup, 2), (ragged, 150)]


def seq_select(M_rows, rank, member_ok):
    """The sequential rule as a plain loop over host neighbour sets (M_rows[i]: neighbour rows of i)."""
    NONE = 0xFFFFFFFF
    n = len(rank)
    owner = [-1] * n
    index = []
    for i in sorted((k for k in range(n) if rank[k] != NONE), key=lambda k: rank[k]):
        if owner[i] >= 0:
            continue
        owner[i] = i
        index.append(i)
        for j in M_rows[i]:
            if owner[j] < 0 and member_ok[j]:
                owner[j] = int(i)
    return index, np.asarray(owner, dtype=np.int64)


def rows_of(M):
    return [np.flatnonzero(M[i]).tolist() for i in range(M.shape[0])]


@pytest.mark.parametrize("shape", [(300, 5008), (1000, 1008), (129, 257), (700, 333), (2500, 10240)])
def test_neighbor_lists_equal_the_r32_square(gpu, shape):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = shape
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=11 + n), gpu)
    R = r32_square(p)
    S = np.multiply(R, R, dtype=np.float32)
    for pos, w in windows_for(n, n):
        for t in (0.05, 0.2, 0.5, 0.8):
            for strict in (False, True):
                nb = ops.ld_neighbors(p, pos, window_bp=w, r2=t, strict=strict)
                check_csr(nb, R, pos, w, ops.r2_bound(t, strict))
        # t = an observed s: the equality pairs are in under >= and out under >
        inwin = (np.abs(pos[:, None] - pos[None, :]) <= w) & ~np.eye(n, dtype=bool) & (S > 0.01)
        if inwin.any():
            t0 = float(S[inwin][len(S[inwin]) // 2])
            eq = int((inwin & (S == np.float32(t0))).sum())
            assert eq > 0
            ge = ops.ld_neighbors(p, pos, window_bp=w, r2=t0)
            gt = ops.ld_neighbors(p, pos, window_bp=w, r2=t0, strict=True)
            assert ops.r2_bound(t0) == np.float32(t0) and ops.r2_bound(t0, True) > np.float32(t0)
            Mge = check_csr(ge, R, pos, w, np.float32(t0))
            Mgt = check_csr(gt, R, pos, w, ops.r2_bound(t0, True))
            assert int(Mge.sum()) - int(Mgt.sum()) == eq
    # window_snps: positions 0 .. n-1
    nb = ops.ld_neighbors(p, window_snps=7, r2=0.2)
    check_csr(nb, R, np.arange(n), 7, ops.r2_bound(0.2))


@pytest.mark.parametrize("shape", [(1000, 1008), (700, 333), (2500, 10240)])
def test_fp4_and_int8_bands_give_identical_lists(gpu, shape):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = shape
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=3 + n, miss=0.01, mono=0.02), gpu)
    for pos, w in windows_for(n, 5)[1:4]:
        a = ops.ld_neighbors(p, pos, window_bp=w, r2=0.2)
        b = ops.ld_neighbors(p, pos, window_bp=w, r2=0.2, path="mfma")
        oa, ha = csr_of(a)
        ob, hb = csr_of(b)
        assert np.array_equal(oa, ob) and np.array_equal(ha, hb)
    with pytest.raises(ops._lib.LdxError, match="UNSUPPORTED|popcount"):
        ops.ld_neighbors(p, window_snps=3, path="popcount")


@pytest.mark.parametrize("path", [None, "mfma"])
def test_missing_codes_and_degenerate_snps(gpu, path):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = 900, 1008
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=23, miss=0.02, mono=0.06, miss_rows=0.5), gpu)
    R = r32_square(p)
    live = ops.live_snps(p.alt_counts(), p.ref_counts())
    assert (~live).sum() > 0
    pos = 1 + 50 * np.arange(n, dtype=np.int64)
    for t in (0.05, 0.5, 1.0):
        nb = ops.ld_neighbors(p, pos, window_bp=3000, r2=t, path=path)
        check_csr(nb, R, pos, 3000, ops.r2_bound(t))
        off, hh = csr_of(nb)
        dead = np.flatnonzero(~live)
        assert (np.diff(off)[dead] == 0).all() and not np.isin(hh[:, 1], dead).any()
    big = np.abs(R) > 1
    big[np.abs(pos[:, None] - pos[None, :]) > 3000] = False
    np.fill_diagonal(big, False)
    if big.any():   # |r| > 1 (missing codes) passes through unchanged: checked bit for bit by check_csr above at t = 1
        off, hh = csr_of(ops.ld_neighbors(p, pos, window_bp=3000, r2=1.0, path=path))
        assert (np.abs(hh[:, 2].view(np.float32)) > 1).sum() == big.sum()


def test_overflow_retry_gives_the_same_lists(gpu):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = 2000, 1008
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=8), gpu)
    pos = synth.synth_positions(n)
    full = ops.ld_neighbors(p, pos, window_bp=20_000, r2=0.1)
    assert len(full) > 5000
    tiny = ops.ld_neighbors(p, pos, window_bp=20_000, r2=0.1, hit_capacity=256)
    o1, h1 = csr_of(full)
    o2, h2 = csr_of(tiny)
    assert np.array_equal(o1, o2) and np.array_equal(h1, h2)
    i, j, r = full.pairs()
    assert (i < j).all() and len(i) * 2 == len(full)


def clump_ref(M, p, p1, p2, live):
    from ld_tools_amd import ops
    rank, ok = ops.clump_ranks(p, p1, p2, live)
    return seq_select(rows_of(M), rank, ok)


def check_clumps(res, M, p, p1, p2, live):
    from ld_tools_amd import ops
    index, owner = clump_ref(M, p, p1, p2, live)
    assert res.index.tolist() == index
    assert np.array_equal(res.owner, owner)
    rank, _ = ops.clump_ranks(p, p1, p2, live)
    for j in np.flatnonzero((rank != ops.NONE_U32) & (res.owner != np.arange(len(p)))):
        # a removed candidate has a neighbour index of smaller rank
        nbr = np.flatnonzero(M[j])
        assert any(res.owner[k] == k and rank[k] < rank[j] for k in nbr)
    for k, mem in res.clumps():
        assert np.array_equal(mem, np.sort(mem)) and (res.owner[mem] == k).all()


def test_clump_and_prune_equal_the_sequential_loop(gpu):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h = 1500, 2008
    p = PackedPanel.from_codes(synth.synth_codes_host(n, h, seed=19, miss=0.005, mono=0.03), gpu)
    R = r32_square(p)
    live = ops.live_snps(p.alt_counts(), p.ref_counts())
    pos = np.cumsum(np.random.default_rng(2).integers(0, 300, size=n)).astype(np.int64) + 1
    rng = np.random.default_rng(7)
    pv = 10.0 ** -rng.uniform(0, 9, size=n)
    pv[rng.random(n) < 0.05] = np.nan
    pv[rng.random(n) < 0.1] = pv[rng.integers(0, n, size=n)][rng.random(n) < 0.1][0]   # ties
    pv[::97] = 1e-5                                                                     # more ties
    for p1, p2, r2, w in [(1e-4, 1e-2, 0.5, 250_000), (1e-3, 1e-3, 0.2, 20_000), (0.5, 1.0, 0.1, 5_000),
                          (1e-6, 0.05, 0.8, 0)]:
        res = ops.ld_clump(p, pos, pv, p1=p1, p2=p2, r2=r2, window_bp=w)
        M = host_mask(R, pos, w, ops.r2_bound(r2))
        check_clumps(res, M, pv, p1, p2, live)
        assert np.array_equal(res.nan_p, np.flatnonzero(np.isnan(pv)))
        assert np.array_equal(res.degenerate, np.flatnonzero(~live))
    maf = np.minimum(p.fa.cpu().numpy()[:n], p.fr.cpu().numpy()[:n])
    for r2, w, prio in [(0.2, 250_000, None), (0.5, 3_000, None), (0.1, 10_000, rng.integers(0, 5, size=n).astype(float))]:
        res = ops.ld_prune(p, pos, r2=r2, window_bp=w, priority=prio)
        M = host_mask(R, pos, w, ops.r2_bound(r2, True))
        rank = ops.priority_ranks(maf if prio is None else prio, live)
        index, _ = seq_select(rows_of(M), rank, live)
        keep = np.zeros(n, dtype=bool)
        keep[index] = True
        assert np.array_equal(res.keep, keep)
        kk = np.flatnonzero(res.keep)
        assert not M[np.ix_(kk, kk)].any() and not res.keep[~live].any()
    # window_snps for pruning
    res = ops.ld_prune(p, r2=0.3, window_snps=20)
    M = host_mask(R, np.arange(n), 20, ops.r2_bound(0.3, True))
    index, _ = seq_select(rows_of(M), ops.priority_ranks(maf, live), live)
    assert np.flatnonzero(res.keep).tolist() == sorted(index)


def test_long_chain_converges_to_the_sequential_result(gpu):
    import torch
    from ld_tools_amd import PackedPanel, ops
    n, h = 3000, 1024
    rng = np.random.default_rng(12)
    codes = np.empty((n, h), dtype=np.int8)
    codes[0] = rng.random(h) < 0.5
    for k in range(1, n):   # consecutive rows highly correlated: a path graph under window_snps = 1
        flip = rng.random(h) < 0.02
        codes[k] = np.where(flip, 1 - codes[k - 1], codes[k - 1])
    p = PackedPanel.from_codes(torch.as_tensor(codes).to(gpu))
    pv = 1e-9 * (1.0 + np.arange(n))   # rank increases along the path
    res = ops.ld_clump(p, None, pv, p1=1.0, p2=1.0, r2=0.5, window_snps=1)
    off, hh = csr_of(res.neighbors)
    assert np.array_equal(np.diff(off), np.r_[1, np.full(n - 2, 2), 1])   # a path
    assert res.index.tolist() == list(range(0, n, 2))
    assert 0 < res.rounds <= n + 32   # (batches of 32 rounds; at most one round per candidate is needed)
    own = np.arange(n) - (np.arange(n) % 2)
    assert np.array_equal(res.owner, own)
    pr = ops.ld_prune(p, r2=0.5, window_snps=1, priority=-np.arange(n, dtype=float))
    assert np.flatnonzero(pr.keep).tolist() == list(range(0, n, 2))


def test_scale_40k_band_and_greedy(gpu):
    from ld_tools_amd import PackedPanel, ops, synth
    n, h, w = 40_000, 5008, 250_000
    p = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=5))
    pos = synth.synth_positions(n)
    nb = ops.ld_neighbors(p, pos, window_bp=w, r2=0.2)
    off, hh = csr_of(nb)
    tri = ops.ld_triangle(p, fmt="r32")
    b = ops.r2_bound(0.2)
    reach = w // 500
    M_rows = []
    for r0 in range(0, n, 2048):
        r1 = min(n, r0 + 2048)
        c0, c1 = max(0, r0 - reach), min(n, r1 + reach)
        R = tri.r_matrix(rows=(r0, r1), cols=(c0, c1)).cpu().numpy()
        M = host_mask(R, pos, w, b, row0=r0, col0=c0)
        ii, jj = np.nonzero(M)
        seg = hh[off[r0]:off[r1]]
        assert np.array_equal(seg[:, 0].astype(np.int64), ii + r0) and np.array_equal(seg[:, 1].astype(np.int64), jj + c0)
        assert np.array_equal(seg[:, 2].view(np.uint32), R[ii, jj].view(np.uint32))
        M_rows += [(np.flatnonzero(M[k]) + c0).tolist() for k in range(r1 - r0)]
    del tri
    live = ops.live_snps(p.alt_counts(), p.ref_counts())
    pv = 10.0 ** -np.random.default_rng(1).uniform(0, 10, size=n)
    res = ops.ld_clump(p, pos, pv, p1=1e-4, p2=1e-2, r2=0.2, window_bp=w)
    rank, ok = ops.clump_ranks(pv, 1e-4, 1e-2, live)
    index, owner = seq_select(M_rows, rank, ok)
    assert res.index.tolist() == index and np.array_equal(res.owner, owner)
    pr = ops.ld_prune(p, pos, r2=0.2, window_bp=w)
    Ms = [[j for j in row] for row in M_rows]   # (no s exactly at the bound here: > and >= agree, checked below)
    assert (hh[:, 3].view(np.float32) != b).all()
    maf = np.minimum(p.fa.cpu().numpy()[:n], p.fr.cpu().numpy()[:n])
    index, _ = seq_select(Ms, ops.priority_ranks(maf, live), live)
    assert np.flatnonzero(pr.keep).tolist() == sorted(index)


def chrom_rows_of(vcf):
    seen, rows = set(), []
    for rec in vcf.records:
        if rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
            seen.add(rec.id)
            rows.append([rec.pos, rec.id])
    return rows


def test_drivers_write_the_sequential_result(gpu, tmp_path):
    import torch
    from ld_tools_amd import PackedPanel, ops
    from ld_tools_amd.drivers.clump import clump, write_clumped
    from ld_tools_amd.drivers.ingest import codes_matrix
    from ld_tools_amd.drivers.prune import prune, write_prune
    from ld_tools_amd.drivers.triangle import fetch_variants
    vcf, names = fakevcf.make_chromosome(n_variants=120, n_samples=60)
    rows = chrom_rows_of(vcf)
    rows_in = rows[::-1]
    rng = np.random.default_rng(9)
    p_in = 10.0 ** -rng.uniform(0, 7, size=len(rows_in))
    p_in[3] = np.nan
    tab = clump(vcf, "6", rows_in, names, p_in, p1=1e-3, p2=0.2, r2=0.1, window_bp=3_000)
    # the expected file from the sequential loop over the r32 square
    cv = fetch_variants(vcf, "6", rows_in, names)
    panel = PackedPanel.from_codes(codes_matrix(cv.genotypes))
    R = r32_square(panel)
    pos = np.asarray(cv.poss, dtype=np.int64)
    order = sorted(range(len(rows_in)), key=lambda k: rows_in[k][0])
    pv = p_in[order]
    live = ops.live_snps(panel.alt_counts(), panel.ref_counts())
    M = host_mask(R, pos, 3_000, ops.r2_bound(0.1))
    index, owner = clump_ref(M, pv, 1e-3, 0.2, live)
    assert len(index) > 1
    lines = [" CHR    F          SNP         BP        P    TOTAL   NSIG    S05    S01   S001  S0001    SP2"]
    for k in index:
        mem = [j for j in range(len(pv)) if owner[j] == k and j != k]
        mp = pv[mem]
        cnt = [int((mp > 0.05).sum()), int(((mp > 0.01) & (mp <= 0.05)).sum()), int(((mp > 0.001) & (mp <= 0.01)).sum()),
               int(((mp > 1e-4) & (mp <= 0.001)).sum()), int((mp <= 1e-4).sum())]
        sp2 = ",".join(cv.rs_ids[j] + "(1)" for j in mem) or "NONE"
        lines.append("%4s %4d %12s %10d %8s %8d %6d %6d %6d %6d %6d    %s" % ("6", 1, cv.rs_ids[k], cv.poss[k],
                                                                             "%.3g" % pv[k], len(mem), *cnt, sp2))
    path = write_clumped(str(tmp_path / "chr6.clumped"), tab)
    assert Path(path).read_bytes() == ("\n".join(lines + ["", ""]) + "\n").encode()
    # pruning
    pt = prune(vcf, "6", rows_in, names, r2=0.1, window_bp=3_000)
    Mp = host_mask(R, pos, 3_000, ops.r2_bound(0.1, True))
    maf = np.minimum(panel.fa.cpu().numpy()[:len(pv)], panel.fr.cpu().numpy()[:len(pv)])
    kept, _ = seq_select(rows_of(Mp), ops.priority_ranks(maf, live), live)
    kept = set(kept)
    base = str(tmp_path / "chr6")
    pin, pout = write_prune(base, pt)
    assert Path(pin).read_text() == "".join(cv.rs_ids[k] + "\n" for k in range(len(pv)) if k in kept)
    assert Path(pout).read_text() == "".join(cv.rs_ids[k] + "\n" for k in range(len(pv)) if k not in kept)

"""GPU: stored LD bands (ldx_ld_band_dev, ldx_band_score_dev, ldx_band_matvec_dev; ops.ld_band, ops.ld_cross_score,
LDBand.matvec, ld_ridge(band=), drivers/band.py).

Contract (include/ldx.h, "stored bands"): values[offsets[i] + j - lo[i]] is ld_triangle(fmt="r32")'s cell (i, j) bit for bit
for every pair i > j inside the window, each once and nothing else; the consumers' sums are exact integer sums of the
stored cells' terms.  Everything here is compared as bits or integers; the one tolerance -- 4 float32 ulps against the
exact oracle -- is the r32 cell's own contract.
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import fakevcf  # noqa: E402
import ld_band_cases as bc  # noqa: E402
import ld_dosage_exact as dx  # noqa: E402
import ld_exact as lx  # noqa: E402

pytestmark = pytest.mark.gpu

# smallest panel; smallest with in-window pairs; across one 128-column tile and a 64-row group; several tiles with
# half-filled passes; the LDS limit
SHAPES = [(1, 2), (5, 6), (129, 256), (130, 130), (300, 1008), (130, 10240)]
PATHS = ("fp4", "mfma")
CANARY = 0x5CA1AB1E


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


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def device_case(shape):
    """(codes, panel, haplotype r32 square, dosage r32 square) of one shape: computed once, shared by the tests."""
    from ld_tools_amd import PackedPanel, ld_triangle
    codes = dx.panel(shape)[0]
    p = PackedPanel.from_codes(codes)
    R = ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()
    Rd = ld_triangle(p, fmt="r32", dosage=True).r_matrix().cpu().numpy()
    R.setflags(write=False)
    Rd.setflags(write=False)
    return codes, p, R, Rd


def band_cells(R, lo, n):
    """The band's cells from the square, in layout order."""
    rows = [R[i, lo[i]:i] for i in range(n)]
    return np.concatenate(rows) if rows else np.zeros(0, dtype=np.float32)


def in_window_lower(pos, w):
    m = lx.window_mask(pos, w)
    return np.tril(m, -1)


def raw_store(p, pos_d, w, lo, offsets, buf, n_cells, path, dosage):
    """ldx_ld_band_dev / ldx_ld_band_dosage_dev straight into `buf`."""
    import torch
    from ld_tools_amd import _lib, ops
    from ld_tools_amd.panel import _stream_ptr
    lib = _lib.lib
    ws = torch.empty(lib.ldx_ld_band_workspace_bytes(p.n_snps, p.n_hap), dtype=torch.uint8, device=p.device)
    if dosage:
        rc = lib.ldx_ld_band_dosage_dev(p.alt.data_ptr(), p.dosage_stats()[1].data_ptr(), p.n_snps, p.n_hap, pos_d.data_ptr(), w,
                                        ops.PATHS[path], lo.data_ptr(), offsets.data_ptr(), buf.data_ptr(), n_cells,
                                        ws.data_ptr(), ws.numel(), _stream_ptr())
    else:
        rc = lib.ldx_ld_band_dev(p.alt.data_ptr(), p.acnt.data_ptr(), p.rcnt.data_ptr(), p.fa.data_ptr(), p.fr.data_ptr(),
                                 p.n_snps, p.n_hap, pos_d.data_ptr(), w, ops.PATHS[path], lo.data_ptr(), offsets.data_ptr(),
                                 buf.data_ptr(), n_cells, ws.data_ptr(), ws.numel(), _stream_ptr())
    _lib.check(rc, "band store")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_cells(gpu, shape):
    """Every stored cell is the r32 triangle's, every in-window pair is present once, nothing beyond `values` is touched,
    both paths and a relaunch into a NaN-filled buffer give the same bytes; the dosage form against the dosage triangle;
    the cells against the exact oracles."""
    import torch
    from ld_tools_amd import ops
    codes, p, R, Rd = device_case(shape)
    n, h = shape
    ex = {False: lx.Exact(codes), True: dx.panel(shape)[2]}
    worst = 0.0
    for pos, w in lx.score_windows(n, n):
        lo, off = ops.band_layout_host(pos, w)
        lower = in_window_lower(pos, w)
        assert int(off[n]) == int(lower.sum())           # every in-window pair, none twice
        for dosage, square in ((False, R), (True, Rd)):
            want = band_cells(square, lo, n)
            got = {}
            for path in (PATHS if not dosage else ("fp4",)):
                b = ops.ld_band(p, pos, window_bp=w, path=path, dosage=dosage)
                assert np.array_equal(b.lo.cpu().numpy().view(np.uint32), lo)
                assert np.array_equal(b.offsets.cpu().numpy().view(np.uint64), off)
                assert b.n_cells == int(off[n]) and b.dosage == dosage and b.window == w
                got[path] = b.values.cpu().numpy()
                assert np.array_equal(bits(got[path]), bits(want)), (shape, w, path, dosage)
                assert np.array_equal(bits(b.diag.cpu().numpy()), bits(np.diagonal(square)))
                # a relaunch into a NaN-filled buffer with canary words behind it: the same bytes, the canaries untouched
                buf = torch.full((b.n_cells + 64,), float("nan"), dtype=torch.float32, device=gpu)
                buf[b.n_cells:].view(torch.int32).fill_(CANARY)
                pos_d = torch.as_tensor(pos).to(gpu)
                raw_store(p, pos_d, w, b.lo, b.offsets, buf, b.n_cells, path, dosage)
                back = buf.cpu().numpy()
                assert np.array_equal(bits(back[:b.n_cells]), bits(want)), (shape, w, path, dosage)
                assert (back[b.n_cells:].view(np.uint32) == CANARY).all()
            if not dosage:
                assert np.array_equal(bits(got["fp4"]), bits(got["mfma"]))
            # the cells against the exact oracle: -0.0f for a degenerate pair, +0.0f for num == 0, else within 4 ulps
            e = ex[dosage]
            ii, jj = np.nonzero(lower)                   # row-major: the layout's order
            v = got["fp4"]
            deg, zero = e.degenerate[ii, jj], e.zero_num[ii, jj]
            assert (bits(v)[deg] == np.uint32(0x80000000)).all() and (bits(v)[zero] == 0).all()
            rest = ~deg & ~zero
            if rest.any():
                err = lx.ulp32_err(v[rest], e.r64[ii, jj][rest])
                worst = max(worst, float(err.max()))
                assert err.max() <= 4.0
            # row(), to_dense(), to_csr(): the same cells through the host views
            if n <= 130 and w == lx.score_windows(n, n)[2][1]:
                dense = np.where(lx.window_mask(pos, w), square, np.float32(0.0))
                assert np.array_equal(bits(b.to_dense()), bits(dense))
                assert np.array_equal(bits(b.to_dense((n // 3, n))), bits(dense[n // 3:, n // 3:]))
                indptr, indices, data = b.to_csr()
                full = np.zeros((n, n), dtype=np.float32)
                for i in range(n):
                    full[i, indices[indptr[i]:indptr[i + 1]]] = data[indptr[i]:indptr[i + 1]]
                    assert (np.diff(indices[indptr[i]:indptr[i + 1]]) > 0).all()
                assert np.array_equal(bits(full), bits(dense)) and indptr[n] == 2 * b.n_cells + n
                cols, r = b.row(n - 1)
                assert np.array_equal(cols, np.arange(lo[n - 1], n - 1)) and np.array_equal(bits(r), bits(square[n - 1, lo[n - 1]:n - 1]))
    print(f"{shape}: worst cell error {worst:.3f} float32 ulps")


def test_a_foreign_layout_never_writes_outside_values(gpu):
    """A lo / offsets pair that belongs to another window gives wrong cells, never a write at or beyond n_cells."""
    import torch
    from ld_tools_amd import ops
    shape = (300, 1008)
    codes, p, R, Rd = device_case(shape)
    n = shape[0]
    pos = 1 + 100 * np.arange(n, dtype=np.int64)
    wide = ops.band_layout_host(pos, int(pos[-1]))        # every pair
    narrow = ops.band_layout_host(pos, 300)
    n_cells = int(narrow[1][n])
    lo_d = torch.as_tensor(wide[0].view(np.int32)).to(gpu)
    off_d = torch.as_tensor(wide[1].view(np.int64)).to(gpu)
    buf = torch.zeros(n_cells + 4096, dtype=torch.float32, device=gpu)
    buf[n_cells:].view(torch.int32).fill_(CANARY)
    raw_store(p, torch.as_tensor(pos).to(gpu), int(pos[-1]), lo_d, off_d, buf, n_cells, "fp4", False)
    assert (buf.cpu().numpy()[n_cells:].view(np.uint32) == CANARY).all()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_self_score_is_ld_score(gpu, shape):
    from ld_tools_amd import ops
    codes, p, R, Rd = device_case(shape)
    n = shape[0]
    for pos, w in lx.score_windows(n, n):
        for dosage in (False, True):
            b = ops.ld_band(p, pos, window_bp=w, dosage=dosage)
            got = ops.ld_cross_score(b, b)
            want = ops.ld_score(p, pos, window_bp=w, dosage=dosage).sums.cpu().numpy().view(np.uint64)[:, 0]
            assert got.sums.dtype == np.int64 and np.array_equal(got.sums.view(np.uint64), want), (shape, w, dosage)
            assert np.array_equal(np.asarray(got), want.astype(np.float64) / 2.0 ** 32)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_cross_score(gpu, shape):
    """Two populations: disjoint haplotype subsets of different sizes; the sums are the host's exact int64 sums of T over the
    two r32 squares inside the window, in either order of the arguments; a dosage band may be one side."""
    from ld_tools_amd import ld_triangle, ops
    codes, p, R, Rd = device_case(shape)
    n, h = shape
    h1 = max(1, h // 3) if h > 2 else 1
    h1 += (h1 % 2) if h > 2 else 0                        # whole individuals, so that the dosage form applies too
    pa, pb = p.select(haplotypes=np.arange(h1)), p.select(haplotypes=np.arange(h1, h))
    assert pa.n_hap != pb.n_hap or h == 2
    Ra = ld_triangle(pa, fmt="r32").r_matrix().cpu().numpy()
    Rb = ld_triangle(pb, fmt="r32").r_matrix().cpu().numpy()
    dos = h1 % 2 == 0 and (h - h1) % 2 == 0
    Rbd = ld_triangle(pb, fmt="r32", dosage=True).r_matrix().cpu().numpy() if dos else None
    for pos, w in lx.score_windows(n, n):
        inside = lx.window_mask(pos, w)
        ba, bb = ops.ld_band(pa, pos, window_bp=w), ops.ld_band(pb, pos, window_bp=w)
        want = np.where(inside, ops.cross_terms(Ra, Rb), 0).sum(axis=1, dtype=np.int64)
        ab, ba_ = ops.ld_cross_score(ba, bb), ops.ld_cross_score(bb, ba)
        assert np.array_equal(ab.sums, want), (shape, w)
        assert np.array_equal(ba_.sums, want), (shape, w)
        if dos:
            bd = ops.ld_band(pb, pos, window_bp=w, dosage=True)
            wantd = np.where(inside, ops.cross_terms(Ra, Rbd), 0).sum(axis=1, dtype=np.int64)
            assert np.array_equal(ops.ld_cross_score(ba, bd).sums, wantd), (shape, w)
    if n > 1:
        from ld_tools_amd import LdxError
        pos, w = lx.score_windows(n, n)[2]
        with pytest.raises(LdxError, match="layout"):
            ops.ld_cross_score(ops.ld_band(pa, pos, window_bp=w), ops.ld_band(pb, pos, window_bp=w + 100))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_matvec_is_ld_matvec(gpu, shape):
    from ld_tools_amd import ops
    codes, p, R, Rd = device_case(shape)
    n = shape[0]
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((n, 8)) * np.exp2(rng.integers(-12, 3, size=(n, 8)))).astype(np.float32)
    x[:, 5] = 0
    for pos, w in lx.score_windows(n, n):
        b = ops.ld_band(p, pos, window_bp=w)
        for power in (1, 2):
            for cols in ([1], [4, 5, 6], list(range(8))):
                got = b.matvec(x[:, cols], power=power)
                want = ops.ld_matvec(p, x[:, cols], pos, window_bp=w, power=power)
                assert got.sums.dtype == want.sums.dtype and got.sums.shape == (n, len(cols))
                assert np.array_equal(got.sums.cpu().numpy(), want.sums.cpu().numpy()), (shape, w, power, cols)
                assert np.array_equal(got.values().cpu().numpy(), want.values().cpu().numpy())
        y1 = b.matvec(x[:, 0])
        assert y1.values().shape == (n,)


def test_ridge_from_the_band_takes_the_same_steps(gpu):
    from ld_tools_amd import ops
    shape = (300, 1008)
    codes, p, R, Rd = device_case(shape)
    n = shape[0]
    pos, w = lx.score_windows(n, n)[2]
    z = np.random.default_rng(3).standard_normal((n, 3))
    b = ops.ld_band(p, pos, window_bp=w)
    plain = ops.ld_ridge(p, z, pos, window_bp=w, lam=2.0, max_iter=40)
    stored = ops.ld_ridge(p, z, lam=2.0, max_iter=40, band=b)
    assert np.array_equal(plain.beta.cpu().numpy().view(np.uint64), stored.beta.cpu().numpy().view(np.uint64))
    assert np.array_equal(plain.iterations, stored.iterations) and np.array_equal(plain.converged, stored.converged)
    assert np.array_equal(plain.residual, stored.residual) and (plain.iterations >= 2).all()
    one = ops.ld_ridge(p, z[:, 0], lam=2.0, max_iter=40, band=b)
    assert np.array_equal(one.beta.cpu().numpy().view(np.uint64), ops.ld_ridge(p, z[:, 0], pos, window_bp=w, lam=2.0, max_iter=40)
                          .beta.cpu().numpy().view(np.uint64))


def test_driver(gpu, tmp_path):
    """drivers/band.py: write_band round-trips through np.load; cross_scores_by_group is the operator on the groups' codes."""
    import gzip
    from ld_tools_amd import PackedPanel, ops
    from ld_tools_amd.drivers.band import band_matrix, cross_scores_by_group, write_band, write_cross_score
    from ld_tools_amd.drivers.ingest import codes_matrix, haplotype_columns
    vcf, names = fakevcf.make_chromosome()
    seen, rows = set(), []
    for rec in vcf.records:
        if rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
            seen.add(rec.id)
            rows.append([rec.pos, rec.id])
    m = band_matrix(vcf, "6", rows, names, window_bp=2_000)
    carried = [nm for nm in names if nm in vcf.records[0].samples]
    by_id = {rec.id: rec for rec in reversed(vcf.records)}              # the first record of an id, as the driver finds it
    codes = np.asarray(codes_matrix([[a for nm in carried for a in by_id[r].samples[nm]["GT"]] for r in m.rs_ids]), dtype=np.int8)
    pos = np.asarray(m.poss, dtype=np.int64)
    want = ops.ld_band(PackedPanel.from_codes(codes), pos, window_bp=2_000)
    assert m.band.n_cells > 0 and np.array_equal(bits(m.band.values.cpu().numpy()), bits(want.values.cpu().numpy()))
    paths = write_band(str(tmp_path / "b"), m, cells_per_block=100)
    assert [Path(x).name for x in paths] == ["b.band.values.npy", "b.band.offsets.npy", "b.band.lo.npy", "b.band.diag.npy",
                                             "b.variants.tsv"]
    values, offsets, lo = np.load(paths[0]), np.load(paths[1]), np.load(paths[2])
    assert values.dtype == np.float32 and offsets.dtype == np.uint64 and lo.dtype == np.uint32
    assert np.array_equal(bits(values), bits(want.values.cpu().numpy()))
    hl, ho = ops.band_layout_host(pos, 2_000)
    assert np.array_equal(lo, hl) and np.array_equal(offsets, ho)
    assert np.array_equal(bits(np.load(paths[3])), bits(want.diag.cpu().numpy()))
    lines = Path(paths[4]).read_text().splitlines()
    assert len(lines) == m.n + 1 and [ln.split("\t")[1] for ln in lines[1:]] == m.rs_ids
    # cross scores for every pair of groups, one pass over the VCF
    groups = {"a": carried[:12], "b": carried[12:], "c": carried[5:25]}
    tabs = cross_scores_by_group(vcf, "6", rows, groups, window_bp=2_000)
    assert list(tabs) == [("a", "b"), ("a", "c"), ("b", "c")]
    bands = {g: ops.ld_band(PackedPanel.from_codes(np.ascontiguousarray(codes[:, haplotype_columns(carried, mem)])), pos,
                            window_bp=2_000) for g, mem in groups.items()}
    for (ga, gb), tab in tabs.items():
        ref = ops.ld_cross_score(bands[ga], bands[gb])
        assert tab.rs_ids == m.rs_ids and np.array_equal(tab.sums, ref.sums) and np.array_equal(tab.scores, np.asarray(ref))
        path = write_cross_score(str(tmp_path / "x"), tab)
        with gzip.open(path, "rt") as f:
            out = f.read().splitlines()
        keep = np.flatnonzero(tab.live)
        assert out[0].split("\t") == ["CHR", "SNP", "BP", f"{ga}_{gb}L2"]
        assert [ln.split("\t")[1] for ln in out[1:]] == [tab.rs_ids[k] for k in keep]
        assert [ln.split("\t")[3] for ln in out[1:]] == ["%.3f" % tab.scores[k] for k in keep]


# ======================================================================================================================
# Past the first tile and span: the layout kernel's 4096-SNP tiles and its carry, the sweep's 2048-column spans, the store
# over dozens of 128-column tiles (tests/ld_band_cases.py; tests/test_ld_band_host.py pins what the cases cover).
# ======================================================================================================================
CANARY64 = 0x5CA1AB1E5CA1AB1E
GARBAGE64 = 0x5A5A5A5A12345678    # what `sums` holds before a consumer runs: the calls need no memset


@pytest.mark.parametrize("n", bc.layout_sizes + (bc.layout_size_64,))
def test_layout_kernel_past_one_tile(gpu, n):
    """ldx_ld_band_layout_dev alone on uploaded positions (it needs no panel): lo and offsets bit for bit the host mirror's
    over arrays pre-filled with 0xFF bytes, the canary words behind lo[n] and offsets[n + 1] untouched."""
    import torch
    from ld_tools_amd import _lib, ops
    from ld_tools_amd.panel import _stream_ptr
    cases = bc.position_cases_64(n) if n == bc.layout_size_64 else bc.position_cases(n)
    for k, (pos, w) in enumerate(cases):
        want_lo, want_off = ops.band_layout_host(pos, w)
        pos_d = torch.as_tensor(pos).to(gpu)
        lo = torch.full((n + 16,), -1, dtype=torch.int32, device=gpu)
        off = torch.full((n + 1 + 16,), -1, dtype=torch.int64, device=gpu)
        lo[n:] = CANARY
        off[n + 1:] = CANARY64
        _lib.check(_lib.lib.ldx_ld_band_layout_dev(pos_d.data_ptr(), n, w, lo.data_ptr(), off.data_ptr(), _stream_ptr()),
                   "ldx_ld_band_layout_dev")
        torch.cuda.synchronize()
        got_lo, got_off = lo.cpu().numpy().view(np.uint32), off.cpu().numpy().view(np.uint64)
        bad = np.flatnonzero(got_lo[:n] != want_lo)
        assert bad.size == 0, f"n {n}, case {k} (window {w}): lo differs first at SNP {bad[0]} (tile {bad[0] // bc.LAYOUT_TILE})"
        bad = np.flatnonzero(got_off[:n + 1] != want_off)
        assert bad.size == 0, (f"n {n}, case {k} (window {w}): offsets differ first at {bad[0]} (tile "
                               f"{(max(int(bad[0]), 1) - 1) // bc.LAYOUT_TILE}): {got_off[bad[0]]} for {want_off[bad[0]]}")
        assert (got_lo[n:] == CANARY).all() and (got_off[n + 1:] == CANARY64).all()
    if n == bc.layout_size_64:
        assert int(ops.band_layout_host(*cases[0])[1][n]) > 1 << 32        # the carry crossed 32 bits


@functools.lru_cache(maxsize=None)
def sweep_layout(k):
    """(positions, window, lo, offsets, rows, cols) of sweep case k on the host; computed once, shared, read-only."""
    from ld_tools_amd import ops
    pos, w = bc.sweep_cases()[k]
    lo, off = ops.band_layout_host(pos, w)
    rows, cols = bc.cell_rows_cols(lo, off)
    for a in (pos, lo, off, rows, cols):
        a.setflags(write=False)
    return pos, w, lo, off, rows, cols


@functools.lru_cache(maxsize=None)
def synthetic_band(k, big, second=False):
    """An LDBand over synthetic cells on sweep case k's layout -- the consumers are defined on any float32 cells (include/ldx.h,
    "stored bands") -- with a random diagonal (some -0.0f); (band, cells on the host, diagonal on the host)."""
    import torch
    from ld_tools_amd import ops
    pos, w, lo, off, rows, cols = sweep_layout(k)
    n = len(pos)
    dev = torch.device("cuda", 0)
    v = bc.synthetic_cells(rows.size, bc.CELL_SEEDS[k] + (100 if second else 0), big=big)
    rng = np.random.default_rng(1000 + k + (100 if second else 0))
    d = rng.uniform(-1.25, 1.25, n).astype(np.float32)
    d[rng.random(n) < 0.02] = np.float32(-0.0)
    v.setflags(write=False)
    d.setflags(write=False)
    band = ops.LDBand(torch.as_tensor(np.array(v)).to(dev), torch.as_tensor(lo.view(np.int32).copy()).to(dev),
                      torch.as_tensor(off.view(np.int64).copy()).to(dev), torch.as_tensor(np.array(d)).to(dev), pos, w, False, 0)
    return band, v, d


def raw_score(b1, b2, diagonals=True):
    """ldx_band_score_dev into sums full of garbage; int64 [n] on the host."""
    import torch
    from ld_tools_amd import _lib
    from ld_tools_amd.panel import _stream_ptr
    n = b1.n_snps
    sums = torch.full((n,), GARBAGE64, dtype=torch.int64, device=b1.values.device)
    _lib.check(_lib.lib.ldx_band_score_dev(b1.values.data_ptr(), b2.values.data_ptr(), b1.diag.data_ptr() if diagonals else None,
                                           b2.diag.data_ptr() if diagonals else None, b1.lo.data_ptr(), b1.offsets.data_ptr(), n,
                                           sums.data_ptr(), _stream_ptr()), "ldx_band_score_dev")
    return sums.cpu().numpy()


def raw_matvec(b, x32, power, diagonal=True):
    """ldx_band_matvec_dev on float32 [n, k] weights into sums full of garbage; int64 [n, k] on the host."""
    import torch
    from ld_tools_amd import _lib
    from ld_tools_amd.panel import _stream_ptr
    n, k = x32.shape
    x_d = torch.as_tensor(np.ascontiguousarray(x32)).to(b.values.device)
    sums = torch.full((n, k), GARBAGE64, dtype=torch.int64, device=b.values.device)
    _lib.check(_lib.lib.ldx_band_matvec_dev(b.values.data_ptr(), b.diag.data_ptr() if diagonal else None, b.lo.data_ptr(),
                                            b.offsets.data_ptr(), n, x_d.data_ptr(), k, power, sums.data_ptr(), _stream_ptr()),
               "ldx_band_matvec_dev")
    return sums.cpu().numpy()


def first_difference(got, want, what):
    """Fail with the first differing SNP, its 16-row group and how far it reaches back."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, f"{what}: {len(bad)} sums differ, the first at {bad[0].tolist()} (16-row group {int(bad[0][0]) // 16})"


@pytest.mark.parametrize("k", range(3), ids=["everything", "grid2100", "clustered"])
def test_score_sweep_past_one_span(gpu, k):
    """ldx_band_score_dev on synthetic cells: the host's exact integer sum of T over the stored cells, to both SNPs of every
    cell, plus T of the diagonals -- in either order of the bands, with NULL diagonals, and through ops.ld_cross_score."""
    from ld_tools_amd import ops
    pos, w, lo, off, rows, cols = sweep_layout(k)
    n = len(pos)
    b1, v1, d1 = synthetic_band(k, False)
    b2, v2, d2 = synthetic_band(k, False, second=True)
    assert not np.array_equal(v1, v2) and float(np.abs(v1).max()) <= 1.0 and float(np.abs(v2).max()) <= 1.0   # T is defined
    terms = ops.cross_terms(v1, v2)
    pairs = bc.pair_sums(n, rows, cols, terms)
    want = pairs + ops.cross_terms(d1, d2)
    first_difference(raw_score(b1, b2), want, f"score, case {k}")
    first_difference(raw_score(b2, b1), want, f"score, case {k}, swapped")
    first_difference(raw_score(b1, b2, diagonals=False), pairs, f"score, case {k}, no diagonals")
    got = ops.ld_cross_score(b1, b2)
    assert got.sums.dtype == np.int64 and np.array_equal(got.sums, want)


@functools.lru_cache(maxsize=None)
def host_matvec(k, big, power):
    """(x float32 [n, 8], x32 the scaled weights, pair sums int64 [n, 8], own terms int64 [n, 8]) of sweep case k: the
    integer sums of prod_terms over the stored cells in wrapping int64, one column per thread; computed once per
    (case, big, power) and shared by the widths."""
    from concurrent.futures import ThreadPoolExecutor
    from test_gpu_exact_oracle import rhs
    from ld_tools_amd import ops
    pos, w, lo, off, rows, cols = sweep_layout(k)
    n = len(pos)
    _, v, d = synthetic_band(k, big)
    x = rhs(n, n)
    x32 = ops.matvec_rhs(x, n, power)[0].cpu().numpy()
    pv = ops.prod_values(v, power)
    own = ops.prod_terms(ops.prod_values(d, power)[:, None], x32)

    def column(c):
        xc = np.ascontiguousarray(x32[:, c])
        s = np.zeros(n, dtype=np.int64)
        with np.errstate(over="ignore"):
            np.add.at(s, rows, ops.prod_terms(pv, xc[cols]))     # cell (i, j) feeds row i with the value at j ...
            np.add.at(s, cols, ops.prod_terms(pv, xc[rows]))     # ... and column j with the value at i
        return s

    with ThreadPoolExecutor(max_workers=8) as pool:
        pairs = np.stack(list(pool.map(column, range(8))), axis=1)
    for a in (x, x32, pairs, own):
        a.setflags(write=False)
    return x, x32, pairs, own


@pytest.mark.parametrize("big", [False, True], ids=["unit", "big"])
@pytest.mark.parametrize("k", range(3), ids=["everything", "grid2100", "clustered"])
def test_matvec_sweep_past_one_span(gpu, k, big):
    """ldx_band_matvec_dev on synthetic cells, powers 1 and 2, widths 1, 3 (a pass of two and a pass of one) and 8: the
    host's wrapping int64 sums of prod_terms.  ``big``: cells of +-2^22 .. 2^30 reach the clamp, and SNPs that collect
    several wrap (tests/test_ld_band_host.py pins both)."""
    from ld_tools_amd import ops
    b, v, d = synthetic_band(k, big)
    for power in (1, 2):
        x, x32, pairs, own = host_matvec(k, big, power)
        with np.errstate(over="ignore"):
            want = pairs + own
        for cols in ([1], [4, 5, 6], list(range(8))):
            got = raw_matvec(b, x32[:, cols], power)
            first_difference(got, want[:, cols], f"matvec, case {k}, big {big}, power {power}, columns {cols}")
        via = b.matvec(x[:, [4, 5, 6]], power=power)             # the Python entry scales the columns itself
        assert np.array_equal(via.x32.cpu().numpy(), x32[:, [4, 5, 6]])
        first_difference(via.sums.cpu().numpy(), want[:, [4, 5, 6]], f"LDBand.matvec, case {k}, big {big}, power {power}")
        if k == 2:
            first_difference(raw_matvec(b, x32[:, [0, 3]], power, diagonal=False), pairs[:, [0, 3]],
                             f"matvec, case {k}, big {big}, power {power}, no diagonal")


# ---- the store at size -------------------------------------------------------------------------------------------------
STORE_SHAPE = (4500, 130)          # 36 tiles of 128 columns; 130 is even: the dosage form applies
STORE_SPECIAL = (2045, 2048, 4497)  # a monomorphic, an all-ALT and an all-missing row from each: both sides of a tile edge, the last tile


@functools.lru_cache(maxsize=None)
def store_case():
    """(codes, panel, haplotype r32 square, dosage r32 square) of the 4500-SNP panel: computed once, shared, read-only."""
    from ld_tools_amd import PackedPanel, ld_triangle, synth
    n, h = STORE_SHAPE
    codes = synth.synth_codes_host(n, h, seed=3 * n + h, block_len=200, rho=0.97, miss=0.01, miss_rows=0.5)
    for r0 in STORE_SPECIAL:
        codes[r0], codes[r0 + 1], codes[r0 + 2] = 0, 1, 2
    assert STORE_SPECIAL[0] + 2 == 2047 and STORE_SPECIAL[1] % 128 == 0 and STORE_SPECIAL[2] // 128 == (n - 1) // 128
    p = PackedPanel.from_codes(codes)
    codes.setflags(write=False)
    R = ld_triangle(p, fmt="r32").r_matrix().cpu().numpy()
    Rd = ld_triangle(p, fmt="r32", dosage=True).r_matrix().cpu().numpy()
    R.setflags(write=False)
    Rd.setflags(write=False)
    return codes, p, R, Rd


def first_cell_difference(got, want, lo, off, what):
    bad = np.flatnonzero(bits(got) != bits(want))
    if bad.size:
        i = int(np.searchsorted(off.astype(np.int64), bad[0], side="right")) - 1
        j = int(lo[i]) + int(bad[0]) - int(off[i])
        raise AssertionError(f"{what}: {bad.size} cells differ, the first is word {bad[0]} = cell ({i}, {j}): row tile {i // 128}, "
                             f"column tile {j // 128}, {(i // 128) - (j // 128)} tiles apart")


@pytest.mark.parametrize("k", range(3), ids=["everything", "grid2100", "clustered"])
def test_store_past_three_tiles(gpu, k):
    """The store epilogue over bands of up to 36 tiles: values, lo / offsets and diag against the r32 squares, both paths and
    the dosage form, and a relaunch into a NaN-filled buffer with canary words behind it."""
    import torch
    from ld_tools_amd import ops
    codes, p, R, Rd = store_case()
    n = STORE_SHAPE[0]
    pos, w, lo, off, rows, cols = sweep_layout(k)
    pos_d = torch.as_tensor(pos).to(gpu)
    wants = {False: band_cells(R, lo, n), True: band_cells(Rd, lo, n)}
    assert wants[False].size == int(off[n]) and (bits(wants[False]) == 0x80000000).any()   # degenerate rows take part
    for dosage, path in ((False, "fp4"), (False, "mfma"), (True, "fp4")):
        square, want = (Rd, wants[True]) if dosage else (R, wants[False])
        what = f"store, case {k}, {path}, dosage {dosage}"
        b = ops.ld_band(p, pos, window_bp=w, path=path, dosage=dosage)
        assert np.array_equal(b.lo.cpu().numpy().view(np.uint32), lo), what
        assert np.array_equal(b.offsets.cpu().numpy().view(np.uint64), off), what
        assert b.n_cells == int(off[n]) and b.dosage == dosage and b.window == w
        first_cell_difference(b.values.cpu().numpy(), want, lo, off, what)
        assert np.array_equal(bits(b.diag.cpu().numpy()), bits(np.diagonal(square))), what
        buf = torch.full((b.n_cells + 64,), float("nan"), dtype=torch.float32, device=gpu)
        buf[b.n_cells:].view(torch.int32).fill_(CANARY)
        raw_store(p, pos_d, w, b.lo, b.offsets, buf, b.n_cells, path, dosage)
        back = buf.cpu().numpy()
        first_cell_difference(back[:b.n_cells], want, lo, off, what + ", relaunch")
        assert (back[b.n_cells:].view(np.uint32) == CANARY).all(), what
        del b, buf


def test_real_band_at_size_feeds_the_consumers(gpu):
    """The 4500-SNP panel's band with 2100 SNPs each side, tied to the operators that are proven at size: its self score is
    ld_score's column 0 and its products are ld_matvec's, bit for bit."""
    from ld_tools_amd import ops
    codes, p, R, Rd = store_case()
    n = STORE_SHAPE[0]
    pos, w, lo, off, rows, cols = sweep_layout(1)
    b = ops.ld_band(p, pos, window_bp=w)
    got = ops.ld_cross_score(b, b)
    want = ops.ld_score(p, pos, window_bp=w).sums.cpu().numpy().view(np.uint64)[:, 0]
    first_difference(got.sums.view(np.uint64), want, "self score at 4500")
    from test_gpu_exact_oracle import rhs
    x = rhs(n, n)[:, [1, 3, 6]]
    for power in (1, 2):
        mine = b.matvec(x, power=power)
        ref = ops.ld_matvec(p, x, pos, window_bp=w, power=power)
        assert mine.sums.shape == (n, 3) and np.array_equal(mine.exps.cpu().numpy(), ref.exps.cpu().numpy())
        first_difference(mine.sums.cpu().numpy(), ref.sums.cpu().numpy(), f"band matvec at 4500, power {power}")


def test_stored_cells_at_the_lds_limit_against_the_exact_oracle(gpu):
    """lr2500 (2500 x 10240 = LDX_MAX_HAPS, LD across tiles): the stored cells of the everything window (20 tiles) and of
    129 SNPs each side against exact counts -- -0.0f iff degenerate, +0.0f iff num == 0, else within 4 ulps with num's sign."""
    from test_gpu_exact_oracle import check_cells
    from ld_tools_amd import PackedPanel, ops
    codes, _, ex = lx.long_range_panel("lr2500")
    n = ex.n_snps
    p = PackedPanel.from_codes(np.array(codes), gpu)
    windows = lx.neighbour_windows(n)
    for pos, w in (windows[0], windows[1]):
        lo, off = ops.band_layout_host(pos, w)
        rows, cols = bc.cell_rows_cols(lo, off)
        b = ops.ld_band(p, pos, window_bp=w)
        assert b.n_cells == rows.size > 0
        worst = check_cells(b.values.cpu().numpy(), ex, rows, cols, f"lr2500 band, window {w}")
        print(f"lr2500 band, window {w}: {rows.size} cells, worst error {worst:.3f} float32 ulps")
        del b

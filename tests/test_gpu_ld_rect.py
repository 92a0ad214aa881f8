"""GPU: rectangular LD (ops.ld_rect, ops.ld_rect_hits, drivers/rect.py; include/ldx.h, "rectangular LD") -- bit for bit
against the r32 triangle, against the exact integer oracles (tests/ld_exact.py, tests/ld_dosage_exact.py) across the
kernel's edges, symmetry, the untouched surroundings of the output, the hit lists against their host mirror and the driver.

Contract: cell (i, j) = the r32 cell of the two SNPs -- within 4 float32 ulps of the exact r, +0.0f exactly when the numerator
is 0, -0.0f on a degenerate pair -- whether or not the two rows are the same variant.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import fakevcf  # noqa: E402
import ld_dosage_exact as dx  # noqa: E402
import ld_exact as lx  # noqa: E402
import ld_rect_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

NEG0, POS0 = np.uint32(0x80000000), np.uint32(0)
ULPS = 4.0   # include/ldx.h: the bound of every r32 cell


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


def bits(t) -> np.ndarray:
    """uint32 bit patterns of a float32 device tensor / host array."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


_PAIRS = {}


def pair(shape, n_hap, family=0):
    """(codes_i, codes_j, panel_i, panel_j) of one case, built once and left unchanged."""
    from ld_tools_amd import PackedPanel
    key = (shape, n_hap, family)
    if key not in _PAIRS:
        ci, cj = rc.pair_codes(shape[0], shape[1], n_hap, seed=1000 * shape[0] + shape[1] + n_hap, family=family)
        _PAIRS[key] = (ci, cj, PackedPanel.from_codes(ci), PackedPanel.from_codes(cj))
    return _PAIRS[key]


def check_block(got32, ex, n_i, what):
    """The rectangle's cells against an oracle: the off-diagonal block [0, n_i) x [n_i, n) of an Exact / DosageExact over the
    stacked codes, or an ExactBlock / DosageExactBlock of the two sides (which IS that block)."""
    def field(name):
        a = getattr(ex, name)
        return a if isinstance(ex, lx.ExactBlock) else a[:n_i, n_i:]

    b = np.ascontiguousarray(got32).view(np.uint32)
    deg = field("degenerate")
    zero = field("zero_num")
    assert deg.shape == b.shape
    assert np.array_equal(b == NEG0, deg), f"{what}: -0.0f <=> degenerate"
    assert np.array_equal(b == POS0, zero), f"{what}: +0.0f <=> num == 0"
    one = (field("num2") == field("den2")) & ~deg   # num^2 == den2: exactly +1.0f / -1.0f (include/ldx.h)
    assert np.array_equal(got32[one], np.sign(field("num")[one]).astype(np.float32)), f"{what}: |r| = 1 cells"
    rest = ~deg & ~zero
    if rest.any():
        err = lx.ulp32_err(got32[rest], field("r64")[rest])
        print(f"{what}: {int(rest.sum())} cells, max error {float(err.max()):.3f} float32 ulps")
        assert float(err.max()) <= ULPS, f"{what}: {float(err.max())} ulps"
    return int(rest.sum())


# ---- 1. bit for bit against the triangle --------------------------------------------------------------------------------
@pytest.mark.parametrize("dosage", [False, True])
def test_rect_cells_are_the_triangles_cells_bit_for_bit(gpu, dosage):
    from ld_tools_amd import PackedPanel, ops
    codes, rows, cols = rc.triangle_panel()
    assert codes.shape == (400, 1008) and len(set(rows.tolist())) < rows.size and set(rows.tolist()) & set(cols.tolist())
    P = PackedPanel.from_codes(codes)
    got = ops.ld_rect(P.select(snps=rows), P.select(snps=cols), dosage=dosage)
    assert got.shape == (rows.size, cols.size) and got.dtype.is_floating_point and got.element_size() == 4
    tri = ops.ld_triangle(P, fmt="r32", dosage=dosage).r_matrix().cpu().numpy()[rows][:, cols]
    g, t = bits(got), bits(tri)
    same = rows[:, None] == cols[None, :]
    assert same.any() and (~same).any()
    assert np.array_equal(g[~same], t[~same])
    # the same variant on both sides: still the pair formula -- within 4 ulps of the exact diagonal, -0.0f when degenerate
    ex = dx.DosageExact(codes) if dosage else lx.Exact(codes)
    diag, live = ex.diagonal(), ex.live
    a, b = np.nonzero(same)
    snp = rows[a]
    cell, cell_bits = got.cpu().numpy()[a, b], g[a, b]
    assert (~live[snp]).any() and live[snp].any()
    assert np.array_equal(cell_bits[~live[snp]], np.full(int((~live[snp]).sum()), NEG0))
    err = lx.ulp32_err(cell[live[snp]], diag[snp][live[snp]])
    print(f"same-variant cells (dosage={dosage}): {int(live[snp].sum())}, max error {float(err.max()):.3f} ulps")
    assert float(err.max()) <= ULPS


# ---- 2. against the exact oracle, across the edges ----------------------------------------------------------------------
def test_edge_cases_cover_what_they_must():
    haps = sorted({h for _, h in rc.EDGE_CASES})
    assert haps == [2, 254, 256, 258, 1008, 5008] and set(s for s, _ in rc.EDGE_CASES) == set(rc.SHAPES)
    for h in haps:
        assert sum(1 for _, hh in rc.EDGE_CASES if hh == h) >= 2
    for s in rc.SHAPES:
        assert len({h for ss, h in rc.EDGE_CASES if ss == s}) >= 2


@pytest.mark.parametrize("shape,n_hap", rc.EDGE_CASES, ids=[f"{s[0]}x{s[1]}x{h}" for s, h in rc.EDGE_CASES])
def test_rect_against_the_exact_oracle(gpu, shape, n_hap):
    from ld_tools_amd import ops
    ci, cj, pi, pj = pair(shape, n_hap)
    n_i = shape[0]
    stacked = np.concatenate([ci, cj])
    got = ops.ld_rect(pi, pj).cpu().numpy()
    assert got.shape == shape and got.dtype == np.float32
    ex = lx.Exact(stacked)
    check_block(got, ex, n_i, f"haplotype r {shape} x {n_hap}")   # (tests/test_ld_rect_host.py pins that |r| = 1 cells exist)
    gd = ops.ld_rect(pi, pj, dosage=True).cpu().numpy()   # (every n_hap of the list is even)
    check_block(gd, dx.DosageExact(stacked), n_i, f"dosage r {shape} x {n_hap}")


# ---- 3. symmetry and self --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dosage", [False, True])
def test_rect_is_symmetric_and_self_is_the_square(gpu, dosage):
    from ld_tools_amd import ops
    _, _, A, B = pair((129, 257), 256)
    ab, ba = ops.ld_rect(A, B, dosage=dosage), ops.ld_rect(B, A, dosage=dosage)
    assert np.array_equal(bits(ab), bits(ba).T)
    for P in (A, B):
        sq = ops.ld_rect(P, dosage=dosage)
        assert sq.shape == (P.n_snps, P.n_snps)
        assert np.array_equal(bits(sq), bits(ops.ld_rect(P, P, dosage=dosage)))
        assert np.array_equal(bits(sq), bits(sq).T)


# ---- 4. nothing else is written ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n_hap", [((300, 130), 258), ((5, 700), 254), ((1, 1), 2)])
def test_rect_writes_its_cells_and_nothing_else(gpu, shape, n_hap):
    import torch
    from ld_tools_amd import ops
    _, _, pi, pj = pair(shape, n_hap)
    n_i, n_j = shape
    fill = 0x7FC12345   # a quiet NaN with a payload no kernel produces
    buf = torch.full((n_i + 3, n_j + 5), fill, dtype=torch.int32, device=gpu).view(torch.float32)
    ret = ops.ld_rect(pi, pj, out=buf[:n_i])
    assert ret.data_ptr() == buf.data_ptr() and ret.shape == (n_i, n_j) and ret.stride(0) == n_j + 5
    b = bits(buf)
    assert (b[:, n_j:] == fill).all() and (b[n_i:] == fill).all()
    assert np.array_equal(b[:n_i, :n_j], bits(ops.ld_rect(pi, pj)))
    assert not np.isnan(buf[:n_i, :n_j].cpu().numpy()).any()


# ---- 4b. the walk: full bands of 16 I blocks, band indices above 0, a short last band ----------------------------------------
_WALK = {}


def walk_pair(shape, n_hap):
    """(codes_i, codes_j, panel_i, panel_j) of one walk case, built once and left unchanged."""
    from ld_tools_amd import PackedPanel
    key = (shape, n_hap)
    if key not in _WALK:
        ci, cj = rc.walk_codes(shape, n_hap)
        _WALK[key] = (ci, cj, PackedPanel.from_codes(ci), PackedPanel.from_codes(cj))
    return _WALK[key]


def walk_cells(gpu, shape, n_hap, dosage):
    """ops.ld_rect of a walk case into the inside of a padded buffer full of a NaN payload: every cell of [n_i, n_j]
    written, every word outside it intact.  Returns the cells on the host."""
    import torch
    from ld_tools_amd import ops
    _, _, pi, pj = walk_pair(shape, n_hap)
    n_i, n_j = shape
    fill = 0x7FC12345   # a quiet NaN with a payload no kernel produces
    buf = torch.full((n_i + 3, n_j + 5), fill, dtype=torch.int32, device=gpu).view(torch.float32)
    ret = ops.ld_rect(pi, pj, dosage=dosage, out=buf[:n_i])
    assert ret.data_ptr() == buf.data_ptr() and ret.shape == (n_i, n_j) and ret.stride(0) == n_j + 5
    b = bits(buf)
    assert (b[:, n_j:] == fill).all() and (b[n_i:] == fill).all(), f"{shape}: a word outside the rectangle was written"
    left = np.argwhere(b[:n_i, :n_j] == fill)
    assert left.size == 0, f"{shape}: {len(left)} cells never written, the first at {left[0].tolist()}"
    return np.ascontiguousarray(b[:n_i, :n_j]).view(np.float32)


@pytest.mark.parametrize("shape,n_hap", rc.WALK_CASES, ids=[f"{s[0]}x{s[1]}x{h}" for s, h in rc.WALK_CASES])
def test_rect_walk_past_one_band_against_the_exact_oracle(gpu, shape, n_hap):
    """tile_of beyond its first band (tests/test_ld_rect_host.py pins what the table covers): a mis-numbered workgroup
    leaves a tile unwritten, writes one twice with another tile's rows, or pairs the wrong rows -- the fill word, the
    surroundings and the exact oracle of the two sides see each."""
    ci, cj, _, _ = walk_pair(shape, n_hap)
    got = walk_cells(gpu, shape, n_hap, False)
    check_block(got, lx.ExactBlock(ci, cj), shape[0], f"walk, haplotype r {shape} x {n_hap}")
    gd = walk_cells(gpu, shape, n_hap, True)
    check_block(gd, dx.DosageExactBlock(ci, cj), shape[0], f"walk, dosage r {shape} x {n_hap}")


@pytest.mark.parametrize("dosage", [False, True])
def test_rect_walk_swapped_sides_are_bit_transposes(gpu, dosage):
    """(130, 4353) is (4353, 257) with the sides swapped and the short side cut to 130 rows (rc.walk_codes): the long side
    walks 18 I blocks in two bands in one call and 35 J slabs under one band in the other -- the same cells, transposed."""
    (long_shape, h), (short_shape, h2) = rc.WALK_HITS_CASE, rc.WALK_SWAPPED
    assert h == h2
    a = walk_cells(gpu, long_shape, h, dosage)
    b = walk_cells(gpu, short_shape, h2, dosage)
    assert np.array_equal(a[:, :short_shape[0]].view(np.uint32), b.view(np.uint32).T)


def test_rect_walk_hits_are_the_host_mirror_of_the_dense_cells(gpu):
    """The hit lists over two bands of I blocks, and again from a buffer of one batch (the overflow re-run)."""
    from ld_tools_amd import ops
    shape, n_hap = rc.WALK_HITS_CASE
    _, _, pi, pj = walk_pair(shape, n_hap)
    r_host = walk_cells(gpu, shape, n_hap, False)
    m = assert_hits(ops.ld_rect_hits(pi, pj, r2=0.2), r_host, ops.r2_bound(0.2), "walk, r2 >= 0.2")
    i = expect_hits(r_host, ops.r2_bound(0.2))[0]
    assert (i >= 4096).any() and (i < 4096).any()          # hits in both bands
    waves = len(set((i // 64).tolist()))
    assert waves >= 2                                      # two waves with a hit reserve two batches of 256: more than the buffer
    small = ops.ld_rect_hits(pi, pj, r2=0.2, hit_capacity=256)
    assert assert_hits(small, r_host, ops.r2_bound(0.2), "walk, r2 >= 0.2 from a 256-slot buffer") == m
    hd = ops.ld_rect_hits(pi, pj, r2=0.2, dosage=True, hit_capacity=256)
    assert_hits(hd, walk_cells(gpu, shape, n_hap, True), ops.r2_bound(0.2), "walk, dosage, r2 >= 0.2")


# ---- 5. hits -----------------------------------------------------------------------------------------------------------------
def expect_hits(r_host, bound):
    from ld_tools_amd import ops
    i, j = ops.rect_hits_host(r_host, bound)
    offsets = np.zeros(r_host.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(i, minlength=r_host.shape[0]), out=offsets[1:])
    return i, j, r_host[i, j], offsets


def assert_hits(h, r_host, bound, what):
    i, j, r, offsets = expect_hits(r_host, bound)
    print(f"{what}: {i.size} expected hits of {r_host.size} cells")
    assert 0 < i.size <= r_host.size // 2, f"{what}: the expected set must be neither empty nor more than half the cells"
    gi, gj, gr = h.pairs()
    assert np.array_equal(gi, i) and np.array_equal(gj, j), what
    assert np.array_equal(gr.view(np.uint32), np.ascontiguousarray(r).view(np.uint32)), what
    assert np.array_equal(h.offsets.cpu().numpy().astype(np.int64), offsets), what
    assert np.array_equal(h.j.cpu().numpy().astype(np.int64), j) and np.array_equal(bits(h.r), gr.view(np.uint32))
    s = h.hits[:, 3].view(__import__("torch").float32).cpu().numpy()
    assert np.array_equal(s.view(np.uint32), np.multiply(r, r, dtype=np.float32).view(np.uint32))
    assert len(h) == i.size and np.float32(h.bound) == np.float32(bound)
    return i.size


def test_rect_hits_are_the_host_mirror_of_the_dense_cells(gpu):
    from ld_tools_amd import ops
    shape, n_hap = rc.HITS_CASE
    _, _, pi, pj = pair(shape, n_hap, family=rc.FAMILY)
    r_host = ops.ld_rect(pi, pj).cpu().numpy()
    m02 = assert_hits(ops.ld_rect_hits(pi, pj, r2=0.2), r_host, ops.r2_bound(0.2), "r2 >= 0.2")
    assert_hits(ops.ld_rect_hits(pi, pj, r2=1.0), r_host, ops.r2_bound(1.0), "r2 >= 1.0")
    # strict, at a value some cell's float32 square equals exactly: that cell is out, the next larger square is in
    sq = np.multiply(r_host, r_host, dtype=np.float32)
    inner = np.sort(sq[(sq > np.float32(0.3)) & (sq < np.float32(0.9))])
    assert inner.size
    t = float(inner[inner.size // 2])
    b_strict, b_loose = ops.r2_bound(t, strict=True), ops.r2_bound(t)
    assert float(b_loose) == t and float(b_strict) > t
    m_strict = assert_hits(ops.ld_rect_hits(pi, pj, r2=t, strict=True), r_host, b_strict, "r2 > t")
    m_loose = assert_hits(ops.ld_rect_hits(pi, pj, r2=t), r_host, b_loose, "r2 >= t")
    assert m_loose - m_strict == int((sq == np.float32(t)).sum()) >= 1
    # a buffer of one batch: the first run reserves more than it holds, the re-run gives the same CSR
    assert m02 > 256
    small = ops.ld_rect_hits(pi, pj, r2=0.2, hit_capacity=256)
    assert_hits(small, r_host, ops.r2_bound(0.2), "r2 >= 0.2 from a 256-slot buffer")
    # a panel against itself: every non-degenerate SNP pairs with itself at r^2 = 1 (the diagonal of the square)
    self_hits = ops.ld_rect_hits(pj, r2=0.2)
    assert_hits(self_hits, ops.ld_rect(pj).cpu().numpy(), ops.r2_bound(0.2), "self, r2 >= 0.2")


def test_rect_hits_dosage(gpu):
    from ld_tools_amd import ops
    shape, n_hap = rc.HITS_CASE
    _, _, pi, pj = pair(shape, n_hap, family=rc.FAMILY)
    r_host = ops.ld_rect(pi, pj, dosage=True).cpu().numpy()
    h = ops.ld_rect_hits(pi, pj, r2=0.2, dosage=True)
    assert h.dosage
    assert_hits(h, r_host, ops.r2_bound(0.2), "dosage, r2 >= 0.2")


# ---- 6. driver ---------------------------------------------------------------------------------------------------------------
def two_chromosomes():
    a, names = fakevcf.make_chromosome(chrom="6", n_variants=48, seed=11)
    b, names_b = fakevcf.make_chromosome(chrom="7", n_variants=37, seed=23, first_pos=5000, step=211)
    assert names == names_b
    return fakevcf.FakeVcf(a.records + b.records), names


def rs_rows(vcf, chrom):
    seen, rows = set(), []
    for rec in vcf.records:
        if rec.chrom == chrom and rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
            seen.add(rec.id)
            rows.append([rec.pos, rec.id])
    return rows


@pytest.mark.parametrize("dosage", [False, True])
def test_rect_driver(gpu, tmp_path, dosage):
    from ld_tools_amd import PackedPanel, ops
    from ld_tools_amd.drivers import codes_matrix, find_record, rect_matrix, sample_genotypes, write_rect_matrix
    from ld_tools_amd.drivers.rmatrix import VARIANTS_HEADER
    vcf, names = two_chromosomes()
    rows_i, rows_j = rs_rows(vcf, "6")[::-1], rs_rows(vcf, "7")   # (the driver sorts each side by position)
    m = rect_matrix(vcf, "6", rows_i, "7", rows_j, names, dosage=dosage)
    assert (m.rows.n, m.cols.n) == (len(rows_i), len(rows_j)) and m.rows.chrom == "6" and m.cols.chrom == "7"
    sides = []
    for chrom, rows in (("6", rows_i), ("7", rows_j)):   # the same codes, assembled here record by record
        srt = sorted(rows, key=lambda r: r[0])
        sides.append(codes_matrix([sample_genotypes(find_record(vcf, chrom, p, rs), names) for p, rs in srt]))
    assert np.array_equal(sides[0], m.rows.codes) and np.array_equal(sides[1], m.cols.codes)
    want = ops.ld_rect(PackedPanel.from_codes(sides[0]), PackedPanel.from_codes(sides[1]), dosage=dosage)
    assert np.array_equal(bits(m.r), bits(want))
    base = str(tmp_path / "chr6_chr7_r")
    paths = write_rect_matrix(base, m, rows_per_block=7)
    assert paths == [base + ".npy", base + ".rows.tsv", base + ".cols.tsv"]
    got = np.load(base + ".npy", mmap_mode="r")
    assert got.shape == (m.rows.n, m.cols.n) and got.dtype == np.float32
    assert np.array_equal(np.asarray(got).view(np.uint32), bits(m.r))
    for path, side in ((paths[1], m.rows), (paths[2], m.cols)):
        lines = Path(path).read_text().splitlines(keepends=True)
        assert lines[0] == VARIANTS_HEADER and len(lines) == side.n + 1
        fields = [ln.rstrip("\n").split("\t") for ln in lines[1:]]
        assert [f[1] for f in fields] == side.rs_ids and [int(f[2]) for f in fields] == side.poss
        assert [float(f[5]) for f in fields] == side.alt_freqs and len(side.alt_freqs) == side.n
    # two rsID lists of ONE chromosome: the rectangle is a block of that chromosome's square
    half = len(rows_i) // 2
    m2 = rect_matrix(vcf, "6", rows_i[:half], "6", rows_i[half:], names, dosage=dosage)
    sq = ops.ld_rect(PackedPanel.from_codes(sides[0]), dosage=dosage)
    order = sorted(range(len(rows_i)), key=lambda k: rows_i[k][0])        # index of each row in position order
    rank = {k: p for p, k in enumerate(order)}
    ri = sorted(rank[k] for k in range(half))
    rj = sorted(rank[k] for k in range(half, len(rows_i)))
    assert np.array_equal(bits(m2.r), bits(sq)[ri][:, rj])

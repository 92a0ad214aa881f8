"""GPU: pairwise-complete rectangular LD (ops.ld_rect(missing="pairwise"), ops.ld_rect_hits(missing="pairwise"),
ops.ld_rect_counts, drivers/rect.py; include/ldx.h, "pairwise-complete LD") against the exact integer oracle
(tests/ld_pairwise_exact.py), bit for bit against plain ld_rect where no call is missing, and its invariances.

Contract: the pair's integers are exact; the cell is within 4 float32 ulps of the exact r of those integers, -0.0f exactly on a
degenerate pair (n = 0 / N = 0 included), +0.0f exactly where num = 0; a function of the integers alone, symmetric in the two
SNPs; a pair of rows without a missing code gives the ld_rect cell bit for bit.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import fakevcf  # noqa: E402
import ld_exact as lx  # noqa: E402
import ld_pairwise_exact as px  # noqa: E402
import ld_rect_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

NEG0, POS0 = np.uint32(0x80000000), np.uint32(0)
ULPS = 4.0   # include/ldx.h: the bound of every r32 cell
FORMS = [False, True]
PW = "pairwise"


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


_PACKED, _ORACLE = {}, {}


def packed(key, ci, cj):
    """The two PackedPanels of a case, built once."""
    from ld_tools_amd import PackedPanel
    if key not in _PACKED:
        _PACKED[key] = (PackedPanel.from_codes(np.array(ci)), PackedPanel.from_codes(np.array(cj)))   # (copies: the codes are read-only)
    return _PACKED[key]


def oracle(key, ci, cj, dosage):
    if (key, dosage) not in _ORACLE:
        _ORACLE[(key, dosage)] = px.PairwiseExactBlock(ci, cj, dosage)
    return _ORACLE[(key, dosage)]


def check_cells(got32, ex, what):
    """Cells against the oracle: signed zeros exactly, |r| = 1 exactly, 4 ulps elsewhere."""
    b = np.ascontiguousarray(got32).view(np.uint32)
    assert ex.degenerate.shape == b.shape
    assert np.array_equal(b == NEG0, ex.degenerate), f"{what}: -0.0f <=> degenerate"
    assert np.array_equal(b == POS0, ex.zero_num), f"{what}: +0.0f <=> num == 0"
    rest = ~ex.degenerate & ~ex.zero_num
    if rest.any():
        err = lx.ulp32_err(got32[rest], ex.r64[rest])
        print(f"{what}: {int(rest.sum())} cells, max error {float(err.max()):.3f} float32 ulps")
        assert float(err.max()) <= ULPS, f"{what}: {float(err.max())} ulps"


def check_counts(got, ex, what):
    got = got.cpu().numpy()
    assert got.dtype == np.uint32 and got.shape == ex.counts.shape, what
    for s, name in enumerate(ex.names):
        bad = np.argwhere(got[s].astype(np.int64) != ex.counts[s])
        assert bad.size == 0, f"{what}: count {name} differs at {bad[0].tolist()}: {got[s][tuple(bad[0])]} != {ex.counts[s][tuple(bad[0])]}"


def check_case(key, ci, cj, what):
    """Counts, cells and the complete x complete cells of one pair of code matrices, both forms where n_hap is even."""
    from ld_tools_amd import ops
    pi, pj = packed(key, ci, cj)
    both = np.logical_and.outer(px.complete_rows(ci), px.complete_rows(cj))
    for dosage in FORMS:
        ex = oracle(key, ci, cj, dosage)
        w = f"{what}, dosage={dosage}"
        check_counts(ops.ld_rect_counts(pi, pj, dosage=dosage), ex, w)
        got = ops.ld_rect(pi, pj, dosage=dosage, missing=PW)
        assert got.shape == (ci.shape[0], cj.shape[0])
        check_cells(got.cpu().numpy(), ex, w)
        plain = ops.ld_rect(pi, pj, dosage=dosage)
        assert np.array_equal(bits(got)[both], bits(plain)[both]), f"{w}: complete x complete cells are ld_rect's"
    return both


# ---- 1. counts and cells against the oracle, across the kernel's edges ---------------------------------------------------
CASES = rc.EDGE_CASES + (px.BIG_CASE,)


@pytest.mark.parametrize("shape,n_hap", CASES, ids=[f"{s[0]}x{s[1]}x{h}" for s, h in CASES])
def test_pairwise_counts_and_cells_against_the_oracle(gpu, shape, n_hap):
    ci, cj, _ = px.mixed_pair(shape, n_hap)
    key = ("mixed", shape, n_hap)
    both = check_case(key, ci, cj, f"mixed {shape} x {n_hap}")
    if min(shape) >= 5 and n_hap >= 8:
        assert both.any() and (~both).any()
    if (shape, n_hap) == px.BIG_CASE:   # all-ALT complete rows on both sides: the largest counts
        assert int(oracle(key, ci, cj, False).c.max()) == n_hap and int(oracle(key, ci, cj, True).S.max()) == 2 * n_hap


# ---- 2. no holes: the whole matrix is ld_rect's ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n_hap", [((300, 130), 1008), ((129, 257), 254)])
def test_pairwise_without_holes_is_ld_rect_bit_for_bit(gpu, shape, n_hap):
    from ld_tools_amd import ops
    ci, cj = px.complete_pair(shape, n_hap)
    assert px.complete_rows(ci).all() and px.complete_rows(cj).all()
    pi, pj = packed(("complete", shape, n_hap), ci, cj)
    for dosage in FORMS:
        got, plain = ops.ld_rect(pi, pj, dosage=dosage, missing=PW), ops.ld_rect(pi, pj, dosage=dosage)
        assert np.array_equal(bits(got), bits(plain)), f"dosage={dosage}"
        check_counts(ops.ld_rect_counts(pi, pj, dosage=dosage), oracle(("complete", shape, n_hap), ci, cj, dosage),
                     f"complete {shape} x {n_hap}, dosage={dosage}")


# ---- 3. four tile kinds in one launch ---------------------------------------------------------------------------------------
def test_pairwise_tiles_with_and_without_holes_in_one_launch(gpu):
    ci, cj = px.tiles_pair()
    holes_i, holes_j = ~px.complete_rows(ci), ~px.complete_rows(cj)
    assert holes_i[128:256].any() and not holes_i[:128].any() and not holes_i[256:].any()
    assert holes_j[128:256].any() and not holes_j[:128].any() and not holes_j[256:].any()
    both = check_case(("tiles",), ci, cj, "tiles")
    assert both[128:256, 128:256].any()   # complete x complete pairs inside a hole-bearing tile


# ---- 4. a function of the integers alone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dosage", FORMS)
def test_pairwise_swapped_sides_give_the_transpose(gpu, dosage):
    from ld_tools_amd import ops
    shape, n_hap = (129, 257), 256
    ci, cj, _ = px.mixed_pair(shape, n_hap)
    A, B = packed(("mixed", shape, n_hap), ci, cj)
    ab, ba = ops.ld_rect(A, B, dosage=dosage, missing=PW), ops.ld_rect(B, A, dosage=dosage, missing=PW)
    assert np.array_equal(bits(ab), bits(ba).T)
    sq = ops.ld_rect(B, dosage=dosage, missing=PW)
    assert np.array_equal(bits(sq), bits(sq).T)


@pytest.mark.parametrize("dosage", FORMS)
def test_pairwise_permuted_individuals_give_identical_bits(gpu, dosage):
    from ld_tools_amd import ops
    shape, n_hap = (300, 130), 258
    ci, cj, _ = px.mixed_pair(shape, n_hap)
    A, B = packed(("mixed", shape, n_hap), ci, cj)
    pa, pb = packed(("permuted", shape, n_hap), px.permute_individuals(ci, 5), px.permute_individuals(cj, 5))
    assert np.array_equal(bits(ops.ld_rect(A, B, dosage=dosage, missing=PW)), bits(ops.ld_rect(pa, pb, dosage=dosage, missing=PW)))


def test_pairwise_dosage_rephased_genotypes_give_identical_bits(gpu):
    from ld_tools_amd import ops
    shape, n_hap = (300, 130), 258
    ci, cj, _ = px.mixed_pair(shape, n_hap)
    A, B = packed(("mixed", shape, n_hap), ci, cj)
    ri, rj = px.rephase(ci, 8), px.rephase(cj, 9)
    assert not np.array_equal(ri, ci)
    ra, rb = packed(("rephased", shape, n_hap), ri, rj)
    assert np.array_equal(bits(ops.ld_rect(A, B, dosage=True, missing=PW)), bits(ops.ld_rect(ra, rb, dosage=True, missing=PW)))
    assert np.array_equal(ops.ld_rect_counts(A, B, dosage=True).cpu().numpy(), ops.ld_rect_counts(ra, rb, dosage=True).cpu().numpy())


# ---- 5. hits ------------------------------------------------------------------------------------------------------------------
def assert_hits(h, r_host, bound, what):
    from ld_tools_amd import ops
    i, j = ops.rect_hits_host(r_host, bound)
    r = r_host[i, j]
    offsets = np.zeros(r_host.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(i, minlength=r_host.shape[0]), out=offsets[1:])
    print(f"{what}: {i.size} expected hits of {r_host.size} cells")
    assert 0 < i.size <= r_host.size // 2, f"{what}: the expected set must be neither empty nor more than half the cells"
    gi, gj, gr = h.pairs()
    assert np.array_equal(gi, i) and np.array_equal(gj, j), what
    assert np.array_equal(gr.view(np.uint32), np.ascontiguousarray(r).view(np.uint32)), what
    assert np.array_equal(h.offsets.cpu().numpy().astype(np.int64), offsets), what
    s = h.hits[:, 3].view(__import__("torch").float32).cpu().numpy()
    assert np.array_equal(s.view(np.uint32), np.multiply(r, r, dtype=np.float32).view(np.uint32))
    assert len(h) == i.size and np.float32(h.bound) == np.float32(bound)
    return i, j


@pytest.mark.parametrize("dosage", FORMS)
def test_pairwise_hits_are_the_host_mirror_and_agree_with_the_oracle(gpu, dosage):
    from ld_tools_amd import ops
    shape, n_hap = rc.HITS_CASE
    ci, cj, _ = px.mixed_pair(shape, n_hap, family=rc.FAMILY)
    key = ("mixed", shape, n_hap, rc.FAMILY)
    pi, pj = packed(key, ci, cj)
    r_host = ops.ld_rect(pi, pj, dosage=dosage, missing=PW).cpu().numpy()
    bound = ops.r2_bound(px.HITS_R2)
    h = ops.ld_rect_hits(pi, pj, r2=px.HITS_R2, dosage=dosage, missing=PW)
    assert h.missing == PW and h.dosage == dosage
    i, j = assert_hits(h, r_host, bound, f"pairwise hits, dosage={dosage}")
    kept = np.zeros(shape, dtype=bool)
    kept[i, j] = True
    cls = oracle(key, ci, cj, dosage).classes(px.HITS_R2)
    assert kept[cls == px.IN].all() and not kept[cls == px.OUT].any()
    assert int((cls == px.IN).sum()) >= px.MIN_DECIDED_IN
    assert i.size > 256   # a buffer of one batch: the first run reserves more than it holds, the re-run gives the same CSR
    small = ops.ld_rect_hits(pi, pj, r2=px.HITS_R2, dosage=dosage, missing=PW, hit_capacity=256)
    assert_hits(small, r_host, bound, f"pairwise hits from a 256-slot buffer, dosage={dosage}")


# ---- 6. the walk, and nothing else is written ---------------------------------------------------------------------------------
def test_pairwise_walk_past_one_band_against_the_oracle(gpu):
    import torch
    from ld_tools_amd import ops
    shape, n_hap = px.WALK_CASE
    n_i, n_j = shape
    ci, cj, _ = px.mixed_pair(shape, n_hap)
    key = ("mixed", shape, n_hap)
    pi, pj = packed(key, ci, cj)
    fill = 0x7FC12345   # a quiet NaN with a payload no kernel produces
    for dosage in FORMS:
        buf = torch.full((n_i + 3, n_j + 5), fill, dtype=torch.int32, device=gpu).view(torch.float32)
        ret = ops.ld_rect(pi, pj, dosage=dosage, out=buf[:n_i], missing=PW)
        assert ret.data_ptr() == buf.data_ptr() and ret.shape == (n_i, n_j) and ret.stride(0) == n_j + 5
        b = bits(buf)
        assert (b[:, n_j:] == fill).all() and (b[n_i:] == fill).all(), "a word outside the rectangle was written"
        left = np.argwhere(b[:n_i, :n_j] == fill)
        assert left.size == 0, f"{len(left)} cells never written, the first at {left[0].tolist()}"
        check_cells(np.ascontiguousarray(b[:n_i, :n_j]).view(np.float32), oracle(key, ci, cj, dosage), f"walk, dosage={dosage}")


@pytest.mark.parametrize("dosage", FORMS)
def test_pairwise_out_with_a_wider_row_stride(gpu, dosage):
    import torch
    from ld_tools_amd import ops
    shape, n_hap = (300, 130), 258
    n_i, n_j = shape
    ci, cj, _ = px.mixed_pair(shape, n_hap)
    pi, pj = packed(("mixed", shape, n_hap), ci, cj)
    fill = 0x7FC12345
    buf = torch.full((n_i + 3, n_j + 5), fill, dtype=torch.int32, device=gpu).view(torch.float32)
    ret = ops.ld_rect(pi, pj, dosage=dosage, out=buf[:n_i], missing=PW)
    assert ret.data_ptr() == buf.data_ptr() and ret.shape == (n_i, n_j) and ret.stride(0) == n_j + 5
    b = bits(buf)
    assert (b[:, n_j:] == fill).all() and (b[n_i:] == fill).all()
    assert np.array_equal(b[:n_i, :n_j], bits(ops.ld_rect(pi, pj, dosage=dosage, missing=PW)))


# ---- 7. driver ---------------------------------------------------------------------------------------------------------------
def rs_rows(vcf, chrom):
    seen, rows = set(), []
    for rec in vcf.records:
        if rec.chrom == chrom and rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
            seen.add(rec.id)
            rows.append([rec.pos, rec.id])
    return rows


def vcf_with_missing_calls():
    """Two chromosomes whose records carry ./. and .|1 calls beside the multi-allelic record's second-ALT codes."""
    a, names = fakevcf.make_chromosome(chrom="6", n_variants=48, seed=11)
    b, _ = fakevcf.make_chromosome(chrom="7", n_variants=37, seed=23, first_pos=5000, step=211)
    vcf = fakevcf.FakeVcf(a.records + b.records)
    carried = [n for n in names if n in vcf.records[0].samples]
    for k, rec in enumerate(vcf.records):
        if k % 3 == 1:
            rec.samples[carried[k % len(carried)]] = {"GT": (None, None)}
            rec.samples[carried[(k + 5) % len(carried)]] = {"GT": (None, 1)}
    return vcf, names


@pytest.mark.parametrize("dosage", FORMS)
def test_pairwise_driver(gpu, dosage):
    from ld_tools_amd import PackedPanel, ops
    from ld_tools_amd.drivers import rect_matrix
    vcf, names = vcf_with_missing_calls()
    rows_i, rows_j = rs_rows(vcf, "6"), rs_rows(vcf, "7")
    m = rect_matrix(vcf, "6", rows_i, "7", rows_j, names, dosage=dosage, missing=PW)
    assert m.missing == PW and m.dosage == dosage
    ci, cj = m.rows.codes, m.cols.codes
    assert (ci == 2).any() and not px.complete_rows(ci).all() and not px.complete_rows(cj).all()
    half = (np.isin(ci[:, 0::2], (0, 1)) != np.isin(ci[:, 1::2], (0, 1))).any()
    assert half, "a half-missing genotype reached the codes"
    pi, pj = PackedPanel.from_codes(ci), PackedPanel.from_codes(cj)
    assert np.array_equal(bits(m.r), bits(ops.ld_rect(pi, pj, dosage=dosage, missing=PW)))
    check_cells(m.r.cpu().numpy(), px.PairwiseExactBlock(ci, cj, dosage), f"driver, dosage={dosage}")
    plain = rect_matrix(vcf, "6", rows_i, "7", rows_j, names, dosage=dosage)
    assert plain.missing is None
    assert np.array_equal(bits(plain.r), bits(ops.ld_rect(pi, pj, dosage=dosage)))
    assert not np.array_equal(bits(plain.r), bits(m.r))

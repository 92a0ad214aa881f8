"""PLINK .bed rows <-> packed panels on the device (include/ldx.h, ldx_bed_unpack_dev / ldx_bed_pack_dev; PackedPanel.from_bed /
to_bed) against the host converters of ld_tools_amd/plink.py: byte for byte, in both directions.

The sources are random bytes, so all four 2-bit fields occur and the pad fields of a row's last byte are non-zero.  Shapes:
n_ind around the 4-per-byte, 16-per-word and 64-per-chunk strides and at LDX_MAX_HAPS / 2; n_snps around the 32-row workgroup
and the 128-row slab."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIELDS = ("alt", "ref", "acnt", "rcnt", "fa", "fr", "q")
N_INDS = (1, 3, 4, 63, 64, 65, 131, 1000, 5120)
N_SNPS = (1, 127, 129, 300)
MAGIC = bytes((0x6C, 0x1B, 0x01))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


def random_rows(n_snps, n_ind, seed=0, width=None):
    from ld_tools_amd import plink

    rng = np.random.default_rng(1000003 * n_snps + 7 * n_ind + seed)
    rows = rng.integers(0, 256, size=(n_snps, width or plink.row_bytes(n_ind)), dtype=np.uint8)
    if n_ind % 4:
        rows[::2, (n_ind - 1) // 4] |= (0xFF << (2 * (n_ind % 4))) & 0xFF        # pad fields set, whatever the draw
    return rows


def assert_same(p, q, what=""):
    assert (p.n_snps, p.n_hap) == (q.n_snps, q.n_hap), what
    for f in FIELDS:
        assert torch.equal(getattr(p, f), getattr(q, f)), f"{what}: {f} differs"


def at_phase(rows, off, gpu):
    """The rows on the device with the first byte ``off`` bytes past an aligned address; off = 3 is a whole file with its
    header.  A few bytes follow the last row, as in no file."""
    n, w = rows.shape
    flat = torch.full((off + n * w + 5,), 0xA5, dtype=torch.uint8, device=gpu)
    if off == 3:
        flat[:3] = torch.tensor(list(MAGIC), dtype=torch.uint8)
    flat[off:off + n * w] = torch.from_numpy(rows.reshape(-1)).to(gpu)
    view = flat[off:off + n * w].view(n, w)
    assert view.data_ptr() % 4 == off % 4
    return view


_EXPECT = {}


def expected(n_snps, n_ind, alt, gpu):
    """(rows, the panel from_codes makes of the host decoding), made once per shape."""
    key = (n_snps, n_ind, alt)
    if key not in _EXPECT:
        from ld_tools_amd import PackedPanel, plink

        rows = random_rows(n_snps, n_ind)
        _EXPECT[key] = (rows, PackedPanel.from_codes(plink.bed_codes_host(rows, n_ind, alt=alt), gpu))
    return _EXPECT[key]


@pytest.mark.parametrize("n_snps", N_SNPS)
@pytest.mark.parametrize("n_ind", N_INDS)
def test_identity_unpack_equals_from_codes(gpu, n_ind, n_snps):
    from ld_tools_amd import PackedPanel, plink

    for alt in ("a1", "a2"):
        rows, want = expected(n_snps, n_ind, alt, gpu)
        if n_snps * n_ind >= 100:
            assert set(np.unique(plink.bed_fields_host(rows, n_ind)).tolist()) == {0, 1, 2, 3}
        for off in range(4):
            got = PackedPanel.from_bed((at_phase(rows, off, gpu), n_ind), alt=alt)
            assert_same(got, want, f"{n_snps} x {n_ind} alt={alt} phase {off}")
    assert_same(PackedPanel.from_bed((rows, n_ind), alt="a2", device=gpu), want, "host source")


def test_row_stride_wider_than_the_row(gpu):
    from ld_tools_amd import PackedPanel

    n_snps, n_ind = 150, 131                                             # 33 bytes a row, 41 apart: every phase occurs
    _, want = expected(n_snps, n_ind, "a1", gpu)
    wide = random_rows(n_snps, n_ind, seed=9, width=41)
    wide[:, :33] = random_rows(n_snps, n_ind)
    for off in (0, 3):
        assert_same(PackedPanel.from_bed((at_phase(wide, off, gpu), n_ind)), want, f"row_bytes 41, phase {off}")
    assert_same(PackedPanel.from_bed((wide, n_ind), device=gpu, chunk_snps=128), want, "host source, row_bytes 41")
    sliced = at_phase(wide, 1, gpu)[:, :33]                              # a view: 33 bytes of every 41
    assert sliced.stride(0) == 41
    assert_same(PackedPanel.from_bed((sliced, n_ind)), want, "sliced view")


# a source on each side of the LDS / global switch of the gather (7648 individuals), both wider than any panel may be
@pytest.mark.parametrize("n_src", [6000, 9000])
def test_individual_gather(gpu, n_src):
    from ld_tools_amd import LdxError, PackedPanel, _lib, plink

    n_snps = 130
    rows = random_rows(n_snps, n_src)
    dev_rows = at_phase(rows, 3, gpu)
    rng = np.random.default_rng(n_src)
    subset = np.sort(rng.choice(n_src, size=100, replace=False))
    mask = np.zeros(n_src, dtype=bool)
    mask[rng.choice(n_src, size=333, replace=False)] = True
    keeps = {"permuted": rng.permutation(n_src)[:1000], "repeats": rng.integers(0, n_src, size=777),
             "100 of them": subset, "mask": mask, "one": np.array([n_src - 1]), "5120": rng.permutation(n_src)[:5120]}
    for name, keep in keeps.items():
        for alt in ("a1", "a2") if name in ("permuted", "100 of them") else ("a1",):
            want = PackedPanel.from_codes(plink.bed_codes_host(rows, n_src, keep=keep, alt=alt), gpu)
            assert_same(PackedPanel.from_bed((dev_rows, n_src), keep=keep, alt=alt), want, f"{n_src}: keep {name}, alt={alt}")
    assert_same(PackedPanel.from_bed((rows, n_src), keep=subset, device=gpu, chunk_snps=128),
                PackedPanel.from_codes(plink.bed_codes_host(rows, n_src, keep=subset), gpu), "host source with keep")
    # the whole source is more than a panel holds; an index past the source is refused by the Python layer ...
    with pytest.raises(LdxError):
        PackedPanel.from_bed((dev_rows, n_src))
    for bad in (np.array([0, n_src]), np.array([-1, 2]), np.zeros(n_src - 1, dtype=bool)):
        with pytest.raises(LdxError):
            PackedPanel.from_bed((dev_rows, n_src), keep=bad)
    # ... and at the C entry it is a MISSING CALL at that individual (include/ldx.h), never a stray read
    idx = np.array([5, n_src, 17, 0xFFFFFFFF, n_src - 1], dtype=np.uint32)
    out = PackedPanel.empty(n_snps, 2 * idx.size, gpu)
    d_idx = torch.from_numpy(idx.view(np.int32)).to(gpu)
    rc = _lib.lib.ldx_bed_unpack_dev(dev_rows.data_ptr(), dev_rows.stride(0), n_src, n_snps, d_idx.data_ptr(), idx.size, 0, 0,
                                     n_snps, out.alt.data_ptr(), out.ref.data_ptr(), out.acnt.data_ptr(), out.rcnt.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    out.refresh_stats()
    codes = plink.bed_codes_host(rows, n_src, keep=np.array([5, 0, 17, 0, n_src - 1]))
    codes[:, 2:4] = 2
    codes[:, 6:8] = 2
    assert_same(out, PackedPanel.from_codes(codes, gpu), "an index past the source")


def test_full_permutation_of_a_small_source(gpu):
    from ld_tools_amd import PackedPanel, plink

    for n_src, n_snps in ((131, 129), (64, 33), (5, 1)):
        rows = random_rows(n_snps, n_src, seed=2)
        keep = np.random.default_rng(n_src).permutation(n_src)
        for alt in ("a1", "a2"):
            assert_same(PackedPanel.from_bed((at_phase(rows, 2, gpu), n_src), keep=keep, alt=alt),
                        PackedPanel.from_codes(plink.bed_codes_host(rows, n_src, keep=keep, alt=alt), gpu), f"{n_src} permuted")


def poisoned(n_snps, n_hap, gpu):
    from ld_tools_amd import PackedPanel

    p = PackedPanel.empty(n_snps, n_hap, gpu)
    for f in FIELDS:
        getattr(p, f).view(torch.uint8).fill_(0xFF)
    return p


@pytest.mark.parametrize("n_snps", [300, 513])
def test_streaming_into_a_poisoned_panel(gpu, n_snps):
    from ld_tools_amd import LdxError, PackedPanel, _lib, plink

    n_ind = 131
    rows = random_rows(n_snps, n_ind)
    once = PackedPanel.from_bed((rows, n_ind), device=gpu)
    assert_same(once, PackedPanel.from_codes(plink.bed_codes_host(rows, n_ind), gpu), "one shot")
    keep = np.random.default_rng(3).integers(0, n_ind, size=70)
    once_kept = PackedPanel.from_bed((rows, n_ind), keep=keep, device=gpu)
    for chunk in (128, 256):
        for source in (rows, at_phase(rows, 3, gpu)):
            out = poisoned(n_snps, 2 * n_ind, gpu)
            got = PackedPanel.from_bed((source, n_ind), chunk_snps=chunk, out=out)
            assert got is out
            assert_same(out, once, f"chunks of {chunk}")                 # whole tensors: pad rows and their counts included
            out = poisoned(n_snps, 140, gpu)
            assert_same(PackedPanel.from_bed((source, n_ind), keep=keep, chunk_snps=chunk, out=out), once_kept, "chunks, keep")
    assert int(once.acnt[n_snps:].abs().sum()) == 0 and int(once.rcnt[n_snps:].abs().sum()) == 0
    with pytest.raises(LdxError):
        PackedPanel.from_bed((rows, n_ind), out=poisoned(n_snps, 2 * n_ind + 2, gpu))
    # a call owns whole slabs: row0 must be a multiple of 128, n_rows too unless the call reaches the panel's end
    d = torch.from_numpy(rows).to(gpu)
    out = poisoned(n_snps, 2 * n_ind, gpu)

    def call(row0, n_rows):
        return _lib.lib.ldx_bed_unpack_dev(d[row0:].data_ptr(), d.stride(0), n_ind, n_rows, None, n_ind, 0, row0, n_snps,
                                           out.alt.data_ptr(), out.ref.data_ptr(), out.acnt.data_ptr(), out.rcnt.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)

    assert call(64, 64) == -1 and call(129, n_snps - 129) == -1 and call(0, 100) == -1 and call(256, n_snps - 255) == -1
    assert call(128, 128) == 0 and call(256, n_snps - 256) == 0 and call(0, 128) == 0      # any order
    out.refresh_stats()
    assert_same(out, once, "three calls by hand")


def random_codes(n_snps, n_ind, seed=0):
    """Codes over {0, 1, 2}, every pair of them: half-missing calls and hets in both orders included."""
    rng = np.random.default_rng(77 * n_snps + n_ind + seed)
    return rng.choice(np.array([0, 1, 2], dtype=np.int8), size=(n_snps, 2 * n_ind), p=[0.45, 0.4, 0.15])


@pytest.mark.parametrize("n_snps", N_SNPS)
@pytest.mark.parametrize("n_ind", N_INDS)
def test_pack_equals_codes_bed_host(gpu, n_ind, n_snps):
    from ld_tools_amd import PackedPanel, plink

    codes = random_codes(n_snps, n_ind)
    p = PackedPanel.from_codes(codes, gpu)
    for alt in ("a1", "a2"):
        want = plink.codes_bed_host(codes, alt=alt)
        got = p.to_bed(alt=alt)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), f"{n_snps} x {n_ind} alt={alt}"
    assert np.array_equal(p.to_bed(alt="a2", block_snps=100), want)       # moved in blocks
    back = PackedPanel.from_bed((p.to_bed(), n_ind), device=gpu)
    assert_same(back, PackedPanel.from_codes(plink.canonical_codes(codes), gpu), "from_bed(to_bed(p))")


def test_pack_row_range_stride_and_alignment(gpu):
    from ld_tools_amd import PackedPanel, _lib, plink

    n_snps, n_ind = 300, 131
    codes = random_codes(n_snps, n_ind, seed=4)
    p = PackedPanel.from_codes(codes, gpu)
    want = plink.codes_bed_host(codes)
    row0, n_rows, nb, ld = 129, 150, 33, 41
    for off in range(4):
        flat = torch.full((off + n_rows * ld,), 0xAB, dtype=torch.uint8, device=gpu)
        rc = _lib.lib.ldx_bed_pack_dev(p.alt.data_ptr(), p.ref.data_ptr(), n_snps, 2 * n_ind, row0, n_rows,
                                       flat[off:].data_ptr(), ld, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        host = flat.cpu().numpy()
        assert (host[:off] == 0xAB).all()
        got = host[off:].reshape(n_rows, ld)
        assert np.array_equal(got[:, :nb], want[row0:row0 + n_rows]), f"phase {off}"
        assert (got[:, nb:] == 0xAB).all(), "bytes past the row's end were touched"


def test_downstream_operators_do_not_see_the_phase(gpu):
    from ld_tools_amd import PackedPanel, ld_em, ld_rect, plink

    n_snps, n_ind = 200, 150
    rng = np.random.default_rng(12)
    freq = rng.uniform(0.05, 0.95, size=(n_snps, 1))
    codes = (rng.random((n_snps, 2 * n_ind)) < freq).astype(np.int8)      # hets in both orders: "phased" calls
    gone = rng.random((n_snps, n_ind)) < 0.03
    codes[np.repeat(gone, 2, axis=1)] = 2                                 # whole genotypes missing
    assert ((codes[:, 0::2] == 0) & (codes[:, 1::2] == 1)).any() and gone.any()
    rows = plink.codes_bed_host(codes)
    from_file = PackedPanel.from_bed((rows, n_ind), device=gpu)
    from_calls = PackedPanel.from_codes(codes, gpu)
    assert not torch.equal(from_file.alt, from_calls.alt)                 # the hets moved ...
    a, b = ld_em(from_file, from_file, missing="pairwise"), ld_em(from_calls, from_calls, missing="pairwise")
    assert torch.equal(a.r.view(torch.int32), b.r.view(torch.int32))      # ... and nothing downstream notices
    assert torch.equal(a.dprime.view(torch.int32), b.dprime.view(torch.int32))
    ra = ld_rect(from_file, from_file, dosage=True, missing="pairwise")
    rb = ld_rect(from_calls, from_calls, dosage=True, missing="pairwise")
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32))
    assert float(a.r.abs().max()) > 0.0 and float(ra.abs().max()) > 0.0

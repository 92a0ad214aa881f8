"""GPU: sample and SNP subsets of a packed panel (PackedPanel.select / split, ldx_panel_select_dev, ld_scores_by_group).

The truth is numpy on the allele codes, ``sub = codes[rows][:, cols]``: the selected panel's planes are compared bit for bit
after un-tiling (the layout of include/ldx.h, re-derived here) and byte for byte -- planes, counts, fa / fr / q, pad entries
included -- with ``PackedPanel.from_codes(sub)``; the total popcount of each plane equals the count of ones / zeros in
``sub``, so every pad bit is zero.  Codes are 0, 1 and some 2, so the two planes are not complements.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import fakevcf  # noqa: E402
import ld_exact as lx  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(5, 31), (128, 256), (129, 257), (130, 300), (257, 5008), (64, 10240)]
LENGTHS = (1, 32, 33, 128, 129, 256, 257)


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import ld_tools_amd  # noqa: F401  (raises if libldx.so is missing: no fallback)
    return torch.device("cuda", 0)


_SOURCES = {}


def source(shape, gpu):
    """(codes, packed panel) of a shape, made once."""
    if shape not in _SOURCES:
        from ld_tools_amd import PackedPanel

        rng = np.random.default_rng(shape[0] * 100003 + shape[1])
        codes = rng.choice(np.array([0, 1, 2], dtype=np.int8), size=shape, p=[0.55, 0.35, 0.10])
        _SOURCES[shape] = (codes, PackedPanel.from_codes(codes, gpu))
    return _SOURCES[shape]


def untile(plane, n_snps, n_hap):
    """Tiled plane bytes -> bool [padded_snps][n_chunks * 128] (include/ldx.h: slab s, chunk c, row r is the 16-byte group at
    ((s * n_chunks + c) * 128 + r) * 16, bit h % 128 of it, little-endian, haplotype 128 c + h % 128 of SNP 128 s + r)."""
    n_slabs, n_chunks = (n_snps + 127) // 128, 2 * ((n_hap + 255) // 256)
    raw = np.ascontiguousarray(plane.cpu().numpy())
    assert raw.size == n_slabs * n_chunks * 128 * 16
    bits = np.unpackbits(raw.reshape(n_slabs, n_chunks, 128, 16), axis=-1, bitorder="little")   # [s][c][r][128]
    return bits.transpose(0, 2, 1, 3).reshape(n_slabs * 128, n_chunks * 128).astype(bool)


def check_panel(got, sub, gpu, what):
    import torch

    from ld_tools_amd import PackedPanel

    n, h = sub.shape
    assert (got.n_snps, got.n_hap) == (n, h), what
    for plane, code in ((got.alt, 1), (got.ref, 0)):
        bits = untile(plane, n, h)
        assert np.array_equal(bits[:n, :h], sub == code), what
        assert int(bits.sum()) == int((sub == code).sum()), what          # nothing set in pad rows or pad haplotypes
    want = PackedPanel.from_codes(sub, gpu)
    for name in ("alt", "ref", "acnt", "rcnt", "fa", "fr", "q"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (what, name)


def hap_selections(n_hap, rng):
    """(name, columns) of every haplotype selection of a source with n_hap haplotypes."""
    yield "identity", np.arange(n_hap)
    for L in LENGTHS:
        if L <= n_hap:
            yield f"reversal[{L}]", np.arange(n_hap)[::-1][:L]
        if L <= (n_hap + 1) // 2:
            yield f"second[{L}]", np.arange(0, n_hap, 2)[:L]
        yield f"repeat[{L}]", np.full(L, int(rng.integers(n_hap)))
        yield f"random[{L}]", rng.integers(0, n_hap, size=L)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_haplotype_selections(gpu, shape):
    codes, p = source(shape, gpu)
    rng = np.random.default_rng(shape[1])
    count = 0
    for name, cols in hap_selections(shape[1], rng):
        got = p.select(haplotypes=cols)
        check_panel(got, codes[:, cols], gpu, (shape, name))
        assert "_area_plans" not in got.__dict__
        count += 1
    assert count >= 10


def test_more_haplotypes_than_the_source(gpu):
    import torch

    codes, p = source((129, 257), gpu)
    cols = np.random.default_rng(3).integers(0, 257, size=300)
    check_panel(p.select(haplotypes=cols), codes[:, cols], gpu, "300 of 257")
    check_panel(p.select(haplotypes=torch.from_numpy(cols).to(gpu)), codes[:, cols], gpu, "device indices")
    mask = np.random.default_rng(4).random(257) < 0.4
    check_panel(p.select(haplotypes=mask), codes[:, mask], gpu, "mask")


def snp_selections(n_snps, rng):
    yield "one", np.array([n_snps - 1])
    yield "128 descending", np.arange(n_snps)[::-1][:128]
    yield "129 with repeats", rng.integers(0, n_snps, size=129)
    yield "straddle", np.arange(120, min(n_snps, 140))              # rows of source slabs 0 and 1, side by side
    yield "straddle, repeated", np.repeat(np.array([127, 128]), 65)  # 130 rows: two destination slabs


@pytest.mark.parametrize("shape", [(129, 257), (130, 300), (257, 5008)], ids=str)
def test_snp_selections_with_and_without_haplotypes(gpu, shape):
    codes, p = source(shape, gpu)
    rng = np.random.default_rng(shape[0])
    for name, rows in snp_selections(shape[0], rng):
        check_panel(p.select(snps=rows), codes[rows], gpu, (shape, name))
        cols = rng.integers(0, shape[1], size=int(rng.choice(LENGTHS)))
        check_panel(p.select(snps=rows, haplotypes=cols), codes[rows][:, cols], gpu, (shape, name, "with haplotypes"))
    mask = rng.random(shape[0]) < 0.5
    check_panel(p.select(snps=mask), codes[mask], gpu, (shape, "mask"))


def test_dirty_destination_and_out_checks(gpu):
    from ld_tools_amd import LdxError, PackedPanel

    codes, p = source((130, 300), gpu)
    rng = np.random.default_rng(8)
    rows, cols = rng.integers(0, 130, size=129), rng.integers(0, 300, size=257)
    out = PackedPanel.empty(129, 257, gpu)
    for t in (out.alt, out.ref):
        t.fill_(0xFF)
    for t in (out.acnt, out.rcnt):
        t.fill_(-1)
    for t in (out.fa, out.fr, out.q):
        t.fill_(float("nan"))
    assert p.select(snps=rows, haplotypes=cols, out=out) is out
    check_panel(out, codes[rows][:, cols], gpu, "dirty out")
    cols2 = rng.integers(0, 300, size=257)
    p.select(snps=rows, haplotypes=cols2, out=out)                    # a second launch into the used buffer
    check_panel(out, codes[rows][:, cols2], gpu, "reused out")
    with pytest.raises(LdxError):
        p.select(haplotypes=cols, out=out)                             # 130 x 257: not out's shape
    with pytest.raises(LdxError):
        p.select(haplotypes=np.arange(300), out=p)
    with pytest.raises(LdxError):
        p.select()
    for bad in ([300], [-1], [0.5]):
        with pytest.raises(LdxError):
            p.select(haplotypes=bad)
    with pytest.raises(LdxError):
        p.select(snps=[130])


def raw_select(p, snp_idx, n_snps_dst, hap_idx, n_hap_dst, gpu, alt_only=False):
    """ldx_panel_select_dev on index arrays taken as they are (no host check): (alt, ref, acnt, rcnt) tensors, pre-filled
    with ones."""
    import torch

    from ld_tools_amd import _lib

    L = _lib.lib
    pb, npad = L.ldx_plane_bytes(n_snps_dst, n_hap_dst), L.ldx_padded_snps(n_snps_dst)
    alt = torch.full((pb,), 0xFF, dtype=torch.uint8, device=gpu)
    ref = torch.full((pb,), 0xFF, dtype=torch.uint8, device=gpu)
    acnt = torch.full((npad,), -1, dtype=torch.int32, device=gpu)
    rcnt = torch.full((npad,), -1, dtype=torch.int32, device=gpu)
    dev = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32)).to(gpu)  # noqa: E731
    sd, hd = dev(snp_idx), dev(hap_idx)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = L.ldx_panel_select_dev(p.alt.data_ptr(), None if alt_only else p.ref.data_ptr(), p.n_snps, p.n_hap, ptr(sd), n_snps_dst,
                                ptr(hd), n_hap_dst, alt.data_ptr(), None if alt_only else ref.data_ptr(), acnt.data_ptr(),
                                None if alt_only else rcnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ldx_panel_select_dev")
    torch.cuda.synchronize()
    return alt, ref, acnt, rcnt


def test_sentinels_of_the_c_entry(gpu):
    codes, p = source((130, 300), gpu)
    n, h = codes.shape
    rng = np.random.default_rng(21)
    # haplotype sentinel: 0xFFFFFFFF (and n_hap_src itself, the first index past the source) = a missing call
    cols = rng.integers(0, h, size=257).astype(np.int64)
    miss = np.array([0, 31, 32, 127, 128, 200, 256])
    hap_idx = cols.copy()
    hap_idx[miss] = 0xFFFFFFFF
    hap_idx[200] = h
    alt, ref, acnt, rcnt = raw_select(p, None, n, hap_idx, 257, gpu)
    want = codes[:, cols].copy()
    want[:, miss] = 2
    for plane, cnt, code in ((alt, acnt, 1), (ref, rcnt, 0)):
        bits = untile(plane, n, 257)
        assert np.array_equal(bits[:n, :257], want == code) and int(bits.sum()) == int((want == code).sum())
        assert not bits[:, miss].any()
        c = cnt.cpu().numpy()
        assert np.array_equal(c[:n], (want == code).sum(axis=1)) and not c[n:].any()
    # SNP sentinel: n_snps_src = an all-missing row, a = r = 0
    rows = rng.integers(0, n, size=129).astype(np.int64)
    gone = np.array([0, 5, 127, 128])
    snp_idx = rows.copy()
    snp_idx[gone] = n
    snp_idx[5] = 0xFFFFFFFF
    alt, ref, acnt, rcnt = raw_select(p, snp_idx, 129, None, h, gpu)
    want = codes[rows].copy()
    want[gone] = 2
    for plane, cnt, code in ((alt, acnt, 1), (ref, rcnt, 0)):
        bits = untile(plane, 129, h)
        assert np.array_equal(bits[:129, :h], want == code) and int(bits.sum()) == int((want == code).sum())
        c = cnt.cpu().numpy()
        assert np.array_equal(c[:129], (want == code).sum(axis=1)) and not c[129:].any()
        assert not c[gone].any()
    # the ALT plane alone (ref_src = ref_dst = rcnt_dst = NULL): the REF outputs are not touched
    alt, ref, acnt, rcnt = raw_select(p, rows, 129, cols, 257, gpu, alt_only=True)
    bits = untile(alt, 129, 257)
    assert np.array_equal(bits[:129, :257], codes[rows][:, cols] == 1) and int(bits.sum()) == int((codes[rows][:, cols] == 1).sum())
    assert bool((ref == 0xFF).all()) and bool((rcnt == -1).all())


def test_argument_checks_of_the_c_entry(gpu):
    import torch

    from ld_tools_amd import PackedPanel, _lib

    L = _lib.lib
    _, p = source((130, 300), gpu)
    out = PackedPanel.empty(130, 300, gpu)
    idx = torch.zeros(300, dtype=torch.int32, device=gpu)
    s = torch.cuda.current_stream().cuda_stream

    def call(alt_src=p.alt.data_ptr(), ref_src=p.ref.data_ptr(), n_hap_src=300, hap=idx.data_ptr(), n_hap_dst=300,
             alt_dst=out.alt.data_ptr(), ref_dst=out.ref.data_ptr(), rcnt=out.rcnt.data_ptr(), n_snps_dst=130):
        return L.ldx_panel_select_dev(alt_src, ref_src, 130, n_hap_src, None, n_snps_dst, hap, n_hap_dst, alt_dst, ref_dst,
                                      out.acnt.data_ptr(), rcnt, s)

    assert call() == 0
    assert call(alt_dst=p.alt.data_ptr()) == -1                 # LDX_E_ARG: source and destination overlap
    assert call(alt_dst=p.ref.data_ptr() + 16) == -1
    assert call(ref_dst=None) == -1                             # ref_src / ref_dst / rcnt_dst go together
    assert call(ref_src=None, ref_dst=None) == -1
    assert call(hap=None, n_hap_dst=299) == -1                  # identity needs equal sizes
    assert call(n_snps_dst=129) == -1
    assert call(n_hap_dst=0) == -3 and call(n_hap_dst=10241) == -3 and call(n_hap_src=10241) == -3    # LDX_E_UNSUPPORTED
    torch.cuda.synchronize()


def test_split_by_label(gpu):
    from ld_tools_amd import LdxError

    codes, p = source((130, 300), gpu)
    labels = [h % 3 for h in range(300)]
    parts = p.split(labels)
    assert list(parts) == [0, 1, 2]
    for k, sub in parts.items():
        check_panel(sub, codes[:, k::3], gpu, ("split", k))
    named = p.split(["EUR" if h < 100 else "AFR" for h in range(300)])
    check_panel(named["AFR"], codes[:, 100:], gpu, "AFR")
    with pytest.raises(LdxError):
        p.split(labels[:-1])


def test_ld_score_on_a_selected_panel_against_exact_counts(gpu):
    """129 x 257 -> 129 x 100, then ld_score: against tests/ld_exact.py on the selected codes, with the LD-score bound of
    tests/test_gpu_exact_oracle.py (include/ldx.h: |l2 - sum r^2| <= 2^-19 sum r^2 + P 2^-33, P the in-window pairs)."""
    from ld_tools_amd import ops

    codes, p = source((129, 257), gpu)
    cols = np.random.default_rng(5).integers(0, 257, size=100)
    sub = np.ascontiguousarray(codes[:, cols])
    ex = lx.Exact(sub)
    q = p.select(haplotypes=cols)
    pos = 1 + 100 * np.arange(129, dtype=np.int64)
    for w in (1500, 10 ** 6):
        win = lx.window_mask(pos, w)
        L = (ex.r2_64 * win).sum(axis=1)
        bound = 2.0 ** -19 * L + win.sum(axis=1) * 2.0 ** -33
        for path in ("fp4", "mfma"):
            res = ops.ld_score(q, pos, window_bp=w, path=path)
            err = np.abs(res.l2[:, 0] - L)
            print(f"window {w} {path}: worst |l2 - exact| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
            assert (err <= bound).all(), (w, path)
            assert np.array_equal(res.live, ex.live)


def chromosome_rows(vcf):
    seen, rows = set(), []
    for rec in vcf.records:
        if rec.id.startswith("rs") and ";" not in rec.id and rec.id not in seen:
            seen.add(rec.id)
            rows.append([rec.pos, rec.id])
    return rows


def test_ld_scores_by_group(gpu, tmp_path):
    from ld_tools_amd import LdxError
    from ld_tools_amd.drivers import ld_scores, ld_scores_by_group, write_ldscore

    vcf, names = fakevcf.make_chromosome()
    rows = chromosome_rows(vcf)
    groups = {"EUR": names[:17], "AFR": names[17:]}             # disjoint; sample 7 (EUR) is in no record
    ann = np.random.default_rng(6).random((len(rows), 2)) < 0.5
    vcf.fetches = 0
    tabs = ld_scores_by_group(vcf, "6", rows, groups, window_bp=2_000, annot=ann, annot_names=["coding", "enh"])
    assert vcf.fetches == len(rows)                             # one pass over the VCF, not one per group
    assert list(tabs) == ["EUR", "AFR"]
    for label, members in groups.items():
        one = ld_scores(vcf, "6", rows, members, window_bp=2_000, annot=ann, annot_names=["coding", "enh"])
        tab = tabs[label]
        assert tab.rs_ids == one.rs_ids and tab.poss == one.poss and tab.annot_names == one.annot_names
        got, want = tab.scores.sums.cpu().numpy(), one.scores.sums.cpu().numpy()
        assert got.dtype == np.uint64 and got.shape == (len(rows), 3) and np.array_equal(got, want)   # the integer sums
        assert np.array_equal(tab.alt_freqs_exact, one.alt_freqs_exact) and np.array_equal(tab.annot, one.annot)
        assert np.array_equal(tab.scores.live, one.scores.live) and tab.scores.n_hap == one.scores.n_hap
        a = write_ldscore(str(tmp_path / f"{label}_groups"), tab)
        b = write_ldscore(str(tmp_path / f"{label}_alone"), one)
        for fa, fb in zip(a[1:], b[1:]):
            assert Path(fa).read_text() == Path(fb).read_text()
    assert not np.array_equal(tabs["EUR"].scores.sums.cpu().numpy(), tabs["AFR"].scores.sums.cpu().numpy())
    for bad in (30, 0):                                        # mixed ploidy; every second sample haploid throughout
        vcf2, names2 = fakevcf.make_chromosome(haploid_from=bad)
        with pytest.raises(LdxError):
            ld_scores_by_group(vcf2, "6", chromosome_rows(vcf2)[:40], {"a": names2[:20], "b": names2[20:]})
    with pytest.raises(LdxError):
        ld_scores_by_group(vcf, "6", rows, {"EUR": names[:17], "nobody": ["NA00001"]})

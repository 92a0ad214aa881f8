"""CPU: the host side of genotype-dosage LD -- the oracle of tests/ld_dosage_exact.py pinned against np.corrcoef,
ops.dosage_host against the oracle, the E2M1 nibble algebra of the kernel's B operand, the properties of the panels the GPU
tests use (so that they are checked without a GPU), the argument rules, and the header's declarations."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_dosage_exact as dx  # noqa: E402
import ld_exact as lx  # noqa: E402


@pytest.mark.parametrize("shape", dx.SHAPES, ids=str)
def test_oracle_against_corrcoef_and_dosage_host(shape):
    from ld_tools_amd import dosage_host
    codes, _, ex = dx.panel(shape)
    a, hom, v = dosage_host(codes)
    assert np.array_equal(a, ex.a) and np.array_equal(hom, ex.hom) and np.array_equal(v, ex.v)
    assert np.array_equal(a, (codes == 1).sum(axis=1))                  # a is the panel's ALT count
    live = np.flatnonzero(ex.live)
    if live.size >= 2:
        c = np.corrcoef(ex.g[live].astype(np.float64))
        assert np.max(np.abs(ex.r64[np.ix_(live, live)] - c)) <= 1e-12
    assert np.array_equal(ex.r64 == 0.0, ex.degenerate | ex.zero_num)
    assert np.array_equal(np.diagonal(ex.r64), ex.diagonal())


def e2m1(nibble):
    """Value of an FP4 E2M1 nibble (sign, two exponent bits, one mantissa bit)."""
    s, e, m = (nibble >> 3) & 1, (nibble >> 1) & 3, nibble & 1
    mag = 0.5 * m if e == 0 else (1.0 + 0.5 * m) * 2.0 ** (e - 1)
    return -mag if s else mag


def test_nibble_algebra_of_the_b_operand():
    """The kernel's operands for one 32-bit word (ldx_mfma.hip: expand32_a4, expand32_b4_dosage), decoded as E2M1 and
    multiplied position by position: the sum over a word pair is sum over the 16 individuals of H_i(h) g_j(ind(h)), so an
    accumulator holds S_ij.  20 000 random word pairs plus the all-ones word."""
    rng = np.random.default_rng(0)
    wa = np.concatenate([rng.integers(0, 1 << 32, size=20000, dtype=np.uint64), [0xFFFFFFFF, 0xFFFFFFFF, 0]]).astype(np.uint64)
    wb = np.concatenate([rng.integers(0, 1 << 32, size=20000, dtype=np.uint64), [0xFFFFFFFF, 0, 0xFFFFFFFF]]).astype(np.uint64)
    M = np.uint64(0xFFFFFFFF)
    c1, c2, c4 = np.uint64(0x11111111), np.uint64(0x22222222), np.uint64(0x44444444)
    one, two = np.uint64(1), np.uint64(2)
    A = [wa & c1, wa & c2, (wa >> two) & c1, (wa >> two) & c2]
    s = wb >> one
    o, n, x = wb | s, wb & s, wb ^ s
    B = [(((o << two) & M) & c4) | (((n << one) & M) & c2), (((x << one) & M) & c2) | (((n << two) & M) & c4),
         (o & c4) | ((n >> one) & c2), ((x >> one) & c2) | (n & c4)]
    val = np.array([e2m1(k) for k in range(16)])
    got = np.zeros(wa.size)
    for reg in range(4):
        for q in range(8):
            sh = np.uint64(4 * q)
            got += val[((A[reg] >> sh) & np.uint64(15)).astype(np.int64)] * val[((B[reg] >> sh) & np.uint64(15)).astype(np.int64)]
    bits = lambda w: ((w[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & one).astype(np.int64)   # noqa: E731
    ha, hb = bits(wa), bits(wb)
    g = hb[:, 0::2] + hb[:, 1::2]
    want = (ha * np.repeat(g, 2, axis=1)).sum(axis=1)
    assert np.array_equal(got, want.astype(np.float64))
    assert got.max() == 64.0                      # 32 haplotypes x dosage 2: the all-ones pair


def test_panel_properties():
    """What the GPU tests rely on, on exactly their panels."""
    differs = 0
    for shape in dx.SHAPES:
        codes, where, ex = dx.panel(shape)
        hx = lx.Exact(codes)
        n, h = shape
        for k in where.get("all_het", []):
            assert ex.v[k] == 0 and hx.a[k] * hx.r[k] > 0 and ex.a[k] == h // 2 and ex.hom[k] == 0
        for k in where.get("mono", []) + where.get("all_alt", []):
            assert ex.v[k] == 0
        for k in where.get("all_alt", []):
            assert ex.S[k, k] == 4 * (h // 2) and ex.a[k] == h
        for k in where.get("code2", []):
            assert (codes[k] == 2).sum() > 0
        for s_, d_ in zip(where.get("source", []), where.get("duplicate", [])):
            assert ex.live[s_] and ex.num2[s_, d_] == ex.den2[s_, d_] and ex.num[s_, d_] > 0 and ex.r64[s_, d_] == 1.0
        for s_, d_ in zip(where.get("source", []), where.get("complement", [])):
            assert ex.num2[s_, d_] == ex.den2[s_, d_] and ex.num[s_, d_] < 0 and ex.r64[s_, d_] == -1.0
        if n >= 8:
            assert all(kind in where for kind in ("mono", "all_alt", "all_het", "code2", "duplicate", "complement"))
        differs += int((ex.live != hx.live).sum())
        assert not (ex.live & ~hx.live).any()     # a SNP without ALT or without REF codes has no dosage variance either
        # another phase: the same integers
        other = dx.DosageExact(dx.rephased(shape))
        assert np.array_equal(other.a, ex.a) and np.array_equal(other.hom, ex.hom) and np.array_equal(other.S, ex.S)
        if n >= 5:
            assert not np.array_equal(lx.Exact(dx.rephased(shape)).n11, hx.n11)   # ... but other haplotype counts
    assert differs >= len(dx.SHAPES)              # the all-het SNP of every panel: live for the haplotype r, not for the dosage
    assert dx.panel((1, 2))[2].degenerate.all()
    assert dx.SHAPES[-1][1] == dx.MAX_HAPS and 6 % 4 == 2


@pytest.mark.parametrize("shape", dx.SHAPES, ids=str)
def test_neighbour_inputs_are_decided(shape):
    """Per panel and window of the neighbour-list test at r^2 = 0.2: ambiguous pairs are at most 1 % of the in-window pairs;
    a panel of more than 128 SNPs has at least 50 decided-in pairs, one of them across a 128-column tile."""
    _, _, ex = dx.panel(shape)
    n = shape[0]
    for pos, w in dx.neighbour_windows(n):
        din, amb, inw = dx.pair_classes(ex, dx.NEIGHBOUR_R2, pos, w)
        assert amb.sum() <= dx.AMBIGUOUS_SHARE_MAX * max(1, inw.sum())
        if n > 128:
            assert din.sum() >= dx.MIN_DECIDED_IN and dx.tile_crossing(din) >= 1


def dummy_panel(n_snps, n_hap):
    import torch
    from ld_tools_amd import PackedPanel
    z = torch.zeros(1, dtype=torch.uint8)
    return PackedPanel(n_snps, n_hap, z, z, z, z, z, z, z)


def test_argument_rules():
    """Checked before anything touches a device: an odd n_hap, dosage with a cell format other than r32 or with regions /
    unit_range, and the operators that have no dosage form."""
    import ld_tools_amd as L
    from ld_tools_amd import dist
    from ld_tools_amd.drivers.ldscore import ld_scores
    E = L.LdxError
    odd, even = dummy_panel(4, 7), dummy_panel(4, 8)
    pos = np.arange(4, dtype=np.int64)
    assert even.n_ind == 4 and odd.n_ind == 3
    for call in (lambda: L.ld_triangle(odd, fmt="r32", dosage=True), lambda: L.ld_score(odd, pos, dosage=True),
                 lambda: L.ld_neighbors(odd, pos, dosage=True), lambda: L.ld_prune(odd, pos, dosage=True),
                 lambda: L.ld_clump(odd, pos, np.full(4, 1e-6), dosage=True), odd.dosage_stats):
        with pytest.raises(E, match="odd|even"):
            call()
    for fmt in ("ld32", "k16", "k16r", "k16d"):
        with pytest.raises(E, match="r32"):
            L.ld_triangle(even, fmt=fmt, dosage=True)
    with pytest.raises(E, match="unit_range"):
        L.ld_triangle(even, fmt="r32", dosage=True, unit_range=(0, 1))
    with pytest.raises(E, match="regions"):
        L.ld_score(even, pos, regions=np.zeros(4, dtype=np.int64), dosage=True)
    x = np.ones(4, dtype=np.float32)
    for call in (lambda: L.ld_matvec(even, x, pos, dosage=True), lambda: L.ld_decay(even, pos, dosage=True),
                 lambda: L.ld_cross(even, pos, dosage=True), lambda: L.ld_blocks(even, pos, dosage=True),
                 lambda: dist.ld_area_sharded(even, pos, dosage=True)):
        with pytest.raises(E, match="dosage"):
            call()
    with pytest.raises(E, match="even"):
        L.dosage_host(np.zeros((2, 3), dtype=np.int8))
    with pytest.raises(E, match="missing"):
        ld_scores(None, "6", [], [], dosage=True, missing="drop")
    with pytest.raises(E, match="missing"):
        ld_scores(None, "6", [], [], missing="ref")


def test_header_and_exports():
    import ld_tools_amd
    from ld_tools_amd import _lib
    header = (ROOT / "include" / "ldx.h").read_text()
    for sym in ("ldx_dosage_stats_dev", "ldx_triangle_dosage_dev", "ldx_triangle_r_block_dosage_dev", "ldx_ld_score_dosage_dev",
                "ldx_ld_neighbors_dosage_dev"):
        assert sym in header and sym in _lib.SIGNATURES and hasattr(_lib.lib, sym)
    assert "acts as REF" in header and "4 float32 ulps" in header and "bit for bit" in header
    assert "dosage_host" in ld_tools_amd.__all__ and hasattr(ld_tools_amd, "dosage_host")
    assert ld_tools_amd.version() == 102 and "#define LDX_VERSION 102" in header
    import inspect
    for fn in (ld_tools_amd.ld_triangle, ld_tools_amd.ld_score, ld_tools_amd.ld_neighbors, ld_tools_amd.ld_prune,
               ld_tools_amd.ld_clump):
        assert inspect.signature(fn).parameters["dosage"].default is False

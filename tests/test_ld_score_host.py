"""CPU: the LD-score surface without a GPU -- ABI, the host term function, the m / adjusted() helpers and the LDSC writer."""
import gzip
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_score_symbols_declared_exported_and_bound():
    from ld_tools_amd import _lib
    header = (ROOT / "include" / "ldx.h").read_text()
    for name in ("ldx_ld_score_workspace_bytes", "ldx_ld_score_dev"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.ldx_version() == 102


def test_workspace_bytes_is_pure_arithmetic():
    from ld_tools_amd import _lib
    lib = _lib.lib
    for n in (1, 2, 127, 128, 129, 10_000, 100_000, 600_000):
        b = lib.ldx_ld_score_workspace_bytes(n, 5008)
        assert b % 256 == 0 and b >= n + 1024
        assert b == lib.ldx_ld_score_workspace_bytes(n, 1)            # the haplotype count does not enter
    assert lib.ldx_ld_score_workspace_bytes(0, 1) == lib.ldx_ld_score_workspace_bytes(1, 1)


def test_band_workspace_sizes_are_pinned():
    """The byte counts of the band workspaces, recorded from the library before the layout moved into one carve function
    (64 haplotypes; 524 160 SNPs is the last panel with a ticket order, T = 4095, 524 161 the first without)."""
    from ld_tools_amd import _lib
    lib = _lib.lib
    ns = (0, 1, 128, 129, 1000, 100_000, 524_160, 524_161, 600_000)
    band = (2816, 2816, 2816, 2816, 3584, 727_808, 17_368_320, 591_616, 677_120)
    sizes = {"score": band, "cross": band, "decay": band, "fgt": band, "neighbors": band,
             "matvec": band[:7] + (17_368_832, 17_454_336)}      # no order: the order's largest size instead
    for name, want in sizes.items():
        fn = getattr(lib, f"ldx_ld_{name}_workspace_bytes")
        assert tuple(fn(n, 64) for n in ns) == want, name
    assert tuple(lib.ldx_area_workspace_bytes(n, 64, 1) for n in ns) == (
        8960, 9216, 9216, 9216, 9216, 727_552, 17_368_064, 591_360, 676_864)
    assert tuple(lib.ldx_area_workspace_bytes(n, 64, n) for n in ns) == (
        8960, 9216, 9216, 17_920, 70_144, 6_816_256, 35_692_032, 35_700_992, 40_860_928)


def test_score_terms_at_the_edges():
    from ld_tools_amd.ops import score_terms
    f = np.float32
    # the 2^-9 boundary: over consecutive float32 r around 2^-4.5, 2^32 r^2 is an integer -- the term exact -- wherever
    # r^2 >= 2^-9, and below it (where it need not be) the term is its round-half-even
    r = np.nextafter(np.float32(2.0 ** -4.5), np.float32(0), dtype=np.float32)
    rs = (r.view(np.int32) + np.arange(-4000, 4000, dtype=np.int32)).view(np.float32)
    x = np.ldexp(np.multiply(rs, rs, dtype=np.float32).astype(np.float64), 32)
    above = x >= 2.0 ** 23
    assert above.any() and (~above).any()
    assert (x[above] == np.floor(x[above])).all()
    assert (x[~above] != np.floor(x[~above])).any()
    assert np.array_equal(score_terms(rs), np.rint(x).astype(np.uint64))
    assert np.array_equal(score_terms(rs)[above], x[above].astype(np.uint64))
    rng = np.random.default_rng(0)
    big = rng.uniform(2.0 ** -4.4, 1.0, 10_000).astype(np.float32)
    x = np.ldexp((big * big).astype(np.float64), 32)
    assert (x == np.floor(x)).all() and np.array_equal(score_terms(big), x.astype(np.uint64))
    assert score_terms(np.float32(1.0)) == np.uint64(1 << 32)
    assert score_terms(np.float32(-1.0)) == np.uint64(1 << 32)
    # -0.0 (a degenerate SNP's cell) and +0.0 give 0
    assert score_terms(np.float32(-0.0)) == 0 and score_terms(np.float32(0.0)) == 0
    # |r| > 1 (missing codes): r^2 > 1, still exact
    assert score_terms(np.float32(3.0)) == np.uint64(9 << 32)
    assert score_terms(np.float32(-1.5)) == np.uint64(int(2.25 * 2 ** 32))
    # one float32 multiply: r *f32 r, not the double square
    r = np.float32(0.7)
    assert score_terms(r) == np.uint64(int(np.rint(np.ldexp(np.float64(np.float32(r * r)), 32))))
    assert score_terms(r) != np.uint64(int(np.rint(np.ldexp(np.float64(r) ** 2, 32))))
    # a tie in rint (half-way between two integers) rounds to even: r^2 = 2^-33 * 5 and 2^-33 * 3
    t5 = np.float32(np.sqrt(np.float64(5 * 2.0 ** -33)))
    if np.float32(t5 * t5) == np.float32(5 * 2.0 ** -33):
        assert score_terms(t5) == 2
    r2 = np.float32(3 * 2.0 ** -33)                     # 1.5 -> 2
    x = np.ldexp(np.float64(r2), 32)
    assert x == 1.5 and np.rint(x) == 2.0
    r = np.float32(2.0 ** -17)                            # r^2 = 2^-34: 0.25 -> 0
    assert score_terms(r) == 0
    r = np.float32(2.0 ** -16.5)                          # r^2 ~ 2^-33 = 0.5 -> 0 (to even)
    if np.float32(r * r) == np.float32(2.0 ** -33):
        assert score_terms(r) == 0
    r = np.float32(np.sqrt(np.float64(np.float32(1.5 * 2.0 ** -32))))
    if np.float32(r * r) == np.float32(1.5 * 2.0 ** -32):
        assert score_terms(r) == 2                        # 1.5 -> 2 (to even)


def brute_m(pos, w, live, bits, k):
    n = len(pos)
    out = np.zeros((n, 1 + k), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            if abs(int(pos[i]) - int(pos[j])) <= w and live[j]:
                out[i, 0] += 1
                for c in range(k):
                    out[i, 1 + c] += (int(bits[j]) >> c) & 1
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_window_counts_match_brute_force(seed):
    from ld_tools_amd.ops import window_counts
    rng = np.random.default_rng(seed)
    n = 150
    pos = np.sort(rng.integers(1, 60, size=n)).astype(np.int64)     # many duplicates
    live = rng.random(n) < 0.85
    k = int(rng.integers(0, 9))
    bits = rng.integers(0, 256, size=n).astype(np.uint8)
    for w in (0, 1, 3, 17, int(pos[-1] - pos[0]), 10 ** 9):
        assert np.array_equal(window_counts(pos, w, live, bits, k), brute_m(pos, w, live, bits, k)), w
    # a window of 0 counts the SNP's own position only; one covering everything counts every live SNP
    assert np.array_equal(window_counts(pos, 10 ** 9, live)[:, 0], np.full(n, live.sum()))


def test_adjusted_is_the_per_term_formula_summed():
    from ld_tools_amd.ops import adjust_l2
    rng = np.random.default_rng(5)
    n_obs = 5008
    for _ in range(20):
        r2 = rng.random(rng.integers(1, 60)) ** 3
        direct = (r2 - (1.0 - r2) / (n_obs - 2)).sum()
        got = adjust_l2(np.array([r2.sum()]), np.array([r2.size]), n_obs)[0]
        assert abs(got - direct) <= 1e-12 * max(1.0, abs(direct))
    with pytest.raises(Exception):
        adjust_l2(np.ones(1), np.ones(1), 2)


def test_pack_annot():
    from ld_tools_amd import LdxError
    from ld_tools_amd.ops import pack_annot
    a = np.array([[1, 0, 1], [0, 0, 0], [1, 1, 1]])
    bits, k = pack_annot(a, 3)
    assert k == 3 and bits.tolist() == [5, 0, 7]
    bits, k = pack_annot(np.array([True, False, True]), 3)
    assert k == 1 and bits.tolist() == [1, 0, 1]
    with pytest.raises(LdxError, match="at most 8"):
        pack_annot(np.zeros((3, 9), dtype=bool), 3)
    with pytest.raises(LdxError, match="0/1"):
        pack_annot(np.full((3, 2), 2), 3)
    with pytest.raises(LdxError, match="shape"):
        pack_annot(np.zeros((4, 2), dtype=bool), 3)


class _FakeScores:
    """What write_ldscore reads from LDScores, built by hand."""

    def __init__(self, l2, m, live, n_hap):
        from ld_tools_amd.ops import adjust_l2
        self.l2, self.m, self.live, self.n_hap = l2, m, live, n_hap
        self._adj = adjust_l2(l2, m, n_hap)

    def adjusted(self, n_obs=None):
        return self._adj


def test_writer_files(tmp_path):
    from ld_tools_amd.drivers.ldscore import LDScoreTable, write_ldscore
    l2 = np.array([[1.23449, 0.5, 0.7344], [0.0, 0.0, 0.0], [12.0, 0.0004, 11.9996], [3.5, 3.5, 0.0]])
    m = np.array([[3, 1, 2], [3, 1, 2], [2, 1, 1], [2, 2, 0]])
    live = np.array([True, False, True, True])
    annot = np.array([[True, False], [True, True], [False, True], [True, True]])
    fa = np.array([0.5, 0.0, 0.03, 0.96])
    tab = LDScoreTable("22", ["rs1", "rs2", "rs3", "rs4"], [100, 200, 300, 400], fa, annot, ["cod", "enh"],
                       _FakeScores(l2, m, live, 100), adjust=False)
    paths = write_ldscore(str(tmp_path / "x"), tab)
    assert paths == [str(tmp_path / "x.l2.ldscore.gz"), str(tmp_path / "x.l2.M"), str(tmp_path / "x.l2.M_5_50")]
    with gzip.open(paths[0], "rt") as f:
        text = f.read()
    assert text == ("CHR\tSNP\tBP\tcodL2\tenhL2\n"
                    "22\trs1\t100\t0.500\t0.734\n"
                    "22\trs3\t300\t0.000\t12.000\n"
                    "22\trs4\t400\t3.500\t0.000\n")
    assert Path(paths[1]).read_text() == "2\t2\n"          # written SNPs per category (rs2 is degenerate)
    assert Path(paths[2]).read_text() == "1\t0\n"          # ... with MAF > 0.05: rs1 only
    # no annotation: one L2 column (column 0), adjusted values
    tab0 = LDScoreTable("22", ["rs1", "rs2", "rs3", "rs4"], [100, 200, 300, 400], fa, None, [],
                        _FakeScores(l2, m, live, 100), adjust=True)
    write_ldscore(str(tmp_path / "y"), tab0)
    with gzip.open(tmp_path / "y.l2.ldscore.gz", "rt") as f:
        lines = f.read().splitlines()
    adj = tab0.scores.adjusted()
    assert lines[0] == "CHR\tSNP\tBP\tL2"
    assert [ln.split("\t")[3] for ln in lines[1:]] == ["%.3f" % adj[k, 0] for k in (0, 2, 3)]
    assert (tmp_path / "y.l2.M").read_text() == "3\n"
    assert (tmp_path / "y.l2.M_5_50").read_text() == "1\n"


def test_ld_score_needs_a_gpu(monkeypatch):
    import torch

    from ld_tools_amd import LdxError, ld_score
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(LdxError, match="HIP device"):
        ld_score(None, [1, 2, 3])

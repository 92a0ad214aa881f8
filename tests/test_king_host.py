"""CPU: the sample-relatedness definitions (include/ldx.h, "sample relatedness") on the host mirrors -- a hand-counted table,
the loop oracle against the numpy mirror, the squared-difference identity, king_cutoff's rule, the writers' bytes, and a
pedigree that says the kinship cell means what its name says.  No kernel is launched here."""
import numpy as np
import pytest

from ld_king_exact import hand_table, loop_counts, panel_codes


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def cells(counts):
    from ld_tools_amd import ibs_cell_host, king_cell_host

    N, HH, IBS0, HET = counts
    args = (N, HH, IBS0, HET, HET.T)
    return king_cell_host(*args), ibs_cell_host(*args)


def test_hand_counted_table():
    from ld_tools_amd import sample_counts_host

    codes, keep, want, kin, ibs = hand_table()
    assert np.array_equal(loop_counts(codes, keep), want)
    got = sample_counts_host(codes, keep)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    k, s = cells(got)
    assert k.dtype == np.float32 and s.dtype == np.float32
    assert np.array_equal(bits(k), bits(kin)), k          # bit for bit: -0.0f where m == 0, 0.5f on a diagonal with a het
    assert np.array_equal(bits(s), bits(ibs)), s
    assert np.signbit(k[2]).all() and np.signbit(k[:, 2]).all() and (k[2] == 0).all() and (k[:2, :2] != 0).all()
    # the mask is the same as leaving the SNP out; without it SNP 4 counts
    assert np.array_equal(sample_counts_host(codes[keep]), want)
    assert sample_counts_host(codes)[0, 0, 0] == 4


def test_empty_pair_cells():
    from ld_tools_amd import ibs_cell_host, king_cell_host

    z = np.zeros(3, dtype=np.int64)
    assert np.array_equal(bits(king_cell_host(z, z, z, z, z)), bits(np.full(3, -0.0)))
    assert np.array_equal(bits(ibs_cell_host(z, z, z, z, z)), bits(np.full(3, -0.0)))
    # the largest legal counts: every SNP of 2^32 - 1 heterozygous in both
    big = np.array([2 ** 32 - 1])
    assert king_cell_host(big, big, 0, big, big)[0] == np.float32(0.5) and ibs_cell_host(big, big, 0, big, big)[0] == np.float32(1.0)
    # ... or opposite homozygotes at all but one
    assert king_cell_host(big, 1, big - 1, 1, 1)[0] == np.float32(0.5 - (4.0 * (2 ** 32 - 2)) / 4.0)


@pytest.mark.parametrize("holes", ["none", "3%", "single"])
def test_numpy_mirror_against_the_loop(holes):
    from ld_tools_amd import sample_counts_host

    codes = panel_codes(7, 90, seed=11, holes=holes)
    keep = np.random.default_rng(3).random(90) < 0.8
    assert np.array_equal(sample_counts_host(codes, keep), loop_counts(codes, keep))
    assert np.array_equal(sample_counts_host(codes), loop_counts(codes))


def test_squared_difference_identity():
    from ld_tools_amd import sample_counts_host

    codes = panel_codes(9, 400, seed=5, holes="3%")
    N, HH, IBS0, HET = sample_counts_host(codes)
    h0, h1 = codes[:, 0::2], codes[:, 1::2]
    called = np.isin(h0, (0, 1)) & np.isin(h1, (0, 1))
    g = ((h0 == 1).astype(np.int64) + (h1 == 1)) * called
    both = called[:, :, None] & called[:, None, :]
    d2 = (((g[:, :, None] - g[:, None, :]) ** 2) * both).sum(axis=0)
    ibs1 = HET + HET.T - 2 * HH
    assert np.array_equal(d2, 4 * IBS0 + ibs1)
    assert ((N - ibs1 - IBS0) >= 0).all() and (ibs1 >= 0).all()
    assert np.array_equal(N, N.T) and np.array_equal(HH, HH.T) and np.array_equal(IBS0, IBS0.T) and not np.array_equal(HET, HET.T)


def graph(n, edges, value=0.3):
    kin = np.zeros((n, n), dtype=np.float32)
    for a, b in edges:
        kin[a, b] = kin[b, a] = value
    np.fill_diagonal(kin, 0.5)
    return kin


def test_king_cutoff_on_small_graphs():
    from ld_tools_amd import king_cutoff

    keep, why = king_cutoff(graph(4, [(0, 1), (1, 2), (2, 3)]), 0.1)           # a path: the ends first (one edge each)
    assert keep.tolist() == [True, False, False, True] and why.tolist() == [-1, 0, 3, -1]
    keep, why = king_cutoff(graph(5, [(0, 1), (0, 2), (0, 3), (0, 4)]), 0.1)   # a star: the leaves, the centre goes
    assert keep.tolist() == [False, True, True, True, True] and why.tolist() == [1, -1, -1, -1, -1]
    keep, why = king_cutoff(graph(3, [(0, 1), (1, 2), (0, 2)]), 0.1)           # a triangle: the smallest index
    assert keep.tolist() == [True, False, False] and why.tolist() == [-1, 0, 0]
    # strict, as a float32 comparison: a cell equal to the cutoff is no edge, the next float32 is
    keep, _ = king_cutoff(graph(2, [(0, 1)], value=np.float32(0.1)), float(np.float32(0.1)))
    assert keep.all()
    keep, _ = king_cutoff(graph(2, [(0, 1)], value=np.nextafter(np.float32(0.1), np.float32(1))), float(np.float32(0.1)))
    assert keep.tolist() == [True, False]
    keep, why = king_cutoff(np.full((1, 1), 0.5, dtype=np.float32), 0.1)      # the diagonal is no edge
    assert keep.tolist() == [True] and why.tolist() == [-1]


def test_writers_bytes(tmp_path):
    from ld_tools_amd import RelatedPairs
    from ld_tools_amd.drivers import KingTable, write_kin0, write_king_cutoff, write_king_matrix

    table = KingTable(["F1", "F1", "F2"], ["a", "b", "c"], None)
    pairs = RelatedPairs(np.array([1, 2]), np.array([0, 1]), np.array([0.25, -0.0078125], dtype=np.float32), np.array([8, 0]),
                         np.array([2, 0]), np.array([1, 0]))
    assert write_kin0(str(tmp_path / "t.kin0"), table, pairs) == 2
    assert (tmp_path / "t.kin0").read_bytes() == (b"#FID1\tIID1\tFID2\tIID2\tNSNP\tHETHET\tIBS0\tKINSHIP\n"
                                                  b"F1\ta\tF1\tb\t8\t0.25\t0.125\t0.25\n"
                                                  b"F1\tb\tF2\tc\t0\t0\t0\t-0.0078125\n")
    kin = np.array([[0.5, 0.25, 0.0], [0.25, 0.5, 1.0 / 3.0], [0.0, 1.0 / 3.0, 0.5]], dtype=np.float32)
    paths = write_king_matrix(str(tmp_path / "t"), table, kin)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["t.king", "t.king.id"]
    assert (tmp_path / "t.king").read_bytes() == b"0.25\n0\t0.333333\n"
    assert (tmp_path / "t.king.id").read_bytes() == b"#FID\tIID\nF1\ta\nF1\tb\nF2\tc\n"
    paths = write_king_cutoff(str(tmp_path / "t"), table, 0.2, kin)     # edges a - b - c: the ends stay
    assert (tmp_path / "t.king.cutoff.in.id").read_bytes() == b"#FID\tIID\nF1\ta\nF2\tc\n"
    assert (tmp_path / "t.king.cutoff.out.id").read_bytes() == b"#FID\tIID\nF1\tb\n"
    assert [p.rsplit("/", 1)[1] for p in paths] == ["t.king.cutoff.in.id", "t.king.cutoff.out.id"]


@pytest.mark.parametrize("missing", [0.0, 0.03])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_pedigree_plausibility(seed, missing):
    """Two unrelated parents, two children by free recombination, one unrelated individual and a duplicate of the first child
    over 20 000 independent SNPs with ALT frequencies uniform in [0.05, 0.5]: the duplicate is exactly 0.5, first-degree pairs
    are near 0.25, unrelated pairs near 0.  Tolerance 0.02, set when the definition was written (then: a little over twice the
    worst deviation of its own draw of this pedigree, 0.0061 first-degree and 0.0082 unrelated).  This generator's draws, seeds 0
    to 4 with and without 3 % missing calls, are off by at most 0.0092 (first-degree) and 0.0164 (unrelated): the estimator's
    standard deviation over 20 000 SNPs is about 0.006, and the ten panels hold sixty unrelated pairs."""
    from ld_tools_amd import sample_counts_host

    rng = np.random.default_rng(seed)
    n = 20000
    f = rng.uniform(0.05, 0.5, size=n)
    founder = lambda: (rng.random((n, 2)) < f[:, None]).astype(np.int8)  # noqa: E731
    p1, p2, other = founder(), founder(), founder()

    def child():
        pick1, pick2 = rng.integers(0, 2, size=n), rng.integers(0, 2, size=n)
        return np.stack([p1[np.arange(n), pick1], p2[np.arange(n), pick2]], axis=1)

    c1, c2 = child(), child()
    codes = np.concatenate([p1, p2, c1, c2, other, c1.copy()], axis=1)       # individuals 0 .. 5
    if missing:
        gone = rng.random((n, 6)) < missing
        codes[np.repeat(gone, 2, axis=1)] = 2
    kin, _ = cells(sample_counts_host(codes))
    assert kin[2, 5] == np.float32(0.5) and kin[5, 2] == np.float32(0.5)
    assert np.array_equal(bits(kin), bits(kin.T))
    first_degree = [(0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 5), (1, 5), (3, 5)]
    unrelated = [(0, 1), (0, 4), (1, 4), (2, 4), (3, 4), (4, 5)]
    worst1 = max(abs(float(kin[a, b]) - 0.25) for a, b in first_degree)
    worst0 = max(abs(float(kin[a, b])) for a, b in unrelated)
    print(f"seed {seed} missing {missing}: first-degree off by {worst1:.4f}, unrelated by {worst0:.4f}")
    assert worst1 < 0.02 and worst0 < 0.02

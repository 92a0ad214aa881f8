"""CPU: the host side of the genetic relationship matrix (include/ldx.h, "weighted sample products"): the numpy mirror of the
weighted sums against a Python-integer loop, the coefficients on hand-checked SNPs, the shared exponent, the cell, the writers,
the cutoff, and the definition against the exact GRM of the unquantised weights."""
from fractions import Fraction

import numpy as np
import pytest

from ld_grm_exact import EDGES, MAX_W, edge_weights, exact_grm, loop_wprod, panel_codes


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("holes", ["none", "3%", "50%"])
def test_wprod_mirror_equals_the_integer_loop(holes):
    from ld_tools_amd import sample_wprod_host

    for n_ind, n_snps in ((1, 5), (7, 150), (12, 40)):
        codes = panel_codes(n_ind, n_snps, seed=5 + n_ind, holes=holes)
        q = edge_weights(n_snps, seed=n_snps)
        keep = np.random.default_rng(n_ind).random(n_snps) < 0.8
        for k in (None, keep):
            got = sample_wprod_host(codes, q, keep=k)
            assert got.dtype == np.int64 and got.tolist() == loop_wprod(codes, q, k)
            assert np.array_equal(got, got.T)
    assert max(abs(e) for e in EDGES) == MAX_W and {127, 128, -128, -129} <= set(EDGES)


def test_weights_on_hand_checked_snps():
    """counts {n, het, hom}; s = het + 2 hom, p = s / 2n, (w, -2pw, 4p^2 w), w = 1 / (2p(1 - p)).
         0  monomorphic REF   (10, 0, 0)   s = 0            not live
         1  monomorphic ALT   (10, 0, 10)  s = 2n           not live
         2  singleton         (10, 1, 0)   p = 1/20         w = 200/19, -2pw = -20/19, 4p^2 w = 2/19
         3  all het           (10, 10, 0)  p = 1/2          w = 2, -2pw = -2, 4p^2 w = 2
         4  not kept          (10, 4, 2)                    not live (keep)
         5  n = 0             (0, 0, 0)                     not live
         6  p = 1/4           (8, 4, 0)                     w = 8/3, -2pw = -4/3, 4p^2 w = 2/3
    The largest value is 200/19 = 10.53: e = 4, unit 2^(4 - 28)."""
    from ld_tools_amd import grm_weights

    counts = np.array([[10, 0, 0, 0], [10, 0, 10, 0], [10, 1, 0, 0], [10, 10, 0, 0], [10, 4, 2, 0], [0, 0, 0, 0], [8, 4, 0, 0]],
                      dtype=np.uint32)
    keep = np.array([1, 1, 1, 1, 0, 1, 1], dtype=bool)
    q, e, live = grm_weights(counts, keep=keep)
    assert e == 4 and live.dtype == np.uint8 and live.tolist() == [0, 0, 1, 1, 0, 0, 1]
    assert q.dtype == np.int32 and q.shape == (7, 3) and not q[[0, 1, 4, 5]].any()
    unit = Fraction(1, 1 << 24)
    want = {2: (Fraction(200, 19), Fraction(-20, 19), Fraction(2, 19)), 3: (2, -2, 2), 6: (Fraction(8, 3), Fraction(-4, 3), Fraction(2, 3))}
    for i, xs in want.items():
        for k, x in enumerate(xs):
            assert abs(int(q[i, k]) * unit - x) <= unit / 2 + Fraction(1, 1 << 48), (i, k)
    assert q[3].tolist() == [1 << 25, -(1 << 25), 1 << 25]                      # exact values: no rounding at all
    # the same counts as geno_snp_counts hands them over (int32 words), and without the mask SNP 4 is live: p = 2/5
    q2, e2, live2 = grm_weights(counts.view(np.int32))
    assert e2 == 4 and live2.tolist() == [0, 0, 1, 1, 1, 0, 1] and np.array_equal(q2[[2, 3, 6]], q[[2, 3, 6]])
    # MAF exactly at the threshold stays: SNP 2 has MAF 1/20 = 0.05, SNP 6 has 1/4
    assert grm_weights(counts, keep=keep, maf_min=0.05)[2].tolist() == [0, 0, 1, 1, 0, 0, 1]
    assert grm_weights(counts, keep=keep, maf_min=0.25)[2].tolist() == [0, 0, 0, 1, 0, 0, 1]
    assert grm_weights(counts, keep=keep, maf_min=np.nextafter(0.25, 1.0))[2].tolist() == [0, 0, 0, 1, 0, 0, 0]
    # the minor allele may be the REF one: (10, 1, 9) has s = 19, MAF 1/20
    assert grm_weights(np.array([[10, 1, 9, 0]], dtype=np.uint32), maf_min=0.05)[2].tolist() == [1]
    # no live SNP at all: e = 0, all zero
    q0, e0, live0 = grm_weights(counts[[0, 1, 5]])
    assert e0 == 0 and not q0.any() and not live0.any()


def test_shared_exponent_at_a_power_of_two():
    """All-het SNPs give (2, -2, 2) exactly: the largest value IS 2^1, so e = 1 (2 x 2^-1 <= 1) and |q| = 2^28, the bound itself;
    a given exponent is used as it is, and one that does not cover the values is refused."""
    from ld_tools_amd import LdxError, grm_weights
    from ld_tools_amd.ops import grm_exponent

    counts = np.array([[6, 6, 0, 0], [9, 9, 0, 0]], dtype=np.uint32)
    q, e, _ = grm_weights(counts)
    assert e == 1 and q.tolist() == [[MAX_W, -MAX_W, MAX_W]] * 2
    assert [grm_exponent(x) for x in (0.0, 1.0, 1.5, 2.0, np.nextafter(2.0, 3.0), 0.25, 0.3)] == [0, 0, 1, 1, 2, -2, -1]
    q, e, _ = grm_weights(counts, exp=3)
    assert e == 3 and q.tolist() == [[1 << 26, -(1 << 26), 1 << 26]] * 2
    with pytest.raises(LdxError):
        grm_weights(counts, exp=0)


def test_cell_mirror():
    from ld_tools_amd import grm_cell_host

    S = np.array([[3 << 24, -(5 << 24)], [1, (1 << 58) + 1]], dtype=np.int64)
    N = np.array([[3, 2], [0, 7]], dtype=np.int64)
    got = grm_cell_host(S, N, 4)
    assert got.dtype == np.float32 and got[0, 0] == np.float32(1.0) and got[0, 1] == np.float32(-2.5)
    assert bits(got)[1, 0] == bits(np.float32(-0.0)) and np.signbit(got[1, 0])
    assert got[1, 1] == np.float32(float((1 << 58) + 1) * 2.0 ** -24 / 7.0)


def test_writers_round_trip(tmp_path):
    from ld_tools_amd import GrmResult
    from ld_tools_amd.drivers.grm import GrmTable, write_grm_bin, write_grm_cutoff, write_rel

    rng = np.random.default_rng(3)
    n = 5
    S = rng.integers(-(1 << 30), 1 << 30, size=(n, n))
    S = np.tril(S) + np.tril(S, -1).T
    N = rng.integers(1, 50, size=(n, n))
    N = np.tril(N) + np.tril(N, -1).T
    N[3, 1] = N[1, 3] = 0
    fid, iid = [f"F{k // 2}" for k in range(n)], [f"I{k}" for k in range(n)]
    table = GrmTable(fid, iid, GrmResult(S.astype(np.int64), N.astype(np.int64), 5, 40))
    grm = table.grm()
    base = str(tmp_path / "t")
    assert write_grm_bin(base, table) == [base + ".grm.bin", base + ".grm.N.bin", base + ".grm.id"]
    low = [(a, b) for a in range(n) for b in range(a + 1)]
    vals, cnts = np.fromfile(base + ".grm.bin", dtype="<f4"), np.fromfile(base + ".grm.N.bin", dtype="<f4")
    assert vals.size == cnts.size == n * (n + 1) // 2
    assert np.array_equal(bits(vals), bits([grm[a, b] for a, b in low])) and cnts.tolist() == [float(N[a, b]) for a, b in low]
    assert np.signbit(vals[low.index((3, 1))])
    assert open(base + ".grm.id").read() == "".join(f"{f}\t{i}\n" for f, i in zip(fid, iid))
    assert write_rel(base, table) == [base + ".rel", base + ".rel.id"]
    rows = open(base + ".rel").read().split("\n")[:-1]
    assert [len(r.split("\t")) for r in rows] == [1, 2, 3, 4, 5]
    for a, r in enumerate(rows):
        assert r.split("\t") == [f"{float(grm[a, b]):.6g}" for b in range(a + 1)]
    assert open(base + ".rel.id").read() == "#FID\tIID\n" + "".join(f"{f}\t{i}\n" for f, i in zip(fid, iid))
    paths = write_grm_cutoff(base, table, 1e30)
    assert open(paths[0]).read() == open(base + ".rel.id").read() and open(paths[1]).read() == "#FID\tIID\n"


def test_cutoff_on_a_hand_made_matrix():
    """Edges are the pairs ABOVE 0.0625: 0-1, 0-2, 3-4 (2-5 sits on the cutoff: no edge).  Degrees 2 1 1 1 1 0: the rank is
    5, 1, 2, 3, 4, 0 -- 1 and 2 stay and remove 0, 3 stays and removes 4."""
    from ld_tools_amd import grm_cutoff

    g = np.zeros((6, 6), dtype=np.float32)
    for a, b, v in ((0, 1, 0.5), (0, 2, 0.07), (3, 4, 0.25), (2, 5, 0.0625), (1, 4, -0.3)):
        g[a, b] = g[b, a] = v
    np.fill_diagonal(g, 1.0)
    keep, why = grm_cutoff(g, 0.0625)
    assert keep.tolist() == [False, True, True, True, False, True] and why.tolist() == [1, -1, -1, -1, 3, -1]


@pytest.mark.parametrize("holes", ["none", "3%", "50%"])
def test_definition_within_the_derived_bound_of_the_exact_grm(holes):
    """How far the fixed-point GRM may lie from the GRM of the exact rational weights.

    Per live SNP the three coefficients x = (w, -2pw, 4p^2 w) are rounded to q 2^(e - 28): |q 2^(e - 28) - x~| <= 2^(e - 29),
    x~ the fp64 value.  In a pair's term they multiply g_a g_b <= 4, g_a + g_b <= 4 and 1, so the term moves by at most
    (4 + 4 + 1) 2^(e - 29) and
        |S 2^(e - 28) - sum of the exact terms| <= 9 n_live 2^(e - 29)                                    (the issue's bound)
    (n_live bounds the SNPs called in both).  x~ itself carries the fp64 roundings of p, 1 - p, the product, the reciprocal and
    two more products: a relative error below (2 n + 8) 2^-53 (the subtraction 1 - p inherits p's rounding magnified by
    p / (1 - p) <= 2 n), on |x| <= 2^e: 9 n_live 2^e (2 n + 8) 2^-53 more.  The sum is divided by N_ab; the cell then rounds once
    in fp64 (the conversion of S is exact below 2^53, the scaling exact, the division rounds: 2^-53 relative) and once to
    float32 (2^-24 relative).  Measured: the largest |error| / bound over these panels is printed (0.12 to 0.15: the rounding
    errors of the live SNPs do not all point one way)."""
    from ld_tools_amd import ld_grm_host

    worst = Fraction(0)
    for n_ind, n_snps, maf in ((9, 120, None), (14, 60, Fraction(1, 10))):
        codes = panel_codes(n_ind, n_snps, seed=70 + n_ind, holes=holes)
        keep = np.random.default_rng(n_snps).random(n_snps) < 0.9
        res = ld_grm_host(codes, keep=keep, maf_min=None if maf is None else float(maf))
        want, N, n_live = exact_grm(codes, keep, maf)
        assert res.n_live == n_live and res.N.tolist() == N
        got = res.grm()
        two_e = Fraction(2) ** res.exp
        dS = 9 * n_live * (two_e / (1 << 29) + two_e * (2 * n_ind + 8) / (1 << 53))
        for a in range(n_ind):
            for b in range(n_ind):
                if N[a][b] == 0:
                    assert want[a][b] is None and bits(got[a, b]) == bits(np.float32(-0.0))
                    continue
                tol = dS / N[a][b]
                tol += (abs(want[a][b]) + tol) * (Fraction(1, 1 << 53) + Fraction(1, 1 << 24))
                err = abs(Fraction(float(got[a, b])) - want[a][b])
                assert err <= tol, (a, b, float(err), float(tol))
                worst = max(worst, err / tol)
    print(f"holes {holes}: largest |error| / bound = {float(worst):.4f}")
    assert worst > 0


def test_device_entries_fail_loudly_without_gpu():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    import ld_tools_amd as L

    q = np.zeros((4, 3), dtype=np.int32)
    for call in (lambda: L.sample_wprod(None, q), lambda: L.ld_grm(None),
                 lambda: L.ld_grm_from_sums(np.zeros((2, 2), dtype=np.int64), np.ones((2, 2), dtype=np.int64), 0)):
        with pytest.raises(L.LdxError):
            call()

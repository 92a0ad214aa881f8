"""CPU: the banded matrix-vector surface without a GPU -- ABI, the host term function, the column scaling, argument checks
and the conjugate-gradient logic with a host product injected."""
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


def test_matvec_symbols_declared_exported_and_bound():
    from ld_tools_amd import _lib
    header = (ROOT / "include" / "ldx.h").read_text()
    for name in ("ldx_ld_matvec_workspace_bytes", "ldx_ld_matvec_dev"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["ldx_ld_matvec_dev"][1]) == 17
    assert _lib.lib.ldx_version() == 102          # additive symbols: the ABI number stays


def test_workspace_bytes_is_pure_arithmetic():
    from ld_tools_amd import _lib
    lib = _lib.lib
    prev = 0
    for n in (1, 2, 127, 128, 129, 10_000, 100_000, 600_000):
        b = lib.ldx_ld_matvec_workspace_bytes(n, 5008)
        assert b % 256 == 0 and b >= n + 1024
        assert b == lib.ldx_ld_matvec_workspace_bytes(n, 1)            # the haplotype count does not enter
        assert b >= prev                                                # monotone in the SNP count
        prev = b
    assert lib.ldx_ld_matvec_workspace_bytes(0, 1) == lib.ldx_ld_matvec_workspace_bytes(1, 1)


def test_prod_terms_at_the_edges():
    from ld_tools_amd.ops import prod_terms, prod_values
    one = 1 << 40
    assert prod_terms(f32(1.0), f32(1.0)) == one and prod_terms(f32(1.0), f32(-1.0)) == -one
    assert prod_terms(f32(-1.0), f32(-1.0)) == one
    assert prod_terms(f32(0.5), f32(0.25)) == one >> 3
    # zeros of either sign, on either side: 0 (the -0.0f cell of a degenerate SNP adds nothing in both directions)
    for v in (f32(0.0), f32(-0.0)):
        for x in (f32(0.0), f32(-0.0), f32(1.0), f32(-0.75)):
            assert prod_terms(v, x) == 0 and prod_terms(x, v) == 0
    out = prod_terms(f32(0.3), np.array([0.1, -0.2], dtype=f32))
    assert out.dtype == np.int64 and out.shape == (2,)
    # exact halves round to even: 2^40 v x = 0.5, 1.5, 2.5, -0.5, -1.5
    for num, want in ((1, 0), (3, 2), (5, 2), (-1, 0), (-3, -2), (7, 4)):
        assert prod_terms(f32(2.0 ** -20), f32(num * 2.0 ** -21)) == want, num
    # products below 2^-41 vanish, just above round to 1
    assert prod_terms(f32(2.0 ** -21), f32(2.0 ** -21)) == 0
    assert prod_terms(f32(2.0 ** -30), f32(-(2.0 ** -30))) == 0
    assert prod_terms(f32(2.0 ** -20), f32(np.nextafter(f32(2.0 ** -21), f32(1)))) == 1
    # the clamp at +-2^22 (only reachable far outside |x|, |c| <= 1)
    assert prod_terms(f32(4096.0), f32(4096.0)) == 1 << 62
    assert prod_terms(f32(-4096.0), f32(4096.0)) == -(1 << 62)
    assert prod_terms(f32(2048.0), f32(2048.0)) == 1 << 62
    assert prod_terms(f32(2048.0), f32(1024.0)) == 1 << 61
    assert prod_terms(f32(3e38), f32(3e38)) == 1 << 62 and prod_terms(f32(3e38), f32(-3e38)) == -(1 << 62)
    # power 2 multiplies the float32 square, one float32 multiply -- not the fp64 square
    r = f32(0.7)
    v = prod_values(r, 2)
    assert v.dtype == np.float32 and v == f32(r * r)
    assert np.float64(v) != np.float64(r) ** 2
    assert prod_terms(v, f32(1.0)) == int(np.rint(np.ldexp(np.float64(f32(r * r)), 40)))
    assert prod_terms(v, f32(1.0)) != int(np.rint(np.ldexp(np.float64(r) ** 2, 40)))
    assert prod_values(r, 1) == r
    with pytest.raises(Exception):
        prod_values(r, 3)


def test_fp64_product_of_two_float32_is_exact():
    """The contract's 'ONE rounding': v x in fp64 is the exact product, 2^40 v x the exact scaling, so the term is the
    round-half-even of the exact rational -- checked against Python fractions."""
    from ld_tools_amd.ops import prod_terms
    rng = np.random.default_rng(7)
    v = (rng.standard_normal(4000) * np.exp2(rng.integers(-30, 2, 4000))).astype(f32)
    x = (rng.uniform(-1, 1, 4000) * np.exp2(rng.integers(-24, 1, 4000))).astype(f32)
    got = prod_terms(v, x)
    for a, b, g in zip(v.tolist(), x.tolist(), got.tolist()):
        exact = Fraction(a) * Fraction(b)
        assert Fraction(float(np.float64(a) * np.float64(b))) == exact
        assert g == round(exact * (1 << 40))      # Python rounds halves to even
        assert abs(Fraction(g, 1 << 40) - exact) <= Fraction(1, 1 << 41)


def test_column_scaling_round_trips():
    import torch

    from ld_tools_amd.ops import LDProduct, matvec_rhs
    rng = np.random.default_rng(3)
    n = 500
    x = (rng.standard_normal((n, 6)) * np.array([1e-12, 1.0, 37.5, 1e9, 2.0 ** -3, 1.0])).astype(f32)
    x[:, 5] = 0.0                                 # an all-zero column stays as it is
    x[3, 4] = 0.125 * 8                           # column 4's maximum an exact power of two
    x[:, 4] = np.clip(x[:, 4], -1.0, 1.0)
    x32, e, squeeze = matvec_rhs(x, n)
    assert not squeeze and x32.dtype == torch.float32 and x32.shape == (n, 6) and x32.is_contiguous()
    assert e.dtype == torch.int64 and e[5] == 0 and e[4] == 0    # a column with max |x| = 1 is not scaled
    big = x32.abs().amax(dim=0).numpy()
    assert (big[:5] > 0.5).all() and (big <= 1.0).all() and big[4] == 1.0 and big[5] == 0.0
    # float32 in: the scaling is exact, so scaling back gives the input bit for bit
    back = LDProduct(torch.zeros((n, 6), dtype=torch.int64), e, x32, 0, 1).x().numpy()
    assert back.dtype == np.float64 and np.array_equal(back, x.astype(np.float64))
    assert np.array_equal(back.astype(f32).view(np.int32), x.view(np.int32))
    # float64 in: converted after the scaling -- one rounding of x 2^-e, no overflow or underflow on the way
    x64 = rng.standard_normal((n, 2)) * np.array([1e200, 1e-200])
    x32, e, _ = matvec_rhs(x64, n)
    assert np.array_equal(x32.numpy(), np.ldexp(x64, -e.numpy()).astype(f32))
    assert (x32.abs().amax(dim=0) > 0.5).all() and (x32.abs().amax(dim=0) <= 1.0).all()
    # values(): sums 2^(e - 40)
    sums = torch.tensor([[1 << 40, -(1 << 39)]] * n, dtype=torch.int64)
    y = LDProduct(sums, torch.tensor([3, -2]), x32, 0, 1).values().numpy()
    assert np.array_equal(y[0], [8.0, -0.125])
    # one-dimensional x
    x32, e, squeeze = matvec_rhs(x[:, 1], n)
    assert squeeze and x32.shape == (n, 1)
    assert LDProduct(torch.zeros((n, 1), dtype=torch.int64), e, x32, 0, 1, squeeze).values().shape == (n,)
    # torch tensors go the same way
    x32t, et, _ = matvec_rhs(torch.as_tensor(x), n)
    x32n, en, _ = matvec_rhs(x, n)
    assert torch.equal(x32t, x32n) and torch.equal(et, en)


def test_rhs_rejections():
    from ld_tools_amd import LdxError
    from ld_tools_amd.ops import matvec_rhs
    n = 40
    ok = np.ones((n, 3), dtype=f32)
    for bad in (np.nan, np.inf, -np.inf):
        x = ok.copy()
        x[7, 1] = bad
        with pytest.raises(LdxError, match="finite"):
            matvec_rhs(x, n)
    with pytest.raises(LdxError, match="shape"):
        matvec_rhs(ok[:-1], n)
    with pytest.raises(LdxError, match="shape"):
        matvec_rhs(np.ones((n, 2, 2)), n)
    with pytest.raises(LdxError, match="right-hand sides"):
        matvec_rhs(np.ones((n, 0)), n)
    with pytest.raises(LdxError, match="right-hand sides"):
        matvec_rhs(np.ones((n, 9)), n)
    with pytest.raises(LdxError, match="power"):
        matvec_rhs(ok, n, power=3)
    with pytest.raises(LdxError, match="power"):
        matvec_rhs(ok, n, power=0)
    with pytest.raises(LdxError, match="real"):
        matvec_rhs(np.ones((n, 1), dtype=np.complex128), n)
    matvec_rhs(np.ones((n, 8)), n, power=2)


def host_product(R):
    """cg_solve's product callable over a dense host matrix, with the float32 rounding of the direction ld_matvec does."""
    import torch

    from ld_tools_amd.ops import LDProduct, matvec_rhs
    Rt = torch.as_tensor(R)
    calls = []

    def product(p):
        x32, e, _ = matvec_rhs(p, p.shape[0], 1, False)
        q = LDProduct(None, e, x32, 0, 1).x()
        calls.append(p.shape[1])
        return Rt @ q, q
    return product, calls


def test_cg_converges_on_a_small_spd_matrix():
    import torch

    from ld_tools_amd.ops import cg_solve
    rng = np.random.default_rng(11)
    n, h, k = 120, 300, 4
    G = rng.standard_normal((n, h))
    G -= G.mean(axis=1, keepdims=True)
    G /= np.sqrt((G * G).sum(axis=1, keepdims=True))
    R = G @ G.T                                   # a correlation matrix
    lam = 0.1
    z = rng.standard_normal((n, k))
    z[:, 2] = 0.0                                 # an all-zero column: beta = 0 at once
    z[:, 3] *= 1e6                                # the columns have their own scales and step sizes
    product, calls = host_product(R)
    res = cg_solve(product, torch.as_tensor(z), lam, tol=1e-8, max_iter=500, batch=4)
    assert res.converged.all() and not res.indefinite.any()
    assert res.iterations[2] == 0 and (res.iterations[[0, 1, 3]] > 3).all()
    assert len(calls) % 4 == 0 and len(calls) < 500 and set(calls) == {k}     # one product per iteration for all columns
    beta = res.beta.numpy()
    A = R + lam * np.eye(n)
    for c in (0, 1, 3):
        true = np.linalg.norm(A @ beta[:, c] - z[:, c]) / np.linalg.norm(z[:, c])
        assert true <= 2e-8 and res.residual[c] <= 1e-8, (c, true)
        assert np.allclose(beta[:, c], np.linalg.solve(A, z[:, c]), rtol=1e-6, atol=1e-7 * np.abs(beta[:, c]).max())
    assert (beta[:, 2] == 0).all()
    # a column that has converged keeps its beta while the others go on
    easy = np.zeros((n, 2))
    easy[:, 0] = np.linalg.eigh(A)[1][:, -1]      # an eigenvector: one step
    easy[:, 1] = z[:, 0]
    res2 = cg_solve(host_product(R)[0], torch.as_tensor(easy), lam, tol=1e-8, max_iter=500, batch=4)
    assert res2.converged.all() and res2.iterations[0] <= 2 < res2.iterations[1]
    # max_iter is a hard stop: not converged, no exception
    res3 = cg_solve(host_product(R)[0], torch.as_tensor(z[:, :1]), lam, tol=1e-12, max_iter=3, batch=4)
    assert not res3.converged[0] and res3.iterations[0] == 3 and not res3.indefinite[0]


def test_cg_reports_an_indefinite_matrix():
    import torch

    from ld_tools_amd.ops import cg_solve
    rng = np.random.default_rng(5)
    n = 60
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    ev = np.linspace(0.5, 2.0, n)
    ev[0] = -0.7
    R = (Q * ev) @ Q.T
    assert np.linalg.eigvalsh(R).min() < -0.5
    z = rng.standard_normal((n, 2))
    z[:, 1] = Q[:, -1]                            # an eigenvector of a positive eigenvalue: this column is solvable
    res = cg_solve(host_product(R)[0], torch.as_tensor(z), 0.0, tol=1e-8, max_iter=400, batch=4)
    assert res.indefinite[0] and not res.converged[0] and np.isnan(res.beta.numpy()[:, 0]).all()
    assert res.converged[1] and not res.indefinite[1]
    assert np.allclose(res.beta.numpy()[:, 1], Q[:, -1] / ev[-1], atol=1e-7)


def test_ld_matvec_and_ridge_need_a_gpu(monkeypatch):
    import torch

    from ld_tools_amd import LdxError, ld_matvec, ld_ridge
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(LdxError, match="HIP device"):
        ld_matvec(None, [1.0, 2.0, 3.0], [1, 2, 3])
    with pytest.raises(LdxError, match="HIP device"):
        ld_ridge(None, [1.0, 2.0, 3.0], [1, 2, 3])

"""CPU: stored LD bands -- the host mirror of the layout, the ABI of the new entries and the argument rules that are checked
before a device is touched (ops.band_layout_host, ops.ld_band, ops.ld_cross_score, LDBand.matvec; include/ldx.h, "stored
bands").  No kernel is launched here."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ld_band_cases as bc  # noqa: E402
import ld_exact as lx  # noqa: E402

NEW_SYMBOLS = ["ldx_ld_band_layout_dev", "ldx_ld_band_workspace_bytes", "ldx_ld_band_dev", "ldx_ld_band_dosage_dev",
               "ldx_band_score_dev", "ldx_band_matvec_dev"]


def brute_layout(pos, w):
    """lo and offsets by the definition: a double loop."""
    n = len(pos)
    lo = np.zeros(n, dtype=np.uint32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    for i in range(n):
        j = i
        while j > 0 and int(pos[i]) - int(pos[j - 1]) <= w:
            j -= 1
        lo[i] = j
        offsets[i + 1] = offsets[i] + np.uint64(i - j)
    return lo, offsets


def layout_cases():
    cases = []
    for n in (1, 2, 5, 129, 300):
        cases += [(pos, w) for pos, w in lx.score_windows(n, n)]
        grid = 1 + 100 * np.arange(n, dtype=np.int64)
        cases.append((grid, 0))                                           # window 0
        cases.append((np.repeat(np.arange(1, n // 3 + 2), 3)[:n].astype(np.int64), 0))   # duplicate positions
        cases.append((np.repeat(np.arange(1, n // 3 + 2), 3)[:n].astype(np.int64), 1))
        cases.append((grid, 10 * int(grid[-1]) + 5))                      # wider than the panel
        cases.append((grid, 1 << 60))                                     # beyond 2^52: acts as 2^52
    return cases


def test_band_layout_host_is_the_definition():
    from ld_tools_amd import ops
    for pos, w in layout_cases():
        n = len(pos)
        lo, offsets = ops.band_layout_host(pos, w)
        blo, boff = brute_layout(pos, min(w, 1 << 52))
        assert lo.dtype == np.uint32 and offsets.dtype == np.uint64 and lo.shape == (n,) and offsets.shape == (n + 1,)
        assert np.array_equal(lo, blo) and np.array_equal(offsets, boff), (n, w)
        assert int(offsets[n]) == int(np.tril(lx.window_mask(pos, min(w, 1 << 52)), -1).sum())
        if w >= int(pos[-1]) - int(pos[0]):
            assert int(offsets[n]) == n * (n - 1) // 2 and not lo.any()
        if w == 0 and (np.diff(pos) > 0).all():
            assert int(offsets[n]) == 0 and np.array_equal(lo, np.arange(n))
    with pytest.raises(ops._lib.LdxError, match="non-decreasing"):
        ops.band_layout_host([3, 2, 5], 1)
    with pytest.raises(ops._lib.LdxError, match=">= 0"):
        ops.band_layout_host([1, 2, 5], -1)


def matrix_layout(pos, w, block=512):
    """lo[i] = min{j <= i : pos_i - pos_j <= w} from the n x n comparison (in row blocks), offsets its running sum."""
    n = len(pos)
    lo = np.empty(n, dtype=np.uint32)
    cols = np.arange(n)
    for r0 in range(0, n, block):
        rows = np.arange(r0, min(r0 + block, n))
        inside = ((pos[rows, None] - pos[None, :]) <= w) & (cols[None, :] <= rows[:, None])
        lo[rows] = inside.argmax(axis=1)                                  # the first True of the row
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.arange(n, dtype=np.int64) - lo.astype(np.int64)).astype(np.uint64)
    return lo, offsets


def test_band_layout_host_is_the_definition_past_one_tile():
    """The position cases of the GPU layout test (tests/ld_band_cases.py) at 4097 SNPs -- one more than the layout kernel's
    tile -- against the n x n definition: the host mirror is what the device layout is compared with."""
    from ld_tools_amd import ops
    n = 4097
    cases = bc.position_cases(n)
    assert len(cases) == 9
    for pos, w in cases:
        assert pos.dtype == np.int64 and pos.shape == (n,) and (np.diff(pos) >= 0).all()
        lo, offsets = ops.band_layout_host(pos, w)
        mlo, moff = matrix_layout(pos, min(w, 1 << 52))
        assert np.array_equal(lo, mlo) and np.array_equal(offsets, moff), w
    windows = sorted({w for _, w in cases})
    assert windows[0] == 0 and windows[-1] == 1 << 62 and max(int(p[-1]) for p, _ in cases) > 1 << 50


def test_the_sweep_cases_and_cells_cover_what_they_must():
    """Conditions on the INPUTS of the GPU tests of the two consumers and the store (tests/test_gpu_ld_band.py): the reaches,
    the jump of lo inside a 16-row group, the clamp and a wrapping sum.  If one fails, the seed or the share of big cells
    changes -- not the condition."""
    from ld_tools_amd import ops
    n = 4500
    cases = bc.sweep_cases(n)
    assert len(cases) == 3
    reach_max, jump_with_reach = 0, False
    for pos, w in cases:
        lo, off = ops.band_layout_host(pos, w)
        lo = lo.astype(np.int64)
        reach = np.arange(n) - lo
        reach_max = max(reach_max, int(reach.max()))
        assert reach.max() > bc.SWEEP_SPAN                                # every case walks a second span
        first = lo[0::bc.SWEEP_ROWS]
        last = lo[np.minimum(np.arange(0, n, bc.SWEEP_ROWS) + bc.SWEEP_ROWS - 1, n - 1)]
        jump_with_reach |= bool(((last > first) & (reach[0::bc.SWEEP_ROWS] > bc.SWEEP_SPAN)).any())
    assert reach_max > 2 * bc.SWEEP_SPAN                                  # ... and one a third
    assert jump_with_reach
    # the grid with 2100 SNPs each side: after the first rows no group's first column is a multiple of the span
    lo = ops.band_layout_host(*cases[1])[0].astype(np.int64)
    jmin = lo[0::bc.SWEEP_ROWS]
    assert (jmin > 0).any() and (jmin[jmin > 0] % bc.SWEEP_SPAN != 0).all() and (np.arange(n) - lo).max() == 2100
    # clustered, window 0: lo jumps at a row that is no multiple of 16
    lo = ops.band_layout_host(*cases[2])[0].astype(np.int64)
    jumps = np.flatnonzero(np.diff(lo) > 0) + 1
    assert jumps.size and (jumps % bc.SWEEP_ROWS != 0).any() and (np.arange(n) - lo).max() == 2499
    # the cells: specials present, nothing non-finite; big: terms at the clamp and a power-1 sum that wraps
    pos, w = cases[2]
    lo, off = ops.band_layout_host(pos, w)
    rows, cols = bc.cell_rows_cols(lo, off)
    assert rows.size == int(off[n]) and (cols < rows).all() and (cols >= lo[rows]).all()
    plain = bc.synthetic_cells(rows.size, seed=bc.CELL_SEEDS[2])
    pb = plain.view(np.uint32)
    assert (np.abs(plain) <= 1).all() and (pb == 0).any() and (pb == 0x80000000).any() and (plain == 1).any() and (plain == -1).any()
    assert ((np.abs(plain) > 0) & (np.abs(plain) < 2.0 ** -19)).any()
    big = bc.synthetic_cells(rows.size, seed=bc.CELL_SEEDS[2], big=True)
    assert np.isfinite(big).all() and 0 < int((np.abs(big) >= 2.0 ** 22).sum()) < rows.size // 1024
    for v in (2.0 ** 22, 2.0 ** 23, 2.0 ** 30):
        assert (big == v).any() and (big == -v).any()
    from test_gpu_exact_oracle import rhs
    x32 = ops.matvec_rhs(rhs(n, n), n)[0].numpy()[:, 1]                   # the GPU test's right-hand sides; column 1: uniform
    t_row, t_col = ops.prod_terms(big, x32[cols]), ops.prod_terms(big, x32[rows])
    assert int((np.abs(t_row) == 1 << 62).sum()) > 0 and int((np.abs(t_col) == 1 << 62).sum()) > 0
    wrapped = np.zeros(n, dtype=np.int64)
    with np.errstate(over="ignore"):
        np.add.at(wrapped, rows, t_row)
        np.add.at(wrapped, cols, t_col)
    # the same sums without wrapping: 32-bit halves added as int64 (4500 terms of 32 bits: no overflow), joined as Python ints
    hi, lo32 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for idx, t in ((rows, t_row), (cols, t_col)):
        np.add.at(hi, idx, t >> 32)
        np.add.at(lo32, idx, t & 0xFFFFFFFF)
    true = [(int(h) << 32) + int(l) for h, l in zip(hi, lo32)]
    assert all(s % (1 << 64) == int(wv) % (1 << 64) for s, wv in zip(true, wrapped))
    assert sum(1 for s in true if not -(1 << 63) <= s < (1 << 63)) >= 1


def test_cross_terms_are_one_float32_multiply_then_exact_scaling():
    from fractions import Fraction
    from ld_tools_amd import ops
    rng = np.random.default_rng(1)
    a = rng.uniform(-1.1, 1.1, 2000).astype(np.float32)
    b = rng.uniform(-1.1, 1.1, 2000).astype(np.float32)
    a[:4] = [0.0, -0.0, 1.0, -1.0]
    b[:4] = [-0.0, 0.5, -1.0, -1.0]
    t = ops.cross_terms(a, b)
    assert t.dtype == np.int64 and t[0] == 0 and t[1] == 0 and t[2] == -(1 << 32) and t[3] == 1 << 32
    for x, y, got in zip(a[:300], b[:300], t[:300]):
        p = Fraction(float(np.float32(x) * np.float32(y))) * (1 << 32)
        fl = p.numerator // p.denominator
        frac = p - fl
        want = fl + (1 if frac > Fraction(1, 2) or (frac == Fraction(1, 2) and fl % 2) else 0)
        assert int(got) == want
    assert np.array_equal(ops.cross_terms(a, a).astype(np.uint64), ops.score_terms(a))


def test_new_symbols_are_declared_bound_and_exported():
    from ld_tools_amd import _lib
    text = (ROOT / "include" / "ldx.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ldx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/ldx.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libldx.so"
    assert _lib.version() == 102                                           # new symbols only: no version bump
    assert "#define LDX_VERSION 102" in (ROOT / "include" / "ldx.h").read_text().replace("  ", " ")
    import ld_tools_amd
    for name in ("ld_band", "LDBand", "ld_cross_score", "band_layout_host"):
        assert name in ld_tools_amd.__all__ and hasattr(ld_tools_amd, name)
    lib = _lib.lib
    assert lib.ldx_ld_band_workspace_bytes(1000, 1008) == lib.ldx_ld_score_workspace_bytes(1000, 1008) > 0


def test_entries_refuse_bad_arguments_before_any_launch():
    """Argument rules of the C entries: every one of these returns before a device is touched."""
    from ld_tools_amd import _lib
    lib = _lib.lib
    E_ARG, E_UNSUPPORTED = -1, -3
    big = C.create_string_buffer(4096 + 256)
    ptr = (C.addressof(big) + 255) // 256 * 256   # a non-null, 256-byte-aligned stand-in for every pointer (never read)
    need = lib.ldx_ld_band_workspace_bytes(100, 64)

    def band(n_hap=64, path=0, ws_bytes=None, n=100, dosage=False, window=10):
        ws_bytes = need if ws_bytes is None else ws_bytes
        if dosage:
            return lib.ldx_ld_band_dosage_dev(ptr, ptr, n, n_hap, ptr, window, path, ptr, ptr, ptr, 10, ptr, ws_bytes, None)
        return lib.ldx_ld_band_dev(ptr, ptr, ptr, ptr, ptr, n, n_hap, ptr, window, path, ptr, ptr, ptr, 10, ptr, ws_bytes, None)

    assert band(path=1) == E_UNSUPPORTED                                    # LDX_PATH_POPCOUNT
    assert band(n_hap=_lib.MAX_HAPS + 1) == E_UNSUPPORTED
    assert band(n=1 << 24, n_hap=10240, ws_bytes=1 << 40) == E_UNSUPPORTED  # a bit plane of 4 GiB or more
    assert band(ws_bytes=need - 1) == E_ARG and band(window=-1) == E_ARG and band(path=7) == E_ARG
    assert band(n_hap=63, dosage=True) == E_ARG                             # odd n_hap
    assert band(path=2, dosage=True) == E_UNSUPPORTED                       # the dosage form runs on FP4 only
    assert band(path=1, dosage=True) == E_UNSUPPORTED
    assert lib.ldx_ld_band_dev(None, ptr, ptr, ptr, ptr, 100, 64, ptr, 10, 0, ptr, ptr, ptr, 10, ptr, need, None) == E_ARG
    assert lib.ldx_ld_band_dev(ptr, ptr, ptr, ptr, ptr, 100, 64, ptr, 10, 0, ptr, ptr, None, 10, ptr, need, None) == E_ARG
    for n_rhs in (0, 9):
        assert lib.ldx_band_matvec_dev(ptr, ptr, ptr, ptr, 100, ptr, n_rhs, 1, ptr, None) == E_ARG
        assert "n_rhs" in lib.ldx_last_error().decode()
    for power in (0, 3):
        assert lib.ldx_band_matvec_dev(ptr, ptr, ptr, ptr, 100, ptr, 1, power, ptr, None) == E_ARG
        assert "power" in lib.ldx_last_error().decode()
    assert lib.ldx_band_score_dev(ptr, None, ptr, ptr, ptr, ptr, 100, ptr, None) == E_ARG
    assert lib.ldx_band_score_dev(ptr, ptr, ptr, ptr, ptr, ptr, 0, ptr, None) == E_ARG
    assert lib.ldx_ld_band_layout_dev(ptr, 100, -1, ptr, ptr, None) == E_ARG
    assert lib.ldx_ld_band_layout_dev(None, 100, 5, ptr, ptr, None) == E_ARG


def host_band(n, window, dosage=False, n_hap=64):
    """An LDBand over host tensors: enough for the checks that come before the device."""
    import torch
    from ld_tools_amd import ops
    pos = 1 + 100 * np.arange(n, dtype=np.int64)
    lo, off = ops.band_layout_host(pos, window)
    return ops.LDBand(torch.zeros(int(off[n]), dtype=torch.float32), torch.as_tensor(lo.view(np.int32)),
                      torch.as_tensor(off.view(np.int64)), torch.ones(n, dtype=torch.float32), pos, window, dosage, n_hap)


def test_python_argument_rules_come_before_the_device():
    import torch
    from ld_tools_amd import LdxError, PackedPanel, ops
    z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731
    odd = PackedPanel(10, 63, z(1, torch.uint8), z(1, torch.uint8), z(128, torch.int32), z(128, torch.int32),
                      z(128, torch.float64), z(128, torch.float64), z(128, torch.float64))
    with pytest.raises(LdxError, match="even n_hap"):
        ops.ld_band(odd, window_snps=3, dosage=True)
    a, b, c = host_band(50, 300), host_band(50, 500), host_band(49, 300)
    for other in (b, c):
        with pytest.raises(LdxError, match="layout"):
            ops.ld_cross_score(a, other)
    shifted = host_band(50, 300)
    shifted.positions = shifted.positions + 1
    with pytest.raises(LdxError, match="layout"):
        ops.ld_cross_score(a, shifted)
    with pytest.raises(LdxError, match="LDBand"):
        ops.ld_cross_score(a, None)
    x = np.ones((50, 9), dtype=np.float32)
    with pytest.raises(LdxError, match="right-hand sides"):
        a.matvec(x)
    with pytest.raises(LdxError, match="right-hand sides"):
        a.matvec(x[:, :0])
    for power in (0, 3):
        with pytest.raises(LdxError, match="power"):
            a.matvec(x[:, :2], power=power)
    with pytest.raises(LdxError, match="n_snps"):
        a.matvec(x[:49, :2])
    with pytest.raises(LdxError, match="haplotype band"):
        ops.ld_ridge(odd, np.ones(10), band=host_band(10, 300, dosage=True))
    with pytest.raises(LdxError, match="SNPs"):
        ops.ld_ridge(odd, np.ones(10), band=a)
    # the host views need no device either
    cols, r = a.row(7)
    assert np.array_equal(cols, [4, 5, 6]) and r.shape == (3,)
    d = a.to_dense((0, 6))
    assert d.shape == (6, 6) and np.array_equal(np.diagonal(d), np.ones(6, dtype=np.float32))
    indptr, indices, data = a.to_csr()
    assert indptr[-1] == 2 * a.n_cells + 50 and np.array_equal(indices[indptr[7]:indptr[8]], [4, 5, 6, 7, 8, 9, 10])

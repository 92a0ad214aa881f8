"""Signed-r cells (LDX_OUT_R32): the host-side constants and cell order -- no GPU needed."""
import numpy as np

from ld_tools_amd import _lib
from ld_tools_amd._lib import lib


def test_r32_format_constant():
    assert _lib.FORMATS["r32"] == 4
    assert "r32" not in _lib.ONE_MEASURE          # no rounded measure in it


def test_r32_cell_offset_is_the_k16_order():
    r8, c = np.meshgrid(np.arange(8), np.arange(128), indexing="ij")
    got = _lib.cell_offset(r8, c, "r32")
    assert np.array_equal(got, _lib.cell_offset(r8, c, "k16"))
    assert np.array_equal(np.sort(got.ravel()), np.arange(_lib.UNIT_PAIRS))
    assert _lib.cell_offset(5, 77, "r32") == _lib.cell_offset(5, 77, "k16")


def test_r32_cell_index_of_the_library():
    for n, i, j in [(2, 1, 0), (300, 299, 0), (300, 200, 129), (1000, 999, 998), (100_000, 99_999, 0),
                    (100_000, 99_999, 99_998), (100_000, 50_001, 12_345), (100_000, 128, 127)]:
        assert lib.ldx_triangle_cell_index(n, i, j, 4) == lib.ldx_triangle_cell_index(n, i, j, _lib.FORMATS["k16"])


def test_r_block_signature_is_bound():
    assert "ldx_triangle_r_block_dev" in _lib.SIGNATURES
    assert hasattr(lib, "ldx_triangle_r_block_dev")

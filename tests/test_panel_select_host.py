"""CPU: the host side of panel subsets -- the C entry is declared, exported and bound; index normalisation; the column
arithmetic of the group driver.  No kernel is launched here."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_entry_is_declared_exported_and_bound():
    from ld_tools_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ldx.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+ldx_panel_select_dev\s*\(([^)]*)\)", text)
    assert m, "ldx_panel_select_dev is not declared in include/ldx.h"
    n_args = len(m.group(1).split(","))
    assert n_args == 13
    assert hasattr(_lib.lib, "ldx_panel_select_dev")
    res, args = _lib.SIGNATURES["ldx_panel_select_dev"]
    assert len(args) == n_args
    assert _lib.version() == 102                      # additive symbol: the ABI number stays


def test_select_index_masks_and_lists():
    import torch

    from ld_tools_amd import select_index

    mask = np.array([0, 1, 1, 0, 1], dtype=bool)
    got = select_index(mask, 5, "haplotype")
    assert got.dtype == np.uint32 and got.tolist() == [1, 2, 4]
    assert select_index(torch.from_numpy(mask), 5, "haplotype").tolist() == [1, 2, 4]
    for idx in ([4, 0, 0, 3, 4], np.array([4, 0, 0, 3, 4], dtype=np.int64), np.array([4, 0, 0, 3, 4], dtype=np.uint8),
                torch.tensor([4, 0, 0, 3, 4])):
        got = select_index(idx, 5, "SNP")
        assert got.dtype == np.uint32 and got.flags.c_contiguous and got.tolist() == [4, 0, 0, 3, 4]   # order and repeats kept
    assert select_index(np.arange(10)[::-2], 10, "SNP").tolist() == [9, 7, 5, 3, 1]                 # a strided view


@pytest.mark.parametrize("bad, size", [
    (np.ones(4, dtype=bool), 5),             # a mask of another length
    ([0, -1], 5),                            # negative
    ([0, 5], 5),                             # >= size
    (np.array([2 ** 32], dtype=np.uint64), 5),
    ([], 5),                                 # empty list
    (np.zeros(5, dtype=bool), 5),            # empty mask
    (np.zeros(0, dtype=np.int64), 5),
    ([0.0, 1.0], 5),                         # not integers
    (["0"], 5),
    ([[0, 1]], 5),                           # not one-dimensional
], ids=str)
def test_select_index_rejects(bad, size):
    from ld_tools_amd import LdxError, select_index

    with pytest.raises(LdxError):
        select_index(bad, size, "haplotype")


def test_haplotype_columns():
    from ld_tools_amd.drivers import haplotype_columns

    carried = ["A", "B", "C", "D"]
    assert haplotype_columns(carried, ["D", "B"]).tolist() == [2, 3, 6, 7]               # carried order, not chosen order
    assert haplotype_columns(carried, ["B", "ZZ", "A"]).tolist() == [0, 1, 2, 3]         # a chosen sample that is not carried
    assert haplotype_columns(carried, ["C", "C"]).tolist() == [4, 5]
    assert haplotype_columns(carried, ["D", "A"], ploidy=1).tolist() == [0, 3]
    assert haplotype_columns(carried, ["ZZ"]).size == 0
    assert haplotype_columns(carried, carried).tolist() == list(range(8))


def test_columns_match_the_genotype_lists():
    """The columns index the lists sample_genotypes builds for the carried samples."""
    import sys

    sys.path.insert(0, str(ROOT / "tests"))
    import fakevcf
    from ld_tools_amd.drivers import haplotype_columns, sample_genotypes

    vcf, names = fakevcf.make_chromosome()
    rec = vcf.records[0]
    carried = [nm for nm in names if nm in rec.samples]
    assert len(carried) == len(names) - 1                                                # sample 7 is in no record
    chosen = names[5:12]
    whole = sample_genotypes(rec, names)
    assert [whole[c] for c in haplotype_columns(carried, chosen)] == sample_genotypes(rec, chosen)


def test_select_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ld_tools_amd import LdxError, PackedPanel

    z = torch.zeros(1, dtype=torch.uint8)
    p = PackedPanel(4, 8, z, z, z, z, z, z, z)
    with pytest.raises(LdxError):
        p.select(haplotypes=[0, 1])
    with pytest.raises(LdxError):
        p.split([0, 1] * 4)

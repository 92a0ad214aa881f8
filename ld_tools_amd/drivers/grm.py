"""The genetic relationship matrix in the layouts of GCTA's ``--make-grm`` (``.grm.bin``, ``.grm.N.bin``, ``.grm.id``) and PLINK's
``--make-rel`` (``.rel``, ``.rel.id``), and the ``--grm-cutoff`` selection.  Not a reference workflow: it runs ops.ld_grm on a
packed panel -- the weighted sums come from the int8 matrix cores, the jointly called counts from the FP4 ones -- and the cell
is this project's own definition (include/ldx.h, "weighted sample products"), NOT validated against GCTA or PLINK 2; the files
follow their layout, the numbers need not match their last digits.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from ..ops import GrmResult, grm_cutoff, ld_grm
from .king import _ids, _num, _write_ids


@dataclass
class GrmTable:
    """Individual k of the matrix is (fid[k], iid[k])."""

    fid: List[str]
    iid: List[str]
    result: GrmResult
    snp_mask: Optional[np.ndarray] = None   # the SNPs offered (bool over the panel's), None: all

    def grm(self) -> np.ndarray:
        """float32 [n_ind, n_ind] on the host."""
        g = self.result.grm()
        return g if isinstance(g, np.ndarray) else g.cpu().numpy()

    def n(self) -> np.ndarray:
        """int64 [n_ind, n_ind] on the host: the live SNPs called in both."""
        n = self.result.N
        return np.asarray(n).astype(np.int64) if isinstance(n, np.ndarray) else n.cpu().numpy().view(np.uint32).astype(np.int64)


def grm_table(panel, sample_ids: Sequence, keep=None, maf_min: Optional[float] = None) -> GrmTable:
    """The GRM of the individuals of ``panel`` over the live SNPs that pass ``keep`` (bool [n_snps]; None: all) and ``maf_min``.
    ``sample_ids``: one IID, or one (FID, IID) pair, per individual (an IID alone is its own FID)."""
    fid, iid = _ids(sample_ids, panel.n_ind)
    mask = None if keep is None else np.asarray(keep.cpu() if hasattr(keep, "cpu") else keep).astype(bool)
    return GrmTable(fid, iid, ld_grm(panel, keep=keep, maf_min=maf_min), mask)


def write_grm_bin(base: str, table: GrmTable) -> List[str]:
    """GCTA's binary GRM: ``{base}.grm.bin``, the float32 lower triangle with the diagonal, row by row; ``{base}.grm.N.bin``, the
    pairs' SNP counts as float32 in the same order; ``{base}.grm.id``, ``FID IID`` per line without a header."""
    low = np.tril_indices(len(table.iid))                 # row-major: (0,0) (1,0) (1,1) (2,0) ...
    paths = [base + ".grm.bin", base + ".grm.N.bin", base + ".grm.id"]
    table.grm()[low].astype("<f4").tofile(paths[0])
    table.n()[low].astype("<f4").tofile(paths[1])
    with open(paths[2], "w") as f:
        f.writelines(f"{a}\t{b}\n" for a, b in zip(table.fid, table.iid))
    return paths


def write_rel(base: str, table: GrmTable) -> List[str]:
    """PLINK's text form: ``{base}.rel``, individual a = 0 .. n - 1 against b = 0 .. a, one tab-separated line per a, six
    significant digits; ``{base}.rel.id``: the individuals in order."""
    g = table.grm()
    paths = [base + ".rel", base + ".rel.id"]
    with open(paths[0], "w") as f:
        for a in range(g.shape[0]):
            f.write("\t".join(_num(v) for v in g[a, :a + 1].tolist()) + "\n")
    _write_ids(paths[1], table.fid, table.iid, range(len(table.iid)))
    return paths


def write_grm_cutoff(base: str, table: GrmTable, cutoff: float) -> List[str]:
    """``{base}.grm.cutoff.in.id`` / ``.out.id``: ops.grm_cutoff's kept and removed individuals, in order."""
    keep, _ = grm_cutoff(table.grm(), cutoff)
    paths = [base + ".grm.cutoff.in.id", base + ".grm.cutoff.out.id"]
    _write_ids(paths[0], table.fid, table.iid, np.flatnonzero(keep).tolist())
    _write_ids(paths[1], table.fid, table.iid, np.flatnonzero(~keep).tolist())
    return paths

"""max(T) permutation tests of a case/control panel in PLINK's file layout.  Not a reference workflow: the operator
(ops.ld_mperm) is this project's own definition (include/ldx.h, "permutation tests"), NOT validated against PLINK; the file
follows the columns of PLINK 1.9's --assoc mperm, with the observed chi-square beside them.

    write_assoc_mperm    .assoc.mperm / .model.trend.mperm    CHR SNP EMP1 EMP2 CHISQ

EMP1 is the point-wise empirical p-value (n_ge + 1) / (R + 1), EMP2 the family-wise one from the permutations' maxima over all
variants of the table; a flagged variant (ops.MPERM_FLAGS) has NA in the three columns.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from .._lib import LdxError
from ..ops import MpermResult, ld_mperm
from ..panel import PackedPanel
from .qc import _np, _num, _write

MPERM_COLUMNS = ("CHR", "SNP", "EMP1", "EMP2", "CHISQ")
MPERM_SUFFIX = {"allelic": ".assoc.mperm", "trend": ".model.trend.mperm"}


@dataclass
class MpermTable:
    """mperm_table's result: ops.ld_mperm's beside the variants -- row k is (chrom[k], ids[k])."""

    chrom: List[str]
    ids: List[str]
    result: MpermResult


def mperm_table(panel: PackedPanel, case, chrom, ids, test: str = "allelic", n_perm: int = 10000, seed: int = 0, keep=None,
                maxima: Optional[torch.Tensor] = None) -> MpermTable:
    """ops.ld_mperm on a panel with the names of its variants.  ``maxima``: an earlier table's ``result.maxima`` over the same
    permutations (same ``seed``, ``n_perm`` and individuals) and other variants -- a chromosome at a time; EMP2 of the last
    table is then family-wise over all of them."""
    chrom, ids = [str(c) for c in chrom], [str(i) for i in ids]
    if len(chrom) != panel.n_snps or len(ids) != panel.n_snps:
        raise LdxError(f"mperm_table: {len(chrom)} chromosomes and {len(ids)} IDs for {panel.n_snps} variants")
    return MpermTable(chrom, ids, ld_mperm(panel, case, test=test, n_perm=n_perm, seed=seed, keep=keep, maxima=maxima))


def write_assoc_mperm(path: str, table: MpermTable) -> int:
    """``path``: one line per variant of ``table``, tab-separated.  Returns the number of lines."""
    r = table.result
    emp1, emp2, stat = _np(r.emp1), _np(r.emp2), _np(r.stat)
    return _write(path, MPERM_COLUMNS, ((table.chrom[k], table.ids[k], _num(emp1[k]), _num(emp2[k]), _num(stat[k]))
                                        for k in range(len(table.ids))))

"""LD pruning of one chromosome in PLINK's ``.prune.in`` / ``.prune.out`` layout.  Not a reference workflow: it takes the
inputs of drivers/ldscore.py and runs ops.ld_prune (neighbour lists on the matrix-pipe band, then the greedy selection on
the device).

Pruning here is priority clumping -- the SNPs in decreasing priority (default: minor allele frequency), each one kept
unless a kept SNP within the window has r^2 above the threshold with it -- not ``--indep-pairwise``'s sliding-window step
algorithm.  By default r is the haplotype r of the ALT-allele indicators over the panel's haplotypes (include/ldx.h,
LDX_OUT_R32); ``dosage=True`` takes PLINK's own r, the genotype correlation of the ALT dosages over the samples
(ldx_ld_neighbors_dosage_dev; a missing call counts as REF).  Either way the files follow PLINK's layout while the sets
need not match ``--indep-pairwise``'s, whose rule differs.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from ..ops import Pruned, ld_prune
from .clump import chrom_panel


@dataclass
class PruneTable:
    """Row k is variant k of these lists (position-sorted; variants without a matching record are left out)."""

    chrom: str
    rs_ids: List[str]
    poss: List[int]
    pruned: Pruned


def prune(vcf, chrom, chrom_rows: Sequence[Sequence], sample_names: Sequence[str], r2: float = 0.2,
          window_bp: int = 250_000, priority: Optional[Sequence[float]] = None, dosage: bool = False, em: bool = False,
          missing: Optional[str] = None) -> PruneTable:
    """Pruning of one chromosome's variants (VCF rows [pos, rsID]); ``priority``: one value per input row (higher first),
    default the minor allele frequency.  ``dosage``: genotype-dosage r (ops.ld_prune).  ``em``: the EM r of the unphased
    genotypes (``missing="pairwise"``: every pair over the samples called at both variants); ``missing`` is passed through
    only where it is given."""
    panel, rows, rs_ids, poss = chrom_panel(vcf, chrom, chrom_rows, sample_names, "prune")
    pr = None if priority is None else np.asarray(priority, dtype=np.float64)[rows]
    more = {} if missing is None else {"missing": missing}
    res = ld_prune(panel, np.asarray(poss, dtype=np.int64), r2=r2, window_bp=window_bp, priority=pr, dosage=dosage, em=em,
                   **more)
    return PruneTable(str(chrom), rs_ids, poss, res)


def write_prune(base: str, table: PruneTable) -> List[str]:
    """``{base}.prune.in``: the kept variants' rsIDs, one per line in position order; ``{base}.prune.out``: the others
    (degenerate variants included).  Returns the two paths."""
    keep = table.pruned.keep
    paths = [base + ".prune.in", base + ".prune.out"]
    for path, sel in zip(paths, (keep, ~keep)):
        with open(path, "w") as f:
            f.writelines(table.rs_ids[k] + "\n" for k in np.flatnonzero(sel))
    return paths

"""LD clumping of one chromosome's GWAS results in PLINK 1.9's ``.clumped`` layout.  Not a reference workflow: it takes the
inputs of drivers/ldscore.py plus one p-value per input row and runs ops.ld_clump (neighbour lists on the matrix-pipe band,
then the greedy selection on the device).

The rule is PLINK ``--clump``'s: the SNPs with p <= p1, most significant first, each one not yet in a clump becoming an
index that takes every SNP not yet in a clump with p <= p2 and r^2 >= r2 within the window.  By default r is the haplotype
r of the ALT-allele indicators over the panel's haplotypes (include/ldx.h, LDX_OUT_R32), not PLINK's genotype-based estimate,
so the file follows PLINK's layout while its values need not match PLINK's; ``dosage=True`` takes the genotype correlation of
the ALT dosages over the samples instead (ldx_ld_neighbors_dosage_dev; a missing call counts as REF), PLINK's r.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from .._lib import LdxError
from ..ops import Clumps, ld_clump
from ..panel import PackedPanel
from .ingest import RaggedGenotypesError, codes_matrix
from .triangle import fetch_variants

# the S* columns of .clumped: members by p, (lower bound, upper bound]
P_BUCKETS = (("NSIG", 0.05, np.inf), ("S05", 0.01, 0.05), ("S01", 0.001, 0.01), ("S001", 1e-4, 0.001),
             ("S0001", -np.inf, 1e-4))


@dataclass
class ClumpTable:
    """Row k is variant k of these lists (position-sorted; variants without a matching record are left out)."""

    chrom: str
    rs_ids: List[str]
    poss: List[int]
    pvalues: np.ndarray   # float64 [n] in row order
    clumps: Clumps

    @property
    def n(self) -> int:
        return len(self.rs_ids)


def chrom_panel(vcf, chrom, chrom_rows: Sequence[Sequence], sample_names: Sequence[str], what: str):
    """(panel, kept input rows in panel order, rsIDs, positions) of one chromosome: each record fetched once
    (fetch_variants' stable position sort), variants without a matching record left out."""
    order = sorted(range(len(chrom_rows)), key=lambda k: chrom_rows[k][0])   # fetch_variants' stable sort
    cv = fetch_variants(vcf, chrom, chrom_rows, sample_names)
    keep = [k for k, rec in enumerate(cv.recs) if rec is not None]
    if not keep:
        raise LdxError(f"{what}: no variant of chromosome {chrom} has a matching record")
    try:
        codes = codes_matrix([cv.genotypes[k] for k in keep])
    except ZeroDivisionError as exc:   # a record that carries none of the samples
        raise LdxError(f"{what}: a variant of chromosome {chrom} has no genotype of the selected samples") from exc
    except RaggedGenotypesError as exc:
        raise LdxError(f"{what}: mixed ploidy on chromosome {chrom} ({exc}); r needs one haplotype count") from exc
    rows = np.asarray(order, dtype=np.int64)[np.asarray(keep, dtype=np.int64)]
    return PackedPanel.from_codes(codes), rows, [cv.rs_ids[k] for k in keep], [cv.poss[k] for k in keep]


def clump(vcf, chrom, chrom_rows: Sequence[Sequence], sample_names: Sequence[str], pvalues: Sequence[float],
          p1: float = 1e-4, p2: float = 1e-2, r2: float = 0.5, window_bp: int = 250_000, dosage: bool = False,
          em: bool = False, missing: Optional[str] = None) -> ClumpTable:
    """Clumps of one chromosome's variants (VCF rows [pos, rsID], one p-value per input row).  ``dosage``: genotype-dosage
    r (ops.ld_clump).  ``em``: the EM r of the unphased genotypes; with ``missing="pairwise"`` -- every pair over the samples
    called at both variants -- PLINK --clump's own r^2.  ``missing`` is passed through only where it is given."""
    p_in = np.asarray(pvalues, dtype=np.float64)
    if p_in.shape != (len(chrom_rows),):
        raise LdxError("clump: one p-value per input row is needed")
    panel, rows, rs_ids, poss = chrom_panel(vcf, chrom, chrom_rows, sample_names, "clump")
    p = p_in[rows]
    more = {} if missing is None else {"missing": missing}
    res = ld_clump(panel, np.asarray(poss, dtype=np.int64), p, p1=p1, p2=p2, r2=r2, window_bp=window_bp, dosage=dosage, em=em,
                   **more)
    return ClumpTable(str(chrom), rs_ids, poss, p, res)


def clumped_lines(table: ClumpTable) -> List[str]:
    """The lines of the .clumped file: the header, one row per clump in index rank order, then two empty lines."""
    out = [" CHR    F          SNP         BP        P    TOTAL   NSIG    S05    S01   S001  S0001    SP2"]
    for k, members in table.clumps.clumps():
        mp = table.pvalues[members]
        counts = [int(((mp > lo) & (mp <= hi)).sum()) for _, lo, hi in P_BUCKETS]
        sp2 = ",".join(f"{table.rs_ids[j]}(1)" for j in members) if members.size else "NONE"
        out.append("%4s %4d %12s %10d %8s %8d %6d %6d %6d %6d %6d    %s" % (
            table.chrom, 1, table.rs_ids[k], table.poss[k], "%.3g" % table.pvalues[k], members.size, *counts, sp2))
    return out + ["", ""]


def write_clumped(path: str, table: ClumpTable) -> str:
    """PLINK 1.9's .clumped columns: CHR F SNP BP P TOTAL NSIG S05 S01 S001 S0001 SP2.  F = 1; TOTAL = the members (the
    index excluded); the S* columns count the members by p: NSIG p > 0.05, S05 (0.01, 0.05], S01 (0.001, 0.01], S001
    (1e-4, 0.001], S0001 <= 1e-4; SP2 lists the members as rsID(1) in row order, or NONE.  Rows in index rank order."""
    with open(path, "w") as f:
        f.write("\n".join(clumped_lines(table)) + "\n")
    return path

"""Signed-r LD matrix of one chromosome: the square matrix of r between ALT-allele indicators, unrounded, with the variant
list that fixes its allele orientation -- what fine-mapping, colocalisation, summary-statistics imputation and LD-aware PRS
read from a phased reference panel; with ``dosage=True`` the genotype correlation of the ALT dosages over the samples instead
(include/ldx.h, ldx_triangle_dosage_dev), which needs no phase.  Not a reference workflow: the reference only writes rounded r^2 / D' tables
(drivers/triangle.py); this driver takes the same inputs and runs the r32 cell format (include/ldx.h, LDX_OUT_R32)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from .._lib import LdxError
from ..ops import TriangleResult, ld_triangle
from ..panel import PackedPanel
from .ingest import RaggedGenotypesError, codes_matrix
from .triangle import fetch_variants


@dataclass
class RMatrix:
    """Row / column k of the matrix is variant k of these lists (position-sorted; variants without a matching record are
    left out).  r > 0: the ALT alleles (``alts``) co-occur more often than independence predicts."""

    chrom: str
    rs_ids: List[str]
    poss: List[int]
    refs: List[str]
    alts: List[str]                   # the first ALT allele: code 1 of the genotype calls
    alt_freqs: List[float]            # round(a / n, 4), as the reference reports it (calc_ld.py:96-97)
    result: TriangleResult            # the r32 triangle; result.r_matrix() gives blocks of the square

    @property
    def n(self) -> int:
        return len(self.rs_ids)


def r_matrix(vcf, chrom, chrom_rows: Sequence[Sequence], sample_names: Sequence[str], dosage: bool = False) -> RMatrix:
    """The r32 triangle of one chromosome's variants, from the inputs of ``triangle_matrix`` (VCF rows [pos, rsID]; each
    record fetched once).  ``dosage``: genotype-dosage r over the samples (a missing call counts as REF).  Mixed-ploidy panels (genotype lists of different lengths) are out of scope: LdxError."""
    cv = fetch_variants(vcf, chrom, chrom_rows, sample_names)
    keep = [k for k, rec in enumerate(cv.recs) if rec is not None]
    if not keep:
        raise LdxError(f"r_matrix: no variant of chromosome {chrom} has a matching record")
    try:
        codes = codes_matrix([cv.genotypes[k] for k in keep])
    except ZeroDivisionError as exc:   # a record that carries none of the samples
        raise LdxError(f"r_matrix: a variant of chromosome {chrom} has no genotype of the selected samples") from exc
    except RaggedGenotypesError as exc:
        raise LdxError(f"r_matrix: mixed ploidy on chromosome {chrom} ({exc}); signed r needs one haplotype count") from exc
    panel = PackedPanel.from_codes(codes)
    res = ld_triangle(panel, fmt="r32", dosage=dosage)
    return RMatrix(chrom, [cv.rs_ids[k] for k in keep], [cv.poss[k] for k in keep], [cv.recs[k].ref for k in keep],
                   [cv.recs[k].alts[0] for k in keep], panel.alt_freq4().cpu().numpy().tolist(), res)


VARIANTS_HEADER = "index\trsID\tposition\tREF\tALT\talt_freq\n"


def write_r_matrix(base: str, m: RMatrix, rows_per_block: int = 1024) -> List[str]:
    """``{base}.npy``: the square float32 matrix, written in blocks of rows through a memory map (a 40 000-SNP matrix is
    6.4 GB: it never sits in host memory whole, let alone twice); ``{base}.variants.tsv``: a header line, then one line
    per matrix row -- the matrix's index, and what fixes the orientation of the sign.  Returns the two paths."""
    n = m.n
    npy, tsv = base + ".npy", base + ".variants.tsv"
    mm = np.lib.format.open_memmap(npy, mode="w+", dtype=np.float32, shape=(n, n))
    try:
        for r0 in range(0, n, rows_per_block):
            r1 = min(n, r0 + rows_per_block)
            mm[r0:r1] = m.result.r_matrix(rows=(r0, r1)).cpu().numpy()
        mm.flush()
    finally:
        del mm
    with open(tsv, "w") as out:
        out.write(VARIANTS_HEADER)
        for k in range(n):
            out.write(f"{k}\t{m.rs_ids[k]}\t{m.poss[k]}\t{m.refs[k]}\t{m.alts[k]}\t{m.alt_freqs[k]}\n")
    return [npy, tsv]

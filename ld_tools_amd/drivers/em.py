"""Unphased LD by maximum likelihood between two variant lists over the same samples: the EM r and D' of every variant of
one list against every variant of another (what PLINK --r2 dprime reports for unphased genotype calls), as two dense float32
matrices with the two variant lists that fix their rows and columns, and as a PLINK-style ``.ld`` table of the pairs above an
r^2 threshold.  The inputs are those of ``drivers/rect.py``; the work is ``ops.ld_em`` / ``ops.ld_em_hits`` (include/ldx.h,
"unphased LD by EM").  ``missing="pairwise"`` estimates every pair over the samples called at both variants, as PLINK and
Haploview do with ``./.`` calls (include/ldx.h, "pairwise-complete EM")."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from .._lib import LdxError
from ..ops import LDRectHits, ld_em, ld_em_hits
from ..panel import PackedPanel
from .rect import RectSide, read_sides, write_variants

LD_HEADER = "SNP_A\tSNP_B\tR2\tDP\n"


@dataclass
class EmMatrix:
    rows: RectSide
    cols: RectSide
    r: object                         # float32 [n_i, n_j] device tensor: the EM r of rows' variant a and cols' variant b
    dprime: object                    # float32 [n_i, n_j] device tensor: their D'


def em_panels(vcf, chrom_i, rows_i, chrom_j, rows_j, sample_names: Sequence[str]):
    """Both sides read and packed: (RectSide, RectSide, PackedPanel, PackedPanel).  An odd haplotype count (haploid calls) is
    refused: the EM pairs haplotypes 2k and 2k + 1 into individuals."""
    side_i, side_j = read_sides(vcf, chrom_i, rows_i, chrom_j, rows_j, sample_names)
    if side_i.codes.shape[1] % 2:
        raise LdxError(f"em_matrix: {side_i.codes.shape[1]} haplotypes: unphased LD needs diploid calls (an even count)")
    pi, pj = PackedPanel.from_codes(side_i.codes), PackedPanel.from_codes(side_j.codes)
    side_i.alt_freqs = pi.alt_freq4().cpu().numpy().tolist()
    side_j.alt_freqs = pj.alt_freq4().cpu().numpy().tolist()
    return side_i, side_j, pi, pj


def em_matrix(vcf, chrom_i, rows_i: Sequence[Sequence], chrom_j, rows_j: Sequence[Sequence],
              sample_names: Sequence[str], missing: Optional[str] = None) -> EmMatrix:
    """EM r and D' of the variants ``rows_i`` of chromosome ``chrom_i`` against the variants ``rows_j`` of ``chrom_j`` (VCF
    rows [pos, rsID], as for ``rect_matrix``).  ``missing=None``: a missing call counts as REF.  ``missing="pairwise"``: a
    sample takes part in a pair only where it is called at both variants -- a ``./.`` call, a half-missing call (``0/.``)
    and a call with a second ALT allele are all missing at that variant -- and a pair whose jointly called samples are none,
    or monomorphic at either variant, is -0.0 in both matrices."""
    side_i, side_j, pi, pj = em_panels(vcf, chrom_i, rows_i, chrom_j, rows_j, sample_names)
    out = ld_em(pi, pj, missing=missing)
    return EmMatrix(side_i, side_j, out.r, out.dprime)


def write_em_matrix(base: str, m: EmMatrix, rows_per_block: int = 1024) -> List[str]:
    """``{base}.r.npy`` and ``{base}.dprime.npy``: the two float32 [n_i, n_j] matrices, written in blocks of rows through a
    memory map; ``{base}.rows.tsv`` and ``{base}.cols.tsv``: the variants of the rows and of the columns.  Returns the four
    paths."""
    n_i, n_j = m.rows.n, m.cols.n
    paths = [base + ".r.npy", base + ".dprime.npy", base + ".rows.tsv", base + ".cols.tsv"]
    for path, mat in zip(paths, (m.r, m.dprime)):
        mm = np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(n_i, n_j))
        try:
            for r0 in range(0, n_i, rows_per_block):
                block = mat[r0:min(n_i, r0 + rows_per_block)]
                mm[r0:r0 + block.shape[0]] = block.cpu().numpy() if hasattr(block, "cpu") else np.asarray(block, dtype=np.float32)
            mm.flush()
        finally:
            del mm
    write_variants(paths[2], m.rows)
    write_variants(paths[3], m.cols)
    return paths


def em_hits(vcf, chrom_i, rows_i, chrom_j, rows_j, sample_names: Sequence[str], r2: float = 0.2,
            missing: Optional[str] = None):
    """The pairs with EM r^2 >= ``r2``: (rows' RectSide, columns' RectSide, LDRectHits of ops.ld_em_hits).  ``missing``:
    em_matrix's."""
    side_i, side_j, pi, pj = em_panels(vcf, chrom_i, rows_i, chrom_j, rows_j, sample_names)
    return side_i, side_j, ld_em_hits(pi, pj, r2=r2, missing=missing)


def write_ld_table(path: str, rows: RectSide, cols: RectSide, hits: LDRectHits) -> int:
    """A PLINK-style ``.ld`` table of the hits, sorted by (row, column): ``SNP_A SNP_B R2 DP`` with R2 = r^2 in float64 from
    the float32 r cell and DP = the D' cell, six decimals each.  Returns the number of pairs written."""
    i, j, r = hits.pairs()
    dp = hits.dprime.cpu().numpy()
    with open(path, "w") as out:
        out.write(LD_HEADER)
        for a, b, rv, dv in zip(i.tolist(), j.tolist(), r.astype(np.float64).tolist(), dp.astype(np.float64).tolist()):
            out.write(f"{rows.rs_ids[a]}\t{cols.rs_ids[b]}\t{rv * rv:.6f}\t{dv:.6f}\n")
    return int(i.size)

"""Unphased LD by maximum likelihood between two variant lists over the same samples: the EM r and D' of every variant of
one list against every variant of another (what PLINK --r2 dprime reports for unphased genotype calls), as two dense float32
matrices with the two variant lists that fix their rows and columns, and as a PLINK-style ``.ld`` table of the pairs above an
r^2 threshold.  The inputs are those of ``drivers/rect.py``; the work is ``ops.ld_em`` / ``ops.ld_em_hits`` (include/ldx.h,
"unphased LD by EM").  ``missing="pairwise"`` estimates every pair over the samples called at both variants, as PLINK and
Haploview do with ``./.`` calls (include/ldx.h, "pairwise-complete EM").

``em_band`` / ``write_em_band`` / ``em_window_hits`` are the one-chromosome forms -- PLINK ``--r2 dprime --ld-window-kb
--ld-window-r2``: the EM r and D' of every pair of variants within ``window_bp`` of each other in drivers/band.py's layout, and
the ``.ld`` table of the in-window pairs above the threshold, each pair once (ops.ld_em_band / ops.ld_neighbors(em=True);
include/ldx.h, "EM on the band")."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from .._lib import LdxError
from ..ops import LDEmBand, LDRectHits, ld_em, ld_em_band, ld_em_hits, ld_neighbors
from ..panel import PackedPanel
from .clump import chrom_panel
from .rect import RectSide, read_sides, write_variants
from .rmatrix import VARIANTS_HEADER

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


@dataclass
class EmBand:
    """Row k of the two bands is variant k of these lists (position-sorted; variants without a matching record are left out)."""

    chrom: str
    rs_ids: List[str]
    poss: List[int]
    alt_freqs: List[float]            # round(a / n, 4) of code 1 over all haplotypes, as the reference reports it
    bands: LDEmBand

    @property
    def n(self) -> int:
        return len(self.rs_ids)


def _chrom_em_panel(what: str, vcf, chrom, chrom_rows, sample_names):
    panel, _, rs_ids, poss = chrom_panel(vcf, chrom, chrom_rows, sample_names, what)
    if panel.n_hap % 2:
        raise LdxError(f"{what}: {panel.n_hap} haplotypes: unphased LD needs diploid calls (an even count)")
    return panel, rs_ids, poss


def em_band(vcf, chrom, chrom_rows: Sequence[Sequence], sample_names: Sequence[str], window_bp: int = 1_000_000,
            missing: Optional[str] = None) -> EmBand:
    """The stored EM r and D' bands of one chromosome's variants (VCF rows [pos, rsID]; each record fetched once).
    ``missing``: em_matrix's."""
    panel, rs_ids, poss = _chrom_em_panel("em_band", vcf, chrom, chrom_rows, sample_names)
    bands = ld_em_band(panel, np.asarray(poss, dtype=np.int64), window_bp=window_bp, missing=missing)
    return EmBand(str(chrom), rs_ids, poss, panel.alt_freq4().cpu().numpy().tolist(), bands)


def write_em_band(base: str, m: EmBand, cells_per_block: int = 1 << 26) -> List[str]:
    """``{base}.band.r.npy`` and ``{base}.band.dprime.npy`` (float32 [n_cells] each, written in blocks through a memory map),
    ``{base}.band.offsets.npy`` (uint64 [n + 1]), ``{base}.band.lo.npy`` (uint32 [n]) -- cell (i, j), lo[i] <= j < i, is word
    offsets[i] + j - lo[i] of both --, ``{base}.band.diag.npy`` (float32 [n]: +1 where the variant has both alleles among its
    called samples, else -0.0) and ``{base}.variants.tsv`` (index, rsID, position, ALT frequency).  Returns the six paths."""
    b = m.bands.r
    paths = [base + ".band.r.npy", base + ".band.dprime.npy", base + ".band.offsets.npy", base + ".band.lo.npy",
             base + ".band.diag.npy", base + ".variants.tsv"]
    for path, band in zip(paths, (m.bands.r, m.bands.dprime)):
        mm = np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(band.n_cells,))
        try:
            for c0 in range(0, band.n_cells, cells_per_block):
                c1 = min(band.n_cells, c0 + cells_per_block)
                mm[c0:c1] = band.values[c0:c1].cpu().numpy()
            mm.flush()
        finally:
            del mm
    np.save(paths[2], b.offsets.cpu().numpy().view(np.uint64))
    np.save(paths[3], b.lo.cpu().numpy().view(np.uint32))
    np.save(paths[4], b.diag.cpu().numpy())
    with open(paths[5], "w") as out:
        out.write("\t".join(VARIANTS_HEADER.rstrip("\n").split("\t")[:3] + ["alt_freq"]) + "\n")
        for k in range(m.n):
            out.write(f"{k}\t{m.rs_ids[k]}\t{m.poss[k]}\t{m.alt_freqs[k]}\n")
    return paths


def em_window_hits(vcf, chrom, chrom_rows: Sequence[Sequence], sample_names: Sequence[str], r2: float = 0.2,
                   window_bp: int = 1_000_000, missing: Optional[str] = None):
    """The pairs of one chromosome's variants within ``window_bp`` of each other with EM r^2 >= ``r2``, each pair ONCE, the
    variant earlier in position order first: (RectSide of the variants -- both sides of ``write_ld_table`` --, LDRectHits
    with ``em`` set, built from ops.ld_neighbors(em=True)'s records with i < j)."""
    import torch
    panel, rs_ids, poss = _chrom_em_panel("em_window_hits", vcf, chrom, chrom_rows, sample_names)
    nb = ld_neighbors(panel, np.asarray(poss, dtype=np.int64), window_bp=window_bp, r2=r2, missing=missing, em=True)
    once = nb.hits[nb.hits[:, 0] < nb.hits[:, 1]].contiguous()   # (sorted by (i, j) already)
    offsets = torch.zeros(nb.n_snps + 1, dtype=torch.int32, device=once.device)
    offsets[1:] = torch.cumsum(torch.bincount(once[:, 0].to(torch.int64), minlength=nb.n_snps), 0).to(torch.int32)
    side = RectSide(str(chrom), rs_ids, poss, [], [], panel.alt_freq4().cpu().numpy().tolist(), None)
    return side, LDRectHits(offsets, once, nb.n_snps, nb.n_snps, nb.bound, False, True, missing=missing)

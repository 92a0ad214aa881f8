"""The windowed (band) LD matrix of one chromosome, kept on disk, and cross-population LD scores from such bands.

``band_matrix`` / ``write_band``: the signed r of every pair of variants within ``window_bp`` of each other, 4 bytes per
unordered pair, with the variant list that fixes its allele orientation -- the banded LD matrices that summary-statistics
methods (GCTB --make-band-ldm, LDpred2, SBayesR) read, where drivers/rmatrix.py's square matrix is out of reach at
chromosome scale.  ``cross_scores_by_group``: for every pair of sample groups (populations) the cross-population LD score
sum_j r1_ij r2_ij over the window -- the term trans-ethnic genetic-correlation methods (Popcorn, S-LDXR) need beside each
population's own LD scores (drivers/ldscore.py) -- from ONE pass over the VCF.  Not reference workflows: they take the
inputs of drivers/rmatrix.py and run ops.ld_band / ops.ld_cross_score (include/ldx.h, "stored bands").
"""
from __future__ import annotations

import gzip
from dataclasses import dataclass
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from .._lib import LdxError
from ..ops import LDBand, ld_band, ld_cross_score
from .ingest import haplotype_columns
from .ldscore import _check_complete, _check_missing_arg, _fetch_panel, _pairwise
from .rmatrix import VARIANTS_HEADER


@dataclass
class BandMatrix:
    """Row k of the band is variant k of these lists (position-sorted; variants without a matching record are left out).
    r > 0: the ALT alleles (``alts``) co-occur more often than independence predicts."""

    chrom: str
    rs_ids: List[str]
    poss: List[int]
    refs: List[str]
    alts: List[str]                   # the first ALT allele: code 1 of the genotype calls
    alt_freqs: List[float]            # round(a / n, 4), as the reference reports it (calc_ld.py:96-97)
    band: LDBand

    @property
    def n(self) -> int:
        return len(self.rs_ids)


def band_matrix(vcf, chrom, chrom_rows: Sequence[Sequence], sample_names: Sequence[str], window_bp: int = 1_000_000,
                dosage: bool = False, missing: Optional[str] = None) -> BandMatrix:
    """The stored band of one chromosome's variants, from the inputs of ``r_matrix`` (VCF rows [pos, rsID]; each record
    fetched once).  ``dosage`` / ``missing`` as for drivers/ldscore.py's ``ld_scores``.  Mixed-ploidy panels are out of scope:
    LdxError."""
    _check_missing_arg("band_matrix", dosage, missing)
    cv, keep, _, _, panel = _fetch_panel("band_matrix", vcf, chrom, chrom_rows, sample_names, None, None)
    if dosage:
        _check_complete("band_matrix", panel, chrom, missing)
    poss = [cv.poss[k] for k in keep]
    band = ld_band(panel, np.asarray(poss, dtype=np.int64), window_bp=window_bp, dosage=dosage, missing=_pairwise(missing))
    return BandMatrix(str(chrom), [cv.rs_ids[k] for k in keep], poss, [cv.recs[k].ref for k in keep],
                      [cv.recs[k].alts[0] for k in keep], panel.alt_freq4().cpu().numpy().tolist(), band)


def write_band(base: str, m: BandMatrix, cells_per_block: int = 1 << 26) -> List[str]:
    """``{base}.band.values.npy`` (float32 [n_cells], written in blocks through a memory map), ``{base}.band.offsets.npy``
    (uint64 [n + 1]), ``{base}.band.lo.npy`` (uint32 [n]) -- cell (i, j), lo[i] <= j < i, is values[offsets[i] + j - lo[i]] --,
    ``{base}.band.diag.npy`` (float32 [n], the diagonal) and ``{base}.variants.tsv`` in drivers/rmatrix.py's format.  Returns
    the five paths."""
    b = m.band
    paths = [base + ".band.values.npy", base + ".band.offsets.npy", base + ".band.lo.npy", base + ".band.diag.npy",
             base + ".variants.tsv"]
    mm = np.lib.format.open_memmap(paths[0], mode="w+", dtype=np.float32, shape=(b.n_cells,))
    try:
        for c0 in range(0, b.n_cells, cells_per_block):
            c1 = min(b.n_cells, c0 + cells_per_block)
            mm[c0:c1] = b.values[c0:c1].cpu().numpy()
        mm.flush()
    finally:
        del mm
    np.save(paths[1], b.offsets.cpu().numpy().view(np.uint64))
    np.save(paths[2], b.lo.cpu().numpy().view(np.uint32))
    np.save(paths[3], b.diag.cpu().numpy())
    with open(paths[4], "w") as out:
        out.write(VARIANTS_HEADER)
        for k in range(m.n):
            out.write(f"{k}\t{m.rs_ids[k]}\t{m.poss[k]}\t{m.refs[k]}\t{m.alts[k]}\t{m.alt_freqs[k]}\n")
    return paths


@dataclass
class CrossScoreTable:
    """Cross-population LD scores of one pair of groups; row k is variant k of the lists."""

    chrom: str
    groups: Tuple[str, str]
    rs_ids: List[str]
    poss: List[int]
    live: np.ndarray                  # bool [n]: the variant is not degenerate in EITHER group
    sums: np.ndarray                  # int64 [n], units of 2^-32 (ops.ld_cross_score)
    scores: np.ndarray                # float64 [n] = sums 2^-32

    @property
    def n(self) -> int:
        return len(self.rs_ids)


def cross_scores_by_group(vcf, chrom, chrom_rows: Sequence[Sequence], groups: Mapping[str, Sequence[str]],
                          window_bp: int = 1_000_000, dosage: bool = False,
                          missing: Optional[str] = None) -> Dict[Tuple[str, str], CrossScoreTable]:
    """Cross-population LD scores for every unordered pair of the sample groups (label -> sample names) of one chromosome
    from ONE pass over the VCF: the union of the groups is fetched and packed once and split on the device
    (PackedPanel.select), one band is stored per group (ops.ld_band) and every pair of bands gives one table
    (ops.ld_cross_score), keyed by the two labels in the order of ``groups``.  The groups may overlap or differ in size;
    the samples must be diploid in every record, as for ``ld_scores_by_group``.  ``dosage`` / ``missing`` as for ``ld_scores``."""
    what = "cross_scores_by_group"
    _check_missing_arg(what, dosage, missing)
    if len(groups) < 2:
        raise LdxError(f"{what}: at least two groups")
    union = list(dict.fromkeys(name for members in groups.values() for name in members))
    cv, keep, _, _, panel = _fetch_panel(what, vcf, chrom, chrom_rows, union, None, None)
    carried = [name for name in union if name in cv.recs[keep[0]].samples]
    if any([name for name in union if name in cv.recs[k].samples] != carried for k in keep[1:]):
        raise LdxError(f"{what}: the records of chromosome {chrom} do not all carry the same samples")
    if panel.n_hap != 2 * len(carried):
        raise LdxError(f"{what}: {panel.n_hap} haplotypes for {len(carried)} carried samples on chromosome {chrom}: "
                       "haploid or mixed-ploidy calls; the groups' columns are only known for diploid samples")
    if dosage:
        _check_complete(what, panel, chrom, missing)
    poss = [cv.poss[k] for k in keep]
    pos = np.asarray(poss, dtype=np.int64)
    rs_ids = [cv.rs_ids[k] for k in keep]
    bands: Dict[str, LDBand] = {}
    lives: Dict[str, np.ndarray] = {}
    for label, members in groups.items():
        cols = haplotype_columns(carried, members)
        if cols.size == 0:
            raise LdxError(f"{what}: no sample of group {label!r} is carried by the records of chromosome {chrom}")
        sub = panel.select(haplotypes=cols)
        bands[label] = ld_band(sub, pos, window_bp=window_bp, dosage=dosage, missing=_pairwise(missing))
        lives[label] = sub.dosage_live() if dosage else \
            (sub.alt_counts().astype(np.int64) * sub.ref_counts().astype(np.int64)) > 0
    labels = list(groups)
    tables: Dict[Tuple[str, str], CrossScoreTable] = {}
    for x, la in enumerate(labels):
        for lb in labels[x + 1:]:
            sc = ld_cross_score(bands[la], bands[lb])
            tables[(la, lb)] = CrossScoreTable(str(chrom), (la, lb), list(rs_ids), list(poss), lives[la] & lives[lb],
                                               sc.sums, np.asarray(sc, dtype=np.float64))
    return tables


def write_cross_score(base: str, table: CrossScoreTable) -> str:
    """``{base}.{a}_{b}.l2.ldscore.gz`` in write_ldscore's format: tab-separated CHR, SNP, BP and the column ``{a}_{b}L2``,
    values as %.3f, variants that are degenerate in either group left out.  Returns the path."""
    a, b = table.groups
    path = f"{base}.{a}_{b}.l2.ldscore.gz"
    with gzip.open(path, "wt") as out:
        out.write("\t".join(["CHR", "SNP", "BP", f"{a}_{b}L2"]) + "\n")
        for k in np.flatnonzero(table.live):
            out.write("\t".join([table.chrom, table.rs_ids[k], str(table.poss[k]), "%.3f" % table.scores[k]]) + "\n")
    return path

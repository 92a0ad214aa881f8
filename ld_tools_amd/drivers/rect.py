"""Rectangular signed-r LD between two variant lists over the same samples: lead SNPs x a chromosome, an rsID list x another
list of the same chromosome, chromosome A x chromosome B -- the dense float32 matrix with the two variant lists that fix its
rows, its columns and the orientation of its sign.  Not a reference workflow (the reference pairs one list with itself):
this driver takes the inputs of ``drivers/rmatrix.py`` twice and runs ``ops.ld_rect`` (include/ldx.h, ldx_ld_rect_dev)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from .._lib import LdxError
from ..ops import ld_rect
from ..panel import PackedPanel
from .ingest import RaggedGenotypesError, codes_matrix
from .rmatrix import VARIANTS_HEADER
from .triangle import fetch_variants


@dataclass
class RectSide:
    """One side of the rectangle: row (side I) or column (side J) k of the matrix is variant k of these lists
    (position-sorted; variants without a matching record are left out)."""

    chrom: str
    rs_ids: List[str]
    poss: List[int]
    refs: List[str]
    alts: List[str]                   # the first ALT allele: code 1 of the genotype calls
    alt_freqs: List[float]            # round(a / n, 4), as the reference reports it (calc_ld.py:96-97)
    codes: np.ndarray                 # int8 [n][n_hap]: what the side's panel is packed from

    @property
    def n(self) -> int:
        return len(self.rs_ids)


@dataclass
class RectMatrix:
    rows: RectSide
    cols: RectSide
    dosage: bool
    r: object                         # float32 [n_i, n_j] device tensor: r[a, b] = signed r of rows' variant a and cols' variant b
    missing: object = None            # None, or "pairwise": r over the calls present at both variants (ops.ld_rect)


def carried_samples(rec, sample_names: Sequence[str]) -> tuple:
    """The selected samples a record carries, in ``sample_names`` order: whose GT tuples make its genotype list."""
    return tuple(name for name in sample_names if name in rec.samples)


def read_side(vcf, chrom, chrom_rows: Sequence[Sequence], sample_names: Sequence[str], what: str):
    """One side's variants (``fetch_variants``: each record fetched once), its code matrix and the samples its records carry.
    Returns ``(RectSide without alt_freqs, carried sample tuple)``.  Refused with LdxError: no matching record at all, a record
    without any selected sample, mixed ploidy, records that carry different samples."""
    cv = fetch_variants(vcf, chrom, chrom_rows, sample_names)
    keep = [k for k, rec in enumerate(cv.recs) if rec is not None]
    if not keep:
        raise LdxError(f"rect_matrix: no variant of the {what} (chromosome {chrom}) has a matching record")
    carried = {carried_samples(cv.recs[k], sample_names) for k in keep}
    if len(carried) != 1:
        raise LdxError(f"rect_matrix: the records of the {what} (chromosome {chrom}) carry different samples; r needs every "
                       "variant over the same haplotypes")
    try:
        codes = codes_matrix([cv.genotypes[k] for k in keep])
    except ZeroDivisionError as exc:   # a record that carries none of the samples
        raise LdxError(f"rect_matrix: a variant of the {what} (chromosome {chrom}) has no genotype of the selected samples") from exc
    except RaggedGenotypesError as exc:
        raise LdxError(f"rect_matrix: mixed ploidy among the {what} (chromosome {chrom}: {exc}); signed r needs one haplotype "
                       "count") from exc
    side = RectSide(str(chrom), [cv.rs_ids[k] for k in keep], [cv.poss[k] for k in keep], [cv.recs[k].ref for k in keep],
                    [cv.recs[k].alts[0] for k in keep], [], codes)
    return side, carried.pop()


def read_sides(vcf, chrom_i, rows_i, chrom_j, rows_j, sample_names: Sequence[str]):
    """Both sides, checked against each other -- everything ``rect_matrix`` does before it touches the device.  ``vcf``: one
    open VCF for both sides, or a pair (the rows' file, the columns' file) when the chromosomes live in separate files."""
    vcf_i, vcf_j = vcf if isinstance(vcf, (tuple, list)) else (vcf, vcf)
    side_i, carried_i = read_side(vcf_i, chrom_i, rows_i, sample_names, "rows")
    side_j, carried_j = read_side(vcf_j, chrom_j, rows_j, sample_names, "columns")
    if carried_i != carried_j:
        raise LdxError(f"rect_matrix: the samples differ between the two sides ({len(carried_i)} carried by the rows' records, "
                       f"{len(carried_j)} by the columns'); r needs both over the same haplotypes")
    if side_i.codes.shape[1] != side_j.codes.shape[1]:
        raise LdxError(f"rect_matrix: mixed ploidy between the two sides ({side_i.codes.shape[1]} haplotypes in the rows, "
                       f"{side_j.codes.shape[1]} in the columns); signed r needs one haplotype count")
    return side_i, side_j


def rect_matrix(vcf, chrom_i, rows_i: Sequence[Sequence], chrom_j, rows_j: Sequence[Sequence], sample_names: Sequence[str],
                dosage: bool = False, missing=None) -> RectMatrix:
    """Signed r of the variants ``rows_i`` of chromosome ``chrom_i`` against the variants ``rows_j`` of ``chrom_j`` (VCF rows
    [pos, rsID], as for ``r_matrix``; the same chromosome twice for two rsID lists).  ``dosage``: genotype-dosage r over the
    samples (a missing call counts as REF; even haplotype count).  ``missing="pairwise"``: every pair over the calls present
    at both variants (``ops.ld_rect``; missing and multi-allelic calls are left out pair by pair, as PLINK --r2 does).  Mixed
    ploidy and samples that differ between the two sides are out of scope: LdxError."""
    if missing is not None and missing != "pairwise":
        raise LdxError(f'rect_matrix: missing must be None or "pairwise", got {missing!r}')
    side_i, side_j = read_sides(vcf, chrom_i, rows_i, chrom_j, rows_j, sample_names)
    pi, pj = PackedPanel.from_codes(side_i.codes), PackedPanel.from_codes(side_j.codes)
    r = ld_rect(pi, pj, dosage=dosage, missing=missing)
    side_i.alt_freqs = pi.alt_freq4().cpu().numpy().tolist()
    side_j.alt_freqs = pj.alt_freq4().cpu().numpy().tolist()
    return RectMatrix(side_i, side_j, bool(dosage), r, missing)


def write_variants(path: str, side: RectSide) -> None:
    """A side's variant list in the ``VARIANTS_HEADER`` format of drivers/rmatrix.py: one line per matrix row / column."""
    freqs = side.alt_freqs if side.alt_freqs else [""] * side.n
    with open(path, "w") as out:
        out.write(VARIANTS_HEADER)
        for k in range(side.n):
            out.write(f"{k}\t{side.rs_ids[k]}\t{side.poss[k]}\t{side.refs[k]}\t{side.alts[k]}\t{freqs[k]}\n")


def write_rect_matrix(base: str, m: RectMatrix, rows_per_block: int = 1024) -> List[str]:
    """``{base}.npy``: the float32 [n_i, n_j] matrix, written in blocks of rows through a memory map; ``{base}.rows.tsv`` and
    ``{base}.cols.tsv``: the variants of the rows and of the columns.  Returns the three paths."""
    n_i, n_j = m.rows.n, m.cols.n
    npy, rows_tsv, cols_tsv = base + ".npy", base + ".rows.tsv", base + ".cols.tsv"
    mm = np.lib.format.open_memmap(npy, mode="w+", dtype=np.float32, shape=(n_i, n_j))
    try:
        for r0 in range(0, n_i, rows_per_block):
            r1 = min(n_i, r0 + rows_per_block)
            block = m.r[r0:r1]
            mm[r0:r1] = block.cpu().numpy() if hasattr(block, "cpu") else np.asarray(block, dtype=np.float32)
        mm.flush()
    finally:
        del mm
    write_variants(rows_tsv, m.rows)
    write_variants(cols_tsv, m.cols)
    return [npy, rows_tsv, cols_tsv]

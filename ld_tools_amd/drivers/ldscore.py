"""LD scores of one chromosome in the LDSC file layout: for every variant the sum of r^2 over the variants within
``window_bp`` of it (itself included), optionally per annotation category -- the ``l2`` files that LD score regression and
stratified LDSC read.  Not a reference workflow: it takes the inputs of drivers/rmatrix.py and runs ops.ld_score on the
matrix-pipe band (include/ldx.h, ldx_ld_score_dev).

Two modes.  By default r is the haplotype-based correlation of the ALT-allele indicators with n = n_hap (include/ldx.h,
LDX_OUT_R32), and the unbiased estimate (``adjust``) uses n_obs = n_hap: the right r for a phased reference panel, close to
``ldsc.py --l2``'s values but not identical.  With ``dosage=True`` r is the genotype correlation of the ALT dosages 0 / 1 / 2
over the N = n_hap / 2 samples (include/ldx.h, ldx_ld_score_dosage_dev) -- phase-free, so it also suits unphased calls -- with
n_obs = N and ``M_5_50`` from the dosage allele frequency a / (2 N): the quantities ``ldsc.py --l2`` computes.  LDSC has no
missing genotypes; here a missing call would count as REF, so a panel with one is refused unless ``missing="ref"`` says so.
``missing="pairwise"`` (either mode) takes every pair's r over the calls present at both variants instead, as PLINK --r2 does
(ops.ld_score(missing="pairwise")); n_obs stays n_hap, or N with ``dosage``.
"""
from __future__ import annotations

import gzip
from dataclasses import dataclass
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np

from .._lib import LdxError
from ..ops import LDScores, ld_score
from ..panel import PackedPanel
from .ingest import RaggedGenotypesError, codes_matrix, haplotype_columns
from .triangle import fetch_variants


@dataclass
class LDScoreTable:
    """Row k is variant k of these lists (position-sorted; variants without a matching record are left out)."""

    chrom: str
    rs_ids: List[str]
    poss: List[int]
    alt_freqs_exact: np.ndarray       # float64 a / n_hap per variant (the MAF filter of M_5_50; dosage: a / (2 N), the same number)
    annot: Optional[np.ndarray]       # bool [n, K] in row order, or None
    annot_names: List[str]
    scores: LDScores
    adjust: bool

    @property
    def n(self) -> int:
        return len(self.rs_ids)

    def values(self) -> np.ndarray:
        """float64 [n, K or 1]: the written columns (the per-category columns with an annotation, else column 0)."""
        v = self.scores.adjusted() if self.adjust else self.scores.l2
        return v[:, 1:] if self.annot is not None else v[:, :1]


def _fetch_panel(what, vcf, chrom, chrom_rows, sample_names, annot, annot_names):
    """One fetch_variants pass and one packed panel: (cv, kept variant indices, annot rows of the kept variants or None,
    column names, panel)."""
    order = sorted(range(len(chrom_rows)), key=lambda k: chrom_rows[k][0])   # fetch_variants' stable sort
    cv = fetch_variants(vcf, chrom, chrom_rows, sample_names)
    keep = [k for k, rec in enumerate(cv.recs) if rec is not None]
    if not keep:
        raise LdxError(f"{what}: no variant of chromosome {chrom} has a matching record")
    ann = None
    names: List[str] = []
    if annot is not None:
        a = np.asarray(annot)
        if a.ndim == 1:
            a = a[:, None]
        if a.shape[0] != len(chrom_rows):
            raise LdxError(f"{what}: annot needs one row per input row")
        if a.dtype != bool and not np.isin(a, (0, 1)).all():
            raise LdxError(f"{what}: annot must be boolean or 0/1")
        ann = a.astype(bool)[np.asarray(order, dtype=np.int64)][np.asarray(keep, dtype=np.int64)]
        names = list(annot_names) if annot_names is not None else [f"A{k}" for k in range(ann.shape[1])]
        if len(names) != ann.shape[1]:
            raise LdxError(f"{what}: one name per annotation column")
    try:
        codes = codes_matrix([cv.genotypes[k] for k in keep])
    except ZeroDivisionError as exc:   # a record that carries none of the samples
        raise LdxError(f"{what}: a variant of chromosome {chrom} has no genotype of the selected samples") from exc
    except RaggedGenotypesError as exc:
        raise LdxError(f"{what}: mixed ploidy on chromosome {chrom} ({exc}); LD scores need one haplotype count") from exc
    return cv, keep, ann, names, PackedPanel.from_codes(codes)


def _check_missing_arg(what: str, dosage: bool, missing: Optional[str]) -> None:
    if missing not in (None, "ref", "pairwise"):
        raise LdxError(f"{what}: missing must be None, 'ref' or 'pairwise' (got {missing!r})")
    if missing == "ref" and not dosage:
        raise LdxError(f"{what}: missing='ref' belongs to dosage=True (the haplotype r leaves such calls out of both counts)")


def _pairwise(missing: Optional[str]) -> Optional[str]:
    """The ``missing`` argument of the operators: "pairwise" or None ("ref" is this module's acceptance of their own rule)."""
    return "pairwise" if missing == "pairwise" else None


def _check_complete(what: str, panel: PackedPanel, chrom, missing: Optional[str]) -> None:
    """dosage mode: every call must be REF or the first ALT allele unless the caller accepted the REF imputation."""
    if missing in ("ref", "pairwise"):
        return
    short = panel.alt_counts().astype(np.int64) + panel.ref_counts().astype(np.int64) < panel.n_hap
    if short.any():
        raise LdxError(f"{what}: {int(short.sum())} variant(s) of chromosome {chrom} carry a call that is neither REF nor the "
                       "first ALT allele (missing or multi-allelic); the dosage counts it as REF -- pass missing='ref' to "
                       "accept that")


def ld_scores(vcf, chrom, chrom_rows: Sequence[Sequence], sample_names: Sequence[str], window_bp: int = 1_000_000,
              annot=None, annot_names: Optional[Sequence[str]] = None, adjust: bool = True, dosage: bool = False,
              missing: Optional[str] = None) -> LDScoreTable:
    """LD scores of one chromosome's variants, from the inputs of ``r_matrix`` (VCF rows [pos, rsID]; each record fetched
    once).  ``annot``: bool / 0-1 [len(chrom_rows), K], K <= 8, one row per input row; ``annot_names``: K column names
    (default A0, A1, ...).  ``adjust``: write LDSC's unbiased r^2 (LDScores.adjusted) rather than r^2.  Mixed-ploidy panels
    (genotype lists of different lengths) are out of scope: LdxError.  ``dosage``: genotype-dosage r over the samples, n_obs =
    N (the module docstring); a kept variant with a call that is neither REF nor the first ALT allele (a + r < n) then raises
    LdxError unless ``missing="ref"`` accepts that such calls count as REF.  ``missing="pairwise"``: pairwise-complete r."""
    _check_missing_arg("ld_scores", dosage, missing)
    cv, keep, ann, names, panel = _fetch_panel("ld_scores", vcf, chrom, chrom_rows, sample_names, annot, annot_names)
    poss = [cv.poss[k] for k in keep]
    if dosage:
        _check_complete("ld_scores", panel, chrom, missing)
    res = ld_score(panel, np.asarray(poss, dtype=np.int64), window_bp=window_bp, annot=ann, dosage=dosage, missing=_pairwise(missing))
    fa = panel.alt_counts().astype(np.float64) / panel.n_hap
    return LDScoreTable(str(chrom), [cv.rs_ids[k] for k in keep], poss, fa, ann, names, res, adjust)


def ld_scores_by_group(vcf, chrom, chrom_rows: Sequence[Sequence], groups: Mapping[str, Sequence[str]],
                       window_bp: int = 1_000_000, annot=None, annot_names: Optional[Sequence[str]] = None,
                       adjust: bool = True, dosage: bool = False, missing: Optional[str] = None) -> Dict[str, LDScoreTable]:
    """``ld_scores`` for several sample groups (label -> sample names: populations, genders) of one chromosome from ONE pass
    over the VCF: the union of the groups is fetched and packed once, each group is then a haplotype subset of that panel
    taken on the device (PackedPanel.select) and scored.  Every table equals ``ld_scores`` on its group alone.  The other
    arguments are those of ``ld_scores``.  The samples must be diploid in every record (a panel whose haplotype count is not
    twice the number of carried samples -- haploid or mixed-ploidy calls -- is an LdxError), and a group none of whose
    samples is carried is one too.  ``dosage`` / ``missing`` as for ``ld_scores`` (a group's columns are whole samples, so
    its individuals stay pairs of adjacent haplotypes)."""
    what = "ld_scores_by_group"
    _check_missing_arg(what, dosage, missing)
    if not groups:
        raise LdxError(f"{what}: no groups")
    union = list(dict.fromkeys(name for members in groups.values() for name in members))
    cv, keep, ann, names, panel = _fetch_panel(what, vcf, chrom, chrom_rows, union, annot, annot_names)
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
    tables: Dict[str, LDScoreTable] = {}
    for label, members in groups.items():
        cols = haplotype_columns(carried, members)
        if cols.size == 0:
            raise LdxError(f"{what}: no sample of group {label!r} is carried by the records of chromosome {chrom}")
        sub = panel.select(haplotypes=cols)
        res = ld_score(sub, pos, window_bp=window_bp, annot=ann, dosage=dosage, missing=_pairwise(missing))
        fa = sub.alt_counts().astype(np.float64) / sub.n_hap
        tables[label] = LDScoreTable(str(chrom), list(rs_ids), list(poss), fa, ann, list(names), res, adjust)
    return tables


def write_ldscore(base: str, table: LDScoreTable) -> List[str]:
    """``{base}.l2.ldscore.gz``: tab-separated CHR, SNP, BP and one column per category ({name}L2; L2 without an
    annotation), values as %.3f, degenerate variants (no ALT or no REF allele; a dosage table: no variance among the samples'
    dosages) left out; ``{base}.l2.M``: one line, per
    column the number of written variants in the category; ``{base}.l2.M_5_50``: the same for MAF = min(fa, 1 - fa) > 0.05.
    Returns the three paths."""
    live = table.scores.live
    vals = table.values()
    cols = [f"{nm}L2" for nm in table.annot_names] if table.annot is not None else ["L2"]
    inc = table.annot if table.annot is not None else np.ones((table.n, 1), dtype=bool)
    fa = np.asarray(table.alt_freqs_exact, dtype=np.float64)
    common = np.minimum(fa, 1.0 - fa) > 0.05
    gz, mp, m550 = base + ".l2.ldscore.gz", base + ".l2.M", base + ".l2.M_5_50"
    with gzip.open(gz, "wt") as out:
        out.write("\t".join(["CHR", "SNP", "BP"] + cols) + "\n")
        for k in np.flatnonzero(live):
            out.write("\t".join([table.chrom, table.rs_ids[k], str(table.poss[k])] + ["%.3f" % x for x in vals[k]]) + "\n")
    with open(mp, "w") as out:
        out.write("\t".join(str(int((inc[:, c] & live).sum())) for c in range(inc.shape[1])) + "\n")
    with open(m550, "w") as out:
        out.write("\t".join(str(int((inc[:, c] & live & common).sum())) for c in range(inc.shape[1])) + "\n")
    return [gz, mp, m550]

"""PLINK binary filesets as a source and a sink: ``load_bfile`` opens ``prefix.bed/.bim/.fam`` and unpacks the genotype rows
on the device (PackedPanel.from_bed: the file's own bytes, no per-allele codes), and the ``bfile_*`` drivers fill the table
dataclasses of the VCF drivers from it, so that their writers write them unchanged:

    bfile_ld_table   -> (RectSide, LDRectHits) for write_ld_table          PLINK --r2 dprime --ld-window-kb --ld-window-r2
    bfile_clump      -> ClumpTable for write_clumped                       PLINK --clump
    bfile_prune      -> PruneTable for write_prune                         (priority pruning; cf. --indep-pairwise)
    bfile_ld_scores  -> LDScoreTable for write_ldscore                     ldsc.py --l2
    bfile_band       -> BandMatrix for write_band
    bfile_em_band    -> EmBand for write_em_band
    bfile_blocks     -> GabrielTable for write_gabriel_blocks              PLINK --blocks (Gabriel et al.'s D' interval rule)
    bfile_king       -> KingTable for write_kin0 / write_king_cutoff       PLINK 2 --make-king-table / --king-cutoff
    bfile_pca        -> PcaTable for write_eigenvec / write_eigenval       PLINK 2 --pca approx
    bfile_grm        -> GrmTable for write_grm_bin / write_rel             GCTA --make-grm / --grm-cutoff, PLINK 2 --make-rel
    bfile_score      -> ScoreTable for write_sscore                        PLINK --score (sums)
    bfile_glm        -> GlmTables for write_glm_linear                     PLINK 2 --glm (quantitative traits, mean imputation)
    bfile_logistic   -> LogisticTables for write_glm_logistic              PLINK 2 --glm (case/control traits, no Firth fallback)
                        (firth=: write_glm_hybrid / write_glm_firth         PLINK 2 --glm firth-fallback / firth)
    bfile_hardy      -> HardyResult for write_hardy                        PLINK --hardy (exact test, per group)
    bfile_missing    -> write_vmiss / write_smiss / write_test_missing     PLINK 2 --missing, PLINK --test-missing
    bfile_het        -> SampleQC for write_het                             PLINK --het
    bfile_model      -> ModelResult for write_model / write_assoc_fisher   PLINK --model, --assoc fisher
    bfile_mperm      -> MpermTable for write_assoc_mperm                   PLINK --assoc mperm=N, --model trend mperm=N (max(T))
    bfile_qc         -> QcMasks (.qc.in / .qc.out / .qc.keep)              PLINK --mind --geno --maf --hwe

A ``.bed`` holds unphased genotype calls: a het is written (ALT, REF) whatever the truth, so the haplotype r of the phased
operators means nothing here.  Every driver defaults to an unphased form (EM or genotype dosage) and refuses
``dosage=False, em=False``.  ``make_bed`` writes a panel, or a subset of a loaded fileset, back as a fileset.

    python -m ld_tools_amd.drivers.plink {ld,clump,prune,l2,blocks,king,grm,pca,score,glm,logistic,hardy,missing,het,model,mperm,qc,make-bed}
        --bfile P --out O ...
"""
from __future__ import annotations

import argparse
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from .. import plink
from .._lib import LdxError
from ..ops import ld_band, ld_clump, ld_em_band, ld_gabriel_blocks, ld_neighbors, ld_prune, ld_score
from ..panel import PackedPanel, select_index
from .band import BandMatrix
from .blocks import GabrielTable
from .clump import ClumpTable
from .em import EmBand
from .ldscore import LDScoreTable, _check_complete, _check_missing_arg, _pairwise
from .prune import PruneTable
from .rect import RectSide


@dataclass
class Bfile:
    """A loaded fileset: the panel, the ``.bim`` columns of its variants (row k of the panel is entry k) and the ``.fam``
    columns of its individuals (individual k owns haplotypes 2k and 2k + 1).  ``alt``: which allele is code 1."""

    prefix: str
    panel: PackedPanel
    alt: str
    chrom: List[str]
    ids: List[str]
    cm: np.ndarray
    pos: np.ndarray
    a1: List[str]
    a2: List[str]
    fid: List[str]
    iid: List[str]
    father: List[str]
    mother: List[str]
    sex: List[str]
    pheno: List[str]

    @property
    def n(self) -> int:
        return len(self.ids)

    @property
    def alts(self) -> List[str]:
        """The allele that code 1 stands for, per variant."""
        return self.a1 if self.alt == "a1" else self.a2

    @property
    def refs(self) -> List[str]:
        return self.a2 if self.alt == "a1" else self.a1

    def bim(self, snps=None) -> dict:
        k = list(range(self.n)) if snps is None else [int(i) for i in snps]
        return {"chrom": [self.chrom[i] for i in k], "ids": [self.ids[i] for i in k], "cm": self.cm[k], "pos": self.pos[k],
                "a1": [self.a1[i] for i in k], "a2": [self.a2[i] for i in k]}

    def fam(self, individuals=None) -> dict:
        k = list(range(len(self.iid))) if individuals is None else [int(i) for i in individuals]
        return {name: [getattr(self, name)[i] for i in k] for name in ("fid", "iid", "father", "mother", "sex", "pheno")}


def _is_names(x, pairs: bool) -> bool:
    """A selection given by name: a non-empty list of strings (variant IDs) or of (FID, IID) pairs."""
    if isinstance(x, np.ndarray) and x.dtype.kind not in "USO":
        return False
    try:
        first = next(iter(x))
    except (TypeError, StopIteration):
        return False
    if pairs:
        return isinstance(first, (tuple, list)) and len(first) == 2 and all(isinstance(v, str) for v in first)
    return isinstance(first, str)


def _by_name(wanted, have: Sequence, what: str) -> np.ndarray:
    where = {}
    for k, name in enumerate(have):
        where.setdefault(name, k)          # a repeated name means its first entry
    wanted = [tuple(w) if isinstance(w, (tuple, list)) else w for w in wanted]
    unknown = [w for w in wanted if w not in where]
    if unknown:
        raise LdxError(f"load_bfile: {len(unknown)} unknown {what}(s), the first: {unknown[0]!r}")
    return np.asarray([where[w] for w in wanted], dtype=np.int64)


def load_bfile(prefix, chrom=None, keep=None, extract=None, maf_min: Optional[float] = None,
               geno_max: Optional[float] = None, alt: str = "a1") -> Bfile:
    """Open ``prefix.bed/.bim/.fam`` (or a ``plink.BedFile``) and unpack it on the device.
    ``chrom``: keep the variants with this ``.bim`` chromosome; their positions must be non-decreasing.
    ``extract``: variants as an index array / mask over the ``.bim`` lines or a list of variant IDs; ``keep``: individuals as
    an index array / mask over the ``.fam`` lines or a list of (FID, IID) pairs; an unknown name raises.  With ``chrom``,
    ``extract`` is applied first and must name variants of that chromosome only.
    ``maf_min`` / ``geno_max``: PLINK's --maf / --geno, from the kept individuals' counts after the unpack: a variant stays
    when min(a, r) / (a + r) >= maf_min and 1 - (a + r) / n_hap <= geno_max (an all-missing variant has no MAF and goes with
    --maf).  ``alt``: the allele that becomes code 1, "a1" (PLINK's and LDSC's counted allele) or "a2"."""
    bed = prefix if isinstance(prefix, plink.BedFile) else plink.BedFile(prefix)
    snps = None
    if extract is not None:
        snps = _by_name(extract, bed.ids, "variant ID") if _is_names(extract, False) else \
            select_index(extract, bed.n_snps, "SNP").astype(np.int64)
    if chrom is not None:
        on = np.asarray([c == str(chrom) for c in bed.chrom])
        if snps is None:
            snps = np.flatnonzero(on)
        elif not on[snps].all():
            raise LdxError(f"load_bfile: extract names variants outside chromosome {chrom}")
        if snps.size == 0:
            raise LdxError(f"load_bfile: no variant of chromosome {chrom} in {bed.prefix}.bim")
        if snps.size > 1 and (np.diff(bed.pos[snps]) < 0).any():
            raise LdxError(f"load_bfile: the positions of chromosome {chrom} are not in non-decreasing order")
    inds = None
    if keep is not None:
        inds = _by_name(keep, list(zip(bed.fid, bed.iid)), "(FID, IID) pair") if _is_names(keep, True) else \
            select_index(keep, bed.n_ind, "individual").astype(np.int64)
    panel = PackedPanel.from_bed(bed, keep=inds, extract=snps, alt=alt)
    snps = np.arange(bed.n_snps) if snps is None else snps
    if maf_min is not None or geno_max is not None:
        a, r = panel.alt_counts().astype(np.int64), panel.ref_counts().astype(np.int64)
        ok = np.ones(a.size, dtype=bool)
        if maf_min is not None:
            ok &= np.minimum(a, r) >= float(maf_min) * (a + r)
            ok &= (a + r) > 0
        if geno_max is not None:
            ok &= (panel.n_hap - a - r) <= float(geno_max) * panel.n_hap
        if not ok.any():
            raise LdxError("load_bfile: no variant passes maf_min / geno_max")
        if not ok.all():
            panel = panel.select(snps=ok)
            snps = snps[ok]
    b, f = bed.bim(snps), bed.fam(inds)
    return Bfile(bed.prefix, panel, alt, b["chrom"], b["ids"], np.asarray(b["cm"]), np.asarray(b["pos"], dtype=np.int64),
                 b["a1"], b["a2"], f["fid"], f["iid"], f["father"], f["mother"], f["sex"], f["pheno"])


def _unphased(what: str, dosage: Optional[bool], em: Optional[bool], default: str):
    """(dosage, em) of a driver call: None, None -> the driver's default form; one given -> the other off; both off -> the
    haplotype r, which a .bed cannot give."""
    if dosage is None and em is None:
        return default == "dosage", default == "em"
    dosage, em = bool(dosage), bool(em)
    if not dosage and not em:
        raise LdxError(f"{what}: dosage=False, em=False asks for the haplotype r, and a .bed carries no phase (a het is "
                       "stored without an order); use em=True or dosage=True")
    if dosage and em:
        raise LdxError(f"{what}: dosage and em are two different estimates; choose one")
    return dosage, em


def _one_chrom(what: str, bf: Bfile) -> str:
    chroms = list(dict.fromkeys(bf.chrom))
    if len(chroms) != 1:
        raise LdxError(f"{what}: the fileset holds chromosomes {chroms[:4]}...; load one with load_bfile(chrom=)")
    if bf.n > 1 and (np.diff(bf.pos) < 0).any():
        raise LdxError(f"{what}: the positions of chromosome {chroms[0]} are not in non-decreasing order")
    return chroms[0]


def _loaded(src, **load) -> Bfile:
    return src if isinstance(src, Bfile) else load_bfile(src, **load)


def _poss(bf: Bfile) -> List[int]:
    return [int(p) for p in bf.pos]


def bfile_ld_table(src, r2: float = 0.2, window_bp: int = 1_000_000, missing: Optional[str] = None,
                   em: Optional[bool] = None, dosage: Optional[bool] = None, **load):
    """drivers/em.py's ``em_window_hits`` from a fileset: the in-window pairs with EM r^2 >= ``r2``, each once, as
    (RectSide, LDRectHits) for ``write_ld_table``.  The table holds D', so the EM form is the only one."""
    import torch

    bf = _loaded(src, **load)
    dosage, em = _unphased("bfile_ld_table", dosage, em, "em")
    if not em:
        raise LdxError("bfile_ld_table: the .ld table holds D', which only the EM form (em=True) estimates")
    chrom = _one_chrom("bfile_ld_table", bf)
    nb = ld_neighbors(bf.panel, bf.pos, window_bp=window_bp, r2=r2, missing=missing, em=True)
    once = nb.hits[nb.hits[:, 0] < nb.hits[:, 1]].contiguous()
    offsets = torch.zeros(nb.n_snps + 1, dtype=torch.int32, device=once.device)
    offsets[1:] = torch.cumsum(torch.bincount(once[:, 0].to(torch.int64), minlength=nb.n_snps), 0).to(torch.int32)
    from ..ops import LDRectHits

    side = RectSide(chrom, list(bf.ids), _poss(bf), [], [], bf.panel.alt_freq4().cpu().numpy().tolist(), None)
    return side, LDRectHits(offsets, once, nb.n_snps, nb.n_snps, nb.bound, False, True, missing=missing)


def bfile_clump(src, pvalues: Sequence[float], p1: float = 1e-4, p2: float = 1e-2, r2: float = 0.5,
                window_bp: int = 250_000, dosage: Optional[bool] = None, em: Optional[bool] = None,
                missing: Optional[str] = None, **load) -> ClumpTable:
    """drivers/clump.py's ``clump`` from a fileset; one p-value per variant of the loaded fileset.  Default: the EM r
    (``missing="pairwise"`` makes it PLINK --clump's own r^2)."""
    bf = _loaded(src, **load)
    dosage, em = _unphased("bfile_clump", dosage, em, "em")
    chrom = _one_chrom("bfile_clump", bf)
    p = np.asarray(pvalues, dtype=np.float64)
    if p.shape != (bf.n,):
        raise LdxError("bfile_clump: one p-value per variant is needed")
    more = {} if missing is None else {"missing": missing}
    res = ld_clump(bf.panel, bf.pos, p, p1=p1, p2=p2, r2=r2, window_bp=window_bp, dosage=dosage, em=em, **more)
    return ClumpTable(chrom, list(bf.ids), _poss(bf), p, res)


def bfile_prune(src, r2: float = 0.2, window_bp: int = 250_000, priority: Optional[Sequence[float]] = None,
                dosage: Optional[bool] = None, em: Optional[bool] = None, missing: Optional[str] = None, **load) -> PruneTable:
    """drivers/prune.py's ``prune`` from a fileset.  Default: the genotype-dosage r, PLINK's own."""
    bf = _loaded(src, **load)
    dosage, em = _unphased("bfile_prune", dosage, em, "dosage")
    chrom = _one_chrom("bfile_prune", bf)
    pr = None if priority is None else np.asarray(priority, dtype=np.float64)
    if pr is not None and pr.shape != (bf.n,):
        raise LdxError("bfile_prune: one priority per variant is needed")
    more = {} if missing is None else {"missing": missing}
    res = ld_prune(bf.panel, bf.pos, r2=r2, window_bp=window_bp, priority=pr, dosage=dosage, em=em, **more)
    return PruneTable(chrom, list(bf.ids), _poss(bf), res)


def _dosage_only(what: str, dosage, em) -> None:
    dosage, em = _unphased(what, dosage, em, "dosage")
    if em:
        raise LdxError(f"{what}: this operator has no EM form; use dosage=True")


def bfile_ld_scores(src, window_bp: int = 1_000_000, annot=None, annot_names: Optional[Sequence[str]] = None,
                    adjust: bool = True, dosage: Optional[bool] = None, em: Optional[bool] = None,
                    missing: Optional[str] = None, **load) -> LDScoreTable:
    """drivers/ldscore.py's ``ld_scores`` from a fileset (dosage form: ldsc.py --l2's quantities).  ``annot``: bool / 0-1
    [n, K], one row per variant of the loaded fileset.  A missing call needs ``missing="ref"`` or ``"pairwise"``."""
    bf = _loaded(src, **load)
    _dosage_only("bfile_ld_scores", dosage, em)
    _check_missing_arg("bfile_ld_scores", True, missing)
    chrom = _one_chrom("bfile_ld_scores", bf)
    ann, names = None, []
    if annot is not None:
        a = np.asarray(annot)
        a = a[:, None] if a.ndim == 1 else a
        if a.shape[0] != bf.n:
            raise LdxError("bfile_ld_scores: annot needs one row per variant")
        if a.dtype != bool and not np.isin(a, (0, 1)).all():
            raise LdxError("bfile_ld_scores: annot must be boolean or 0/1")
        ann = a.astype(bool)
        names = list(annot_names) if annot_names is not None else [f"A{k}" for k in range(ann.shape[1])]
        if len(names) != ann.shape[1]:
            raise LdxError("bfile_ld_scores: one name per annotation column")
    _check_complete("bfile_ld_scores", bf.panel, chrom, missing)
    res = ld_score(bf.panel, bf.pos, window_bp=window_bp, annot=ann, dosage=True, missing=_pairwise(missing))
    fa = bf.panel.alt_counts().astype(np.float64) / bf.panel.n_hap
    return LDScoreTable(chrom, list(bf.ids), _poss(bf), fa, ann, names, res, adjust)


def bfile_band(src, window_bp: int = 1_000_000, dosage: Optional[bool] = None, em: Optional[bool] = None,
               missing: Optional[str] = None, **load) -> BandMatrix:
    """drivers/band.py's ``band_matrix`` from a fileset: the stored band of the genotype-dosage r."""
    bf = _loaded(src, **load)
    _dosage_only("bfile_band", dosage, em)
    _check_missing_arg("bfile_band", True, missing)
    chrom = _one_chrom("bfile_band", bf)
    _check_complete("bfile_band", bf.panel, chrom, missing)
    band = ld_band(bf.panel, bf.pos, window_bp=window_bp, dosage=True, missing=_pairwise(missing))
    return BandMatrix(chrom, list(bf.ids), _poss(bf), list(bf.refs), list(bf.alts),
                      bf.panel.alt_freq4().cpu().numpy().tolist(), band)


def bfile_em_band(src, window_bp: int = 1_000_000, missing: Optional[str] = None, em: Optional[bool] = None,
                  dosage: Optional[bool] = None, **load) -> EmBand:
    """drivers/em.py's ``em_band`` from a fileset: the stored EM r and D' bands."""
    bf = _loaded(src, **load)
    dosage, em = _unphased("bfile_em_band", dosage, em, "em")
    if not em:
        raise LdxError("bfile_em_band: the EM band is em=True by definition; bfile_band stores the dosage r")
    chrom = _one_chrom("bfile_em_band", bf)
    bands = ld_em_band(bf.panel, bf.pos, window_bp=window_bp, missing=missing)
    return EmBand(chrom, list(bf.ids), _poss(bf), bf.panel.alt_freq4().cpu().numpy().tolist(), bands)


def bfile_blocks(src, window_bp: int = 500_000, missing: Optional[str] = "pairwise", maf_min: float = 0.05, keep_snps=None,
                 **more) -> GabrielTable:
    """Gabriel's D' confidence-interval blocks of a fileset, for ``write_gabriel_blocks``: ops.ld_gabriel_blocks on the genotype
    calls -- the operator is unphased by definition, so a .bed is its natural input.  ``missing``: "pairwise" (the default:
    every pair over the individuals called at both variants, as PLINK treats missing calls) or None (a missing call counts as
    REF).  ``keep_snps``: bool [n] over the loaded variants; ``more``: load_bfile's arguments and the block parameters
    (ops.GABRIEL_DEFAULTS)."""
    from ..ops import GABRIEL_DEFAULTS

    params = {k: more.pop(k) for k in list(more) if k in GABRIEL_DEFAULTS}
    bf = _loaded(src, **more)
    chrom = _one_chrom("bfile_blocks", bf)
    res = ld_gabriel_blocks(bf.panel, bf.pos, window_bp=window_bp, missing=missing, keep=keep_snps, maf_min=maf_min, **params)
    return GabrielTable(chrom, list(bf.ids), _poss(bf), res)


def bfile_king(src, out: Optional[str] = None, keep=None, extract=None, prune_r2: Optional[float] = None,
               prune_window_bp: int = 250_000, prune_missing: Optional[str] = None, kin_min: Optional[float] = None,
               cutoff: Optional[float] = None, matrix: bool = False, **load):
    """drivers/king.py's ``king_table`` from a fileset: the pair counts between its individuals, IDs from the ``.fam``.
    ``keep`` / ``extract``: load_bfile's selections of individuals and variants.  ``prune_r2``: count over the variants
    ``ld_prune`` keeps at this r^2 (genotype-dosage r, ``prune_window_bp``; ``prune_missing="pairwise"`` for a fileset with
    missing calls) -- the mask goes to the count as ``keep``, no panel is rebuilt; the fileset must then hold one chromosome.
    ``out``: a prefix to write ``.kin0`` under (pairs with kinship >= ``kin_min``, all by default), ``.king`` / ``.king.id``
    with ``matrix`` and ``.king.cutoff.in.id`` / ``.out.id`` with ``cutoff``.  Returns the KingTable."""
    from .king import KingTable, write_kin0, write_king_cutoff, write_king_matrix
    from ..ops import sample_counts

    if isinstance(src, Bfile):
        if keep is not None or extract is not None or load:
            raise LdxError("bfile_king: a loaded fileset takes no keep / extract / load arguments")
        bf = src
    else:
        bf = load_bfile(src, keep=keep, extract=extract, **load)
    mask = None
    if prune_r2 is not None:
        _one_chrom("bfile_king", bf)
        more = {} if prune_missing is None else {"missing": prune_missing}
        mask = ld_prune(bf.panel, bf.pos, r2=prune_r2, window_bp=prune_window_bp, dosage=True, **more).keep
    table = KingTable(list(bf.fid), list(bf.iid), sample_counts(bf.panel, keep=mask), kin_min, mask)
    if out is not None:
        write_kin0(out + ".kin0", table)
        kin = table.counts.kinship() if (matrix or cutoff is not None) else None
        if matrix:
            write_king_matrix(out, table, kin.cpu().numpy())
        if cutoff is not None:
            write_king_cutoff(out, table, cutoff, kin)
    return table


GRM_CHUNK_SNPS = 65536            # variants of a fileset that bfile_grm holds on the device at a time


def bfile_grm(src, out: Optional[str] = None, keep=None, extract=None, chrom=None, maf_min: Optional[float] = None,
              cutoff: Optional[float] = None, fmt: str = "gcta", chunk_snps: int = GRM_CHUNK_SNPS, alt: str = "a1"):
    """drivers/grm.py's ``grm_table`` from a fileset: the genetic relationship matrix of its individuals over the live variants
    (``maf_min``: the MAF bound among the called), IDs from the ``.fam``.  A fileset given by its prefix (or a
    ``plink.BedFile``) is STREAMED, ``chunk_snps`` variants at a time, in two passes over the file: the first takes every
    chunk's SNP counts and from them the ONE exponent of the coefficients, the second accumulates S and N over the chunks, each
    with the weights of its own SNP counts -- the same integers, and so the same files, as one call on the whole panel.
    ``keep`` / ``extract`` / ``chrom`` / ``alt``: load_bfile's selections (all chromosomes count when ``chrom`` is None).  A
    loaded ``Bfile`` is taken as it is, in one piece.  ``out``: a prefix to write under -- ``fmt="gcta"``: ``.grm.bin``,
    ``.grm.N.bin``, ``.grm.id``; ``fmt="rel"``: ``.rel``, ``.rel.id``; with ``cutoff`` also ``.grm.cutoff.in.id`` / ``.out.id``.
    Returns the GrmTable."""
    from .grm import GrmTable, grm_table, write_grm_bin, write_grm_cutoff, write_rel
    from ..ops import geno_snp_counts, grm_coefficients, grm_exponent, ld_grm

    if fmt not in ("gcta", "rel"):
        raise LdxError(f"bfile_grm: fmt must be 'gcta' or 'rel', got {fmt!r}")
    if isinstance(src, Bfile):
        if keep is not None or extract is not None or chrom is not None:
            raise LdxError("bfile_grm: a loaded fileset takes no keep / extract / chrom arguments")
        table = grm_table(src.panel, list(zip(src.fid, src.iid)), maf_min=maf_min)
    else:
        chunk_snps = int(chunk_snps)
        if chunk_snps < 1:
            raise LdxError("bfile_grm: chunk_snps must be positive")
        bed = src if isinstance(src, plink.BedFile) else plink.BedFile(src)
        snps = np.arange(bed.n_snps) if extract is None else (
            _by_name(extract, bed.ids, "variant ID") if _is_names(extract, False) else
            select_index(extract, bed.n_snps, "SNP").astype(np.int64))
        if chrom is not None:
            snps = snps[np.asarray([bed.chrom[i] == str(chrom) for i in snps], dtype=bool)]
        if snps.size == 0:
            raise LdxError("bfile_grm: no variant selected")
        inds = None
        if keep is not None:
            inds = _by_name(keep, list(zip(bed.fid, bed.iid)), "(FID, IID) pair") if _is_names(keep, True) else \
                select_index(keep, bed.n_ind, "individual").astype(np.int64)
        chunks = [snps[k:k + chunk_snps] for k in range(0, snps.size, chunk_snps)]
        load = lambda part: PackedPanel.from_bed(bed, keep=inds, extract=part, alt=alt)  # noqa: E731
        big = 0.0
        for part in chunks:                                   # pass 1: the largest coefficient of the fileset
            x, _ = grm_coefficients(geno_snp_counts(load(part)), None, maf_min)
            big = max(big, float(np.abs(x).max()) if x.size else 0.0)
        res = None
        for part in chunks:                                   # pass 2: the sums
            res = ld_grm(load(part), maf_min=maf_min, out=res, exp=grm_exponent(big))
        f = bed.fam(inds)
        table = GrmTable(list(f["fid"]), list(f["iid"]), res)
    if out is not None:
        (write_grm_bin if fmt == "gcta" else write_rel)(out, table)
        if cutoff is not None:
            write_grm_cutoff(out, table, cutoff)
    return table


def _bfile_and_mask(what: str, src, keep, extract, prune_r2, prune_window_bp, prune_missing, load):
    if isinstance(src, Bfile):
        if keep is not None or extract is not None or load:
            raise LdxError(f"{what}: a loaded fileset takes no keep / extract / load arguments")
        bf = src
    else:
        bf = load_bfile(src, keep=keep, extract=extract, **load)
    mask = None
    if prune_r2 is not None:
        _one_chrom(what, bf)
        more = {} if prune_missing is None else {"missing": prune_missing}
        mask = ld_prune(bf.panel, bf.pos, r2=prune_r2, window_bp=prune_window_bp, dosage=True, **more).keep
    return bf, mask


def bfile_pca(src, out: Optional[str] = None, n_pcs: int = 10, keep=None, extract=None, prune_r2: Optional[float] = None,
              prune_window_bp: int = 250_000, prune_missing: Optional[str] = None, king_cutoff: Optional[float] = None,
              oversample: int = 10, n_iter: int = 10, seed: int = 0, **load):
    """drivers/pca.py's ``pca_table`` from a fileset (PLINK 2's --pca approx): the principal components of its individuals, IDs
    from the ``.fam``.  ``keep`` / ``extract`` / ``prune_r2`` ...: as for bfile_king.  ``king_cutoff``: first drop relatives --
    ops.king_cutoff on the KING-robust kinship over the same variants -- decompose the unrelated individuals and project the
    others on their components.  ``out``: a prefix to write ``.eigenvec`` and ``.eigenval`` under.  Returns the PcaTable."""
    from .pca import pca_table, write_eigenval, write_eigenvec
    from ..ops import king_cutoff as cutoff_set, sample_counts

    bf, mask = _bfile_and_mask("bfile_pca", src, keep, extract, prune_r2, prune_window_bp, prune_missing, load)
    unrelated = None
    if king_cutoff is not None:
        unrelated, _ = cutoff_set(sample_counts(bf.panel, keep=mask).kinship(), king_cutoff)
    table = pca_table(bf.panel, list(zip(bf.fid, bf.iid)), n_pcs=min(int(n_pcs), int(bf.panel.n_ind if unrelated is None else
                                                                                     unrelated.sum())),
                      keep=mask, unrelated=unrelated, oversample=oversample, n_iter=n_iter, seed=seed)
    if out is not None:
        write_eigenvec(out + ".eigenvec", table)
        write_eigenval(out + ".eigenval", table)
    return table


def read_score_file(path: str) -> tuple:
    """(ids, alleles, weights float64 [lines, k]) of a whitespace table: variant ID, allele, one or more weights per line; a first
    line whose third field is no number is a header."""
    ids, alleles, rows = [], [], []
    with open(path) as f:
        for no, line in enumerate(f):
            parts = line.split()
            if not parts:
                continue
            if len(parts) < 3:
                raise LdxError(f"{path}: a line with fewer than 3 fields")
            try:
                vals = [float(v) for v in parts[2:]]
            except ValueError:
                if no == 0:
                    continue
                raise LdxError(f"{path}: line {no + 1}: a weight that is no number") from None
            if rows and len(vals) != len(rows[0]):
                raise LdxError(f"{path}: line {no + 1}: {len(vals)} weights beside {len(rows[0])}")
            ids.append(parts[0])
            alleles.append(parts[1])
            rows.append(vals)
    if not rows:
        raise LdxError(f"{path}: no weight line")
    return ids, alleles, np.asarray(rows, dtype=np.float64)


def bfile_score(src, weights, out: Optional[str] = None, impute: str = "mean", keep=None, extract=None, **load):
    """drivers/pca.py's ``score_table`` from a fileset (PLINK's --score sums): ``weights`` is the path of a score file
    (read_score_file) or its (ids, alleles, weights) triple.  A line counts when its ID is a variant of the fileset (the first of a
    repeated ID) and its allele one of the variant's two; a later line of the same variant replaces an earlier one.  A weight w
    for the allele that is code 1 is beta = w; for the other allele beta = -w with the constant 2 w per counted genotype
    (its dosage is 2 - g).  Only matched variants are scored (ALLELE_CT counts them).  ``out``: a prefix to write ``.sscore``
    under.  Returns the ScoreTable, ``n_matched`` / ``n_lines`` set."""
    from .pca import score_table, write_sscore

    bf, _ = _bfile_and_mask("bfile_score", src, keep, extract, None, 0, None, load)
    ids, alleles, w = read_score_file(weights) if isinstance(weights, str) else weights
    w = np.asarray(w, dtype=np.float64)
    w = w[:, None] if w.ndim == 1 else w
    if not (len(ids) == len(alleles) == w.shape[0]):
        raise LdxError("bfile_score: ids, alleles and weights differ in length")
    where = {}
    for k, name in enumerate(bf.ids):
        where.setdefault(name, k)
    beta, offset = np.zeros((bf.n, w.shape[1])), np.zeros((bf.n, w.shape[1]))
    matched, n_matched = np.zeros(bf.n, dtype=bool), 0
    alts, refs = bf.alts, bf.refs
    for name, allele, row in zip(ids, alleles, w):
        k = where.get(name)
        if k is None or allele not in (alts[k], refs[k]):
            continue
        n_matched += 1
        matched[k] = True
        beta[k], offset[k] = (row, 0.0) if allele == alts[k] else (-row, 2.0 * row)
    if not n_matched:
        raise LdxError("bfile_score: no weight line names a variant of the fileset and one of its alleles")
    table = score_table(bf.panel, list(zip(bf.fid, bf.iid)), beta, keep=matched, impute=impute,
                        offset=offset if offset.any() else None)
    table.n_matched, table.n_lines = n_matched, len(ids)
    if out is not None:
        write_sscore(out + ".sscore", table)
    return table


def _sample_rows(what: str, table, bf: Bfile, names) -> tuple:
    """(names, values float64 [individuals of ``bf``, names], NaN where the table has no line for an individual) of a phenotype or
    covariate table -- a path or plink.read_pheno's (fid, iid, names, values) -- restricted to ``names`` when given.  A line is
    matched by (FID, IID); a table without a FID column (``fid`` None) by IID alone, which must then name one individual of the
    fileset only.  An individual on two lines is refused."""
    if isinstance(table, str):
        table = plink.read_covar(table) if what == "covariate" else plink.read_pheno(table)
    fid, iid, have, values = table
    values = np.asarray(values, dtype=np.float64).reshape(len(iid), len(have))
    if names is not None:
        unknown = [n for n in names if n not in have]
        if unknown:
            raise LdxError(f"bfile_glm: no {what} named {unknown[0]!r} (the table has {', '.join(have[:8])} ...)")
        values, have = values[:, [list(have).index(n) for n in names]], list(names)
    where: dict = {}
    for k, key in enumerate(zip(bf.fid, bf.iid) if fid is not None else bf.iid):
        if key in where:
            raise LdxError(f"bfile_glm: the fileset holds {key!r} twice: the {what} table cannot tell its individuals apart"
                           + ("" if fid is not None else " by IID alone; give it a FID column"))
        where[key] = k
    out = np.full((len(bf.iid), len(have)), np.nan)
    filled = np.zeros(len(bf.iid), dtype=bool)
    for key, row in zip(zip(fid, iid) if fid is not None else iid, values):
        k = where.get(key)
        if k is not None:
            if filled[k]:
                raise LdxError(f"bfile_glm: the {what} table names {key!r} on two lines")
            out[k], filled[k] = row, True
    return list(have), out


def bfile_glm(src, pheno, covar=None, out: Optional[str] = None, pheno_names: Optional[Sequence[str]] = None,
              covar_names: Optional[Sequence[str]] = None, max_vif: float = 50.0, allow_binary: bool = False, **load) -> list:
    """drivers/glm.py's ``glm_table`` from a fileset (PLINK 2's --glm for quantitative traits; ops.ld_glm's definition: a missing
    genotype counts as the variant's mean).  ``pheno`` / ``covar``: the path of a phenotype / covariate table (plink.read_pheno,
    plink.read_covar; an ``.eigenvec`` is a covariate table) or its (fid, iid, names, values); ``pheno_names`` / ``covar_names``
    choose columns.  A row is complete for a phenotype when the phenotype and every covariate are finite and the individual is
    in the fileset; the phenotypes are grouped by their set of complete rows, and each group is scanned over its own individuals
    (ld_glm's ``individuals``), at most 64 columns a sweep.  A phenotype whose values all lie in {1, 2} or {0, 1} is a
    case/control trait, which belongs to a logistic model: refused unless ``allow_binary``.  ``out``: a prefix to write one
    ``<out>.<phenotype>.glm.linear`` per phenotype under.  Returns the GlmTables, one per sweep."""
    from .glm import GlmTable, write_glm_linear
    from .._lib import GENO_MAX_COLS
    from ..ops import ld_glm

    bf = _loaded(src, **load)
    names, Y = _sample_rows("phenotype", pheno, bf, pheno_names)
    C = np.empty((len(bf.iid), 0)) if covar is None else _sample_rows("covariate", covar, bf, covar_names)[1]
    for j, name in enumerate(names):
        seen = set(np.unique(Y[np.isfinite(Y[:, j]), j]).tolist())
        if not seen:
            raise LdxError(f"bfile_glm: phenotype {name} has no value for an individual of the fileset")
        if (seen <= {1.0, 2.0} or seen <= {0.0, 1.0}) and not allow_binary:
            raise LdxError(f"bfile_glm: phenotype {name} takes the values {sorted(seen)} only: a case/control trait belongs to a "
                           "logistic model: bfile_logistic (allow_binary=True fits the line anyway)")
    complete = np.isfinite(Y) & np.isfinite(C).all(axis=1)[:, None]
    groups: dict = {}
    for j in range(len(names)):
        groups.setdefault(complete[:, j].tobytes(), []).append(j)
    width = GENO_MAX_COLS - (C.shape[1] + 1)
    if width < 1:
        raise LdxError(f"bfile_glm: {C.shape[1]} covariates leave no column for a phenotype ({GENO_MAX_COLS} a sweep)")
    tables = []
    for cols in groups.values():
        rows = np.flatnonzero(complete[:, cols[0]])
        for at in range(0, len(cols), width):
            batch = cols[at:at + width]
            res = ld_glm(bf.panel, Y[np.ix_(rows, batch)], C[rows] if C.shape[1] else None,
                         individuals=None if rows.size == len(bf.iid) else rows, max_vif=max_vif)   # everybody: no copy of the panel
            tables.append(GlmTable(list(bf.chrom), _poss(bf), list(bf.ids), list(bf.refs), list(bf.alts),
                                   [names[j] for j in batch], res))
    if out is not None:
        for table in tables:
            for name in table.names:
                write_glm_linear(f"{out}.{name}.glm.linear", table, name)
    return tables


def case_control(name: str, values) -> np.ndarray:
    """A case/control phenotype column as 0 (control) / 1 (case), NaN kept: its finite values must all lie in {1, 2} (PLINK's
    control / case; a column of 1s alone is all controls) or in {0, 1}.  Anything else is refused."""
    v = np.asarray(values, dtype=np.float64)
    seen = set(np.unique(v[np.isfinite(v)]).tolist())
    if not seen:
        raise LdxError(f"bfile_logistic: phenotype {name} has no value for an individual of the fileset")
    if seen <= {1.0, 2.0}:
        return v - 1.0
    if seen <= {0.0, 1.0}:
        return v.copy()
    raise LdxError(f"bfile_logistic: phenotype {name} takes the values {sorted(seen)[:6]}: a case/control trait is coded 1 / 2 "
                   "(control / case) or 0 / 1; a quantitative trait belongs to bfile_glm")


def bfile_logistic(src, pheno, covar=None, out: Optional[str] = None, pheno_names: Optional[Sequence[str]] = None,
                   covar_names: Optional[Sequence[str]] = None, max_vif: float = 50.0, firth: Optional[str] = None,
                   **load) -> list:
    """drivers/glm.py's ``logistic_table`` from a fileset (PLINK 2's --glm for case/control traits without its Firth fallback;
    ops.ld_glm_logistic's definition: a missing genotype counts as the variant's mean).  ``pheno`` / ``covar``, their names and
    the grouping of the phenotypes by their complete rows are bfile_glm's; a phenotype's finite values must lie in {1, 2}
    (control / case) or {0, 1} (case_control); at most 13 covariates.  ``out``: a prefix to write one
    ``<out>.<phenotype>.glm.logistic`` per phenotype under.  ``firth`` (ops.ld_glm_logistic's): "fallback" refits the variants
    without a finite maximiser by Firth's penalised likelihood and writes ``<out>.<phenotype>.glm.logistic.hybrid`` (PLINK 2's
    firth-fallback, its default), "always" fits every variant that way and writes ``<out>.<phenotype>.glm.firth``.  Returns the
    LogisticTables, one per group."""
    from .glm import LogisticTable, write_glm_firth, write_glm_hybrid, write_glm_logistic
    from .._lib import LOGIT_MAX_COV
    from ..ops import ld_glm_logistic

    bf = _loaded(src, **load)
    names, Y = _sample_rows("phenotype", pheno, bf, pheno_names)
    C = np.empty((len(bf.iid), 0)) if covar is None else _sample_rows("covariate", covar, bf, covar_names)[1]
    if C.shape[1] > LOGIT_MAX_COV:
        raise LdxError(f"bfile_logistic: {C.shape[1]} covariates are more than {LOGIT_MAX_COV}")
    Y = np.stack([case_control(name, Y[:, j]) for j, name in enumerate(names)], axis=1)
    complete = np.isfinite(Y) & np.isfinite(C).all(axis=1)[:, None]
    groups: dict = {}
    for j in range(len(names)):
        groups.setdefault(complete[:, j].tobytes(), []).append(j)
    tables = []
    for cols in groups.values():
        rows = np.flatnonzero(complete[:, cols[0]])
        res = ld_glm_logistic(bf.panel, Y[np.ix_(rows, cols)], C[rows] if C.shape[1] else None,
                              individuals=None if rows.size == len(bf.iid) else rows, max_vif=max_vif, firth=firth)
        tables.append(LogisticTable(list(bf.chrom), _poss(bf), list(bf.ids), list(bf.refs), list(bf.alts),
                                    [names[j] for j in cols], res))
    if out is not None:
        for table in tables:
            for name in table.names:
                if firth is None:
                    write_glm_logistic(f"{out}.{name}.glm.logistic", table, name)
                elif firth == "fallback":
                    write_glm_hybrid(f"{out}.{name}.glm.logistic.hybrid", table, name)
                else:
                    write_glm_firth(f"{out}.{name}.glm.firth", table, name)
    return tables


def _qc_variants(bf: Bfile):
    from .qc import QcVariants

    return QcVariants(list(bf.chrom), _poss(bf), list(bf.ids), list(bf.alts), list(bf.refs))


def _case_vector(what: str, bf: Bfile, pheno, pheno_name: Optional[str]) -> np.ndarray:
    """0 / 1 / NaN per individual of ``bf`` from a phenotype table (one column: ``pheno_name``, default the first) through
    case_control; None: the ``.fam``'s own phenotype column (1 / 2; 0, -9 and anything else = NaN).  A quantitative column is
    refused."""
    if pheno is None:
        v = np.full(len(bf.iid), np.nan)
        for k, x in enumerate(bf.pheno):
            if x in ("1", "2"):
                v[k] = float(x)
        name = "of the .fam"
    else:
        names, Y = _sample_rows("phenotype", pheno, bf, None if pheno_name is None else [pheno_name])
        v, name = Y[:, 0], names[0]
    try:
        return case_control(name, v)
    except LdxError as exc:
        raise LdxError(f"{what}: {str(exc).replace('bfile_logistic: ', '')}") from None


def bfile_hardy(src, out: Optional[str] = None, groups=None, midp: bool = False, **load):
    """ops.ld_hardy from a fileset (PLINK --hardy): genotype counts and the exact HWE test of every variant, within each group
    of ``groups`` (ops.geno_group_counts'; None: everybody).  ``out``: a prefix to write ``.hardy`` under (one group), or
    ``.<label>.hardy`` per group.  Returns (QcVariants, HardyResult)."""
    from ..ops import ld_hardy
    from .qc import write_hardy

    bf = _loaded(src, **load)
    res, variants = ld_hardy(bf.panel, groups, midp=midp), _qc_variants(bf)
    if out is not None:
        for g, label in enumerate(res.labels):
            write_hardy(f"{out}.hardy" if len(res.labels) == 1 else f"{out}.{label}.hardy", variants, res, g)
    return variants, res


def bfile_missing(src, out: Optional[str] = None, pheno=None, pheno_name: Optional[str] = None, midp: bool = False, **load):
    """Missing-call reports of a fileset (PLINK 2 --missing): ``.vmiss`` per variant and ``.smiss`` per individual; with a
    case/control phenotype (``pheno``: a table or its (fid, iid, names, values), ``pheno_name`` its column) also PLINK's
    --test-missing as ``.missing``.  Returns (QcVariants, called per variant, SampleQC, MissingResult or None)."""
    from ..ops import geno_snp_counts, ld_test_missing, sample_qc
    from .qc import write_smiss, write_test_missing, write_vmiss

    bf = _loaded(src, **load)
    variants = _qc_variants(bf)
    called, qc = geno_snp_counts(bf.panel)[:, 0], sample_qc(bf.panel)
    tm = None if pheno is None else ld_test_missing(bf.panel, _case_vector("bfile_missing", bf, pheno, pheno_name), midp=midp)
    if out is not None:
        write_vmiss(out + ".vmiss", variants, called, bf.panel.n_ind)
        write_smiss(out + ".smiss", bf.fid, bf.iid, qc)
        if tm is not None:
            write_test_missing(out + ".missing", variants, tm)
    return variants, called, qc, tm


def bfile_het(src, out: Optional[str] = None, **load):
    """ops.sample_qc from a fileset (PLINK --het): per individual the observed and expected homozygous calls and the inbreeding
    coefficient F.  ``out``: a prefix to write ``.het`` under.  Returns the SampleQC."""
    from ..ops import sample_qc
    from .qc import write_het

    bf = _loaded(src, **load)
    qc = sample_qc(bf.panel)
    if out is not None:
        write_het(out + ".het", bf.fid, bf.iid, qc)
    return qc


def bfile_model(src, pheno=None, out: Optional[str] = None, pheno_name: Optional[str] = None, midp: bool = False,
                min_cell: int = 5, **load):
    """ops.ld_model from a fileset (PLINK --model and --assoc fisher): the five chi-square table tests and Fisher's exact test on
    the allele counts.  ``pheno``: a case/control phenotype table (case_control: 1 / 2 or 0 / 1; None: the ``.fam``'s column);
    a quantitative trait is refused -- it belongs to bfile_glm.  ``out``: a prefix to write ``.model`` and ``.assoc.fisher``
    under.  Returns (QcVariants, ModelResult)."""
    from ..ops import ld_model
    from .qc import write_assoc_fisher, write_model

    bf = _loaded(src, **load)
    res = ld_model(bf.panel, _case_vector("bfile_model", bf, pheno, pheno_name), midp=midp, min_cell=min_cell)
    variants = _qc_variants(bf)
    if out is not None:
        write_model(out + ".model", variants, res)
        write_assoc_fisher(out + ".assoc.fisher", variants, res)
    return variants, res


def bfile_epistasis(src, pheno=None, out: Optional[str] = None, test: str = "boost", p: float = 1e-4, p_sig: float = 1e-2,
                    set_i: Optional[Sequence[str]] = None, set_j: Optional[Sequence[str]] = None,
                    pheno_name: Optional[str] = None, hit_capacity: Optional[int] = None, **load):
    """drivers/epistasis.py's ``epistasis_table`` from a fileset (PLINK --fast-epistasis, ``test`` "allelic", and
    --fast-epistasis boost, "boost"): the SNP x SNP interaction test of every pair of variants once, or, with the variant ID
    lists ``set_i`` and ``set_j`` (one alone is tested against all variants), of every variant of the first set against every
    variant of the second.  ``pheno``: a case/control phenotype table (case_control: 1 / 2 or 0 / 1; None: the ``.fam``'s
    column); a quantitative trait is refused -- it belongs to bfile_glm.  ``p``: the pairs written; ``p_sig``: the summary's
    threshold.  ``out``: a prefix to write ``.epi.cc`` and ``.epi.cc.summary`` under.  Returns the EpiTable."""
    from .epistasis import epistasis_table, write_epi_cc, write_epi_summary

    bf = _loaded(src, **load)
    case = _case_vector("bfile_epistasis", bf, pheno, pheno_name)
    if set_i is None and set_j is None:
        table = epistasis_table(bf.panel, case, bf.chrom, bf.ids, test=test, p=p, p_sig=p_sig, hit_capacity=hit_capacity)
    else:
        sides = []
        for names in (set_i, set_j):
            if names is None:
                sides.append((bf.panel, list(bf.chrom), list(bf.ids)))
                continue
            if not _is_names(names, False):
                raise LdxError("bfile_epistasis: set_i and set_j are non-empty lists of variant IDs")
            k = _by_name(list(names), bf.ids, "variant")
            sides.append((bf.panel.select(snps=k), [bf.chrom[x] for x in k], [bf.ids[x] for x in k]))
        (pi, ci, ii), (pj, cj, ij) = sides
        table = epistasis_table(pi, case, ci, ii, pj, cj, ij, test=test, p=p, p_sig=p_sig, hit_capacity=hit_capacity)
    if out is not None:
        write_epi_cc(out + ".epi.cc", table)
        write_epi_summary(out + ".epi.cc.summary", table)
    return table


def bfile_mperm(src, pheno=None, out: Optional[str] = None, test: str = "allelic", n_perm: int = 10000, seed: int = 0,
                pheno_name: Optional[str] = None, **load):
    """drivers/mperm.py's ``mperm_table`` from a fileset (PLINK --assoc mperm=N, ``test`` "allelic", and --model trend mperm=N,
    "trend"): the max(T) permutation test of every variant, EMP1 and EMP2.  ``pheno``: a case/control phenotype table
    (case_control: 1 / 2 or 0 / 1; None: the ``.fam``'s column); a quantitative trait is refused.  ``out``: a prefix to write
    ``.assoc.mperm`` (allelic) or ``.model.trend.mperm`` under.  Returns the MpermTable."""
    from .mperm import MPERM_SUFFIX, mperm_table, write_assoc_mperm

    bf = _loaded(src, **load)
    case = _case_vector("bfile_mperm", bf, pheno, pheno_name)
    table = mperm_table(bf.panel, case, bf.chrom, bf.ids, test=test, n_perm=n_perm, seed=seed)
    if out is not None:
        write_assoc_mperm(out + MPERM_SUFFIX[test], table)
    return table


@dataclass
class QcMasks:
    """bfile_qc's result: ``snps`` uint8 device tensor [variants] (an operator's ``keep=``), ``individuals`` bool [individuals]."""

    snps: object
    individuals: np.ndarray

    @property
    def extract(self) -> np.ndarray:
        """The variant mask as bool [variants] on the host: load_bfile's ``extract`` (``individuals`` is its ``keep``)."""
        return self.snps.cpu().numpy().astype(bool)


def bfile_qc(src, out: Optional[str] = None, geno: Optional[float] = None, maf: Optional[float] = None,
             hwe: Optional[float] = None, mind: Optional[float] = None, pheno=None, pheno_name: Optional[str] = None,
             midp: bool = False, **load) -> QcMasks:
    """PLINK's --mind, then --geno --maf --hwe, on a fileset: individuals with a missing-call rate above ``mind`` go first, and
    the variant filters (ops.snp_qc_mask) see the remaining individuals; HWE is tested on the controls when a phenotype is given
    (``pheno`` / ``pheno_name`` as bfile_model; the ``.fam``'s own column is not used), on everybody otherwise.  ``out``: a prefix
    to write the variant lists ``.qc.in`` / ``.qc.out`` and the individual list ``.qc.keep`` (FID IID) under.  The masks go to
    bfile_prune / bfile_king and to every operator's ``keep=`` as they stand."""
    from ..ops import sample_qc_mask, snp_qc_mask

    bf = _loaded(src, **load)
    panel = bf.panel
    ind = sample_qc_mask(panel, mind_max=mind) if mind is not None else np.ones(panel.n_ind, dtype=bool)
    if not ind.any():
        raise LdxError("bfile_qc: no individual passes mind")
    if not ind.all():
        rows = np.flatnonzero(ind)
        panel = panel.select(haplotypes=np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1))
    hwe_group = None
    if pheno is not None and hwe is not None:
        hwe_group = _case_vector("bfile_qc", bf, pheno, pheno_name)[ind] == 0.0
        if not hwe_group.any():
            raise LdxError("bfile_qc: the phenotype leaves no control to test HWE on")
    snps = snp_qc_mask(panel, maf_min=maf, geno_max=geno, hwe_min=hwe, hwe_group=hwe_group, midp=midp)
    if out is not None:
        ok = snps.cpu().numpy().astype(bool)
        for ext, want in ((".qc.in", True), (".qc.out", False)):
            with open(out + ext, "w") as f:
                f.writelines(f"{name}\n" for name, o in zip(bf.ids, ok) if o == want)
        with open(out + ".qc.keep", "w") as f:
            f.writelines(f"{a}\t{b}\n" for a, b, o in zip(bf.fid, bf.iid, ind) if o)
    return QcMasks(snps, ind)


def make_bed(prefix_out, src, snps=None, individuals=None, bim: Optional[dict] = None, fam: Optional[dict] = None,
             alt: Optional[str] = None) -> List[str]:
    """Write a fileset.  ``src``: a ``Bfile`` -- ``snps`` / ``individuals`` (index arrays or masks over ITS variants and
    individuals, e.g. a PruneTable's ``pruned.keep``) choose a subset, taken on the device (PackedPanel.select), and the
    ``.bim`` / ``.fam`` columns follow -- or a bare ``PackedPanel`` with its ``bim`` / ``fam`` columns (plink.write_bfile's).
    ``alt``: which allele code 1 is written as (default: the Bfile's own, "a1" for a panel).  Returns the three paths."""
    if isinstance(src, Bfile):
        panel, alt = src.panel, alt or src.alt
        si = None if snps is None else select_index(snps, src.n, "SNP")
        ii = None if individuals is None else select_index(individuals, panel.n_ind, "individual")
        if si is not None or ii is not None:
            cols = None if ii is None else np.stack([2 * ii, 2 * ii + 1], axis=1).reshape(-1)
            panel = panel.select(snps=si, haplotypes=cols)
        bim, fam = src.bim(si), src.fam(ii)
    elif isinstance(src, PackedPanel):
        if bim is None or fam is None or snps is not None or individuals is not None:
            raise LdxError("make_bed: a bare panel needs its bim and fam columns (and takes no subset)")
        panel, alt = src, alt or "a1"
    else:
        raise LdxError("make_bed: src must be a Bfile or a PackedPanel")
    return plink.write_bfile(prefix_out, panel.to_bed(alt=alt), bim, fam)


# ---------------------------------------------------------------------------------------------- command line
def _read_names(path: str, n_cols: int) -> list:
    out = []
    with open(path) as f:
        for line in f:
            parts = line.split()
            if not parts:
                continue
            if len(parts) < n_cols:
                raise LdxError(f"{path}: a line with fewer than {n_cols} field(s)")
            out.append(parts[0] if n_cols == 1 else (parts[0], parts[1]))
    return out


def _read_pvalues(path: str, ids: Sequence[str], snp_col: str, p_col: str) -> np.ndarray:
    """One p per variant of ``ids`` from a whitespace table with a header (PLINK's --clump file); absent variants get NaN."""
    with open(path) as f:
        head = f.readline().split()
        if snp_col not in head or p_col not in head:
            raise LdxError(f"{path}: no {snp_col} / {p_col} column")
        a, b = head.index(snp_col), head.index(p_col)
        got = {}
        for line in f:
            parts = line.split()
            if len(parts) > max(a, b):
                try:
                    got[parts[a]] = float(parts[b])
                except ValueError:
                    got[parts[a]] = float("nan")
    return np.asarray([got.get(i, float("nan")) for i in ids], dtype=np.float64)


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m ld_tools_amd.drivers.plink",
                                 description="LD tables, clumps, pruned sets and LD scores from a PLINK binary fileset.")
    sub = ap.add_subparsers(dest="command", required=True)

    def common(name, text):
        p = sub.add_parser(name, help=text, description=text)
        p.add_argument("--bfile", required=True, help="prefix of the .bed/.bim/.fam fileset")
        p.add_argument("--out", required=True, help="prefix of the files written")
        p.add_argument("--chr", default=None, help="keep this chromosome (needed when the fileset holds several)")
        p.add_argument("--keep", default=None, help="file of FID IID lines: the individuals to keep")
        p.add_argument("--extract", default=None, help="file of variant IDs: the variants to keep")
        p.add_argument("--maf", type=float, default=None, help="minor allele frequency bound")
        p.add_argument("--geno", type=float, default=None, help="largest missing-call rate of a variant")
        p.add_argument("--alt", choices=plink.ALTS, default="a1", help="the allele counted as ALT (code 1)")
        return p

    p = common("ld", "pairs within a window with EM r^2 above a bound (.ld: SNP_A SNP_B R2 DP)")
    p.add_argument("--ld-window-kb", type=float, default=1000.0)
    p.add_argument("--ld-window-r2", type=float, default=0.2)
    p.add_argument("--missing", choices=("pairwise",), default=None)
    p = common("clump", "PLINK --clump (.clumped)")
    p.add_argument("--clump", required=True, help="association results with a header")
    p.add_argument("--clump-snp-field", default="SNP")
    p.add_argument("--clump-field", default="P")
    p.add_argument("--clump-p1", type=float, default=1e-4)
    p.add_argument("--clump-p2", type=float, default=1e-2)
    p.add_argument("--clump-r2", type=float, default=0.5)
    p.add_argument("--clump-kb", type=float, default=250.0)
    p.add_argument("--dosage", action="store_true", help="the genotype-dosage r instead of the EM r")
    p.add_argument("--missing", choices=("pairwise",), default=None)
    p = common("prune", "priority pruning (.prune.in / .prune.out)")
    p.add_argument("--r2", type=float, default=0.2)
    p.add_argument("--window-kb", type=float, default=250.0)
    p.add_argument("--em", action="store_true", help="the EM r instead of the genotype-dosage r")
    p.add_argument("--missing", choices=("pairwise",), default=None)
    p = common("l2", "LD scores in LDSC's layout (.l2.ldscore.gz, .l2.M, .l2.M_5_50)")
    p.add_argument("--ld-wind-kb", type=float, default=1000.0)
    p.add_argument("--missing", choices=("ref", "pairwise"), default=None)
    p.add_argument("--no-adjust", action="store_true", help="write r^2 sums, not LDSC's unbiased estimate")
    p = common("blocks", "haplotype blocks by Gabriel et al.'s D' confidence-interval rule (.blocks, .blocks.det)")
    p.add_argument("--blocks-max-kb", type=float, default=500.0, help="the window: the largest distance of a block's ends")
    p.add_argument("--blocks-min-maf", type=float, default=0.05)
    p.add_argument("--missing", choices=("pairwise", "ref"), default="pairwise")
    p = common("king", "KING-robust kinship between the individuals (.kin0; --king-cutoff: .king.cutoff.in.id / .out.id)")
    p.add_argument("--king-table-filter", type=float, default=None, help="write only the pairs with kinship >= this")
    p.add_argument("--king-cutoff", type=float, default=None, help="keep a maximal set with no pair above this kinship")
    p.add_argument("--make-king", action="store_true", help="also write the lower triangle (.king, .king.id)")
    p.add_argument("--prune-r2", type=float, default=None, help="count over the variants LD pruning keeps at this r^2")
    p.add_argument("--prune-window-kb", type=float, default=250.0)
    p.add_argument("--missing", choices=("pairwise",), default=None, help="how the pruning treats missing calls")
    p = common("grm", "genetic relationship matrix, streamed (.grm.bin / .grm.N.bin / .grm.id, or .rel / .rel.id; "
                      "--maf: the MAF bound among the called)")
    p.add_argument("--grm-cutoff", type=float, default=None, help="keep a maximal set with no pair above this relationship")
    p.add_argument("--format", choices=("gcta", "rel"), default="gcta", help="GCTA's binary triangle or PLINK's text triangle")
    p.add_argument("--chunk-snps", type=int, default=GRM_CHUNK_SNPS, help="variants held on the device at a time")
    p = common("pca", "principal components of the individuals (.eigenvec, .eigenval)")
    p.add_argument("--pca", type=int, default=10, dest="n_pcs", help="the number of components")
    p.add_argument("--king-cutoff", type=float, default=None, help="decompose a maximal unrelated set, project the others")
    p.add_argument("--prune-r2", type=float, default=None, help="use the variants LD pruning keeps at this r^2")
    p.add_argument("--prune-window-kb", type=float, default=250.0)
    p.add_argument("--missing", choices=("pairwise",), default=None, help="how the pruning treats missing calls")
    p.add_argument("--seed", type=int, default=0)
    p = common("score", "polygenic score sums of the individuals (.sscore)")
    p.add_argument("--score", required=True, help="weights: variant ID, allele, weight per line")
    p.add_argument("--no-mean-imputation", action="store_true", help="a missing genotype adds nothing (default: 2 x frequency)")
    p = common("glm", "linear association scan of quantitative phenotypes (.<phenotype>.glm.linear)")
    p.add_argument("--pheno", required=True, help="phenotype table: '#FID IID', 'FID IID' or '#IID', then one column per phenotype")
    p.add_argument("--pheno-name", nargs="+", default=None, help="the phenotypes to scan (default: every column)")
    p.add_argument("--covar", default=None, help="covariate table in the same layout (an .eigenvec is one)")
    p.add_argument("--covar-name", nargs="+", default=None, help="the covariates to use (default: every column)")
    p.add_argument("--vif", type=float, default=50.0, help="largest variance inflation factor of a variant")
    p = common("logistic", "logistic association scan of case/control phenotypes (.<phenotype>.glm.logistic)")
    p.add_argument("--pheno", required=True, help="phenotype table as for glm; values 1 / 2 (control / case) or 0 / 1")
    p.add_argument("--pheno-name", nargs="+", default=None, help="the phenotypes to scan (default: every column)")
    p.add_argument("--covar", default=None, help="covariate table in the same layout (an .eigenvec is one); at most 13 columns")
    p.add_argument("--covar-name", nargs="+", default=None, help="the covariates to use (default: every column)")
    p.add_argument("--vif", type=float, default=50.0, help="largest variance inflation factor of a variant")
    p.add_argument("--firth", choices=("fallback", "always"), default=None,
                   help="Firth's penalised fit where the likelihood has no finite maximiser (.glm.logistic.hybrid) or for every "
                        "variant (.glm.firth); default: off")
    p = common("hardy", "genotype counts and the exact Hardy-Weinberg test per variant (.hardy)")
    p.add_argument("--midp", action="store_true", help="the mid-p: half of the observed term is taken off")
    p = common("missing", "missing-call rates per variant and individual (.vmiss, .smiss; with --pheno: .missing)")
    p.add_argument("--pheno", default=None, help="case/control phenotype table: adds the test of missingness by status")
    p.add_argument("--pheno-name", default=None, help="its column (default: the first)")
    p.add_argument("--midp", action="store_true")
    common("het", "observed and expected homozygous calls and the inbreeding coefficient per individual (.het)")
    p = common("model", "case/control table tests per variant (.model, .assoc.fisher)")
    p.add_argument("--pheno", default=None, help="case/control phenotype table, 1 / 2 or 0 / 1 (default: the .fam's column)")
    p.add_argument("--pheno-name", default=None, help="its column (default: the first)")
    p.add_argument("--cell", type=int, default=5, help="smallest cell of the genotypic test")
    p.add_argument("--midp", action="store_true", help="the mid-p of Fisher's exact test")
    p = common("qc", "variant and individual filters (.qc.in, .qc.out, .qc.keep); --maf and --geno are applied here, after --mind")
    p.add_argument("--hwe", type=float, default=None, help="smallest exact HWE p of a variant (on the controls with --pheno)")
    p.add_argument("--mind", type=float, default=None, help="largest missing-call rate of an individual")
    p.add_argument("--pheno", default=None, help="case/control phenotype table: HWE is tested on its controls")
    p.add_argument("--pheno-name", default=None, help="its column (default: the first)")
    p.add_argument("--midp", action="store_true")
    p = common("epistasis", "SNP x SNP interaction scan of a case/control trait (.epi.cc, .epi.cc.summary)")
    p.add_argument("--pheno", default=None, help="case/control phenotype table, 1 / 2 or 0 / 1 (default: the .fam's column)")
    p.add_argument("--pheno-name", default=None, help="its column (default: the first)")
    p.add_argument("--test", choices=("boost", "allelic"), default="boost",
                   help="boost: the 4-df likelihood-ratio test (--fast-epistasis boost); allelic: the 1-df test of --fast-epistasis")
    p.add_argument("--epi1", type=float, default=1e-4, help="write the pairs with p at or below this")
    p.add_argument("--epi2", type=float, default=1e-2, help="the summary's threshold")
    p.add_argument("--set-i", default=None, help="file of variant IDs: the first set of a set-by-set scan")
    p.add_argument("--set-j", default=None, help="file of variant IDs: the second set")
    p = common("mperm", "max(T) permutation test of a case/control trait: EMP1 and EMP2 (.assoc.mperm, .model.trend.mperm)")
    p.add_argument("--pheno", default=None, help="case/control phenotype table, 1 / 2 or 0 / 1 (default: the .fam's column)")
    p.add_argument("--pheno-name", default=None, help="its column (default: the first)")
    p.add_argument("--test", choices=("allelic", "trend"), default="allelic",
                   help="allelic: the 1-df allele test of --assoc; trend: the Cochran-Armitage test of --model")
    p.add_argument("--mperm", type=int, default=10000, help="the number of label permutations")
    p.add_argument("--seed", type=int, default=0, help="the permutations' seed")
    common("make-bed", "write the selected variants and individuals as a new fileset")
    return ap


def main(argv=None) -> int:
    from .blocks import write_gabriel_blocks
    from .clump import write_clumped
    from .em import write_ld_table
    from .ldscore import write_ldscore
    from .prune import write_prune

    a = parser().parse_args(argv)
    keep = None if a.keep is None else _read_names(a.keep, 2)
    extract = None if a.extract is None else _read_names(a.extract, 1)
    if a.command == "grm":               # streamed from the file: nothing is loaded in one piece; --maf is the GRM's own bound
        if a.geno is not None:
            raise LdxError("grm: --geno is not supported (a missing call drops out of its pairs)")
        table = bfile_grm(a.bfile, out=a.out, keep=keep, extract=extract, chrom=a.chr, maf_min=a.maf, cutoff=a.grm_cutoff,
                          fmt=a.format, chunk_snps=a.chunk_snps, alt=a.alt)
        print(table.result.n_ind, "individuals,", table.result.n_live, "live variants ->",
              a.out + (".grm.bin" if a.format == "gcta" else ".rel"))
        return 0
    own_filters = a.command == "qc"      # qc applies --maf / --geno itself, after --mind
    bf = load_bfile(a.bfile, chrom=a.chr, keep=keep, extract=extract, maf_min=None if own_filters else a.maf,
                    geno_max=None if own_filters else a.geno, alt=a.alt)
    if a.command == "hardy":
        variants, _ = bfile_hardy(bf, out=a.out, midp=a.midp)
        print(len(variants), "variants ->", a.out + ".hardy")
    elif a.command == "missing":
        variants, _, qc, tm = bfile_missing(bf, out=a.out, pheno=a.pheno, pheno_name=a.pheno_name, midp=a.midp)
        print(len(variants), "variants,", qc.called.size, "individuals ->", a.out + ".vmiss", a.out + ".smiss",
              *([] if tm is None else [a.out + ".missing"]))
    elif a.command == "het":
        print(bfile_het(bf, out=a.out).called.size, "individuals ->", a.out + ".het")
    elif a.command == "model":
        variants, _ = bfile_model(bf, a.pheno, out=a.out, pheno_name=a.pheno_name, midp=a.midp, min_cell=a.cell)
        print(len(variants), "variants ->", a.out + ".model", a.out + ".assoc.fisher")
    elif a.command == "epistasis":
        table = bfile_epistasis(bf, a.pheno, out=a.out, test=a.test, p=a.epi1, p_sig=a.epi2, pheno_name=a.pheno_name,
                                set_i=None if a.set_i is None else _read_names(a.set_i, 1),
                                set_j=None if a.set_j is None else _read_names(a.set_j, 1))
        print(len(table.result), "pairs ->", a.out + ".epi.cc", a.out + ".epi.cc.summary")
    elif a.command == "mperm":
        from .mperm import MPERM_SUFFIX

        table = bfile_mperm(bf, a.pheno, out=a.out, test=a.test, n_perm=a.mperm, seed=a.seed, pheno_name=a.pheno_name)
        print(len(table.ids), "variants,", table.result.n_perm, "permutations ->", a.out + MPERM_SUFFIX[a.test])
    elif a.command == "qc":
        masks = bfile_qc(bf, out=a.out, geno=a.geno, maf=a.maf, hwe=a.hwe, mind=a.mind, pheno=a.pheno, pheno_name=a.pheno_name,
                         midp=a.midp)
        print(int(masks.extract.sum()), "of", bf.n, "variants,", int(masks.individuals.sum()), "of", len(bf.iid),
              "individuals ->", a.out + ".qc.in", a.out + ".qc.out", a.out + ".qc.keep")
    elif a.command == "ld":
        side, hits = bfile_ld_table(bf, r2=a.ld_window_r2, window_bp=int(a.ld_window_kb * 1000), missing=a.missing)
        print(write_ld_table(a.out + ".ld", side, side, hits), "pairs ->", a.out + ".ld")
    elif a.command == "clump":
        p = _read_pvalues(a.clump, bf.ids, a.clump_snp_field, a.clump_field)
        table = bfile_clump(bf, p, p1=a.clump_p1, p2=a.clump_p2, r2=a.clump_r2, window_bp=int(a.clump_kb * 1000),
                            dosage=a.dosage or None, missing=a.missing)
        print(write_clumped(a.out + ".clumped", table))
    elif a.command == "prune":
        table = bfile_prune(bf, r2=a.r2, window_bp=int(a.window_kb * 1000), em=a.em or None, missing=a.missing)
        print(*write_prune(a.out, table))
    elif a.command == "l2":
        table = bfile_ld_scores(bf, window_bp=int(a.ld_wind_kb * 1000), adjust=not a.no_adjust, missing=a.missing)
        print(*write_ldscore(a.out, table))
    elif a.command == "blocks":
        table = bfile_blocks(bf, window_bp=int(a.blocks_max_kb * 1000), missing=None if a.missing == "ref" else a.missing,
                             maf_min=a.blocks_min_maf)
        print(table.result.n_blocks, "blocks ->", *write_gabriel_blocks(a.out, table.result, table.rs_ids, table.chrom))
    elif a.command == "king":
        table = bfile_king(bf, out=a.out, prune_r2=a.prune_r2, prune_window_bp=int(a.prune_window_kb * 1000),
                           prune_missing=a.missing, kin_min=a.king_table_filter, cutoff=a.king_cutoff, matrix=a.make_king)
        print(table.counts.n_ind, "individuals,", table.counts.n_snps, "variants ->", a.out + ".kin0")
    elif a.command == "pca":
        table = bfile_pca(bf, out=a.out, n_pcs=a.n_pcs, prune_r2=a.prune_r2, prune_window_bp=int(a.prune_window_kb * 1000),
                          prune_missing=a.missing, king_cutoff=a.king_cutoff, seed=a.seed)
        print(int(table.in_pca.sum()), "of", len(table.iid), "individuals decomposed,", table.pca.n_used, "variants ->",
              a.out + ".eigenvec", a.out + ".eigenval")
    elif a.command == "glm":
        split = lambda v: None if v is None else [n for part in v for n in part.split(",") if n]  # noqa: E731
        tables = bfile_glm(bf, a.pheno, covar=a.covar, out=a.out, pheno_names=split(a.pheno_name), covar_names=split(a.covar_name),
                           max_vif=a.vif)
        print(*(f"{a.out}.{name}.glm.linear" for t in tables for name in t.names))
    elif a.command == "logistic":
        split = lambda v: None if v is None else [n for part in v for n in part.split(",") if n]  # noqa: E731
        tables = bfile_logistic(bf, a.pheno, covar=a.covar, out=a.out, pheno_names=split(a.pheno_name),
                                covar_names=split(a.covar_name), max_vif=a.vif, firth=a.firth)
        ext = {None: "glm.logistic", "fallback": "glm.logistic.hybrid", "always": "glm.firth"}[a.firth]
        print(*(f"{a.out}.{name}.{ext}" for t in tables for name in t.names))
    elif a.command == "score":
        table = bfile_score(bf, a.score, out=a.out, impute="zero" if a.no_mean_imputation else "mean")
        print(table.n_matched, "of", table.n_lines, "weight lines matched ->", a.out + ".sscore")
    else:
        print(*make_bed(a.out, bf))
    return 0


if __name__ == "__main__":
    sys.exit(main())

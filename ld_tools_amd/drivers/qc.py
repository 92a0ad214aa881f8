"""Variant and sample QC reports and the single-SNP case/control table tests of a panel, in PLINK's file layouts.  Not a
reference workflow: the operators (ops.ld_hardy, ld_model, ld_test_missing, sample_qc) are this project's own definitions
(include/ldx.h, "genotype QC and table tests"), NOT validated against PLINK -- the mid-p halves the observed term only, and
dominant / recessive are with respect to the counted allele, not to the minor one; the files follow PLINK's columns.

    write_hardy          .hardy          PLINK 2    #CHROM ID A1 AX HOM_A1_CT HET_A1_CT TWO_AX_CT O(HET_A1) E(HET_A1) P
    write_vmiss          .vmiss          PLINK 2    #CHROM ID MISSING_CT OBS_CT F_MISS
    write_smiss          .smiss          PLINK 2    #FID IID MISSING_CT OBS_CT F_MISS
    write_het            .het            PLINK 2    #FID IID O(HOM) E(HOM) OBS_CT F
    write_model          .model          PLINK 1.9  CHR SNP A1 A2 TEST AFF UNAFF CHISQ DF P
    write_assoc_fisher   .assoc.fisher   PLINK 1.9  CHR SNP BP A1 F_A F_U A2 P OR
    write_test_missing   .missing        PLINK 1.9  CHR SNP F_MISS_A F_MISS_U P

A1 is the counted allele (code 1, ALT) everywhere.  Numbers are written with the shortest text that reads back to the same
float64; a P below the float64 range is written from its -log10 (drivers/glm.py's p_text); an undefined cell is NA.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List

import numpy as np

from .._lib import LdxError
from ..ops import MODEL_TESTS, HardyResult, MissingResult, ModelResult, SampleQC
from .glm import _txt, p_text

HARDY_COLUMNS = ("#CHROM", "ID", "A1", "AX", "HOM_A1_CT", "HET_A1_CT", "TWO_AX_CT", "O(HET_A1)", "E(HET_A1)", "P")
VMISS_COLUMNS = ("#CHROM", "ID", "MISSING_CT", "OBS_CT", "F_MISS")
SMISS_COLUMNS = ("#FID", "IID", "MISSING_CT", "OBS_CT", "F_MISS")
HET_COLUMNS = ("#FID", "IID", "O(HOM)", "E(HOM)", "OBS_CT", "F")
MODEL_COLUMNS = ("CHR", "SNP", "A1", "A2", "TEST", "AFF", "UNAFF", "CHISQ", "DF", "P")
FISHER_COLUMNS = ("CHR", "SNP", "BP", "A1", "F_A", "F_U", "A2", "P", "OR")
TEST_MISSING_COLUMNS = ("CHR", "SNP", "F_MISS_A", "F_MISS_U", "P")
MODEL_ORDER = ("GENO", "TREND", "ALLELIC", "DOM", "REC")     # the order of PLINK's lines per variant
MODEL_DF = {"GENO": 2, "TREND": 1, "ALLELIC": 1, "DOM": 1, "REC": 1}


@dataclass
class QcVariants:
    """Variant k is (chrom[k], pos[k], ids[k]) with the counted allele a1[k] (code 1) and the other allele ax[k]."""

    chrom: List[str]
    pos: List[int]
    ids: List[str]
    a1: List[str]
    ax: List[str]

    def __len__(self) -> int:
        return len(self.ids)


def _np(x) -> np.ndarray:
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _u32(x) -> np.ndarray:
    return _np(x).astype(np.int64) & 0xFFFFFFFF


def _num(x: float) -> str:
    return "NA" if math.isnan(x) else ("inf" if math.isinf(x) else _txt(x))


def _p(p: float, nlp: float) -> str:
    return "NA" if math.isnan(p) else p_text(float(p), float(nlp))


def _rows(what: str, variants: QcVariants, n: int) -> None:
    if len(variants) != n:
        raise LdxError(f"{what}: {len(variants)} variants beside {n} rows of the result")


def _write(path: str, columns, lines, sep: str = "\t") -> int:
    n = 0
    with open(path, "w") as f:
        f.write(sep.join(columns) + "\n")
        for line in lines:
            f.write(sep.join(line) + "\n")
            n += 1
    return n


def write_hardy(path: str, variants: QcVariants, result: HardyResult, group: int = 0) -> int:
    """``path``: the ``.hardy`` lines of one group of ``result`` (ops.ld_hardy's), tab-separated; a variant without a call in the
    group has NA in the last three columns.  Returns the number of lines."""
    c, o, e = _u32(result.counts)[:, group], _np(result.o_het)[:, group], _np(result.e_het)[:, group]
    p, nlp = _np(result.p)[:, group], _np(result.neglog10_p)[:, group]
    _rows("write_hardy", variants, c.shape[0])
    return _write(path, HARDY_COLUMNS, (
        (variants.chrom[k], variants.ids[k], variants.a1[k], variants.ax[k], str(c[k, 2]), str(c[k, 1]),
         str(c[k, 0] - c[k, 1] - c[k, 2]), _num(o[k]), _num(e[k]), _p(p[k], nlp[k])) for k in range(len(variants))))


def write_vmiss(path: str, variants: QcVariants, called, n_ind: int) -> int:
    """``path``: the ``.vmiss`` lines from the called individuals per variant (column 0 of geno_snp_counts, or of one group of
    geno_group_counts with that group's size as ``n_ind``)."""
    n = _u32(called).reshape(-1)
    _rows("write_vmiss", variants, n.size)
    return _write(path, VMISS_COLUMNS, ((variants.chrom[k], variants.ids[k], str(n_ind - n[k]), str(n_ind),
                                         _num((n_ind - n[k]) / n_ind if n_ind else math.nan)) for k in range(n.size)))


def write_smiss(path: str, fid, iid, qc: SampleQC) -> int:
    """``path``: the ``.smiss`` lines of ops.sample_qc's result: missing and observed calls over the kept variants."""
    miss = qc.f_miss
    return _write(path, SMISS_COLUMNS, ((str(fid[k]), str(iid[k]), str(qc.n_kept - int(qc.called[k])), str(qc.n_kept), _num(float(miss[k])))
                                        for k in range(len(iid))))


def write_het(path: str, fid, iid, qc: SampleQC) -> int:
    """``path``: the ``.het`` lines of ops.sample_qc's result: observed and expected homozygous calls, called variants and F."""
    return _write(path, HET_COLUMNS, ((str(fid[k]), str(iid[k]), str(int(qc.called[k] - qc.het[k])), _num(float(qc.e_hom[k])),
                                       str(int(qc.called[k])), _num(float(qc.f[k]))) for k in range(len(iid))))


def model_cells(case_counts, ctrl_counts) -> dict:
    """{TEST: (AFF, UNAFF)} as PLINK writes them, arrays of strings per variant: GENO hom A1 / het / hom A2, TREND and ALLELIC
    A1 / A2 alleles, DOM (hom A1 + het) / hom A2, REC hom A1 / (het + hom A2)."""
    out = {}
    for name, c in (("AFF", _u32(case_counts)), ("UNAFF", _u32(ctrl_counts))):
        n, het, hom = c[:, 0], c[:, 1], c[:, 2]
        ref, a = n - het - hom, het + 2 * hom
        out[name] = {"GENO": [f"{x}/{y}/{z}" for x, y, z in zip(hom, het, ref)],
                     "TREND": [f"{x}/{y}" for x, y in zip(a, 2 * n - a)],
                     "DOM": [f"{x}/{y}" for x, y in zip(hom + het, ref)],
                     "REC": [f"{x}/{y}" for x, y in zip(hom, het + ref)]}
        out[name]["ALLELIC"] = out[name]["TREND"]
    return {t: (out["AFF"][t], out["UNAFF"][t]) for t in MODEL_ORDER}


def write_model(path: str, variants: QcVariants, result: ModelResult) -> int:
    """``path``: the ``.model`` lines of ops.ld_model's result, five per variant in PLINK's order GENO, TREND, ALLELIC, DOM, REC;
    a flagged test has NA in CHISQ, DF and P.  Returns the number of lines."""
    chisq, p, nlp, flags = (_np(x) for x in (result.chisq, result.p, result.neglog10_p, result.flags))
    _rows("write_model", variants, chisq.shape[0])
    cells = model_cells(result.case_counts, result.ctrl_counts)

    def lines():
        for k in range(len(variants)):
            for test in MODEL_ORDER:
                t = MODEL_TESTS.index(test)
                tail = ("NA", "NA", "NA") if flags[k, t] else (_txt(chisq[k, t]), str(MODEL_DF[test]), _p(p[k, t], nlp[k, t]))
                yield (variants.chrom[k], variants.ids[k], variants.a1[k], variants.ax[k], test, cells[test][0][k],
                       cells[test][1][k]) + tail

    return _write(path, MODEL_COLUMNS, lines())


def _freq(c: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.where(c[:, 0] > 0, (c[:, 1] + 2 * c[:, 2]) / np.where(c[:, 0] > 0, 2.0 * c[:, 0], 1.0), np.nan)


def write_assoc_fisher(path: str, variants: QcVariants, result: ModelResult) -> int:
    """``path``: the ``.assoc.fisher`` lines of an ops.ld_model result made with ``fisher``: the A1 frequencies of cases and
    controls, Fisher's exact P on the allele counts and the allelic odds ratio.  The ``clump`` subcommand reads it with
    ``--clump-snp-field SNP --clump-field P``."""
    if result.fisher_p is None:
        raise LdxError("write_assoc_fisher: the result was made with fisher=False")
    p, nlp, odds = _np(result.fisher_p), _np(result.fisher_neglog10_p), _np(result.odds)
    fa, fu = _freq(_u32(result.case_counts)), _freq(_u32(result.ctrl_counts))
    _rows("write_assoc_fisher", variants, p.size)
    return _write(path, FISHER_COLUMNS, ((variants.chrom[k], variants.ids[k], str(variants.pos[k]), variants.a1[k], _num(fa[k]), _num(fu[k]),
                                          variants.ax[k], _p(p[k], nlp[k]), _num(odds[k])) for k in range(p.size)))


def write_test_missing(path: str, variants: QcVariants, result: MissingResult) -> int:
    """``path``: the ``.missing`` lines of ops.ld_test_missing's result: the missing-call rates of cases and controls and
    Fisher's exact P."""
    fa, fu, p, nlp = (_np(x) for x in (result.f_miss_case, result.f_miss_ctrl, result.p, result.neglog10_p))
    _rows("write_test_missing", variants, p.size)
    return _write(path, TEST_MISSING_COLUMNS, ((variants.chrom[k], variants.ids[k], _num(fa[k]), _num(fu[k]), _p(p[k], nlp[k]))
                                               for k in range(p.size)))

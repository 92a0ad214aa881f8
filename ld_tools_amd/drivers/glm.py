"""Linear association scans of the variants of a panel, in the layout of PLINK 2's ``.glm.linear`` (--glm on a quantitative
trait).  Not a reference workflow: ops.ld_glm is this project's own definition (include/ldx.h, "association scan"), NOT
validated against PLINK 2 -- a missing genotype counts as the variant's mean, where PLINK refits over the called individuals, so
the numbers differ wherever a call is missing; the file follows PLINK's layout.  Numbers are written with the shortest text that
reads back to the same float64; a P below the float64 range is written from its -log10, so it keeps its exponent.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from .._lib import LdxError
from ..ops import LOGIT_FLAGS, GlmResult, LogitResult, ld_glm, ld_glm_logistic

GLM_COLUMNS = ("#CHROM", "POS", "ID", "REF", "ALT", "A1", "TEST", "OBS_CT", "BETA", "SE", "T_STAT", "P")
LOGISTIC_COLUMNS = ("#CHROM", "POS", "ID", "REF", "ALT", "A1", "TEST", "OBS_CT", "OR", "LOG(OR)_SE", "Z_STAT", "P", "ERRCODE")
HYBRID_COLUMNS = LOGISTIC_COLUMNS[:6] + ("FIRTH?",) + LOGISTIC_COLUMNS[6:]   # PLINK 2's .glm.logistic.hybrid
LOGISTIC_ERRCODES = {k: v.upper().replace(" ", "_") for k, v in LOGIT_FLAGS.items() if k}   # the name of a flag as one word


@dataclass
class GlmTable:
    """Variant k is (chrom[k], pos[k], ids[k]) with the alleles ref[k], alt[k]; ``alt`` is the counted allele (A1: the sign of
    BETA).  ``names``: one per phenotype column of ``result`` (ops.ld_glm's)."""

    chrom: List[str]
    pos: List[int]
    ids: List[str]
    ref: List[str]
    alt: List[str]
    names: List[str]
    result: GlmResult


@dataclass
class LogisticTable(GlmTable):
    """A GlmTable whose ``result`` is the one of ops.ld_glm_logistic."""

    result: LogitResult


def logistic_table(panel, variants: dict, Y, covar=None, names: Optional[Sequence[str]] = None, **more) -> LogisticTable:
    """ops.ld_glm_logistic of ``panel`` with the columns of its variants, as glm_table: ``Y`` holds 0 (control) and 1 (case);
    ``more``: the individuals, keep, max_vif and firth (None, "fallback" or "always") of ld_glm_logistic."""
    cols = {}
    for key in ("chrom", "pos", "ids", "ref", "alt"):
        if key not in variants or len(variants[key]) != panel.n_snps:
            raise LdxError(f"logistic_table: variants[{key!r}] needs one entry per SNP of the panel ({panel.n_snps})")
        cols[key] = list(variants[key])
    res = ld_glm_logistic(panel, Y, covar, **more)
    n_pheno = res.design.n_pheno
    names = [f"PHENO{j + 1}" for j in range(n_pheno)] if names is None else [str(n) for n in names]
    if len(names) != n_pheno:
        raise LdxError(f"logistic_table: {len(names)} names for {n_pheno} phenotypes")
    return LogisticTable([str(c) for c in cols["chrom"]], [int(p) for p in cols["pos"]], [str(i) for i in cols["ids"]],
                         [str(a) for a in cols["ref"]], [str(a) for a in cols["alt"]], names, res)


def glm_table(panel, variants: dict, Y, covar=None, names: Optional[Sequence[str]] = None, **more) -> GlmTable:
    """ops.ld_glm of ``panel`` with the columns of its variants: ``variants`` holds ``chrom``, ``pos``, ``ids``, ``ref`` and
    ``alt`` (the allele that is code 1), one entry per SNP of the panel.  ``names``: the phenotypes' names (default PHENO1 ...);
    ``more``: ld_glm's individuals, keep and max_vif."""
    cols = {}
    for key in ("chrom", "pos", "ids", "ref", "alt"):
        if key not in variants or len(variants[key]) != panel.n_snps:
            raise LdxError(f"glm_table: variants[{key!r}] needs one entry per SNP of the panel ({panel.n_snps})")
        cols[key] = list(variants[key])
    res = ld_glm(panel, Y, covar, **more)
    n_pheno = res.design.n_pheno
    names = [f"PHENO{j + 1}" for j in range(n_pheno)] if names is None else [str(n) for n in names]
    if len(names) != n_pheno:
        raise LdxError(f"glm_table: {len(names)} names for {n_pheno} phenotypes")
    return GlmTable([str(c) for c in cols["chrom"]], [int(p) for p in cols["pos"]], [str(i) for i in cols["ids"]],
                    [str(a) for a in cols["ref"]], [str(a) for a in cols["alt"]], names, res)


def _txt(x: float) -> str:
    return repr(float(x))


def p_text(p: float, neglog10_p: float) -> str:
    """The text of a p-value: the shortest that reads back to ``p`` while p is a normal float64; below that m e-X from
    ``neglog10_p`` (six digits of m), "0" where that is infinite."""
    if p >= 2.2250738585072014e-308:
        return _txt(p)
    if math.isinf(neglog10_p):
        return "0"
    ex = math.floor(-neglog10_p)
    m = f"{10.0 ** (-neglog10_p - ex):.6g}"
    if m == "10":            # the mantissa rounded up to the next decade
        m, ex = "1", ex + 1
    return f"{m}e{ex}"


def write_glm_linear(path: str, table: GlmTable, pheno=0) -> int:
    """``path``: the ``.glm.linear`` lines of one phenotype of ``table`` (its name or column number), tab-separated:
    ``#CHROM POS ID REF ALT A1 TEST OBS_CT BETA SE T_STAT P``, TEST = ADD, one line per variant; the cells of a flagged variant
    (ops.GLM_FLAGS other than 0 and 5) are NA.  Returns the number of lines."""
    j = table.names.index(pheno) if isinstance(pheno, str) else int(pheno)
    r = table.result
    beta, se, t, p, nlp = (x[:, j].cpu().numpy() for x in (r.beta, r.se, r.t, r.p, r.neglog10_p))
    flags, n_obs = r.flags[:, j].cpu().numpy(), r.n_obs
    with open(path, "w") as f:
        f.write("\t".join(GLM_COLUMNS) + "\n")
        for k in range(len(table.ids)):
            head = "\t".join((table.chrom[k], str(table.pos[k]), table.ids[k], table.ref[k], table.alt[k], table.alt[k], "ADD",
                              str(int(n_obs[k])))) + "\t"
            if flags[k] not in (0, 5):
                f.write(head + "NA\tNA\tNA\tNA\n")
            else:
                f.write(head + f"{_txt(beta[k])}\t{_txt(se[k])}\t{_txt(t[k])}\t{p_text(float(p[k]), float(nlp[k]))}\n")
    return len(table.ids)


def write_glm_logistic(path: str, table: LogisticTable, pheno=0) -> int:
    """``path``: the ``.glm.logistic`` lines of one phenotype of ``table`` (its name or column number), tab-separated, in the
    columns of PLINK 2: ``#CHROM POS ID REF ALT A1 TEST OBS_CT OR LOG(OR)_SE Z_STAT P ERRCODE``, TEST = ADD, OR = exp(beta),
    ERRCODE "." for a fitted variant; a flagged variant (ops.LOGIT_FLAGS other than 0) has NA in the four numbers and the name of
    its flag (LOGISTIC_ERRCODES) as ERRCODE -- flag 5, NO_FINITE_MAXIMISER, is where PLINK would have refitted by Firth
    regression.  Returns the number of lines."""
    j = table.names.index(pheno) if isinstance(pheno, str) else int(pheno)
    r = table.result
    beta, se, z, p, nlp = (x[:, j].cpu().numpy() for x in (r.beta, r.se, r.z, r.p, r.neglog10_p))
    flags, n_obs = r.flags[:, j].cpu().numpy(), r.n_obs
    with open(path, "w") as f:
        f.write("\t".join(LOGISTIC_COLUMNS) + "\n")
        for k in range(len(table.ids)):
            head = "\t".join((table.chrom[k], str(table.pos[k]), table.ids[k], table.ref[k], table.alt[k], table.alt[k], "ADD",
                              str(int(n_obs[k])))) + "\t"
            if flags[k] != 0:
                f.write(head + f"NA\tNA\tNA\tNA\t{LOGISTIC_ERRCODES[int(flags[k])]}\n")
            else:
                f.write(head + f"{_txt(math.exp(beta[k]))}\t{_txt(se[k])}\t{_txt(z[k])}\t{p_text(float(p[k]), float(nlp[k]))}\t.\n")
    return len(table.ids)


def _write_firth(path: str, table: LogisticTable, pheno, hybrid: bool) -> int:
    j = table.names.index(pheno) if isinstance(pheno, str) else int(pheno)
    r = table.result
    if r.firth is None:
        raise LdxError(f"{'write_glm_hybrid' if hybrid else 'write_glm_firth'}: the table holds a scan without firth=")
    beta, se, z, p, nlp = (x[:, j].cpu().numpy() for x in (r.beta, r.se, r.z, r.p, r.neglog10_p))
    flags, mark, n_obs = r.flags[:, j].cpu().numpy(), r.firth[:, j].cpu().numpy(), r.n_obs
    with open(path, "w") as f:
        f.write("\t".join(HYBRID_COLUMNS if hybrid else LOGISTIC_COLUMNS) + "\n")
        for k in range(len(table.ids)):
            head = (table.chrom[k], str(table.pos[k]), table.ids[k], table.ref[k], table.alt[k], table.alt[k])
            if hybrid:
                head += ("Y" if mark[k] else "N",)
            head = "\t".join(head + ("ADD", str(int(n_obs[k])))) + "\t"
            if flags[k] != 0:
                f.write(head + f"NA\tNA\tNA\tNA\t{LOGISTIC_ERRCODES[int(flags[k])]}\n")
            else:
                f.write(head + f"{_txt(math.exp(beta[k]))}\t{_txt(se[k])}\t{_txt(z[k])}\t{p_text(float(p[k]), float(nlp[k]))}\t.\n")
    return len(table.ids)


def write_glm_hybrid(path: str, table: LogisticTable, pheno=0) -> int:
    """``path``: the ``.glm.logistic.hybrid`` lines of one phenotype of a ``table`` scanned with ``firth=`` (PLINK 2's file of
    --glm firth-fallback): the columns of write_glm_logistic with ``FIRTH?`` in front of TEST -- Y where the line holds a Firth fit
    (the result's ``firth``), N elsewhere; a flagged variant as in write_glm_logistic.  Returns the number of lines."""
    return _write_firth(path, table, pheno, True)


def write_glm_firth(path: str, table: LogisticTable, pheno=0) -> int:
    """``path``: the ``.glm.firth`` lines of one phenotype of a ``table`` scanned with ``firth="always"`` (PLINK 2's file of
    --glm firth): the columns of write_glm_logistic, every fitted line a Firth fit.  Returns the number of lines."""
    return _write_firth(path, table, pheno, False)

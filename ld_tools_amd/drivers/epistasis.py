"""SNP x SNP interaction scans of a case/control panel in PLINK's file layouts.  Not a reference workflow: the operator
(ops.ld_epistasis_hits) is this project's own definition (include/ldx.h, "epistasis scan"), NOT validated against PLINK; the
files follow the columns of PLINK 1.9's --fast-epistasis.

    write_epi_cc         .epi.cc           CHR1 SNP1 CHR2 SNP2 STAT DIR P
    write_epi_summary    .epi.cc.summary   CHR SNP N_SIG N_TOT PROP BEST_CHISQ BEST_CHR BEST_SNP

STAT is the chi-square of the test (1 df for allelic, 4 df for boost) and DIR the difference of the two groups' log odds
ratios, case minus control (NA where an allele cell is empty).  P is written from the cell's float32 chi-square; one below the
float64 range is written from its -log10 (drivers/glm.py's p_text).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from .._lib import LdxError
from ..ops import EpiHits, epi_tail_host, ld_epistasis_hits
from ..panel import PackedPanel
from .glm import _txt, p_text
from .qc import _write

EPI_CC_COLUMNS = ("CHR1", "SNP1", "CHR2", "SNP2", "STAT", "DIR", "P")
EPI_SUMMARY_COLUMNS = ("CHR", "SNP", "N_SIG", "N_TOT", "PROP", "BEST_CHISQ", "BEST_CHR", "BEST_SNP")


@dataclass
class EpiTable:
    """epistasis_table's result: the hits and the summary (ops.EpiHits) beside the variants of the two sides -- row i of the
    scan is (chrom_i[i], ids_i[i]), column j is (chrom_j[j], ids_j[j])."""

    chrom_i: List[str]
    ids_i: List[str]
    chrom_j: List[str]
    ids_j: List[str]
    result: EpiHits


def epistasis_table(panel: PackedPanel, case, chrom, ids, panel_j: Optional[PackedPanel] = None, chrom_j=None, ids_j=None,
                    test: str = "boost", p: float = 1e-4, p_sig: float = 1e-2, chisq: Optional[float] = None,
                    hit_capacity: Optional[int] = None) -> EpiTable:
    """ops.ld_epistasis_hits on a panel with the names of its variants; ``panel_j`` (with ``chrom_j`` / ``ids_j``) makes it a
    set-by-set scan, None the scan of every pair of ``panel`` once."""
    chrom, ids = [str(c) for c in chrom], [str(i) for i in ids]
    if len(chrom) != panel.n_snps or len(ids) != panel.n_snps:
        raise LdxError(f"epistasis_table: {len(chrom)} chromosomes and {len(ids)} IDs for {panel.n_snps} variants")
    if panel_j is None:
        chrom_j, ids_j = chrom, ids
    else:
        if chrom_j is None or ids_j is None:
            raise LdxError("epistasis_table: panel_j needs chrom_j and ids_j")
        chrom_j, ids_j = [str(c) for c in chrom_j], [str(i) for i in ids_j]
        if len(chrom_j) != panel_j.n_snps or len(ids_j) != panel_j.n_snps:
            raise LdxError(f"epistasis_table: {len(chrom_j)} chromosomes and {len(ids_j)} IDs for {panel_j.n_snps} variants of panel_j")
    res = ld_epistasis_hits(panel, case, panel_j, test=test, chisq=chisq, p=p, p_sig=p_sig, hit_capacity=hit_capacity)
    return EpiTable(chrom, ids, chrom_j, ids_j, res)


def _num(x: float) -> str:
    return "NA" if math.isnan(x) else _txt(x)


def write_epi_cc(path: str, table: EpiTable) -> int:
    """``path``: one ``.epi.cc`` line per hit of ``table``, sorted by (row, column), tab-separated.  Returns the number of
    lines."""
    i, j, x, d = table.result.pairs()
    _, p, nlp = epi_tail_host(x.astype(np.float64), table.result.test)
    return _write(path, EPI_CC_COLUMNS, ((table.chrom_i[i[k]], table.ids_i[i[k]], table.chrom_j[j[k]], table.ids_j[j[k]],
                                          _txt(x[k]), _num(float(d[k])), p_text(float(p[k]), float(nlp[k]))) for k in range(i.size)))


def write_epi_summary(path: str, table: EpiTable) -> int:
    """``path``: the ``.epi.cc.summary`` lines, one per variant of the scan's rows: the tests at or above the summary's bound,
    the valid tests, their ratio, and the best chi-square with its partner (NA where the variant has no valid test)."""
    s = table.result.summary
    n_sig, n_tot = (t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF for t in (s.n_sig, s.n_tot))
    best, partner = s.best_chisq.cpu().numpy(), s.best_partner.cpu().numpy()

    def lines():
        for k in range(n_tot.size):
            if n_tot[k]:
                tail = (_txt(n_sig[k] / n_tot[k]), _txt(best[k]), table.chrom_j[partner[k]], table.ids_j[partner[k]])
            else:
                tail = ("NA", "NA", "NA", "NA")
            yield (table.chrom_i[k], table.ids_i[k], str(n_sig[k]), str(n_tot[k])) + tail

    return _write(path, EPI_SUMMARY_COLUMNS, lines())

"""Principal components and polygenic scores of the individuals of a panel, in the layouts of PLINK 2's ``.eigenvec`` /
``.eigenval`` (--pca) and ``.sscore`` (--score).  Not a reference workflow: ops.sample_pca and ops.polygenic_score run on the
genotype products of the matrix cores (include/ldx.h, "genotype products"), and both are this project's own definitions, NOT
validated against PLINK 2, GCTA or FastPCA; the files follow their layout, the numbers need not match their digits.  Numbers
are written with the shortest text that reads back to the same float64.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from .._lib import LdxError
from ..ops import SamplePCA, Scores, polygenic_score, sample_pca
from .king import _ids, _write_ids  # noqa: F401


@dataclass
class PcaTable:
    """Individual k is (fid[k], iid[k]) with the coordinates ``coords[k]`` (float64 [n_ind, n_pcs]): its entries of the
    eigenvectors when it took part in the decomposition (``in_pca[k]``), else its projection on them."""

    fid: List[str]
    iid: List[str]
    pca: SamplePCA
    coords: np.ndarray
    in_pca: np.ndarray


@dataclass
class ScoreTable:
    """Individual k is (fid[k], iid[k]); ``scores``: ops.polygenic_score's result; ``n_matched`` of ``n_lines`` weight lines
    named a variant and one of its alleles (drivers/plink.py's bfile_score sets them)."""

    fid: List[str]
    iid: List[str]
    scores: Scores
    n_matched: Optional[int] = None
    n_lines: Optional[int] = None


def pca_table(panel, sample_ids: Sequence, n_pcs: int = 10, keep=None, unrelated=None, **more) -> PcaTable:
    """ops.sample_pca of ``panel`` over the SNPs that pass ``keep``.  ``sample_ids``: one IID, or one (FID, IID) pair, per
    individual.  ``unrelated`` (bool [n_ind]; None: everybody): the individuals decomposed; the others are projected on their
    components (SamplePCA.project).  ``more``: sample_pca's oversample, n_iter and seed."""
    fid, iid = _ids(sample_ids, panel.n_ind)
    if unrelated is None or np.asarray(unrelated).all():
        pca = sample_pca(panel, n_pcs=n_pcs, keep=keep, **more)
        return PcaTable(fid, iid, pca, pca.eigenvectors, np.ones(panel.n_ind, dtype=bool))
    inside = np.asarray(unrelated).astype(bool)
    if inside.shape != (panel.n_ind,) or not inside.any():
        raise LdxError(f"pca_table: unrelated must be a bool array [{panel.n_ind}] with an individual set")

    def columns(mask):
        k = np.flatnonzero(mask)
        return np.stack([2 * k, 2 * k + 1], axis=1).reshape(-1)

    pca = sample_pca(panel.select(haplotypes=columns(inside)), n_pcs=n_pcs, keep=keep, loadings=True, **more)
    coords = np.empty((panel.n_ind, pca.eigenvectors.shape[1]), dtype=np.float64)
    coords[inside] = pca.eigenvectors
    coords[~inside] = pca.project(panel.select(haplotypes=columns(~inside)), keep=keep)
    return PcaTable(fid, iid, pca, coords, inside)


def _txt(x: float) -> str:
    return repr(float(x))


def write_eigenvec(path: str, table: PcaTable) -> int:
    """``path``: ``#IID PC1 PC2 ...`` (tab-separated; ``#FID IID ...`` when a FID differs from its IID), one line per
    individual.  Returns the number of lines."""
    with_fid = any(f != i for f, i in zip(table.fid, table.iid))
    n_pcs = table.coords.shape[1]
    with open(path, "w") as f:
        f.write(("#FID\tIID\t" if with_fid else "#IID\t") + "\t".join(f"PC{j + 1}" for j in range(n_pcs)) + "\n")
        for k, row in enumerate(table.coords.tolist()):
            f.write((f"{table.fid[k]}\t" if with_fid else "") + table.iid[k] + "\t" + "\t".join(_txt(v) for v in row) + "\n")
    return len(table.iid)


def write_eigenval(path: str, table: PcaTable) -> int:
    """``path``: one eigenvalue per line, largest first."""
    with open(path, "w") as f:
        f.writelines(_txt(v) + "\n" for v in table.pca.eigenvalues.tolist())
    return int(table.pca.eigenvalues.size)


def score_table(panel, sample_ids: Sequence, beta, keep=None, impute: str = "mean", offset=None) -> ScoreTable:
    """ops.polygenic_score of ``panel`` with the IDs of its individuals."""
    fid, iid = _ids(sample_ids, panel.n_ind)
    return ScoreTable(fid, iid, polygenic_score(panel, beta, keep=keep, impute=impute, offset=offset))


def write_sscore(path: str, table: ScoreTable) -> int:
    """``path``: ``#IID ALLELE_CT SCORE1_SUM SCORE2_SUM ...`` (tab-separated; ``#FID IID ...`` when a FID differs from its IID).
    Returns the number of lines."""
    with_fid = any(f != i for f, i in zip(table.fid, table.iid))
    s = table.scores
    with open(path, "w") as f:
        f.write(("#FID\tIID\t" if with_fid else "#IID\t") + "ALLELE_CT\t"
                + "\t".join(f"SCORE{j + 1}_SUM" for j in range(s.sum.shape[1])) + "\n")
        for k, row in enumerate(s.sum.tolist()):
            f.write((f"{table.fid[k]}\t" if with_fid else "") + f"{table.iid[k]}\t{int(s.allele_ct[k])}\t"
                    + "\t".join(_txt(v) for v in row) + "\n")
    return len(table.iid)

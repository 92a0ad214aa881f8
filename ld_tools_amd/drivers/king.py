"""Sample relatedness tables in the layouts of PLINK 2's KING-robust outputs: ``.kin0`` (one line per pair), ``.king`` +
``.king.id`` (the lower triangle as text) and ``.king.cutoff.in.id`` / ``.king.cutoff.out.id`` (a maximal set of unrelated
individuals).  Not a reference workflow: it runs ops.sample_counts on a packed panel -- the panel is transposed on the device
and the pair counts come from the FP4 matrix cores -- and the cells are this project's own definition (include/ldx.h,
"sample relatedness"), NOT validated against PLINK 2 or KING; the files follow their layout, the numbers need not match
their last digits.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .._lib import LdxError
from ..ops import RelatedPairs, SampleCounts, king_cutoff, sample_counts

KIN0_HEADER = "#FID1\tIID1\tFID2\tIID2\tNSNP\tHETHET\tIBS0\tKINSHIP"


@dataclass
class KingTable:
    """Individual k of the counts is (fid[k], iid[k]).  ``kin_min``: the bound of the pair table (None: every pair)."""

    fid: List[str]
    iid: List[str]
    counts: SampleCounts
    kin_min: Optional[float] = None
    snp_mask: Optional[np.ndarray] = None   # the SNPs counted (bool over the panel's), None: all

    def pairs(self) -> RelatedPairs:
        """The pairs a > b of the table, row-major: all of them, or those with kinship >= kin_min."""
        return self.counts.related(float("-inf") if self.kin_min is None else self.kin_min)


def _ids(sample_ids, n_ind: int) -> Tuple[List[str], List[str]]:
    ids = list(sample_ids)
    if len(ids) != n_ind:
        raise LdxError(f"king_table: {len(ids)} sample IDs for {n_ind} individuals")
    if ids and isinstance(ids[0], (tuple, list)):
        return [str(f) for f, _ in ids], [str(i) for _, i in ids]
    return [str(i) for i in ids], [str(i) for i in ids]


def king_table(panel, sample_ids: Sequence, keep=None, kin_min: Optional[float] = None) -> KingTable:
    """The counts of every pair of individuals of ``panel`` over the SNPs that pass ``keep`` (bool [n_snps]; None: all).
    ``sample_ids``: one IID, or one (FID, IID) pair, per individual (an IID alone is its own FID)."""
    fid, iid = _ids(sample_ids, panel.n_ind)
    mask = None if keep is None else np.asarray(keep.cpu() if hasattr(keep, "cpu") else keep).astype(bool)
    return KingTable(fid, iid, sample_counts(panel, keep=keep), kin_min, mask)


def _num(x: float) -> str:
    return f"{float(x):.6g}"


def kin0_lines(fid: Sequence[str], iid: Sequence[str], pairs: RelatedPairs) -> List[str]:
    """The lines of a ``.kin0`` table without the header: individual 1 is the pair's smaller index."""
    out = []
    for a, b, kin, n, hh, i0 in zip(pairs.a.tolist(), pairs.b.tolist(), pairs.kin.tolist(), pairs.n.tolist(),
                                    pairs.hethet.tolist(), pairs.ibs0.tolist()):
        den = n if n else 1
        out.append(f"{fid[b]}\t{iid[b]}\t{fid[a]}\t{iid[a]}\t{n}\t{_num(hh / den)}\t{_num(i0 / den)}\t{_num(kin)}")
    return out


def write_kin0(path: str, table: KingTable, pairs: Optional[RelatedPairs] = None) -> int:
    """``path``: ``#FID1 IID1 FID2 IID2 NSNP HETHET IBS0 KINSHIP`` (tab-separated), one line per pair of the table (or of
    ``pairs``); HETHET and IBS0 are fractions of NSNP, six significant digits.  Returns the number of pairs."""
    lines = kin0_lines(table.fid, table.iid, table.pairs() if pairs is None else pairs)
    with open(path, "w") as f:
        f.write(KIN0_HEADER + "\n")
        f.writelines(line + "\n" for line in lines)
    return len(lines)


def _write_ids(path: str, fid: Sequence[str], iid: Sequence[str], rows) -> None:
    with open(path, "w") as f:
        f.write("#FID\tIID\n")
        f.writelines(f"{fid[k]}\t{iid[k]}\n" for k in rows)


def write_king_matrix(base: str, table: KingTable, kin=None) -> List[str]:
    """``{base}.king``: the kinship of individual a = 1 .. n - 1 against b = 0 .. a - 1, one tab-separated line per a, six
    significant digits; ``{base}.king.id``: the individuals in order.  Returns the two paths."""
    k = table.counts.kinship().cpu().numpy() if kin is None else np.asarray(kin)
    paths = [base + ".king", base + ".king.id"]
    with open(paths[0], "w") as f:
        for a in range(1, k.shape[0]):
            f.write("\t".join(_num(v) for v in k[a, :a].tolist()) + "\n")
    _write_ids(paths[1], table.fid, table.iid, range(len(table.iid)))
    return paths


def write_king_cutoff(base: str, table: KingTable, cutoff: float, kin=None) -> List[str]:
    """``{base}.king.cutoff.in.id`` / ``.out.id``: ops.king_cutoff's kept and removed individuals, in order."""
    k = table.counts.kinship() if kin is None else kin
    keep, _ = king_cutoff(k, cutoff)
    paths = [base + ".king.cutoff.in.id", base + ".king.cutoff.out.id"]
    _write_ids(paths[0], table.fid, table.iid, np.flatnonzero(keep).tolist())
    _write_ids(paths[1], table.fid, table.iid, np.flatnonzero(~keep).tolist())
    return paths

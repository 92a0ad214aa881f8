"""Haplotype blocks as text: PLINK's ``.blocks`` / ``.blocks.det`` pair from an ``ops.LDBlocks``."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from ..ops import NOT_KEPT


def write_blocks(prefix: str, result, ids: Optional[Sequence[str]] = None, chrom: str = "1") -> Tuple[str, str]:
    """``{prefix}.blocks``: one ``* id id ...`` line per block of at least two SNPs; ``{prefix}.blocks.det``: PLINK's table
    ``CHR BP1 BP2 KB NSNPS SNPS`` of the same blocks, KB = (BP2 - BP1 + 1) / 1000 and the ids joined by ``|``.  ``result`` is
    an ``ops.LDBlocks`` (anything with ``block_of`` and ``positions``); ``ids`` default to ``snp{row}``.  The blocks are the
    greedy left-to-right (Hudson-Kaplan) partition, not Haploview's block-picking order.  Returns the two paths."""
    block_of = np.asarray(result.block_of)
    pos = result.positions
    pos = np.asarray(pos.cpu().numpy() if hasattr(pos, "cpu") else pos, dtype=np.int64)
    n = block_of.shape[0]
    if ids is None:
        ids = ["snp%d" % i for i in range(n)]
    if len(ids) != n or pos.shape != (n,):
        raise ValueError("ids and positions must have one entry per SNP")
    kept = np.flatnonzero(block_of != NOT_KEPT)
    cuts = np.flatnonzero(np.diff(block_of[kept].astype(np.int64)) != 0) + 1
    plain, det = [], ["CHR\tBP1\tBP2\tKB\tNSNPS\tSNPS\n"]
    for members in np.split(kept, cuts):
        if members.size < 2:
            continue
        names = [str(ids[i]) for i in members]
        bp1, bp2 = int(pos[members[0]]), int(pos[members[-1]])
        plain.append("* " + " ".join(names) + "\n")
        det.append("%s\t%d\t%d\t%.3f\t%d\t%s\n" % (chrom, bp1, bp2, (bp2 - bp1 + 1) / 1000.0, members.size, "|".join(names)))
    paths = (prefix + ".blocks", prefix + ".blocks.det")
    with open(paths[0], "w", encoding="ascii", newline="\n") as f:
        f.write("".join(plain))
    with open(paths[1], "w", encoding="ascii", newline="\n") as f:
        f.write("".join(det))
    return paths

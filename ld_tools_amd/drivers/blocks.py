"""Haplotype blocks as text: PLINK's ``.blocks`` / ``.blocks.det`` pair from an ``ops.LDBlocks`` (four-gamete partition) or an
``ops.GabrielBlocks`` (D' confidence-interval blocks), and the Gabriel blocks of one chromosome of a VCF."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..ops import NO_BLOCK, NOT_KEPT, GabrielBlocks, ld_gabriel_blocks


@dataclass
class GabrielTable:
    """Row k of ``result.block_of`` is variant k of these lists (position-sorted)."""

    chrom: str
    rs_ids: List[str]
    poss: List[int]
    result: GabrielBlocks

    @property
    def n(self) -> int:
        return len(self.rs_ids)


def gabriel_blocks(vcf, chrom, chrom_rows: Sequence[Sequence], sample_names: Sequence[str], window_bp: int = 500_000,
                   missing: Optional[str] = None, maf_min: float = 0.05, keep=None, **params) -> GabrielTable:
    """Gabriel's D' confidence-interval blocks of one chromosome's variants (VCF rows [pos, rsID]; each record fetched once):
    ops.ld_gabriel_blocks on the unphased genotypes.  ``missing``, ``maf_min``, ``keep`` and ``params`` are its."""
    from .em import _chrom_em_panel

    panel, rs_ids, poss = _chrom_em_panel("gabriel_blocks", vcf, chrom, chrom_rows, sample_names)
    res = ld_gabriel_blocks(panel, np.asarray(poss, dtype=np.int64), window_bp=window_bp, missing=missing, keep=keep,
                            maf_min=maf_min, **params)
    return GabrielTable(str(chrom), rs_ids, poss, res)


def gabriel_block_rows(result, ids: Optional[Sequence[str]] = None) -> list:
    """[(bp1, bp2, [member ids])] of every block of an ``ops.GabrielBlocks`` (anything with ``block_of`` and ``ci.positions`` or
    ``positions``), in position order.  Only members are listed: a SNP that is not kept may lie between a block's ends."""
    block_of = np.asarray(result.block_of)
    pos = result.ci.positions if hasattr(result, "ci") else result.positions
    pos = np.asarray(pos.cpu().numpy() if hasattr(pos, "cpu") else pos, dtype=np.int64)
    n = block_of.shape[0]
    if ids is None:
        ids = ["snp%d" % i for i in range(n)]
    if len(ids) != n or pos.shape != (n,):
        raise ValueError("ids and positions must have one entry per SNP")
    members = np.flatnonzero(block_of < NO_BLOCK)
    order = np.argsort(block_of[members], kind="stable")
    members = members[order]
    cuts = np.flatnonzero(np.diff(block_of[members].astype(np.int64)) != 0) + 1
    rows = []
    for m in (np.split(members, cuts) if members.size else []):
        rows.append((int(pos[m[0]]), int(pos[m[-1]]), [str(ids[i]) for i in m]))
    return rows


def write_gabriel_blocks(prefix: str, result, ids: Optional[Sequence[str]] = None, chrom: str = "1") -> Tuple[str, str]:
    """``write_blocks``' two files for an ``ops.GabrielBlocks``: one ``* id id ...`` line and one ``CHR BP1 BP2 KB NSNPS SNPS``
    row per block, members only.  (``write_blocks`` merges runs of equal ``block_of`` and would join two blocks across SNPs
    that are in none.)  Returns the two paths."""
    plain, det = [], ["CHR\tBP1\tBP2\tKB\tNSNPS\tSNPS\n"]
    for bp1, bp2, names in gabriel_block_rows(result, ids):
        plain.append("* " + " ".join(names) + "\n")
        det.append("%s\t%d\t%d\t%.3f\t%d\t%s\n" % (chrom, bp1, bp2, (bp2 - bp1 + 1) / 1000.0, len(names), "|".join(names)))
    paths = (prefix + ".blocks", prefix + ".blocks.det")
    with open(paths[0], "w", encoding="ascii", newline="\n") as f:
        f.write("".join(plain))
    with open(paths[1], "w", encoding="ascii", newline="\n") as f:
        f.write("".join(det))
    return paths


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

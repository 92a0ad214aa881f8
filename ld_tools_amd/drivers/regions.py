"""LD-independent regions as text: an ldetect-style ``.bed`` and a ``.regions.det`` table from an ``ops.LDRegions``."""
from __future__ import annotations

from typing import Tuple

import numpy as np


def write_regions(prefix: str, result, chrom: str = "1") -> Tuple[str, str]:
    """``{prefix}.bed``: ldetect's table, header ``chr start stop`` (tab-separated), one line per region with start = the
    position of the region's first SNP and stop = the position of the next region's first SNP (the last region: its last
    position + 1), so the intervals are half-open and tile the chromosome.  ``{prefix}.regions.det``: ``CHR BP1 BP2 KB NSNPS
    CUT_R2`` per region -- first and last position, (BP2 - BP1 + 1) / 1000, the SNP count and the r^2 that crosses the cut
    in front of the region (0 for the first).  ``result`` is an ``ops.LDRegions`` (anything with ``starts``, ``ends``,
    ``sizes``, ``positions`` and ``cross_at_cuts``).  Returns the two paths."""
    pos = np.asarray(result.positions, dtype=np.int64)
    starts, ends, sizes = (np.asarray(v, dtype=np.int64) for v in (result.starts, result.ends, result.sizes))
    at_cut = np.concatenate([[0.0], np.asarray(result.cross_at_cuts, dtype=np.float64)])
    if not starts.shape == ends.shape == sizes.shape == at_cut.shape:
        raise ValueError("starts, ends, sizes and cross_at_cuts do not describe the same regions")
    stops = np.concatenate([pos[starts[1:]], [pos[-1] + 1]])
    bed = ["chr\tstart\tstop\n"] + ["chr%s\t%d\t%d\n" % (chrom, pos[s], e) for s, e in zip(starts, stops)]
    det = ["CHR\tBP1\tBP2\tKB\tNSNPS\tCUT_R2\n"]
    for s, e, m, c in zip(starts, ends, sizes, at_cut):
        bp1, bp2 = int(pos[s]), int(pos[e])
        det.append("%s\t%d\t%d\t%.3f\t%d\t%.4f\n" % (chrom, bp1, bp2, (bp2 - bp1 + 1) / 1000.0, m, c))
    paths = (prefix + ".bed", prefix + ".regions.det")
    for path, lines in zip(paths, (bed, det)):
        with open(path, "w", encoding="ascii", newline="\n") as f:
            f.write("".join(lines))
    return paths

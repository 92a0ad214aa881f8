"""LD decay curves as text: PopLDdecay's ``.stat`` table from an ``ops.LDDecay``."""
from __future__ import annotations

import gzip
from typing import Optional, Sequence

import numpy as np

from ..ops import LDDecay


def write_decay(prefix: str, result: LDDecay, rebin: Optional[Sequence[int]] = None) -> str:
    """``{prefix}.stat.gz``: tab-separated ``#Dist  Mean_r^2  Sum_r^2  NumberPairs``, one line per non-empty bin, Dist the
    bin's upper edge (the window + 1 for the last one: its distances end at the window).  ``rebin``: edges for
    ``LDDecay.rebin`` -- the coarse second stage of PopLDdecay's binning over the kernel's fine bins.  The file is
    deterministic: fixed float formats, no file name and no time stamp in the gzip header.  Returns the path."""
    if rebin is None:
        sums, counts = result.sum_r2, result.counts
        upper = np.minimum(result.distance + result.bin_width, result.window + 1)
    else:
        sums, counts = result.rebin(rebin)
        upper = np.minimum(np.asarray(rebin, dtype=np.int64)[1:], result.window + 1)
    lines = ["#Dist\tMean_r^2\tSum_r^2\tNumberPairs\n"]
    for d, s, c in zip(upper, sums, counts):
        if c > 0:
            lines.append("%d\t%.6f\t%.4f\t%d\n" % (int(d), s / c, s, int(c)))
    path = prefix + ".stat.gz"
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as out:
        out.write("".join(lines).encode("ascii"))
    return path

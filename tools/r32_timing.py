"""Kernel time of the signed-r cells against the 4-byte k16 and the 2-byte k16r cells, and the export rate of r_matrix().

    python tools/r32_timing.py [--snps 10000 40000] [--haps 5008] [--regions 7] [--reps 10] [--export 40000] [--out FILE]

Per panel the three formats are timed INTERLEAVED (r32, k16, k16r, r32, ...) so that clock drift hits all of them alike:
each region is `reps` launches of ld_triangle(p, fmt=..., out=...) between two device events; the median region over
`regions` is reported per launch.  The export rate is bytes written + strip bytes read over the time of one whole
r_matrix() of the largest panel (median of three).  One JSON object is printed (and written to --out).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from ld_tools_amd import PackedPanel, ops, synth  # noqa: E402

FMTS = ("r32", "k16", "k16r")


def region_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, nargs="+", default=[10_000, 40_000])
    ap.add_argument("--haps", type=int, default=5008)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--export", type=int, default=40_000, help="panel size of the r_matrix() rate (0: skip)")
    ap.add_argument("--once", action="store_true", help="one r32 launch only (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    report = {"haps": a.haps, "triangle_ms": {}}
    for n in a.snps:
        codes = synth.synth_codes_device(n, a.haps, device=dev)
        p = PackedPanel.from_codes(codes, dev)
        del codes
        if a.once:
            ops.ld_triangle(p, fmt="r32")
            torch.cuda.synchronize()
            print(json.dumps({"once": n}))
            return
        outs = {f: ops.ld_triangle(p, fmt=f) for f in FMTS}
        for f in FMTS:                                   # warm-up
            for _ in range(3):
                ops.ld_triangle(p, fmt=f, out=outs[f])
        times = {f: [] for f in FMTS}
        for _ in range(a.regions):
            for f in FMTS:
                times[f].append(region_ms(lambda: ops.ld_triangle(p, fmt=f, out=outs[f]), a.reps))
        med = {f: statistics.median(v) for f, v in times.items()}
        report["triangle_ms"][str(n)] = {"median": med, "regions": times,
                                         "r32_over_k16": med["r32"] / med["k16"], "r32_over_k16r": med["r32"] / med["k16r"]}
        if n == a.export:
            res = outs["r32"]
            del outs
            torch.cuda.empty_cache()
            ex = [region_ms(lambda: res.r_matrix(), 1) for _ in range(4)][1:]
            ms = statistics.median(ex)
            written = 4.0 * n * n
            read = 4.0 * res.r32.numel()
            report["export"] = {"snps": n, "ms": ms, "written_GB": written / 1e9, "read_GB": read / 1e9,
                                "GB_per_s": (written + read) / ms / 1e6, "fraction_of_6300": (written + read) / ms / 1e6 / 6300}
        del p
        torch.cuda.empty_cache()
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

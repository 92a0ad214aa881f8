"""Time of ld_cross (the band with one-sided sums), its scan and the optimal-cut kernel against ld_score on the same panel
and window.

    python tools/ld_regions_timing.py [--snps 100000] [--haps 5008] [--window 250000] [--min-snps 500] [--max-snps 5000]
                                      [--regions 5] [--reps 5] [--once]

The panel is synthetic 100 000 x 5008 with positions 1 + 500 i and w = 250 kb (500 neighbours each side).  Four calls are
timed INTERLEAVED (score K = 0, the cross band with its scan, the scan alone over the band's `sides`, the split over its
profile, score, ...) so that clock drift hits all of them alike: each region is `reps` calls between two device events, and
the median region over `regions` is reported per call.  All calls reuse one workspace and device positions; nothing is read
back inside a region.  The band alone is cross - scan.  `--once` makes one ld_regions call and exits (for a profiler run).
One JSON object is printed (and written to --out).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from ld_tools_amd import PackedPanel, _lib, ops, synth  # noqa: E402


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
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--haps", type=int, default=5008)
    ap.add_argument("--window", type=int, default=250_000)
    ap.add_argument("--min-snps", type=int, default=500)
    ap.add_argument("--max-snps", type=int, default=5000)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one ld_regions call, then exit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, h, w, mn, mx = a.snps, a.haps, a.window, a.min_snps, a.max_snps
    p = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev), dev)
    pos = torch.as_tensor(synth.synth_positions(n, step=500)).to(dev)
    if a.once:
        res = ops.ld_regions(p, pos, window_bp=w, min_snps=mn, max_snps=mx)
        print(json.dumps({"once": True, "snps": n, "n_regions": res.n_regions, "total_cross": res.total_cross}))
        return
    ws = torch.empty(max(_lib.lib.ldx_ld_score_workspace_bytes(n, h), _lib.lib.ldx_ld_cross_workspace_bytes(n, h)),
                     dtype=torch.uint8, device=dev)
    sides = torch.empty((n, 2), dtype=torch.uint64, device=dev)
    cross = torch.empty(n + 1, dtype=torch.uint64, device=dev)
    cuts = torch.empty(max(1, n // mn), dtype=torch.int32, device=dev)
    n_out = torch.empty(2, dtype=torch.int32, device=dev)
    sws = torch.empty(_lib.lib.ldx_ld_split_workspace_bytes(n), dtype=torch.uint8, device=dev)
    fp4 = ops.PATHS["fp4"]
    calls = {
        "score_k0": lambda: ops.ld_score(p, pos, window_bp=w, workspace=ws, check_positions=False),
        "cross": lambda: ops._cross_launch(p, pos, w, fp4, sides, cross, ws),
        "scan": lambda: _lib.check(_lib.lib.ldx_ld_cross_scan_dev(sides.data_ptr(), n, cross.data_ptr(), ops._stream_ptr())),
        "split": lambda: ops._split_launch(cross, n, mn, mx, cuts, n_out, sws),
    }
    for f in calls.values():   # warm-up (the scan's and the split's inputs are the band's outputs from here on)
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.regions):
        for k, f in calls.items():
            times[k].append(region_ms(f, a.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = n_out.cpu().numpy().view("uint32").tolist()
    report = {
        "snps": n, "haps": h, "window": w, "min_snps": mn, "max_snps": mx, "lib": str(_lib.LIB_PATH),
        "n_cuts": out[0], "flag": out[1],
        "timing": f"median of {a.regions} interleaved regions of {a.reps} calls (HIP events), ms per call",
        "median_ms": med, "regions_ms": times,
        "cross_band_ms": med["cross"] - med["scan"],
        "cross_over_score": med["cross"] / med["score_k0"],
        "scan_over_cross": med["scan"] / med["cross"],
        "split_over_cross": med["split"] / med["cross"],
    }
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

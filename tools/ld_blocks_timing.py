"""Time of ld_fgt (the four-gamete band) and of the block scan against ld_score and ld_decay on the same panel and window.

    python tools/ld_blocks_timing.py [--snps 100000] [--haps 5008] [--window 250000] [--regions 5] [--reps 5] [--once]

The panel is synthetic 100 000 x 5008 with positions 1 + 500 i and w = 250 kb (500 neighbours each side).  Four calls are
timed INTERLEAVED (score K = 0, decay with 1 kb bins, the four-gamete band at min_count 1, the block scan over its `left`,
score, ...) so that clock drift hits all of them alike: each region is `reps` calls between two device events, and the median
region over `regions` is reported per call.  All calls reuse one workspace and device positions; nothing is read back
inside a region.  A synthetic panel has next to no block structure (nearly every distant pair is recombinant), which is the
band's dense regime -- every row hits in every pass -- and the scan's worst case: one block per one or two SNPs.
`--once` makes one ld_blocks call and exits (for a profiler run).  One JSON object is printed (and written to --out).
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
    ap.add_argument("--min-count", type=int, default=1)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one ld_blocks call, then exit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, h, w, m = a.snps, a.haps, a.window, a.min_count
    p = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev), dev)
    pos = torch.as_tensor(synth.synth_positions(n, step=500)).to(dev)
    ws = torch.empty(max(_lib.lib.ldx_ld_score_workspace_bytes(n, h), _lib.lib.ldx_ld_decay_workspace_bytes(n, h),
                         _lib.lib.ldx_ld_fgt_workspace_bytes(n, h)), dtype=torch.uint8, device=dev)
    if a.once:
        res = ops.ld_blocks(p, pos, window_bp=w, min_count=m, workspace=ws, check_positions=False)
        torch.cuda.synchronize()
        print(json.dumps({"once": True, "snps": n, "n_blocks": res.n_blocks}))
        return
    left = torch.empty(n, dtype=torch.int32, device=dev)
    block_of = torch.empty(n, dtype=torch.int32, device=dev)
    n_out = torch.empty(2, dtype=torch.int32, device=dev)
    fp4 = ops.PATHS["fp4"]
    calls = {
        "score_k0": lambda: ops.ld_score(p, pos, window_bp=w, workspace=ws, check_positions=False),
        "decay_1kb": lambda: ops.ld_decay(p, pos, window_bp=w, bin_bp=1000, workspace=ws, check_positions=False),
        "fgt": lambda: ops._fgt_launch(p, pos, w, m, None, fp4, left, ws),
        "block_scan": lambda: ops._blocks_launch(left, pos, None, n, w, block_of, n_out),
    }
    for f in calls.values():   # warm-up (the scan's `left` is the band's output from here on)
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.regions):
        for k, f in calls.items():
            times[k].append(region_ms(f, a.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = n_out.cpu().tolist()
    report = {
        "snps": n, "haps": h, "window": w, "min_count": m, "lib": str(_lib.LIB_PATH),
        "n_blocks": out[0], "rm": out[1], "snps_with_a_partner": int((left != 0).sum().item()),
        "timing": f"median of {a.regions} interleaved regions of {a.reps} calls (HIP events), ms per call",
        "median_ms": med, "regions_ms": times,
        "fgt_over_decay": med["fgt"] / med["decay_1kb"],
        "fgt_over_score": med["fgt"] / med["score_k0"],
        "block_scan_over_fgt": med["block_scan"] / med["fgt"],
    }
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

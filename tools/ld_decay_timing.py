"""Time of ld_decay (LD decay curves on the matrix-pipe band) against ld_score on the same panel and window.

    python tools/ld_decay_timing.py [--snps 100000] [--haps 5008] [--window 250000] [--regions 5] [--reps 5] [--once BINS]

The panel is synthetic 100 000 x 5008 with positions 1 + 500 i and w = 250 kb (500 neighbours each side).  Three calls are
timed INTERLEAVED (score K = 0, decay with 1 kb bins = 251 bins, decay with 1 000 bins, score K = 0, ...) so that clock drift
hits all of them alike: each region is `reps` calls between two device events, and the median region over `regions` is
reported per call.  All calls reuse one workspace and device positions; nothing is read back inside a region.  The same
script run with LDX_LIB pointing at a build with -DLDX_AB_DECAY_UNIFORM gives the wave-uniform side of the A/B.
`--once BINS` makes one decay call with that many bins and exits (for a profiler run).  One JSON object is printed (and
written to --out).
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


def width_for(window, bins):
    """The smallest bin width that gives at most `bins` bins."""
    return window // bins + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--haps", type=int, default=5008)
    ap.add_argument("--window", type=int, default=250_000)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", type=int, default=None, help="one ld_decay call with this many bins, then exit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, h, w = a.snps, a.haps, a.window
    p = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev), dev)
    pos = torch.as_tensor(synth.synth_positions(n, step=500)).to(dev)
    ws = torch.empty(max(_lib.lib.ldx_ld_score_workspace_bytes(n, h), _lib.lib.ldx_ld_decay_workspace_bytes(n, h)),
                     dtype=torch.uint8, device=dev)

    def decay(width):
        return ops.ld_decay(p, pos, window_bp=w, bin_bp=width, workspace=ws, check_positions=False)

    if a.once is not None:
        decay(width_for(w, a.once))
        torch.cuda.synchronize()
        print(json.dumps({"once": a.once, "snps": n}))
        return
    w1000 = width_for(w, 1000)
    calls = {
        "score_k0": lambda: ops.ld_score(p, pos, window_bp=w, workspace=ws, check_positions=False),
        "decay_1kb": lambda: decay(1000),
        "decay_1000bins": lambda: decay(w1000),
    }
    for f in calls.values():   # warm-up
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.regions):
        for k, f in calls.items():
            times[k].append(region_ms(f, a.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = decay(1000)
    report = {
        "snps": n, "haps": h, "window": w, "lib": str(_lib.LIB_PATH), "bins": {"decay_1kb": ops.decay_bins(w, 1000),
                                                                               "decay_1000bins": ops.decay_bins(w, w1000)},
        "pairs_in_window": int(res.counts.sum()),
        "timing": f"median of {a.regions} interleaved regions of {a.reps} calls (HIP events), ms per call",
        "median_ms": med, "regions_ms": times,
        "decay_1kb_over_score": med["decay_1kb"] / med["score_k0"],
        "decay_1000bins_over_score": med["decay_1000bins"] / med["score_k0"],
    }
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

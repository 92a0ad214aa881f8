"""Time of ld_score (LD scores on the matrix-pipe band) against the ld_area scan on the same panel and window.

    python tools/ld_score_timing.py [--snps 100000] [--haps 5008] [--window 500000] [--regions 7] [--reps 10] [--once K]

The panel is BASELINE.json configs[2]'s: synthetic 100 000 x 5008, positions 1 + 500 i, w = 500 kb (1 000 neighbours each
side).  Three calls are timed INTERLEAVED (score K = 0, score K = 8, ld_area(thres=0.8), score K = 0, ...) so that clock drift
hits all of them alike: each region is `reps` calls between two device events, and the median region over `regions` is
reported per call.  The score calls reuse one workspace and device positions; nothing is read back.  The FP4 roofline
fraction counts 2 n_hap operations per pair of the window, as bench.py does for the triangle.  `--once K` makes one score
call with K categories and exits (for a profiler run).  One JSON object is printed (and written to --out).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ld_tools_amd import PackedPanel, _lib, ops, synth  # noqa: E402

MFMA_FP4_PEAK_TOPS = 10000.0   # bench.py


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
    ap.add_argument("--window", type=int, default=500_000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--once", type=int, default=None, help="one ld_score call with this many categories, then exit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, h, w = a.snps, a.haps, a.window
    p = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev), dev)
    pos_h = synth.synth_positions(n, step=500)
    pos = torch.as_tensor(pos_h).to(dev)
    ann = np.random.default_rng(7).random((n, 8)) < 0.3
    ws = torch.empty(_lib.lib.ldx_ld_score_workspace_bytes(n, h), dtype=torch.uint8, device=dev)

    def score(k):
        return ops.ld_score(p, pos, window_bp=w, annot=ann[:, :k] if k else None, workspace=ws, check_positions=False)

    if a.once is not None:
        score(a.once)
        torch.cuda.synchronize()
        print(json.dumps({"once": a.once, "snps": n}))
        return
    calls = {
        "score_k0": lambda: score(0),
        "score_k8": lambda: score(8),
        "area_thres0.8": lambda: ops.ld_area(p, pos, None, w, "r_square", 0.8, check_positions=False),
    }
    for f in calls.values():   # warm-up (the ld_area plan's graph is captured on its second call)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.regions):
        for k, f in calls.items():
            times[k].append(region_ms(f, a.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    lo, _ = ops.window_bounds(pos_h, w)
    pairs = int((np.arange(n) - lo).sum())          # unordered pairs i > j of the window
    ops_k0 = 2.0 * h * pairs
    report = {
        "snps": n, "haps": h, "window": w, "pairs_in_window": pairs, "timing": f"median of {a.regions} interleaved regions "
        f"of {a.reps} calls (HIP events), ms per call", "median_ms": med, "regions_ms": times,
        "k8_over_k0": med["score_k8"] / med["score_k0"], "k0_over_area": med["score_k0"] / med["area_thres0.8"],
        "roofline": {"bound": "mfma", "achieved": ops_k0 / (med["score_k0"] * 1e-3) / 1e12, "peak": MFMA_FP4_PEAK_TOPS,
                     "unit": "TOP/s", "frac": ops_k0 / (med["score_k0"] * 1e-3) / 1e12 / MFMA_FP4_PEAK_TOPS,
                     "of": "score_k0, whole call"},
    }
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

"""Time of the rectangle (ops.ld_rect, ldx_ld_rect_dev) against the only way to get the same cells without it: the r32 triangle
of the two panels stacked into one, then the off-diagonal block of its square (TriangleResult.r_matrix).

    python tools/ld_rect_timing.py [--haps 5008] [--reps 20] [--warmup 2] [--shapes 10000x10000,512x100000] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  One process, one device.  Per shape: a synthetic stacked panel of
n_i + n_j SNPs, its two halves as sub-panels (PackedPanel.select), a check that the two legs' cells are bit-identical on a
sample of 10^5 cells, a warm-up of each leg, then `reps` (at least 20) timed calls per leg, ALTERNATED call by call so that clock
drift hits both alike; every call sits between two device events of its own.

    rect       ld_rect(I, J) into a preallocated [n_i, n_j] tensor
    stacked    ld_triangle(stacked, fmt="r32") into a preallocated result + r_matrix(rows = I, cols = J)

The rectangle passes when its median is below the stacked leg's by more than the stacked leg's spread (max - min over its
repeats).  The roofline figures: 2 n_i n_j K operations (K = n_hap padded to K-blocks of 256) over the FP4 peak, the bytes of
the output and of both bit planes over HBM.  One JSON object is printed (and written to --out).
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

from ld_tools_amd import PackedPanel, ops, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, read or write
MFMA_FP4_PEAK_TOPS = 10000.0   # bench.py
SAMPLE_CELLS = 100_000


def call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "calls": len(ms)}


def one_shape(n_i, n_j, h, reps, warmup, dev):
    n = n_i + n_j
    stacked = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev), dev)
    pi = stacked.select(snps=np.arange(0, n_i, dtype=np.uint32))
    pj = stacked.select(snps=np.arange(n_i, n, dtype=np.uint32))
    out = torch.empty((n_i, n_j), dtype=torch.float32, device=dev)
    tri = ops.ld_triangle(stacked, fmt="r32")   # allocates the strips once; the timed calls reuse them

    def rect():
        return ops.ld_rect(pi, pj, out=out)

    def stacked_block():
        ops.ld_triangle(stacked, fmt="r32", out=tri)
        return tri.r_matrix(rows=(0, n_i), cols=(n_i, n))

    # the two legs give the same cells: a sample of 10^5, bit for bit
    rng = np.random.default_rng(7)
    si = torch.as_tensor(rng.integers(0, n_i, SAMPLE_CELLS)).to(dev)
    sj = torch.as_tensor(rng.integers(0, n_j, SAMPLE_CELLS)).to(dev)
    a = rect()[si, sj].view(torch.int32)
    b = stacked_block()[si, sj].view(torch.int32)
    differ = int((a != b).sum())
    if differ:
        raise SystemExit(f"{n_i} x {n_j}: {differ} of {SAMPLE_CELLS} sampled cells differ between the two legs")
    del a, b
    for _ in range(warmup):
        rect()
        stacked_block()
    torch.cuda.synchronize()
    t_rect, t_stack = [], []
    for _ in range(reps):   # alternated
        t_rect.append(call_ms(rect))
        t_stack.append(call_ms(stacked_block))
    sr, ss = stats(t_rect), stats(t_stack)
    k_pad = (h + 255) // 256 * 256
    pairs = n_i * n_j
    ops_rect = 2.0 * pairs * k_pad
    tri_pairs = n * (n - 1) // 2
    plane = lambda m: ((m + 127) // 128 * 128) * (k_pad // 8)   # noqa: E731  bytes of one tiled bit plane
    bytes_rect = 4.0 * pairs + plane(n_i) + plane(n_j)
    sec = sr["median_ms"] * 1e-3
    return {
        "n_i": n_i, "n_j": n_j, "n_hap": h, "k_padded": k_pad, "sampled_cells_bit_identical": SAMPLE_CELLS,
        "rect": sr, "stacked": ss,
        "speedup": ss["median_ms"] / sr["median_ms"],
        "faster_by_more_than_the_spread_of_stacked": ss["median_ms"] - sr["median_ms"] > ss["spread_ms"],
        "rect_pairs_per_s": pairs / sec,
        "rect_tops": ops_rect / sec / 1e12, "rect_frac_of_fp4_peak": ops_rect / sec / 1e12 / MFMA_FP4_PEAK_TOPS,
        "rect_min_bytes": bytes_rect, "rect_gbs": bytes_rect / sec / 1e9, "rect_frac_of_hbm": bytes_rect / sec / 1e9 / HBM_PEAK_GBS,
        "mfma_floor_ms": ops_rect / (MFMA_FP4_PEAK_TOPS * 1e12) * 1e3, "hbm_floor_ms": bytes_rect / (HBM_PEAK_GBS * 1e9) * 1e3,
        "stacked_pairs": tri_pairs, "stacked_pairs_per_s": tri_pairs / (ss["median_ms"] * 1e-3),
        "stacked_tops": 2.0 * tri_pairs * k_pad / (ss["median_ms"] * 1e-3) / 1e12,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--haps", type=int, default=5008)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="10000x10000,512x100000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("ld_rect_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    report = {"timing": "one HIP event pair per call, legs alternated call by call, ms", "shapes": []}
    for spec in a.shapes.split(","):
        n_i, n_j = (int(x) for x in spec.lower().split("x"))
        report["shapes"].append(one_shape(n_i, n_j, a.haps, a.reps, max(1, a.warmup), dev))
        torch.cuda.empty_cache()
    report["accepted"] = all(s["faster_by_more_than_the_spread_of_stacked"] for s in report["shapes"])
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    if not report["accepted"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

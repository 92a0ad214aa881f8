"""Time of ld_score(dosage=True) (genotype-dosage r on the FP4 band) against the haplotype ld_score of the same build, on
the same panel and window.

    python tools/ld_dosage_timing.py [--snps 100000] [--haps 5008] [--window 500000] [--regions 7] [--reps 10] [--once]

The panel is tools/ld_score_timing.py's (BASELINE.json configs[2]): synthetic 100 000 x 5008, positions 1 + 500 i, w = 500 kb
(1 000 neighbours each side).  The calls are timed INTERLEAVED (haplotype K = 0, dosage K = 0, haplotype K = 8, dosage K = 8,
haplotype K = 0, ...) so that clock drift hits all of them alike: each region is `reps` calls between two device events, and
the median region over `regions` is reported per call, after three warm-up calls each.  The calls reuse one workspace and
device positions, the dosage table is built before the first region (it is cached on the panel), and nothing is read back.
The two kernels differ in the B-side expansion of the K loop only (expand32_b4 / expand32_b4_dosage, ldx_mfma.hip), so the
ratio is the price of those instructions.  `--once` makes one dosage call and exits (for a profiler run).  One JSON object is
printed (and written to --out).
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
    ap.add_argument("--once", action="store_true", help="one ld_score(dosage=True) call, then exit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, h, w = a.snps, a.haps, a.window
    p = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev), dev)
    pos = torch.as_tensor(synth.synth_positions(n, step=500)).to(dev)
    ann = np.random.default_rng(7).random((n, 8)) < 0.3
    ws = torch.empty(_lib.lib.ldx_ld_score_workspace_bytes(n, h), dtype=torch.uint8, device=dev)
    p.dosage_stats()

    def score(k, dosage):
        return ops.ld_score(p, pos, window_bp=w, annot=ann[:, :k] if k else None, workspace=ws, check_positions=False,
                            dosage=dosage)

    if a.once:
        score(0, True)
        torch.cuda.synchronize()
        print(json.dumps({"once": "dosage_k0", "snps": n}))
        return
    calls = {
        "haplotype_k0": lambda: score(0, False),
        "dosage_k0": lambda: score(0, True),
        "haplotype_k8": lambda: score(8, False),
        "dosage_k8": lambda: score(8, True),
    }
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.regions):
        for k, f in calls.items():
            times[k].append(region_ms(f, a.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    report = {
        "snps": n, "haps": h, "window": w, "timing": f"median of {a.regions} interleaved regions of {a.reps} calls (HIP events), "
        "ms per call", "median_ms": med, "regions_ms": times,
        "dosage_over_haplotype_k0": med["dosage_k0"] / med["haplotype_k0"],
        "dosage_over_haplotype_k8": med["dosage_k8"] / med["haplotype_k8"],
    }
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

"""Time of ld_matvec (banded R x on the matrix-pipe band) next to ld_score on the same panel and window, and one ld_ridge solve.

    python tools/ld_matvec_timing.py [--snps 100000] [--haps 5008] [--window 250000] [--regions 7] [--reps 10] [--out FILE]

The panel is synthetic 100 000 x 5008, positions 1 + 500 i, w = 250 kb (500 neighbours each side).  The calls are timed
INTERLEAVED (score, matvec 1 / 4 / 8 right-hand sides at power 1, 1 at power 2, score, ...) so that clock drift hits all of
them alike: each region is `reps` calls between two device events, and the median region over `regions` is reported per
call.  The calls reuse one workspace, device positions and device right-hand sides with the host-side checks off; nothing is
read back.  The matvec figure includes the column scaling of the Python layer (a few small torch kernels).  Then one
ld_ridge solve of four columns (lam = 1, tol = 1e-6) is timed whole: iterations and ms per iteration.  One JSON object is
printed (and written to --out).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
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
    ap.add_argument("--window", type=int, default=250_000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, h, w = a.snps, a.haps, a.window
    p = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev), dev)
    pos = torch.as_tensor(synth.synth_positions(n, step=500)).to(dev)
    x = torch.as_tensor(np.random.default_rng(7).standard_normal((n, 8)).astype(np.float32)).to(dev)
    ws = torch.empty(max(_lib.lib.ldx_ld_score_workspace_bytes(n, h), _lib.lib.ldx_ld_matvec_workspace_bytes(n, h)),
                     dtype=torch.uint8, device=dev)

    def matvec(k, power):
        return ops.ld_matvec(p, x[:, :k].contiguous(), pos, window_bp=w, power=power, workspace=ws, check_positions=False,
                             check_finite=False)

    calls = {
        "score_k0": lambda: ops.ld_score(p, pos, window_bp=w, workspace=ws, check_positions=False),
        "matvec_1": lambda: matvec(1, 1),
        "matvec_4": lambda: matvec(4, 1),
        "matvec_8": lambda: matvec(8, 1),
        "matvec_1_power2": lambda: matvec(1, 2),
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
    z = x[:, :4].to(torch.float64)
    ops.ld_ridge(p, z, pos, window_bp=w, lam=1.0, max_iter=8, check_positions=False)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ops.ld_ridge(p, z, pos, window_bp=w, lam=1.0, tol=1e-6, check_positions=False)
    torch.cuda.synchronize()
    ridge_ms = (time.perf_counter() - t0) * 1e3
    its = int(res.iterations.max())
    report = {
        "snps": n, "haps": h, "window": w, "timing": f"median of {a.regions} interleaved regions of {a.reps} calls (HIP events), "
        "ms per call", "median_ms": med, "regions_ms": times,
        "matvec_1_over_score": med["matvec_1"] / med["score_k0"], "matvec_8_over_matvec_1": med["matvec_8"] / med["matvec_1"],
        "ridge": {"columns": 4, "lam": 1.0, "tol": 1e-6, "iterations": res.iterations.tolist(),
                  "converged": res.converged.tolist(), "indefinite": res.indefinite.tolist(), "wall_ms": ridge_ms,
                  "ms_per_iteration": ridge_ms / max(its, 1)},
    }
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

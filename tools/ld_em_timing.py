"""Time of dense unphased LD by EM (ops.ld_em, ldx_ld_em_rect_dev) against the dosage rectangle (ops.ld_rect(dosage=True)) on
the same two panels, with the EM kernel's K loop alone (ops.ld_em_counts) beside it, and the share of pairs that take each
path of the EM epilogue.

    python tools/ld_em_timing.py [--haps 5008] [--reps 20] [--warmup 2] [--shapes 10000x10000,2048x20000] [--out FILE]

Runs on a GPU only.  One process, one device.  Per shape: a synthetic blocky panel of n_i + n_j SNPs (synth's LD blocks), its
two halves as sub-panels, a warm-up of each leg, then `reps` (at least 20) timed calls per leg, ALTERNATED call by call so
that clock drift hits all alike; every call sits between two device events of its own.

    em         ld_em(I, J) into two preallocated [n_i, n_j] tensors (r and D')
    em_r       ld_em(I, J, want_dprime=False): one output
    counts     ld_em_counts(I, J): the K loop and two uint32 stores per cell, no epilogue
    dosage     ld_rect(I, J, dosage=True) into a preallocated [n_i, n_j] tensor

Epilogue paths, classified on the host from the kernel's own counts on a sample of rows (the decision sequence of em_cell,
ldx_em_tile.h, in numpy): degenerate; H = 0 (closed form); g monotone on [0, H]; one rising branch with a sign change (one
root, no logarithm); two candidates (two roots and the likelihood comparison).  No time or ratio is promised: the JSON
object that is printed (and written to --out) is the record.
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

PATH_ROWS = 512   # rows of side I whose cells are classified


def call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "calls": len(ms)}


def path_shares(n_ind, a_i, a_j, S, H):
    """Shares of the cells [n_i, n_j] per epilogue path: em_cell's decisions in float64 numpy."""
    T = 2.0 * n_ind
    ai, aj = a_i[:, None].astype(np.float64), a_j[None, :].astype(np.float64)
    S, H = S.astype(np.float64), H.astype(np.float64)
    n1 = (S - H) / 2.0
    n2, n3, n4 = ai - n1 - H, aj - n1 - H, T - ai - aj + n1
    deg = (ai == 0) | (ai == T) | (aj == 0) | (aj == T)
    phased = ~deg & (H == 0)
    c2 = n1 + n4 - n2 - n3 - 3.0 * H
    c1 = (n2 + H) * (n3 + H) - H * (n1 + n4) + n1 * n4
    disc = c2 * c2 - 6.0 * c1
    mono = ~deg & ~phased & (disc <= 0)
    rest = ~deg & ~phased & ~mono
    sq = np.sqrt(np.where(rest, disc, 0.0))
    xa, xb = (-c2 - sq) / 6.0, (-c2 + sq) / 6.0

    def g(x):
        return x * ((n2 + H - x) * (n3 + H - x)) - (H - x) * ((n1 + x) * (n4 + x))

    have1 = rest & (xa > 0) & (g(np.minimum(xa, H)) >= 0)
    have2 = rest & (xb < H) & (g(np.maximum(xb, 0.0)) <= 0)
    two = have1 & have2
    total = float(deg.size)
    return {"degenerate": float(deg.sum()) / total, "h_zero": float(phased.sum()) / total, "monotone": float(mono.sum()) / total,
            "one_branch": float((rest & ~two).sum()) / total, "two_candidates": float(two.sum()) / total, "cells": int(total)}


def one_shape(n_i, n_j, h, reps, warmup, dev):
    n = n_i + n_j
    stacked = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev), dev)
    pi = stacked.select(snps=np.arange(0, n_i, dtype=np.uint32))
    pj = stacked.select(snps=np.arange(n_i, n, dtype=np.uint32))
    out_r = torch.empty((n_i, n_j), dtype=torch.float32, device=dev)
    out_d = torch.empty((n_i, n_j), dtype=torch.float32, device=dev)
    out_g = torch.empty((n_i, n_j), dtype=torch.float32, device=dev)
    pi.dosage_stats(), pj.dosage_stats()   # the dosage leg's per-SNP table, built once outside the timed calls
    legs = {
        "em": lambda: ops.ld_em(pi, pj, out_r=out_r, out_dprime=out_d),
        "em_r": lambda: ops.ld_em(pi, pj, out_r=out_r, want_dprime=False),
        "counts": lambda: ops.ld_em_counts(pi, pj),
        "dosage": lambda: ops.ld_rect(pi, pj, dosage=True, out=out_g),
    }
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):   # alternated
        for k, fn in legs.items():
            times[k].append(call_ms(fn))
    rows = min(PATH_ROWS, n_i)
    head = pi.select(snps=np.arange(0, rows, dtype=np.uint32))
    S, H = (t.cpu().numpy() for t in ops.ld_em_counts(head, pj))
    shares = path_shares(h // 2, head.acnt.cpu().numpy()[:rows], pj.acnt.cpu().numpy()[:n_j], S, H)
    res = {k: stats(v) for k, v in times.items()}
    return {"n_i": n_i, "n_j": n_j, "n_hap": h, **res,
            "em_over_dosage": res["em"]["median_ms"] / res["dosage"]["median_ms"],
            "em_r_over_dosage": res["em_r"]["median_ms"] / res["dosage"]["median_ms"],
            "counts_over_dosage": res["counts"]["median_ms"] / res["dosage"]["median_ms"],
            "em_pairs_per_s": n_i * n_j / (res["em"]["median_ms"] * 1e-3), "epilogue_paths": shares}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--haps", type=int, default=5008)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="10000x10000,2048x20000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    if a.haps % 2:
        raise SystemExit("--haps must be even")
    if not torch.cuda.is_available():
        raise SystemExit("ld_em_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    report = {"timing": "one HIP event pair per call, legs alternated call by call, ms", "shapes": []}
    for spec in a.shapes.split(","):
        n_i, n_j = (int(x) for x in spec.lower().split("x"))
        report["shapes"].append(one_shape(n_i, n_j, a.haps, a.reps, max(1, a.warmup), dev))
        torch.cuda.empty_cache()
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

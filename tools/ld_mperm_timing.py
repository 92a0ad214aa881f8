"""Time of the max(T) permutation test (ops.perm_labels, ops.ld_mperm) on one card:

    python tools/ld_mperm_timing.py [--snps 100000] [--inds 2504] [--perms 10000] [--miss 0,0.03] [--reps 3] [--warmup 1] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  The panel is synthetic (synth.synth_codes_device, seeded): --snps SNPs
over --inds individuals, half of them cases, once per missing-call rate of --miss.  Per rate, every launch between two device
events, the sub-panel, its count table and the observed statistic made before:
  labels    ldx_perm_labels_dev: the label plane of --perms permutations
  allelic   ldx_perm_scan_dev, n_ge and maxima zeroed before each call
  loops     the allelic launch with every SNP's stat NaN: the K loops and the staging alone, no cell's epilogue
  trend     the same with the Cochran-Armitage statistic
  torch     the same scan in torch on the same card: the label matrix (fp16) against the dosage and the called matrix in
            chunks of 1000 permutations (fp16 GEMMs over at most 1000 individuals each, so that every partial sum is an
            exact fp16, added in fp32), the allelic statistic elementwise in fp64, amax and a compare-and-sum; its n_ge and
            maxima are compared with the scan's
No threshold is applied: one JSON object per measurement is printed (and all written to --out)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ld_tools_amd import PackedPanel, perm_labels, synth  # noqa: E402
from ld_tools_amd._lib import check, lib  # noqa: E402
from ld_tools_amd.ops import _MpermRun, _stream_ptr  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(name, fn, a, **extra):
    for _ in range(a.warmup):
        fn()
    ms = [event_ms(fn) for _ in range(a.reps)]
    rec = {"what": name, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms), **extra}
    print(json.dumps(rec), flush=True)
    return rec


def torch_scan(g16, c16, labels16, N, G, stat, chunk=1000, k_part=1000, rows=25000):
    """(n_ge int64 [n], maxima float64 [R]) of the allelic scan from torch GEMMs; ``g16`` / ``c16`` fp16 [n, inds], ``labels16``
    fp16 [inds, R], N and G float64 [n, 1], stat float64 [n] (NaN: the SNP takes no part)."""
    n, P = g16.shape[0], labels16.shape[1]
    n_ge = torch.zeros(n, dtype=torch.int64, device=g16.device)
    maxima = torch.zeros(P, dtype=torch.float64, device=g16.device)
    bound = torch.where(torch.isnan(stat), torch.full_like(stat, float("inf")), stat)[:, None]
    live = ~torch.isnan(stat)[:, None]
    for p0 in range(0, P, chunk):
        L = labels16[:, p0:p0 + chunk]
        for r0 in range(0, n, rows):
            sl = slice(r0, r0 + rows)
            a = sum(torch.mm(g16[sl, k:k + k_part], L[k:k + k_part]).float() for k in range(0, L.shape[0], k_part)).double()
            R = sum(torch.mm(c16[sl, k:k + k_part], L[k:k + k_part]).float() for k in range(0, L.shape[0], k_part)).double()
            Nn, Gg = N[sl], G[sl]
            b, c = 2.0 * R - a, Gg - a
            d = 2.0 * (Nn - R) - c
            det = a * d - b * c
            den = (a + b) * (c + d) * ((a + c) * (b + d))
            valid = (den != 0.0) & live[sl]
            x = torch.where(valid, ((2.0 * Nn) * (det * det)) / torch.where(valid, den, torch.ones_like(den)), torch.zeros_like(den))
            maxima[p0:p0 + chunk] = torch.maximum(maxima[p0:p0 + chunk], x.amax(dim=0))
            n_ge[sl] += (valid & (x >= bound[sl])).sum(dim=1)
    return n_ge, maxima


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=100000)
    ap.add_argument("--inds", type=int, default=2504)
    ap.add_argument("--perms", type=int, default=10000)
    ap.add_argument("--miss", default="0,0.03")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ld_mperm_timing: no HIP device")
    dev = torch.device("cuda", 0)
    n, n_ind, P = a.snps, a.inds, a.perms
    case = np.zeros(n_ind)
    case[: n_ind // 2] = 1.0
    report = {"timing": "one HIP event pair around each launch, ms, medians of --reps calls after --warmup calls", "snps": n,
              "inds": n_ind, "perms": P, "cells": n * P, "products": 2 * n * P * n_ind, "lib": str(lib._name), "results": []}
    for miss in (float(x) for x in a.miss.split(",")):
        rec = lambda r: report["results"].append({"miss": miss, **r})  # noqa: E731
        codes = synth.synth_codes_device(n, 2 * n_ind, seed=synth.BENCH_SEED, miss=miss, device=dev)[:, :2 * n_ind].contiguous()
        panel = PackedPanel.from_codes(codes, dev)
        plane = torch.empty(lib.ldx_plane_bytes(P, 2 * n_ind), dtype=torch.uint8, device=dev)
        rec(timed("labels", lambda: check(lib.ldx_perm_labels_dev(7, 0, P, 2 * n_ind, n_ind // 2, plane.data_ptr(), _stream_ptr())), a))
        run = _MpermRun("ld_mperm_timing", panel, case, P, 7, 0, None, None, None)
        n_ge = torch.zeros(n, dtype=torch.int32, device=dev)
        maxima = torch.zeros(P, dtype=torch.float64, device=dev)
        kept = {}
        for code, name in ((0, "allelic"), (1, "trend")):
            stat, flags = run.observed(code)

            def scan():
                n_ge.zero_()
                maxima.zero_()
                check(lib.ldx_perm_scan_dev(*run.head(), code, stat.data_ptr(), n_ge.data_ptr(), maxima.data_ptr(), _stream_ptr()))

            rec(timed(name, scan, a, flagged=int((flags != 0).sum())))
            if code == 0:
                kept = {"stat": stat, "n_ge": n_ge.clone(), "maxima": maxima.clone()}
                none = torch.full_like(stat, float("nan"))   # every SNP out: the K loops and the staging, no epilogue
                rec(timed("loops", lambda: check(lib.ldx_perm_scan_dev(*run.head(), 0, none.data_ptr(), n_ge.data_ptr(),
                                                                       maxima.data_ptr(), _stream_ptr())), a))
        ok = (codes[:, 0::2] >= 0) & (codes[:, 0::2] <= 1) & (codes[:, 1::2] >= 0) & (codes[:, 1::2] <= 1)
        g16 = (((codes[:, 0::2] == 1).to(torch.int8) + (codes[:, 1::2] == 1).to(torch.int8)) * ok).to(torch.float16)
        c16 = ok.to(torch.float16)
        del codes, ok
        labels16 = torch.from_numpy(perm_labels(n_ind, n_ind // 2, P, 7, device=dev).to_array().T.copy()).to(dev).to(torch.float16)
        N = c16.sum(dim=1, dtype=torch.float64)[:, None]
        G = g16.sum(dim=1, dtype=torch.float64)[:, None]
        t_ge, t_max = torch_scan(g16, c16, labels16, N, G, kept["stat"])
        same = bool((t_ge == kept["n_ge"].to(torch.int64)).all()) and bool((t_max == kept["maxima"]).all())
        rec(timed("torch", lambda: torch_scan(g16, c16, labels16, N, G, kept["stat"]), a, equals_scan=same))
        del g16, c16, labels16, panel, run, plane
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

"""Time of the logistic association scan (ops.ld_glm_logistic: ldx_geno_snp_counts_dev, ldx_glm_logistic_dev) against the same scan
written as batched fp64 IRLS in torch on the same card, with the same start (the null fit), the same stopping rule (Newton
decrement <= 2^-60, that step applied, the information once more) and the same cap:

    python tools/ld_logistic_timing.py [--inds 2504] [--snps 100000] [--phenos 1,20] [--covars 10] [--reps 5] [--warmup 1]
                                       [--torch-reps 3] [--chunk 2048] [--miss 0.03] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  Per number of phenotypes:
    scan        one launch of ldx_glm_logistic_dev between two device events (a launch is tens of milliseconds and more: one launch
                is a window of its own), --reps times, interleaved with
    counts      ldx_geno_snp_counts_dev, and
    torch_irls  the baseline: per phenotype and per chunk of --chunk SNPs the design [B | x] as one fp64 tensor [chunk, m, N]
                (x = the centred dosage, built beforehand for the whole panel: 8 bytes per genotype), torch.bmm for eta, I and U,
                torch.linalg.cholesky_ex and cholesky_solve per evaluation, every SNP of the chunk iterated until the last one of
                it has converged (a converged SNP keeps its value) -- what a user would write; --torch-reps times.
and on a host clock around work that ends in a synchronise: design (ops.logit_design: numpy on the host) and ld_glm_logistic as
a whole.  Before timing, beta and se of the baseline are compared with ours (|d beta| <= 1e-8 se), and the flags are counted.
Reported with the times: the mean n_iter over the cells that iterate, the v_mfma_f64_16x16x4_f64 instructions issued -- n_iter x
ceil(N / 4) per such cell, counted from the result -- and their rate over the scan's time (2 x 16 x 16 x 4 flop each).  No threshold
is applied: one JSON object per scan is printed (and all written to --out)."""
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

from ld_tools_amd import PackedPanel, ld_glm_logistic, logit_design, ops, synth  # noqa: E402
from ld_tools_amd._lib import LOGIT_MAX_ITER, check, lib  # noqa: E402

CHUNK = 65536
DECREMENT = 2.0 ** -60


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def centred_dosage(codes, n_ind, dev):
    """float64 [n_snps, n_ind]: g - mu over the called, 0 where missing (the scan's genotype column)."""
    n_snps = codes.shape[0]
    x = torch.empty((n_snps, n_ind), dtype=torch.float64, device=dev)
    for s in range(0, n_snps, CHUNK):
        c = codes[s:s + CHUNK, :2 * n_ind]
        h0, h1 = c[:, 0::2], c[:, 1::2]
        called = (((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1))).to(torch.float64)
        g = ((h0 == 1).to(torch.float64) + (h1 == 1).to(torch.float64)) * called
        mu = g.sum(dim=1) / called.sum(dim=1).clamp(min=1.0)
        x[s:s + CHUNK] = (g - mu[:, None]) * called
    return x


def torch_irls(x, basis, y, theta0, chunk):
    """(beta, se, n_iter) float64 / int32 [n_snps, n_pheno] by batched IRLS; NaN where the fit fails."""
    n_snps, n_ind = x.shape
    P, p = basis.shape[0], y.shape[0]
    beta = torch.full((n_snps, p), float("nan"), dtype=torch.float64, device=x.device)
    se, iters = beta.clone(), torch.zeros((n_snps, p), dtype=torch.int32, device=x.device)
    for j in range(p):
        yj = y[j].to(torch.float64)
        for s in range(0, n_snps, chunk):
            xs = x[s:s + chunk]
            S = xs.shape[0]
            V = torch.cat([basis[None].expand(S, P, n_ind), xs[:, None, :]], dim=1)           # [S, m, N]
            th = torch.cat([theta0[j][None].expand(S, P), torch.zeros((S, 1), dtype=torch.float64, device=x.device)], dim=1)
            active = torch.ones(S, dtype=torch.bool, device=x.device)      # still iterating
            last = torch.zeros(S, dtype=torch.bool, device=x.device)       # the next evaluation is the final one
            bad = torch.zeros(S, dtype=torch.bool, device=x.device)
            n_it = torch.zeros(S, dtype=torch.int32, device=x.device)
            out_se = torch.full((S,), float("nan"), dtype=torch.float64, device=x.device)
            for _ in range(LOGIT_MAX_ITER):
                eta = torch.bmm(th[:, None, :], V)[:, 0, :]
                mu = torch.sigmoid(eta)
                w = mu * (1.0 - mu)
                info = torch.bmm(V * w[:, None, :], V.transpose(1, 2))
                grad = torch.bmm(V, (yj[None, :] - mu)[:, :, None])
                L, fail = torch.linalg.cholesky_ex(info)
                n_it += active.to(torch.int32)
                bad |= active & (fail != 0)
                done_now = active & last & (fail == 0)
                out_se = torch.where(done_now, 1.0 / L[:, P, P], out_se)
                active = active & ~last & (fail == 0)
                L = torch.where((fail == 0)[:, None, None], L, torch.eye(P + 1, dtype=torch.float64, device=x.device)[None])
                delta = torch.cholesky_solve(grad, L)[:, :, 0]
                dec = (grad[:, :, 0] * delta).sum(dim=1)
                th = torch.where(active[:, None], th + delta, th)
                last = active & (dec <= DECREMENT)
                if not bool(active.any().item()):
                    break
            ok = ~bad & ~active & torch.isfinite(out_se)
            beta[s:s + S, j] = torch.where(ok, th[:, P], torch.full_like(out_se, float("nan")))
            se[s:s + S, j] = torch.where(ok, out_se, torch.full_like(out_se, float("nan")))
            iters[s:s + S, j] = n_it
    return beta, se, iters


def one_scan(panel, x, n_pheno, n_covar, a, dev):
    n_ind, n_snps = panel.n_ind, panel.n_snps
    rng = np.random.default_rng(n_pheno)
    C = rng.standard_normal((n_ind, n_covar))
    eta = -0.3 + 0.4 * C[:, :1] + 0.2 * rng.standard_normal((n_ind, n_pheno))
    Y = (rng.random((n_ind, n_pheno)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.uint8)
    design_s, des = host_s(lambda: logit_design(Y, C))
    basis, y8, theta0 = (torch.from_numpy(v).to(dev) for v in (des.basis, des.y, des.theta0))
    counts = ops._snp_counts(panel, None)
    outs = [torch.empty((n_snps, n_pheno), dtype=torch.float64, device=dev) for _ in range(5)]
    flags, n_iter = (torch.empty((n_snps, n_pheno), dtype=torch.uint8, device=dev) for _ in range(2))

    def scan():
        check(lib.ldx_glm_logistic_dev(panel.alt.data_ptr(), panel.ref.data_ptr(), n_snps, panel.n_hap, None, counts.data_ptr(),
                                       basis.data_ptr(), n_ind, des.n_cov, y8.data_ptr(), theta0.data_ptr(), n_pheno, 50.0,
                                       *(o.data_ptr() for o in outs), flags.data_ptr(), n_iter.data_ptr(), n_pheno, None),
              "ldx_glm_logistic_dev")

    scan()
    torch.cuda.synchronize()
    live = flags == 0
    t_beta, t_se, t_it = torch_irls(x, basis, y8, theta0, a.chunk)
    both = live & torch.isfinite(t_beta)
    gap = ((outs[0] - t_beta).abs() / t_se)[both].max().item()
    if not gap <= 1e-8:
        raise SystemExit(f"the torch baseline's beta differs from ours by {gap} se")
    regions = {"scan": scan, "counts": lambda: ops._snp_counts(panel, None)}
    for _ in range(a.warmup):
        for fn in regions.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in regions}
    times["torch_irls"] = []
    for rep in range(a.reps):   # interleaved
        for name, fn in regions.items():
            times[name].append(event_ms(fn))
        if rep < a.torch_reps:
            times["torch_irls"].append(event_ms(lambda: torch_irls(x, basis, y8, theta0, a.chunk)))
    out = {name: stats(ms) for name, ms in times.items()}
    whole = [host_s(lambda: ld_glm_logistic(panel, Y, C))[0] for _ in range(3)]
    it = n_iter.to(torch.int64)
    iterating = it > 0
    mfma = int(it.sum().item()) * ((n_ind + 3) // 4)
    scan_ms = out["scan"]["median_ms"]
    return {"n_ind": n_ind, "n_snps": n_snps, "n_pheno": n_pheno, "n_covar": n_covar, "cells": n_snps * n_pheno,
            "flag_counts": torch.bincount(flags.flatten().to(torch.int64), minlength=6).tolist(),
            "baseline_beta_gap_in_se": gap, "baseline_fits": int(torch.isfinite(t_beta).sum().item()),
            "mean_n_iter": it[iterating].double().mean().item(), "max_n_iter": int(it.max().item()),
            "baseline_mean_n_iter": t_it.double().mean().item(),
            "mfma_f64_16x16x4_issued": mfma, "mfma_gflops_over_scan_time": mfma * 2048.0 / (scan_ms * 1e-3) / 1e9,
            "design_host_s": design_s, "ld_glm_logistic_whole_s": min(whole), **out,
            "ratio_torch_over_scan": out["torch_irls"]["median_ms"] / (scan_ms + out["counts"]["median_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inds", type=int, default=2504)
    ap.add_argument("--snps", type=int, default=100000)
    ap.add_argument("--phenos", default="1,20")
    ap.add_argument("--covars", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--miss", type=float, default=0.03)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 3 or not 1 <= a.torch_reps <= a.reps:
        raise SystemExit("--reps must be at least 3 and --torch-reps between 1 and --reps")
    if not torch.cuda.is_available():
        raise SystemExit("ld_logistic_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    codes = synth.synth_codes_device(a.snps, 2 * a.inds, seed=synth.BENCH_SEED, miss=a.miss, device=dev)[:, :2 * a.inds]
    panel = PackedPanel.from_codes(codes, dev)
    x = centred_dosage(codes, a.inds, dev)
    del codes
    report = {"timing": "one HIP event pair around each launch (scan, counts) or each whole baseline scan (torch_irls), ms, interleaved "
                        "rep by rep; design and ld_glm_logistic: host clock, s", "miss": a.miss, "chunk": a.chunk, "scans": []}
    for n_pheno in (int(v) for v in a.phenos.split(",")):
        report["scans"].append(one_scan(panel, x, n_pheno, a.covars, a, dev))
        print(json.dumps(report["scans"][-1]), flush=True)
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

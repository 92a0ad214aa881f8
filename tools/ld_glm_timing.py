"""Time of the linear association scan (ops.ld_glm: ldx_geno_rmatmul_dev, ldx_geno_snp_counts_dev, ldx_glm_linear_dev) against the
same scan up to t written with torch.mm on float32 dosage and called matrices plus elementwise fp64, on one card:

    python tools/ld_glm_timing.py [--inds 2504] [--snps 100000] [--phenos 1,20] [--covars 10] [--reps 10] [--warmup 2]
                                  [--inner 20] [--miss 0.03] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  Per number of phenotypes, each region is --inner back-to-back launches
between two device events of its own (a single launch of 0.03 to 0.3 ms is too short a window; the figure is the window over
--inner), the regions INTERLEAVED rep by rep so that clock drift hits all alike:
    reverse        GenoOperator.rmatmul_q of the quantised design [Q | Y~]
    counts         ldx_geno_snp_counts_dev
    statistics     ldx_glm_linear_dev: beta, se, t, the tail, the flags
    statistics_t0  the same launch with the phenotype columns of z, zc zeroed: every t is 0 and the tail returns at once, so
                   statistics - statistics_t0 is the time of the Student-t tail (torch has none; it is reported apart as tail_ms)
    torch_to_t     G32 @ [U32 | 1] and C32 @ [U32 | 1] (float32, matrices built beforehand; the column of ones gives s and n for
                   free, as GenoOperator.stats does), e2 = (G32 o G32) @ 1 from a squared matrix built beforehand, then mu, gg, h,
                   d, b, beta, s2, se, t elementwise in fp64: three passes over 1 GB matrices and no temporary of that size
and on a host clock around work that ends in a synchronise: design (ops.glm_design and the upload: numpy on the host) and
ld_glm as a whole.  The float32 baseline is NOT exact (its sums round); before timing its t is compared loosely with ours.  No
threshold is applied: one JSON object with the medians and the ratio torch_to_t / (reverse + counts + statistics_t0) is printed
(and written to --out)."""
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

from ld_tools_amd import GenoOperator, PackedPanel, glm_design, ld_glm, ops, synth  # noqa: E402
from ld_tools_amd._lib import check, lib  # noqa: E402

CHUNK = 65536


def region_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def host_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def float_matrices(codes, n_ind, dev):
    """float32 [n_snps, n_ind] x 2: the dosage of the called genotypes and the called flag."""
    n_snps = codes.shape[0]
    g32 = torch.empty((n_snps, n_ind), dtype=torch.float32, device=dev)
    c32 = torch.empty((n_snps, n_ind), dtype=torch.float32, device=dev)
    for s in range(0, n_snps, CHUNK):
        c = codes[s:s + CHUNK, :2 * n_ind]
        h0, h1 = c[:, 0::2], c[:, 1::2]
        called = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1))
        g32[s:s + CHUNK] = ((h0 == 1).to(torch.float32) + (h1 == 1).to(torch.float32)) * called
        c32[s:s + CHUNK] = called.to(torch.float32)
    return g32, c32


def one_scan(panel, g32, c32, sq32, n_pheno, n_covar, reps, warmup, inner, dev):
    n_ind, n_snps = panel.n_ind, panel.n_snps
    rng = np.random.default_rng(n_pheno)
    Y, C = rng.standard_normal((n_ind, n_pheno)), rng.standard_normal((n_ind, n_covar))
    design_s, des = host_s(lambda: glm_design(Y, C))
    n_cov, k = des.n_cov, des.n_cov + n_pheno
    op = GenoOperator(panel)
    q = torch.from_numpy(des.q).to(dev)
    exps, yy = torch.from_numpy(des.exps).to(dev), torch.from_numpy(des.yy).to(dev)
    z, zc = op.rmatmul_q(q)
    counts = ops._snp_counts(panel, None)
    z0, zc0 = z.clone(), zc.clone()
    z0[:, n_cov:], zc0[:, n_cov:] = 0, 0
    outs = [torch.empty((n_snps, n_pheno), dtype=torch.float64, device=dev) for _ in range(5)]
    flags = torch.empty((n_snps, n_pheno), dtype=torch.uint8, device=dev)

    def statistics_of(zz, zzc):
        check(lib.ldx_glm_linear_dev(zz.data_ptr(), zzc.data_ptr(), k, counts.data_ptr(), n_snps, n_ind, n_cov, n_pheno,
                                     exps.data_ptr(), yy.data_ptr(), 50.0, *(o.data_ptr() for o in outs), flags.data_ptr(), n_pheno,
                                     None), "ldx_glm_linear_dev")

    u32 = (q.to(torch.float64) * ops._pow2(exps - 30)[None, :]).to(torch.float32)
    u32 = torch.cat([u32, torch.ones((n_ind, 1), dtype=torch.float32, device=dev)], dim=1).contiguous()
    ones = torch.ones(n_ind, dtype=torch.float32, device=dev)
    yy_d, df = yy[None, :], float(des.df)

    def torch_to_t():
        Z, Zc = torch.mm(g32, u32).to(torch.float64), torch.mm(c32, u32).to(torch.float64)
        n, s, e2 = Zc[:, k], Z[:, k], torch.mv(sq32, ones).to(torch.float64)
        mu = s / n
        gg = (n * e2 - s * s) / n
        h = Z[:, :n_cov] - mu[:, None] * Zc[:, :n_cov]
        d = (gg - (h * h).sum(dim=1))[:, None]
        b = Z[:, n_cov:k] - mu[:, None] * Zc[:, n_cov:k]
        beta = b / d
        se = torch.sqrt((yy_d - b * b / d) / df / d)
        return beta / se

    statistics_of(z, zc)
    torch.cuda.synchronize()
    if bool((flags == 6).any().item()):
        raise SystemExit("a cell hit the tail's iteration cap (flag 6)")
    live = flags == 0
    dev_t, ref_t = outs[2][live], torch_to_t()[live]
    if not torch.allclose(dev_t, ref_t, rtol=1e-2, atol=1e-2):
        raise SystemExit(f"the float32 baseline's t differs from ours by {(dev_t - ref_t).abs().max().item()}")

    regions = {
        "reverse": lambda: op.rmatmul_q(q),
        "counts": lambda: ops._snp_counts(panel, None),
        "statistics": lambda: statistics_of(z, zc),
        "statistics_t0": lambda: statistics_of(z0, zc0),
        "torch_to_t": torch_to_t,
    }
    for _ in range(warmup):
        for fn in regions.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in regions}
    for _ in range(reps):   # interleaved
        for name, fn in regions.items():
            times[name].append(region_ms(fn, inner))
    out = {name: stats(ms) for name, ms in times.items()}
    med = {name: s["median_ms"] for name, s in out.items()}
    whole = [host_s(lambda: ld_glm(panel, Y, C))[0] for _ in range(3)]
    ours_to_t = med["reverse"] + med["counts"] + med["statistics_t0"]
    return {"n_ind": n_ind, "n_snps": n_snps, "n_pheno": n_pheno, "n_covar": n_covar, "k": k, "live_cells": int(live.sum().item()),
            "design_host_s": design_s, "ld_glm_whole_s": min(whole), **out, "tail_ms": med["statistics"] - med["statistics_t0"],
            "ours_to_t_ms": ours_to_t, "ratio_torch_over_ours_to_t": med["torch_to_t"] / ours_to_t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inds", type=int, default=2504)
    ap.add_argument("--snps", type=int, default=100000)
    ap.add_argument("--phenos", default="1,20")
    ap.add_argument("--covars", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--miss", type=float, default=0.03)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("ld_glm_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    codes = synth.synth_codes_device(a.snps, 2 * a.inds, seed=synth.BENCH_SEED, miss=a.miss, device=dev)[:, :2 * a.inds]
    panel = PackedPanel.from_codes(codes, dev)
    g32, c32 = float_matrices(codes, a.inds, dev)
    sq32 = g32 * g32
    del codes
    report = {"timing": "one HIP event pair around --inner launches per region, ms per launch, the regions interleaved rep by rep; "
                        "design and ld_glm: host clock, s", "inner": a.inner,
              "miss": a.miss, "scans": []}
    for n_pheno in (int(x) for x in a.phenos.split(",")):
        report["scans"].append(one_scan(panel, g32, c32, sq32, n_pheno, a.covars, a.reps, max(1, a.warmup), max(1, a.inner), dev))
        print(json.dumps(report["scans"][-1]), flush=True)
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

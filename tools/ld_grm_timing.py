"""Time of the genetic relationship matrix (ops.ld_grm: SNP counts, the coefficients on the host, ldx_sample_planes_dev +
ldx_sample_wprod_dev for S, the FP4 counts for N, ldx_grm_cells_dev) against the same GRM in torch on the same card, on two kinds
of synthetic panel: without a missing call, and with missing calls (--miss, default 3 %).

    python tools/ld_grm_timing.py [--inds 2504] [--snps 100000,1000000] [--reps 5] [--warmup 1] [--miss 0.03] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  Three regions, each between two device events of its own and INTERLEAVED
rep by rep so that clock drift hits all alike:
    ld_grm   the whole operator from the packed panel to the float32 matrix (its host step, the coefficients, included)
    wprod    ops.sample_wprod alone on the coefficients of that run: the transposition and the int8 products
    torch    the baseline: Z Z^T / (C C^T) with torch.mm -- Z float32 [n_ind, n_snps], the standardised genotype
             c (g - 2 p) / sqrt(2 p (1 - p)) of the live SNPs (0 where the call is missing), C the called flags as fp16 with an
             fp32 result (exact below 2^24) -- both matrices built BEFORE the clock starts
Before timing, both results are compared with GCTA's formula in fp64 (the same two products in float64, SNP chunk by chunk): the
largest |grm - fp64| over all cells is reported for each.  No threshold is applied to the times: one JSON object with the
medians and the ratio torch / ld_grm is printed (and written to --out)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from ld_tools_amd import PackedPanel, geno_snp_counts, grm_weights, ld_grm, sample_wprod, synth  # noqa: E402

CHUNK = 32768   # SNPs per step while the baseline's matrices and the fp64 reference are built


def region_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def baseline_matrices(codes, n_ind, live, dev):
    """(Z float32 [n_ind, n_snps], C fp16 [n_ind, n_snps], the fp64 reference GRM [n_ind, n_ind]) from the int8 codes."""
    n_snps = codes.shape[0]
    Z = torch.zeros((n_ind, n_snps), dtype=torch.float32, device=dev)
    C = torch.zeros((n_ind, n_snps), dtype=torch.float16, device=dev)
    A = torch.zeros((n_ind, n_ind), dtype=torch.float64, device=dev)
    N = torch.zeros((n_ind, n_ind), dtype=torch.float64, device=dev)
    for s in range(0, n_snps, CHUNK):
        c = codes[s:s + CHUNK, :2 * n_ind]
        h0, h1 = c[:, 0::2], c[:, 1::2]
        called = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1)) & live[s:s + CHUNK, None]
        g = ((h0 == 1).to(torch.float64) + (h1 == 1).to(torch.float64)) * called
        n = called.sum(dim=1, keepdim=True).to(torch.float64).clamp(min=1)
        p = g.sum(dim=1, keepdim=True) / (2.0 * n)
        sd = torch.sqrt(2.0 * p * (1.0 - p))
        z = torch.where(called, (g - 2.0 * p) / torch.where(sd > 0, sd, torch.ones_like(sd)), torch.zeros_like(g)).T
        c64 = called.T.to(torch.float64)
        A += z @ z.T
        N += c64 @ c64.T
        Z[:, s:s + CHUNK] = z.to(torch.float32)
        C[:, s:s + CHUNK] = c64.to(torch.float16)
    ref = torch.where(N > 0, A / N.clamp(min=1), torch.zeros_like(A))
    return Z, C, ref, N


def one_panel(kind, n_ind, n_snps, miss, reps, warmup, dev):
    codes = synth.synth_codes_device(n_snps, 2 * n_ind, seed=synth.BENCH_SEED, miss=miss, device=dev)[:, :2 * n_ind]
    panel = PackedPanel.from_codes(codes, dev)
    q, e, live = grm_weights(geno_snp_counts(panel))
    Z, C, ref, n_ref = baseline_matrices(codes, n_ind, torch.from_numpy(live.astype(bool)).to(dev), dev)
    del codes
    out = {}

    def ours():
        out["grm"] = ld_grm(panel).grm()

    def wprod():
        out["S"] = sample_wprod(panel, q, keep=live)

    def mm_f32():
        out["torch"] = torch.mm(Z, Z.T) / torch.mm(C, C.T, out_dtype=torch.float32).clamp(min=1)

    def mm_plain():   # where mm has no fp32 result for fp16 operands: the flags as float32
        c32 = out.setdefault("C32", C.to(torch.float32))
        out["torch"] = torch.mm(Z, Z.T) / torch.mm(c32, c32.T).clamp(min=1)

    try:
        mm_f32()
        baseline, form = mm_f32, "torch.mm(Z f32) / torch.mm(C fp16, out_dtype=float32)"
    except (RuntimeError, TypeError):
        baseline, form = mm_plain, "torch.mm(Z f32) / torch.mm(C f32)"
    ours(), wprod(), baseline()
    torch.cuda.synchronize()
    pairs = n_ref > 0
    err_ours = float((out["grm"].to(torch.float64) - ref)[pairs].abs().max())
    err_torch = float((out["torch"].to(torch.float64) - ref)[pairs].abs().max())
    for _ in range(warmup):
        ours(), wprod(), baseline()
    torch.cuda.synchronize()
    t_ours, t_wprod, t_torch = [], [], []
    for _ in range(reps):   # interleaved
        t_ours.append(region_ms(ours))
        t_wprod.append(region_ms(wprod))
        t_torch.append(region_ms(baseline))
    so, sw, st = stats(t_ours), stats(t_wprod), stats(t_torch)
    tiles = (n_ind + 127) // 128
    macs = tiles * (tiles + 1) // 2 * 1024 * ((n_snps + 255) // 256) * (32 * 32 * 32)   # 1024 MFMAs per 128 x 128 x 256 block, lower tiles
    return {"panel": kind, "n_ind": n_ind, "n_snps": n_snps, "miss": miss, "n_live": int(live.sum()), "exp": e, "ld_grm": so,
            "sample_wprod": sw, "torch": st, "torch_form": form, "ratio_torch_over_ld_grm": st["median_ms"] / so["median_ms"],
            "ratio_torch_over_wprod": st["median_ms"] / sw["median_ms"],
            "wprod_int8_tops_issued": 2 * macs / (sw["median_ms"] * 1e-3) / 1e12,
            "max_abs_error_vs_fp64": {"ld_grm": err_ours, "torch_f32": err_torch}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inds", type=int, default=2504)
    ap.add_argument("--snps", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--miss", type=float, default=0.03)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 3:
        raise SystemExit("--reps must be at least 3")
    if not torch.cuda.is_available():
        raise SystemExit("ld_grm_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    report = {"timing": "one HIP event pair per region, the three regions interleaved rep by rep, ms", "panels": []}
    for n_snps in (int(x) for x in a.snps.split(",")):
        for kind, miss in (("no_holes", 0.0), ("holes", a.miss)):
            report["panels"].append(one_panel(kind, a.inds, n_snps, miss, a.reps, max(1, a.warmup), dev))
            torch.cuda.empty_cache()
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

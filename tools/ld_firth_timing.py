"""Time of the Firth logistic scan (ops.ld_glm_logistic(firth=): ldx_glm_firth_dev) on one card:

    python tools/ld_firth_timing.py [--inds 2504] [--snps 100000] [--phenos 1,20] [--covars 10] [--reps 5] [--warmup 1]
                                    [--torch-reps 2] [--chunk 2048] [--miss 0.03] [--rare 0.02] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).
  * firth="always" (mode 0, one launch of ldx_glm_firth_dev between two device events, --reps times) per number of phenotypes, against
    torch_firth: the same scan as batched fp64 Firth scoring in torch on the same card -- the design [B | x] of a chunk of --chunk SNPs
    as one tensor [chunk, m, N], torch.bmm for eta and I, T = L^-1 V by solve_triangular, U* by a pairwise torch.sum, cholesky_ex / cholesky_solve, the same
    start (the null fit), the same stopping rule (lambda*^2 <= 2^-88, that step applied, the information once more), the same
    step-length safeguard and the same cap,
    every SNP of the chunk iterated until the last one of it has converged -- what a user would write; --torch-reps times,
    interleaved.  Before timing, beta of the baseline is compared with ours (|d beta| <= 1e-8 se).
  * firth="fallback" for the first phenotype count: the ML launch alone (ldx_glm_logistic_dev, the kernel as it was before the
    fallback existed) and the mode-1 launch behind it, on the ordinary panel and on a copy with --rare of the SNPs replaced by planted
    rare variants (3 - 8 heterozygous carriers, all of them cases of phenotype 0); the share of flag-5 cells is reported with the
    overhead.
Reported with the times: the mean information evaluations per fitted cell and the v_mfma_f64_16x16x4_f64 instructions issued --
per cell n_iter x ceil(N / 4) in pass A and (n_iter - 1) x 4 ceil(N / 16) in pass B, counted from the result -- and their rate over
the launch.  A library built with another -DLDX_FIRTH_MIN_WAVES=n (ld_tools_amd/build.py --out libldx_wN.so -DLDX_FIRTH_MIN_WAVES=N)
is timed by LDX_LIB=...; --skip-torch leaves the baseline out of such a run.  No threshold is applied: one JSON object per scan is
printed (and all written to --out)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ld_tools_amd import FIRTH_STOP, PackedPanel, logit_design, ops, synth  # noqa: E402
from ld_tools_amd._lib import FIRTH_MAX_ITER, check, lib  # noqa: E402

CHUNK = 65536


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


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


def torch_firth(x, basis, y, theta0, chunk):
    """(beta, se, n_iter) float64 / int32 [n_snps, n_pheno] by batched Firth scoring; NaN where the fit fails."""
    n_snps, n_ind = x.shape
    P, p = basis.shape[0], y.shape[0]
    dev = x.device
    beta = torch.full((n_snps, p), float("nan"), dtype=torch.float64, device=dev)
    se, iters = beta.clone(), torch.zeros((n_snps, p), dtype=torch.int32, device=dev)
    eye = torch.eye(P + 1, dtype=torch.float64, device=dev)[None]
    for j in range(p):
        yj = y[j].to(torch.float64)
        for s in range(0, n_snps, chunk):
            xs = x[s:s + chunk]
            n_real = xs.shape[0]
            if n_real < chunk and n_snps > chunk:
                # the tail is filled up with copies of its first SNP: every batch then has the size of the first, which is the
                # only batch size at which the batched factorisation of this torch build was seen to return sound status words
                xs = torch.cat([xs, xs[:1].expand(chunk - n_real, n_ind)], dim=0)
            S = xs.shape[0]
            V = torch.cat([basis[None].expand(S, P, n_ind), xs[:, None, :]], dim=1)           # [S, m, N]
            th = torch.cat([theta0[j][None].expand(S, P), torch.zeros((S, 1), dtype=torch.float64, device=dev)], dim=1)
            active = torch.ones(S, dtype=torch.bool, device=dev)      # still iterating
            last = torch.zeros(S, dtype=torch.bool, device=dev)       # the next evaluation is the final one
            bad = torch.zeros(S, dtype=torch.bool, device=dev)
            n_it = torch.zeros(S, dtype=torch.int32, device=dev)
            out_se = torch.full((S,), float("nan"), dtype=torch.float64, device=dev)
            length = torch.ones(S, dtype=torch.float64, device=dev)
            before = torch.full((S,), float("inf"), dtype=torch.float64, device=dev)
            start, step = th.clone(), torch.zeros_like(th)
            for _ in range(FIRTH_MAX_ITER):
                eta = torch.bmm(th[:, None, :], V)[:, 0, :]
                mu = torch.sigmoid(eta)
                w = mu * (1.0 - mu)
                info = torch.bmm(V * w[:, None, :], V.transpose(1, 2))
                # a cell that is done or lost is factored as the identity: a non-finite matrix in the batch (a monomorphic SNP, one
                # step after its singular information) must not reach the batched factorisation, which then fails its neighbours
                sound = active & torch.isfinite(info).all(dim=2).all(dim=1)
                bad |= active & ~sound
                L, fail = torch.linalg.cholesky_ex(torch.where(sound[:, None, None], info, eye))
                n_it += active.to(torch.int32)
                bad |= active & (fail != 0)
                active = active & sound
                done_now = active & last & (fail == 0)
                out_se = torch.where(done_now, 1.0 / L[:, P, P], out_se)
                active = active & ~last & (fail == 0)
                if not bool(active.any().item()):
                    break
                L = torch.where((fail == 0)[:, None, None], L, eye)
                T = torch.linalg.solve_triangular(L, V, upper=False)
                h = w * (T * T).sum(dim=1)
                # U* by torch.sum, which adds pairwise, as the device and the mirror do (ops._firth_scoring): a running sum over
                # thousands of individuals can keep lambda*^2 above the stop constant
                score = (V * (yj[None, :] - mu + h * (0.5 - mu))[:, None, :]).sum(dim=2)[:, :, None]
                delta = torch.cholesky_solve(score, L)[:, :, 0]
                dec = (score[:, :, 0] * delta).sum(dim=1)
                # the safeguard of the iteration: a point whose lambda*^2 did not fall is given up for one half as far along
                # the step before, and the length stays halved
                back = active & (dec >= before)
                fwd = active & ~back
                length = torch.where(back, 0.5 * length, length)
                start = torch.where(fwd[:, None], th, start)
                step = torch.where(fwd[:, None], delta, step)
                before = torch.where(fwd, dec, before)
                th = torch.where(active[:, None], start + length[:, None] * step, th)
                last = fwd & (dec <= FIRTH_STOP)
            ok = ~bad & ~active & torch.isfinite(out_se)
            beta[s:s + n_real, j] = torch.where(ok, th[:, P], torch.full_like(out_se, float("nan")))[:n_real]
            se[s:s + n_real, j] = torch.where(ok, out_se, torch.full_like(out_se, float("nan")))[:n_real]
            iters[s:s + n_real, j] = n_it[:n_real]
    return beta, se, iters


class Buffers:
    """The device arguments of the two entries for one panel and design."""

    def __init__(self, panel, des, dev):
        self.panel, self.des, self.p = panel, des, des.n_pheno
        self.basis, self.y8, self.theta0 = (torch.from_numpy(v).to(dev) for v in (des.basis, des.y, des.theta0))
        self.counts = ops._snp_counts(panel, None)
        self.outs = [torch.empty((panel.n_snps, self.p), dtype=torch.float64, device=dev) for _ in range(5)]
        self.flags, self.n_iter, self.mark = (torch.empty((panel.n_snps, self.p), dtype=torch.uint8, device=dev) for _ in range(3))

    def args(self):
        pn = self.panel
        return (pn.alt.data_ptr(), pn.ref.data_ptr(), pn.n_snps, pn.n_hap, None, self.counts.data_ptr(), self.basis.data_ptr(),
                pn.n_ind, self.des.n_cov, self.y8.data_ptr(), self.theta0.data_ptr(), self.p, 50.0,
                *(o.data_ptr() for o in self.outs), self.flags.data_ptr(), self.n_iter.data_ptr(), self.p)

    def ml(self):
        check(lib.ldx_glm_logistic_dev(*self.args(), None), "ldx_glm_logistic_dev")

    def firth(self, mode):
        check(lib.ldx_glm_firth_dev(*self.args(), mode, self.mark.data_ptr(), None), "ldx_glm_firth_dev")

    def mfma(self):
        """fp64 MFMAs of the Firth fits the buffers hold: pass A and pass B."""
        n_ind = self.panel.n_ind
        it = self.n_iter.to(torch.int64)[self.mark != 0]
        return int(it.sum().item()) * ((n_ind + 3) // 4) + int((it - 1).clamp(min=0).sum().item()) * 4 * ((n_ind + 15) // 16)


def traits(n_ind, n_pheno, n_covar):
    rng = np.random.default_rng(n_pheno)
    C = rng.standard_normal((n_ind, n_covar))
    eta = -0.3 + 0.4 * C[:, :1] + 0.2 * rng.standard_normal((n_ind, n_pheno))
    return (rng.random((n_ind, n_pheno)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.uint8), C


def always_scan(panel, x, n_pheno, a, dev):
    Y, C = traits(panel.n_ind, n_pheno, a.covars)
    buf = Buffers(panel, logit_design(Y, C), dev)
    buf.firth(0)
    torch.cuda.synchronize()
    cells = panel.n_snps * n_pheno
    out = {"n_ind": panel.n_ind, "n_snps": panel.n_snps, "n_pheno": n_pheno, "n_covar": a.covars, "cells": cells,
           "flag_counts": torch.bincount(buf.flags.flatten().to(torch.int64), minlength=6).tolist()}
    it = buf.n_iter.to(torch.int64)
    out["mean_n_iter"], out["max_n_iter"] = it[buf.mark != 0].double().mean().item(), int(it.max().item())
    out["mfma_f64_16x16x4_issued"] = buf.mfma()
    if not a.skip_torch:
        t_beta, t_se, t_it = torch_firth(x, buf.basis, buf.y8, buf.theta0, a.chunk)
        both = (buf.flags == 0) & torch.isfinite(t_beta)
        gap = ((buf.outs[0] - t_beta).abs() / t_se)[both].max().item()
        if not gap <= 1e-8:
            raise SystemExit(f"the torch baseline's beta differs from ours by {gap} se")
        missed = int(((buf.flags == 0) & ~torch.isfinite(t_beta)).sum().item())
        if missed:
            raise SystemExit(f"the torch baseline fits {missed} cells fewer than we do: its time would not be that of the same scan")
        out.update(baseline_beta_gap_in_se=gap, baseline_fits=int(torch.isfinite(t_beta).sum().item()),
                   baseline_mean_n_iter=t_it.double().mean().item())
    for _ in range(a.warmup):
        buf.firth(0)
    torch.cuda.synchronize()
    times = {"firth_always": [], "ml_scan": [], "torch_firth": []}
    for rep in range(a.reps):   # interleaved
        times["firth_always"].append(event_ms(lambda: buf.firth(0)))
        times["ml_scan"].append(event_ms(buf.ml))
        if not a.skip_torch and rep < a.torch_reps:
            times["torch_firth"].append(event_ms(lambda: torch_firth(x, buf.basis, buf.y8, buf.theta0, a.chunk)))
    out.update({name: stats(ms) for name, ms in times.items() if ms})
    ms = out["firth_always"]["median_ms"]
    out["mfma_gflops_over_launch"] = out["mfma_f64_16x16x4_issued"] * 2048.0 / (ms * 1e-3) / 1e9
    out["ratio_firth_over_ml"] = ms / out["ml_scan"]["median_ms"]
    if times["torch_firth"]:
        out["ratio_torch_over_firth"] = out["torch_firth"]["median_ms"] / ms
    return out


def fallback_scan(panel, name, n_pheno, a, dev, Y, C):
    buf = Buffers(panel, logit_design(Y, C), dev)
    for _ in range(max(1, a.warmup)):
        buf.ml()
        buf.firth(1)
    torch.cuda.synchronize()
    times = {"ml_scan": [], "fallback_launch": []}
    for _ in range(a.reps):
        times["ml_scan"].append(event_ms(buf.ml))           # rewrites the flags the next launch reads
        times["fallback_launch"].append(event_ms(lambda: buf.firth(1)))
    cells = panel.n_snps * n_pheno
    refit = int((buf.mark != 0).sum().item())
    out = {"panel": name, "n_pheno": n_pheno, "cells": cells, "refitted_cells": refit, "share_flag_5": refit / cells,
           "flag_5_left": int((buf.flags == 5).sum().item()), "mfma_f64_16x16x4_issued_by_the_refits": buf.mfma()}
    if refit:
        out["mean_n_iter_of_the_refits"] = buf.n_iter.to(torch.float64)[buf.mark != 0].mean().item()
    out.update({k: stats(ms) for k, ms in times.items()})
    out["overhead"] = out["fallback_launch"]["median_ms"] / out["ml_scan"]["median_ms"]
    return out


def plant_rare(codes, y0, share, seed):
    """A copy of ``codes`` with ``share`` of the SNPs replaced by variants of 3 - 8 heterozygous carriers, all cases of y0."""
    rng = np.random.default_rng(seed)
    n_snps = codes.shape[0]
    rows = rng.choice(n_snps, size=max(1, int(share * n_snps)), replace=False)
    cases = np.flatnonzero(y0 != 0)
    block = np.zeros((len(rows), codes.shape[1]), dtype=np.int8)
    for k in range(len(rows)):
        block[k, 2 * rng.choice(cases, size=int(rng.integers(3, 9)), replace=False)] = 1
    out = codes.clone()
    out[torch.from_numpy(rows).to(codes.device)] = torch.from_numpy(block).to(codes.device)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inds", type=int, default=2504)
    ap.add_argument("--snps", type=int, default=100000)
    ap.add_argument("--phenos", default="1,20")
    ap.add_argument("--covars", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--miss", type=float, default=0.03)
    ap.add_argument("--rare", type=float, default=0.02)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-fallback", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 3 or not 1 <= a.torch_reps <= a.reps:
        raise SystemExit("--reps must be at least 3 and --torch-reps between 1 and --reps")
    if not torch.cuda.is_available():
        raise SystemExit("ld_firth_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    codes = synth.synth_codes_device(a.snps, 2 * a.inds, seed=synth.BENCH_SEED, miss=a.miss, device=dev)[:, :2 * a.inds].contiguous()
    panel = PackedPanel.from_codes(codes, dev)
    x = None if a.skip_torch else centred_dosage(codes, a.inds, dev)
    report = {"timing": "one HIP event pair around each launch (firth_always, ml_scan, fallback_launch) or each whole baseline scan "
                        "(torch_firth), ms, interleaved rep by rep", "miss": a.miss, "chunk": a.chunk, "stop": FIRTH_STOP,
              "lib": str(lib._name), "scans": [], "fallback": []}
    phenos = [int(v) for v in a.phenos.split(",")]
    for n_pheno in phenos:
        report["scans"].append(always_scan(panel, x, n_pheno, a, dev))
        print(json.dumps(report["scans"][-1]), flush=True)
    del x
    if not a.skip_fallback:
        Y, C = traits(a.inds, phenos[0], a.covars)
        report["fallback"].append(fallback_scan(panel, "ordinary", phenos[0], a, dev, Y, C))
        print(json.dumps(report["fallback"][-1]), flush=True)
        planted = PackedPanel.from_codes(plant_rare(codes, Y[:, 0], a.rare, 11), dev)
        report["fallback"].append(fallback_scan(planted, f"{a.rare:g} of the SNPs rare and all-case", phenos[0], a, dev, Y, C))
        print(json.dumps(report["fallback"][-1]), flush=True)
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

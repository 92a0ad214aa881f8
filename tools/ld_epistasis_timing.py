"""Time of the epistasis scan (ops.ld_epistasis, ld_epistasis_hits, ld_epistasis_counts) on one card:

    python tools/ld_epistasis_timing.py [--snps 10000] [--inds 2504] [--miss 0,0.03] [--reps 3] [--warmup 1] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  The panels are synthetic (synth.synth_codes_device, seeded): two SNP
sets of --snps SNPs over --inds individuals, split in half into cases and controls, once per missing-call rate of --miss.
Per rate, every launch between two device events, its two sides (the four group panels and their count tables) made before:
  counts    ldx_epi_counts_dev alone: the K loops and 72 bytes per pair of stores
  allelic   ldx_epi_rect_dev, chisq + dir + flags
  boost     the same with the iterative fit per cell; the mean cycle count of a sample of its cells is reported beside it
  hits      ldx_epi_hits_dev at p = 1e-4 with the per-SNP summary (boost), the buffer large enough
  em_pw     ops.ld_em(missing="pairwise") on the same two panels: the five-set pairwise EM tile as the per-set yardstick
  torch     the same 18 tables as torch.mm products of fp16 indicator matrices (nine per group, fp32 accumulation, exact at
            these sizes) plus the allelic statistic elementwise in fp64, in row blocks of 1000 SNPs, on the same card
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

from ld_tools_amd import PackedPanel, epi_chisq_bound, ld_em, ld_epistasis_from_counts, synth  # noqa: E402
from ld_tools_amd._lib import check, lib  # noqa: E402
from ld_tools_amd.ops import _epi_sides, _stream_ptr  # noqa: E402


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


def indicators(codes, member):
    """fp16 [3, n_snps, group size]: the individuals of the group with genotype 0 / 1 / 2, called at both haplotypes."""
    c = codes[:, torch.from_numpy(np.repeat(member, 2)).to(codes.device)]
    ok = (c[:, 0::2] <= 1) & (c[:, 1::2] <= 1) & (c[:, 0::2] >= 0) & (c[:, 1::2] >= 0)
    g = (c[:, 0::2] == 1).to(torch.int8) + (c[:, 1::2] == 1).to(torch.int8)
    return torch.stack([((g == v) & ok).to(torch.float16) for v in range(3)])


def torch_allelic(ind_i, ind_j, block=1000):
    """The allelic chi-square of every pair from torch.mm tables, float64 [n_i, n_j]."""
    n_i, n_j = ind_i[0].shape[1], ind_j[0].shape[1]
    out = torch.empty((n_i, n_j), dtype=torch.float64, device=ind_i[0].device)
    w = torch.arange(3, dtype=torch.float64, device=out.device)
    for r0 in range(0, n_i, block):
        L, V = [], []
        for gi, gj in zip(ind_i, ind_j):
            t = torch.stack([torch.mm(gi[x, r0:r0 + block], gj[y].T) for x in range(3) for y in range(3)]).to(torch.float64)
            t = t.view(3, 3, *t.shape[1:])
            N, A, B = t.sum(dim=(0, 1)), torch.tensordot(w, t.sum(dim=1), 1), torch.tensordot(w, t.sum(dim=0), 1)
            S = torch.tensordot(torch.outer(w, w), t, 2)
            ca, cb, cc, cd = S, 2 * A - S, 2 * B - S, 4 * N - 2 * A - 2 * B + S
            L.append(torch.log((ca * cd) / (cb * cc)))
            V.append((1 / ca + 1 / cd) + (1 / cb + 1 / cc))
        z = (L[0] - L[1]) / torch.sqrt(V[0] + V[1])
        out[r0:r0 + block] = z * z
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=10000)
    ap.add_argument("--inds", type=int, default=2504)
    ap.add_argument("--miss", default="0,0.03")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ld_epistasis_timing: no HIP device")
    dev = torch.device("cuda", 0)
    n, n_ind = a.snps, a.inds
    case = np.zeros(n_ind)
    case[: n_ind // 2] = 1.0
    report = {"timing": "one HIP event pair around each launch, ms, medians of --reps calls after --warmup calls", "snps": n,
              "inds": n_ind, "pairs": n * n, "lib": str(lib._name), "results": []}
    for miss in (float(x) for x in a.miss.split(",")):
        codes_i = synth.synth_codes_device(n, 2 * n_ind, seed=synth.BENCH_SEED, miss=miss, device=dev)[:, :2 * n_ind].contiguous()
        codes_j = synth.synth_codes_device(n, 2 * n_ind, seed=synth.BENCH_SEED + 1, miss=miss, device=dev)[:, :2 * n_ind].contiguous()
        pi, pj = PackedPanel.from_codes(codes_i, dev), PackedPanel.from_codes(codes_j, dev)
        si, sj, hc, hu = _epi_sides("ld_epistasis_timing", pi, case, pj, None)
        counts = torch.empty((18, n, n), dtype=torch.int32, device=dev)
        chisq = torch.empty((n, n), dtype=torch.float32, device=dev)
        dirn, flags = torch.empty_like(chisq), torch.empty((n, n), dtype=torch.uint8, device=dev)
        rec = lambda r: report["results"].append({"miss": miss, **r})  # noqa: E731
        rec(timed("counts", lambda: check(lib.ldx_epi_counts_dev(si.ref, sj.ref, hc, hu, counts.data_ptr(), n, _stream_ptr())), a,
                  miss=miss))
        sample = counts[:, :: max(1, n // 100), :: max(1, n // 100)].contiguous()
        cells = ld_epistasis_from_counts(sample, "boost")
        cycles = cells.cycles.to(torch.float64)
        for code, name in ((0, "allelic"), (1, "boost")):
            extra = {"mean_cycles": float(cycles.mean()), "max_cycles": int(cycles.max())} if code else {}
            rec(timed(name, lambda: check(lib.ldx_epi_rect_dev(si.ref, sj.ref, hc, hu, code, chisq.data_ptr(), dirn.data_ptr(),
                                                               flags.data_ptr(), n, _stream_ptr())), a, miss=miss, **extra))
        del counts
        cap = 1 << 23
        raw = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        n_hits = torch.zeros(1, dtype=torch.int64, device=dev)
        n_tot, n_sig = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        best = torch.zeros(n, dtype=torch.int64, device=dev)
        bound, bound_sig = float(epi_chisq_bound(1e-4, "boost")), float(epi_chisq_bound(1e-2, "boost"))

        def hits():
            for t in (n_tot, n_sig, best):
                t.zero_()
            check(lib.ldx_epi_hits_dev(si.ref, sj.ref, hc, hu, 1, 0, bound, raw.data_ptr(), cap, n_hits.data_ptr(), bound_sig,
                                       n_tot.data_ptr(), n_sig.data_ptr(), best.data_ptr(), _stream_ptr()))

        r = timed("hits", hits, a, miss=miss)
        r["slots_reserved"] = int(n_hits.item())
        rec(r)
        out_r = torch.empty((n, n), dtype=torch.float32, device=dev)
        out_d = torch.empty_like(out_r)
        rec(timed("em_pw", lambda: ld_em(pi, pj, out_r=out_r, out_dprime=out_d, missing="pairwise"), a, miss=miss))
        del out_r, out_d, raw
        groups = [case == 1.0, case == 0.0]
        ind_i, ind_j = [indicators(codes_i, g) for g in groups], [indicators(codes_j, g) for g in groups]
        ref = torch_allelic(ind_i, ind_j)
        check(lib.ldx_epi_rect_dev(si.ref, sj.ref, hc, hu, 0, chisq.data_ptr(), dirn.data_ptr(), flags.data_ptr(), n, _stream_ptr()))
        ok = torch.isfinite(ref) & torch.isfinite(chisq)
        err = float(((ref - chisq.to(torch.float64)).abs() / ref.clamp(min=1.0))[ok].max())
        del ref
        rec(timed("torch", lambda: torch_allelic(ind_i, ind_j), a, miss=miss, max_rel_diff_to_scan=err))
        del ind_i, ind_j, codes_i, codes_j, pi, pj, si, sj
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

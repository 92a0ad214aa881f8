"""Time of pairwise-complete EM (ops.ld_em(missing="pairwise"), ldx_ld_em_rect_pw_dev) against plain ops.ld_em on the same two
panels, on two kinds of panel:

    no_holes    a panel without a missing code: every tile of the pairwise kernel takes the shortcut (ld_em's two-set K loop)
    all_holes   missing codes (--miss, default 2 %) in every SNP, hence in every slab: every tile runs the general loop (five
                counts per pair, four passes over K)

    python tools/ld_em_pairwise_timing.py [--haps 5008] [--reps 20] [--warmup 2] [--shapes 10000x10000] [--miss 0.02] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  One process, one device: plain ld_em is the yardstick and is timed in
the same process, its calls ALTERNATED with the pairwise ones so that clock drift hits both alike; every call sits between two
device events of its own.  Before timing, the no_holes panel's matrices are compared bit for bit (they must be equal), and on
both panels the five integers of 64 x 64 sampled rows (ops.ld_em_counts(missing="pairwise") on those rows) are compared with a
host count from the codes, and the sampled cells with the list epilogue on those integers, bit for bit.  No threshold is
applied to the times: one JSON object with the medians and the ratio pairwise / plain per panel is printed (and written to
--out).
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

SAMPLE_ROWS = 64   # the check pairs this many rows of each side: 4096 cells


def call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "calls": len(ms)}


def host_counts(ci, cj) -> np.ndarray:
    """int64 [5, n_i, n_j], N A B S H over the individuals called at both SNPs (include/ldx.h, "pairwise-complete EM"):
    float64 GEMMs of 0/1/2 matrices, exact."""
    def planes(c):
        called = (c == 0) | (c == 1)
        q = called[:, 0::2] & called[:, 1::2]
        g = ((c[:, 0::2] == 1).astype(np.int64) + (c[:, 1::2] == 1).astype(np.int64)) * q
        return q.astype(np.float64), g.astype(np.float64), (g == 1).astype(np.float64)

    (qi, gi, ti), (qj, gj, tj) = planes(ci), planes(cj)
    return np.stack([qi @ qj.T, gi @ qj.T, qi @ gj.T, gi @ gj.T, ti @ tj.T]).astype(np.int64)


def one_panel(kind, n_i, n_j, h, miss, reps, warmup, dev):
    codes = synth.synth_codes_device(n_i + n_j, h, seed=synth.BENCH_SEED, miss=miss, device=dev)
    stacked = PackedPanel.from_codes(codes, dev)
    pi = stacked.select(snps=np.arange(0, n_i, dtype=np.uint32))
    pj = stacked.select(snps=np.arange(n_i, n_i + n_j, dtype=np.uint32))
    holes_i = int(((pi.acnt[:n_i] + pi.rcnt[:n_i]) != h).sum())
    holes_j = int(((pj.acnt[:n_j] + pj.rcnt[:n_j]) != h).sum())
    outs = [torch.empty((n_i, n_j), dtype=torch.float32, device=dev) for _ in range(4)]

    def plain():
        return ops.ld_em(pi, pj, out_r=outs[0], out_dprime=outs[1])

    def pairwise():
        return ops.ld_em(pi, pj, out_r=outs[2], out_dprime=outs[3], missing="pairwise")

    a, b = plain(), pairwise()
    if holes_i == 0 and holes_j == 0:
        differ = int((a.r.view(torch.int32) != b.r.view(torch.int32)).sum() + (a.dprime.view(torch.int32) != b.dprime.view(torch.int32)).sum())
        if differ:
            raise SystemExit(f"{kind}: {differ} cells differ from plain ld_em on a panel without holes")
    rows_i = np.linspace(0, n_i - 1, SAMPLE_ROWS).astype(np.int64)
    rows_j = np.linspace(0, n_j - 1, SAMPLE_ROWS).astype(np.int64)
    host = codes[:, :h].cpu().numpy()
    want = host_counts(host[rows_i], host[n_i + rows_j])
    si, sj = pi.select(snps=rows_i.astype(np.uint32)), pj.select(snps=rows_j.astype(np.uint32))
    got = ops.ld_em_counts(si, sj, missing="pairwise").cpu().numpy().astype(np.int64)
    if not np.array_equal(got, want):
        raise SystemExit(f"{kind}: the integers of the sampled rows differ from the host count")
    lr, ld_, _ = ops.ld_em_from_counts(*(k.reshape(-1) for k in want))
    ti, tj = torch.as_tensor(rows_i).to(dev), torch.as_tensor(rows_j).to(dev)
    for name, cells, lst in (("r", b.r, lr), ("D'", b.dprime, ld_)):
        if not torch.equal(cells[ti][:, tj].reshape(-1).view(torch.int32), lst.view(torch.int32)):
            raise SystemExit(f"{kind}: sampled {name} cells differ from the list epilogue on the host's integers")
    for _ in range(warmup):
        plain()
        pairwise()
    torch.cuda.synchronize()
    t_plain, t_pw = [], []
    for _ in range(reps):   # alternated
        t_plain.append(call_ms(plain))
        t_pw.append(call_ms(pairwise))
    sp, sw = stats(t_plain), stats(t_pw)
    return {"panel": kind, "n_i": n_i, "n_j": n_j, "n_hap": h, "miss": miss, "rows_with_holes": [holes_i, holes_j],
            "plain": sp, "pairwise": sw, "ratio": sw["median_ms"] / sp["median_ms"],
            "pairwise_pairs_per_s": n_i * n_j / (sw["median_ms"] * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--haps", type=int, default=5008)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="10000x10000")
    ap.add_argument("--miss", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    if a.haps % 2:
        raise SystemExit("--haps must be even: individual k owns haplotypes 2k and 2k + 1")
    if not torch.cuda.is_available():
        raise SystemExit("ld_em_pairwise_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    report = {"timing": "one HIP event pair per call, plain and pairwise alternated call by call, ms", "panels": []}
    for spec in a.shapes.split(","):
        n_i, n_j = (int(x) for x in spec.lower().split("x"))
        for kind, miss in (("no_holes", 0.0), ("all_holes", a.miss)):
            report["panels"].append(one_panel(kind, n_i, n_j, a.haps, miss, a.reps, max(1, a.warmup), dev))
            torch.cuda.empty_cache()
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

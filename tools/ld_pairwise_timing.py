"""Time of pairwise-complete LD (ops.ld_rect(missing="pairwise"), ldx_ld_rect_pw_dev) against plain ops.ld_rect on the same two
panels, in both forms (haplotype r and genotype dosage), on two kinds of panel:

    no_holes    a panel without a missing code: every tile of the pairwise kernel takes the one-count shortcut
    all_holes   missing codes (--miss, default 2 %) in every SNP, hence in every slab: every tile runs the general loop
                (4 counts per pair, 6 in the dosage form)

    python tools/ld_pairwise_timing.py [--haps 5008] [--reps 20] [--warmup 2] [--shapes 10000x10000] [--miss 0.02] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  One process, one device: plain ld_rect is the yardstick and is timed
in the same process, its calls ALTERNATED with the pairwise ones so that clock drift hits both alike; every call sits between
two device events of its own.  Before timing, the no_holes panel's two matrices are compared bit for bit (they must be equal),
and on both panels the cells of 64 x 64 sampled rows are compared with the host mirror of the definitions
(ops.pairwise_counts_host / ops.pairwise_cell_host; the same signed zeros, otherwise at most one float32 ulp apart).  No
threshold is applied to the times: one JSON object with the medians and the ratio pairwise / plain per panel and form is
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

from ld_tools_amd import PackedPanel, ops, synth  # noqa: E402

SAMPLE_ROWS = 64   # the host check pairs this many rows of each side: 4096 cells per form


def call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "calls": len(ms)}


def one_panel(kind, n_i, n_j, h, miss, reps, warmup, dev):
    codes = synth.synth_codes_device(n_i + n_j, h, seed=synth.BENCH_SEED, miss=miss, device=dev)
    stacked = PackedPanel.from_codes(codes, dev)
    pi = stacked.select(snps=np.arange(0, n_i, dtype=np.uint32))
    pj = stacked.select(snps=np.arange(n_i, n_i + n_j, dtype=np.uint32))
    holes_i = int(((pi.acnt[:n_i] + pi.rcnt[:n_i]) != h).sum())
    holes_j = int(((pj.acnt[:n_j] + pj.rcnt[:n_j]) != h).sum())
    out_a = torch.empty((n_i, n_j), dtype=torch.float32, device=dev)
    out_b = torch.empty((n_i, n_j), dtype=torch.float32, device=dev)
    report = {"panel": kind, "n_i": n_i, "n_j": n_j, "n_hap": h, "miss": miss, "rows_with_holes": [holes_i, holes_j], "forms": {}}
    rows_i = np.linspace(0, n_i - 1, SAMPLE_ROWS).astype(np.int64)
    rows_j = np.linspace(0, n_j - 1, SAMPLE_ROWS).astype(np.int64)
    host = codes[:, :h].cpu().numpy()
    for dosage in (False, True):
        def plain():
            return ops.ld_rect(pi, pj, dosage=dosage, out=out_a)

        def pairwise():
            return ops.ld_rect(pi, pj, dosage=dosage, out=out_b, missing="pairwise")

        a, b = plain(), pairwise()
        if holes_i == 0 and holes_j == 0:
            differ = int((a.view(torch.int32) != b.view(torch.int32)).sum())
            if differ:
                raise SystemExit(f"{kind}, dosage={dosage}: {differ} cells differ from plain ld_rect on a panel without holes")
        want = ops.pairwise_cell_host(ops.pairwise_counts_host(host[rows_i], host[n_i + rows_j], dosage), dosage)
        got = b[torch.as_tensor(rows_i).to(dev)][:, torch.as_tensor(rows_j).to(dev)].cpu().numpy()
        gb, wb = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
        zero = (want == 0.0) | (got == 0.0)
        if not np.array_equal(gb[zero], wb[zero]) or int(np.abs(gb - wb)[~zero].max(initial=0)) > 1:
            raise SystemExit(f"{kind}, dosage={dosage}: sampled cells differ from the host mirror")
        for _ in range(warmup):
            plain()
            pairwise()
        torch.cuda.synchronize()
        t_plain, t_pw = [], []
        for _ in range(reps):   # alternated
            t_plain.append(call_ms(plain))
            t_pw.append(call_ms(pairwise))
        sp, sw = stats(t_plain), stats(t_pw)
        report["forms"]["dosage" if dosage else "haplotype"] = {
            "plain": sp, "pairwise": sw, "ratio": sw["median_ms"] / sp["median_ms"],
            "pairwise_pairs_per_s": n_i * n_j / (sw["median_ms"] * 1e-3),
        }
    return report


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
        raise SystemExit("--haps must be even: the dosage form is timed too")
    if not torch.cuda.is_available():
        raise SystemExit("ld_pairwise_timing needs a HIP device: there is no CPU path")
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

"""Time of the pairwise-complete band operators (ops.ld_band / ld_score / ld_neighbors with missing="pairwise";
ldx_pwband.hip) at chromosome scale, in both forms (haplotype r and genotype dosage), against two yardsticks:

    (a) the plain operator (missing=None) on the panel without holes, where both compute the same bytes;
    (b) the expectation written down before anything was measured: pwc_kernel's cost per tile -- ops.ld_rect(missing=
        "pairwise") over a --square x --square block of the same panel, divided by its tiles -- times the tiles the band walks.

    python tools/ld_pwband_timing.py [--snps 100000] [--haps 5008] [--window-snps 1000] [--square 10000] [--reps 20]
                                     [--warmup 2] [--miss 0.02] [--out FILE]

The panels are tools/ld_pairwise_timing.py's: no_holes (every tile takes the one-count shortcut) and all_holes (--miss of the
codes missing in every SNP: every tile runs the general loop).  Runs on a GPU only.  One process, one device; the calls of an
operator and of its yardstick are ALTERNATED call by call, every call between two device events of its own, so the times are
those of the whole ops call (layout, allocation and the one host read of ld_band / ld_neighbors included, alike on both
sides).  Before timing, the no_holes results are compared with the plain operators' bit for bit.  No threshold is applied to
the times: one JSON object is printed (and written to --out).
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

PW = "pairwise"
R2 = 0.2


def call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(f, g, reps, warmup):
    """Medians (ms) of ``reps`` calls of f and of g, alternated call by call."""
    for _ in range(warmup):
        f()
        g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(call_ms(f))
        tg.append(call_ms(g))
    return statistics.median(tf), statistics.median(tg)


def tiles_walked(n: int, window_snps: int) -> int:
    """Tiles of the band kernel's walk for positions 0 .. n - 1: I block ti meets the slabs lo[256 ti] / 128 .. (r1 - 1) / 128."""
    return sum((min(256 * (ti + 1), n) - 1) // 128 - max(0, 256 * ti - window_snps) // 128 + 1 for ti in range((n + 255) // 256))


def one_panel(kind, n, h, w, square, miss, reps, warmup, dev):
    codes = synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, miss=miss, device=dev)
    panel = PackedPanel.from_codes(codes, dev)
    del codes
    sq = panel.select(snps=np.arange(0, square, dtype=np.uint32))
    holes = int(((panel.acnt[:n] + panel.rcnt[:n]) != h).sum())
    out_sq = torch.empty((square, square), dtype=torch.float32, device=dev)
    walked, sq_tiles = tiles_walked(n, w), ((square + 255) // 256) * ((square + 127) // 128)
    report = {"panel": kind, "n_snps": n, "n_hap": h, "window_snps": w, "miss": miss, "rows_with_holes": holes,
              "tiles_walked": walked, "square": square, "square_tiles": sq_tiles, "forms": {}}
    for dosage in (False, True):
        ops_pw = {
            "ld_band": lambda m=PW: ops.ld_band(panel, window_snps=w, dosage=dosage, missing=m),
            "ld_score": lambda m=PW: ops.ld_score(panel, window_snps=w, dosage=dosage, missing=m),
            "ld_neighbors": lambda m=PW: ops.ld_neighbors(panel, window_snps=w, r2=R2, dosage=dosage, missing=m),
        }

        def rect():
            return ops.ld_rect(sq, sq, dosage=dosage, out=out_sq, missing=PW)

        if holes == 0:   # the same bytes as the plain operators
            a, b = ops_pw["ld_band"](), ops_pw["ld_band"](None)
            if not (torch.equal(a.values.view(torch.int32), b.values.view(torch.int32)) and torch.equal(a.diag.view(torch.int32), b.diag.view(torch.int32))):
                raise SystemExit(f"{kind}, dosage={dosage}: the pairwise band differs from ld_band on a panel without holes")
            del a, b
            if not torch.equal(ops_pw["ld_score"]().sums.view(torch.int64), ops_pw["ld_score"](None).sums.view(torch.int64)):
                raise SystemExit(f"{kind}, dosage={dosage}: the pairwise sums differ from ld_score's on a panel without holes")
            if not torch.equal(ops_pw["ld_neighbors"]().hits, ops_pw["ld_neighbors"](None).hits):
                raise SystemExit(f"{kind}, dosage={dosage}: the pairwise lists differ from ld_neighbors' on a panel without holes")
        form = {}
        for name, fn in ops_pw.items():
            t_pw, t_rect = alternated(fn, rect, reps, warmup)
            expected = t_rect / sq_tiles * walked
            entry = {"pairwise_ms": t_pw, "rect_square_ms": t_rect, "expected_ms": expected, "ratio_to_expected": t_pw / expected}
            if holes == 0:
                t_pw2, t_plain = alternated(fn, lambda: fn(None), reps, warmup)
                entry.update(plain_ms=t_plain, pairwise_beside_plain_ms=t_pw2, ratio_to_plain=t_pw2 / t_plain)
            form[name] = entry
            torch.cuda.empty_cache()
        report["forms"]["dosage" if dosage else "haplotype"] = form
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--haps", type=int, default=5008)
    ap.add_argument("--window-snps", type=int, default=1000)
    ap.add_argument("--square", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--miss", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    if a.haps % 2:
        raise SystemExit("--haps must be even: the dosage form is timed too")
    if a.square > a.snps:
        raise SystemExit("--square must not exceed --snps")
    if not torch.cuda.is_available():
        raise SystemExit("ld_pwband_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    report = {"timing": "one HIP event pair per ops call, an operator and its yardstick alternated call by call, medians, ms",
              "panels": []}
    for kind, miss in (("no_holes", 0.0), ("all_holes", a.miss)):
        report["panels"].append(one_panel(kind, a.snps, a.haps, a.window_snps, a.square, miss, a.reps, max(1, a.warmup), dev))
        torch.cuda.empty_cache()
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

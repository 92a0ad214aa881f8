"""Time of the EM band operators (ops.ld_em_band, ops.ld_neighbors(em=True); ldx_emband.hip) against the only way the parent
commit had to the same cells: the full rectangle ops.ld_em(panel, panel) / ops.ld_em_hits(panel, panel) of the same panel.

    python tools/ld_emband_timing.py [--snps 20000] [--haps 5008] [--window-snps 500] [--reps 20] [--warmup 2] [--miss 0.02]
                                     [--out FILE]

Two panels, tools/ld_pairwise_timing.py's: no_holes, timed in the plain form (every tile runs the two-set loop), and all_holes
(--miss of the codes missing in every SNP), timed with missing="pairwise" (every tile runs the five-set general loop).  Runs on
a GPU only.  One process, one device; the band call and its yardstick are ALTERNATED call by call, every call between two
device events of its own, so the times are those of the whole ops call (the band: layout, plan, allocation, the per-SNP stats
and the one host read; the rectangle writes into buffers allocated once).  Before timing, the band's cells are compared with
the rectangle's bit for bit, and the neighbour records with the rectangle's hits inside the window.  Reported per panel: ms,
tiles (the band: tiles_walked with 128-row I blocks; the rectangle: its 128 x 128 tiles) and ms per tile for both, and the
ratios.  No threshold is applied to the times: one JSON object is printed (and written to --out).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

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
    """(median of f, median of g, the quartiles of each) in ms over ``reps`` calls, alternated call by call."""
    for _ in range(warmup):
        f()
        g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(call_ms(f))
        tg.append(call_ms(g))
    q = lambda t: [round(x, 4) for x in statistics.quantiles(t, n=4)]   # noqa: E731
    return statistics.median(tf), statistics.median(tg), q(tf), q(tg)


def tiles_walked(n: int, window_snps: int) -> int:
    """Tiles of the band kernel's walk for positions 0 .. n - 1: I block ti meets the slabs lo[128 ti] / 128 .. (r1 - 1) / 128."""
    return sum((min(128 * (ti + 1), n) - 1) // 128 - max(0, 128 * ti - window_snps) // 128 + 1 for ti in range((n + 127) // 128))


def window_hits(hits, w: int):
    """The records of a rectangle's hit list inside the window, the diagonal left out: what the neighbour list holds."""
    d = (hits.hits[:, 0] - hits.hits[:, 1]).abs()
    return hits.hits[(d <= w) & (d > 0)]


def one_panel(kind, missing, n, h, w, miss, reps, warmup, dev):
    codes = synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, miss=miss, device=dev)
    panel = PackedPanel.from_codes(codes, dev)
    del codes
    holes = int(((panel.acnt[:n] + panel.rcnt[:n]) != h).sum())
    out_r = torch.empty((n, n), dtype=torch.float32, device=dev)
    out_d = torch.empty((n, n), dtype=torch.float32, device=dev)
    walked, sq_tiles = tiles_walked(n, w), ((n + 127) // 128) ** 2

    def band():
        return ops.ld_em_band(panel, window_snps=w, missing=missing)

    def rect():
        return ops.ld_em(panel, panel, out_r=out_r, out_dprime=out_d, missing=missing)

    def nbr():
        return ops.ld_neighbors(panel, window_snps=w, r2=R2, em=True, missing=missing)

    def rect_hits():
        return window_hits(ops.ld_em_hits(panel, panel, r2=R2, missing=missing), w)

    # the same cells, the same records
    b = band()
    rect()
    lo = b.r.lo.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    length = torch.arange(n, device=dev) - lo
    rows = torch.repeat_interleave(torch.arange(n, device=dev), length)
    cols = torch.arange(b.n_cells, device=dev) - torch.repeat_interleave(b.r.offsets[:-1] - lo, length)
    for name, got, sq in (("r", b.r.values, out_r), ("D'", b.dprime.values, out_d)):
        if not torch.equal(got.view(torch.int32), sq.reshape(-1)[rows * n + cols].view(torch.int32)):
            raise SystemExit(f"{kind}: the band's {name} cells differ from the rectangle's")
    n_cells = b.n_cells
    del b, rows, cols, length, lo
    got, want = nbr().hits, rect_hits()
    if not torch.equal(got, want):
        raise SystemExit(f"{kind}: the neighbour records differ from the rectangle's hits inside the window")
    n_records = int(got.shape[0])
    del got, want
    torch.cuda.empty_cache()

    report = {"panel": kind, "missing": missing, "n_snps": n, "n_hap": h, "window_snps": w, "miss": miss, "rows_with_holes": holes,
              "band_cells": n_cells, "neighbour_records": n_records, "tiles_walked": walked, "square_tiles": sq_tiles,
              "tile_ratio": sq_tiles / walked}
    for name, f, g in (("ld_em_band", band, rect), ("ld_neighbors_em", nbr, rect_hits)):
        t_band, t_rect, q_band, q_rect = alternated(f, g, reps, warmup)
        report[name] = {"band_ms": t_band, "rect_ms": t_rect, "band_quartiles_ms": q_band, "rect_quartiles_ms": q_rect,
                        "band_ms_per_tile": t_band / walked, "rect_ms_per_tile": t_rect / sq_tiles,
                        "per_tile_ratio": (t_band / walked) / (t_rect / sq_tiles), "speedup": t_rect / t_band}
        torch.cuda.empty_cache()
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=20_000)
    ap.add_argument("--haps", type=int, default=5008)
    ap.add_argument("--window-snps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--miss", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 4:
        raise SystemExit("--reps must be at least 4")
    if a.haps % 2:
        raise SystemExit("--haps must be even: the EM pairs haplotypes into individuals")
    if not torch.cuda.is_available():
        raise SystemExit("ld_emband_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    report = {"timing": "one HIP event pair per ops call, the band call and the rectangle alternated call by call, medians, ms",
              "panels": []}
    for kind, missing, miss in (("no_holes", None, 0.0), ("all_holes", PW, a.miss)):
        report["panels"].append(one_panel(kind, missing, a.snps, a.haps, a.window_snps, miss, a.reps, max(1, a.warmup), dev))
        torch.cuda.empty_cache()
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

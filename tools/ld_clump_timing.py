"""Time of the neighbour band (ld_neighbors: ldx_ld_neighbors_dev + ldx_area_finish_ex_dev) against ld_score on the same
panel and window, and of the greedy selection rounds (ldx_ld_select_dev).

    python tools/ld_clump_timing.py [--snps 100000] [--haps 5008] [--window 250000] [--r2 0.2 0.5] [--regions 5] [--reps 5]

The panel is synthetic (synth_codes_device, BENCH_SEED) with positions 1 + 500 i (synth_positions), so +-250 kb is +-500
neighbours.  Per threshold, three things are timed INTERLEAVED (neighbours, ld_score, selection) -- each region `reps` calls
between two device events, the median region over `regions` reported per call:
  * nbr_ms: the band kernel and the finishing kernels, with a buffer big enough for the records (no overflow run), no host
    read; the record count is reported beside it;
  * score_ms: ld_score(K = 0) over the same window (one workspace, device positions);
  * select_ms: pruning's selection (MAF priority, every live SNP a candidate) -- all rounds until convergence, enqueued in
    batches of 32 with one host read of the undecided count per batch; `rounds` is the number of rounds it needed (counted
    with batches of 1).
One JSON object is printed (and written to --out).
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

from ld_tools_amd import PackedPanel, _lib, ops, synth  # noqa: E402
from ld_tools_amd.panel import _stream_ptr  # noqa: E402


def region_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--haps", type=int, default=5008)
    ap.add_argument("--window", type=int, default=250_000)
    ap.add_argument("--r2", type=float, nargs="+", default=[0.2, 0.5])
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, h, w = a.snps, a.haps, a.window
    lib = _lib.lib
    p = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev), dev)
    pos = torch.as_tensor(synth.synth_positions(n, step=500)).to(dev)
    live = ops.live_snps(p.alt_counts(), p.ref_counts())
    maf = np.minimum(p.fa.cpu().numpy()[:n], p.fr.cpu().numpy()[:n])
    rank = ops.priority_ranks(maf, live)
    score_ws = torch.empty(lib.ldx_ld_score_workspace_bytes(n, h), dtype=torch.uint8, device=dev)
    nbr_ws = torch.empty(lib.ldx_ld_neighbors_workspace_bytes(n, h), dtype=torch.uint8, device=dev)
    fin_bytes = lib.ldx_area_finish_workspace_bytes(n)
    fin = torch.empty(fin_bytes, dtype=torch.uint8, device=dev)
    report = {"snps": n, "haps": h, "window": w, "timing": f"median of {a.regions} interleaved regions of {a.reps} calls "
              "(HIP events), ms per call", "results": []}
    for t in a.r2:
        nb = ops.ld_neighbors(p, pos, window_bp=w, r2=t, strict=True, workspace=nbr_ws, check_positions=False)
        m = len(nb)
        cap = m + m // 8 + (1 << 20)
        raw = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        hits = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        n_hits = torch.zeros(1, dtype=torch.int64, device=dev)
        summary = torch.zeros(2, dtype=torch.int64, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
        bound = float(ops.r2_bound(t, True))

        def nbr():
            _lib.check(lib.ldx_ld_neighbors_dev(p.alt.data_ptr(), p.acnt.data_ptr(), p.rcnt.data_ptr(), p.fa.data_ptr(),
                                                p.fr.data_ptr(), n, h, pos.data_ptr(), w, bound, ops.PATHS["fp4"],
                                                raw.data_ptr(), cap, n_hits.data_ptr(), lib.ldx_area_finish_counts(fin.data_ptr()),
                                                nbr_ws.data_ptr(), nbr_ws.numel(), _stream_ptr()))
            _lib.check(lib.ldx_area_finish_ex_dev(raw.data_ptr(), n_hits.data_ptr(), cap, n, hits.data_ptr(),
                                                  offsets.data_ptr(), summary.data_ptr(), fin.data_ptr(), fin_bytes, 1,
                                                  _stream_ptr()))

        def score():
            ops.ld_score(p, pos, window_bp=w, workspace=score_ws, check_positions=False)

        def select():
            ops.select_dev(nb, rank, live.astype(np.uint8))

        calls = {"nbr_ms": nbr, "score_ms": score, "select_ms": select}
        for f in calls.values():
            f()
        torch.cuda.synchronize()
        assert int(summary[1].item()) <= cap
        times = {k: [] for k in calls}
        for _ in range(a.regions):
            for k, f in calls.items():
                times[k].append(region_ms(f, a.reps))
        _, _, rounds = ops.select_dev(nb, rank, live.astype(np.uint8), batch=1)
        med = {k: statistics.median(v) for k, v in times.items()}
        report["results"].append({"r2_gt": t, "records": m, "records_per_snp": m / n, "rounds": rounds, **med,
                                  "nbr_over_score": med["nbr_ms"] / med["score_ms"], "regions_ms": times})
        del raw, hits, nb
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

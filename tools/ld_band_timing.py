"""Time of the band store (ldx_ld_band_dev) and of the stored band's matrix-vector product against the operators that do the
same work without keeping the cells.

    python tools/ld_band_timing.py [--snps 100000] [--haps 5008] [--window 1000000] [--regions 5] [--reps 5] [--no-neighbors]

The panel is synthetic (100 000 x 5008, positions 1 + 500 i; w = 1 Mb: 2 000 neighbours each side).  Timed, INTERLEAVED so that
clock drift hits all alike (each region is `reps` calls between two device events; the median region is reported per call):

    band_store     ldx_ld_band_dev into a preallocated band (layout computed once, outside the timing)
    score_k0       ld_score on the same window: the same passes and matrix work, the cells reduced instead of stored
    matvec_k1/k8   ld_matvec (the band kernel, every cell re-derived) with 1 and 8 right-hand sides
    stored_k1/k8   LDBand.matvec on the stored cells
    cross_score    ld_cross_score(band, band)
    neighbors      ld_neighbors at the smallest positive float32 bound, once per region: the same information the old way
                   (16-byte records in both orientations plus the sort into a CSR)

The store's extra over score_k0 is compared with the time HBM needs to take the cells (4 bytes per pair), the stored
products with the time it needs to deliver them.  One JSON object is printed (and written to --out).
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

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, read or write
MFMA_FP4_PEAK_TOPS = 10000.0   # bench.py


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
    ap.add_argument("--window", type=int, default=1_000_000)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-neighbors", action="store_true", help="leave the ld_neighbors comparison out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, h, w = a.snps, a.haps, a.window
    lib = _lib.lib
    p = PackedPanel.from_codes(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev), dev)
    pos_h = synth.synth_positions(n, step=500)
    pos = torch.as_tensor(pos_h).to(dev)
    band = ops.ld_band(p, pos, window_bp=w, check_positions=False)
    pairs = band.n_cells
    ws_band = torch.empty(lib.ldx_ld_band_workspace_bytes(n, h), dtype=torch.uint8, device=dev)
    ws_score = torch.empty(lib.ldx_ld_score_workspace_bytes(n, h), dtype=torch.uint8, device=dev)
    ws_prod = torch.empty(lib.ldx_ld_matvec_workspace_bytes(n, h), dtype=torch.uint8, device=dev)
    x = torch.as_tensor(np.random.default_rng(5).uniform(-1, 1, (n, 8)).astype(np.float32)).to(dev)
    x1 = x[:, :1].contiguous()

    def store():
        _lib.check(lib.ldx_ld_band_dev(p.alt.data_ptr(), p.acnt.data_ptr(), p.rcnt.data_ptr(), p.fa.data_ptr(), p.fr.data_ptr(),
                                       n, h, pos.data_ptr(), w, ops.PATHS["fp4"], band.lo.data_ptr(), band.offsets.data_ptr(),
                                       band.values.data_ptr(), pairs, ws_band.data_ptr(), ws_band.numel(), _stream_ptr()),
                   "ldx_ld_band_dev")

    calls = {
        "band_store": store,
        "score_k0": lambda: ops.ld_score(p, pos, window_bp=w, workspace=ws_score, check_positions=False),
        "matvec_k1": lambda: ops._matvec_launch(p, pos, w, x1, 1, ops.PATHS["fp4"], ws_prod),
        "matvec_k8": lambda: ops._matvec_launch(p, pos, w, x, 1, ops.PATHS["fp4"], ws_prod),
        "stored_k1": lambda: band._matvec_launch(x1, 1),
        "stored_k8": lambda: band._matvec_launch(x, 1),
        "cross_score": lambda: ops.ld_cross_score(band, band),
    }
    reps = {k: a.reps for k in calls}
    if not a.no_neighbors:
        tiny = float(np.nextafter(np.float32(0), np.float32(1)))
        cap = 2 * pairs + pairs // 16 + (1 << 20)
        calls["neighbors"] = lambda: ops.ld_neighbors(p, pos, window_bp=w, r2=tiny, hit_capacity=cap, check_positions=False)
        reps["neighbors"] = 1
    for k, f in calls.items():   # warm-up
        for _ in range(1 if k == "neighbors" else 2):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.regions):
        for k, f in calls.items():
            times[k].append(region_ms(f, reps[k]))
    med = {k: statistics.median(v) for k, v in times.items()}
    cell_bytes = 4.0 * pairs
    extra_ms = med["band_store"] - med["score_k0"]
    floor_ms = cell_bytes / (HBM_PEAK_GBS * 1e9) * 1e3
    ops_band = 2.0 * h * pairs
    report = {
        "snps": n, "haps": h, "window": w, "pairs_in_window": pairs, "bytes_per_pair": 4.0,
        "layout_bytes_per_snp": 12.0, "band_bytes": cell_bytes,
        "timing": f"median of {a.regions} interleaved regions (HIP events), ms per call", "median_ms": med, "regions_ms": times,
        "store_over_score": med["band_store"] / med["score_k0"],
        "store_extra_ms": extra_ms, "hbm_write_floor_ms": floor_ms,
        "store_extra_write_gbs": cell_bytes / (extra_ms * 1e-3) / 1e9 if extra_ms > 0 else None,
        "store_roofline": {"bound": "mfma", "achieved": ops_band / (med["band_store"] * 1e-3) / 1e12, "peak": MFMA_FP4_PEAK_TOPS,
                           "unit": "TOP/s", "frac": ops_band / (med["band_store"] * 1e-3) / 1e12 / MFMA_FP4_PEAK_TOPS},
        "stored_matvec": {
            f"k{k}": {"ms": med[f"stored_k{k}"], "band_kernel_ms": med[f"matvec_k{k}"],
                      "speedup": med[f"matvec_k{k}"] / med[f"stored_k{k}"],
                      "read_gbs": cell_bytes / (med[f"stored_k{k}"] * 1e-3) / 1e9,
                      "frac_of_hbm": cell_bytes / (med[f"stored_k{k}"] * 1e-3) / 1e9 / HBM_PEAK_GBS} for k in (1, 8)},
        "cross_score_read_gbs": cell_bytes / (med["cross_score"] * 1e-3) / 1e9,
    }
    if "neighbors" in med:
        report["neighbors_over_store"] = med["neighbors"] / med["band_store"]
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

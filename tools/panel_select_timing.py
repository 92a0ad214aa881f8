"""Time of PackedPanel.select against what a user does without it: keep the int8 code matrix resident, index_select it, and
pack the result (PackedPanel.pack_from).

    python tools/panel_select_timing.py [--snps 100000] [--haps 5008] [--regions 5] [--reps 5] [--out FILE]

The panel is synthetic 100 000 x 5008.  Three haplotype selections: 1008 of 5008 as one contiguous block, 1008 at random, and
5008 drawn with repeats (a bootstrap).  For each, two calls are timed INTERLEAVED (select, gather-and-repack, select, ...) so
that clock drift hits both alike: each region is `reps` calls between two device events, and the median region over
`regions` is reported per call.  Both calls write into panels made once, read device-resident indices and end with the
per-SNP statistics; nothing is read back inside a region.  The select call is the C entry plus ldx_snp_stats_dev, as
PackedPanel.select runs them after its host-side index check.  Bytes: the algorithmic traffic of a selection is the source
planes once plus the destination planes once; of gather-and-repack, the gathered codes read, written and read again plus the
destination planes.  One JSON object is printed (and written to --out).
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

from ld_tools_amd import PackedPanel, _lib, synth  # noqa: E402


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
    ap.add_argument("--subset", type=int, default=1008)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, h, k = a.snps, a.haps, a.subset
    L = _lib.lib
    codes = synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, device=dev)
    p = PackedPanel.from_codes(codes, dev)
    rng = np.random.default_rng(1)
    start = (h - k) // 2
    selections = {
        "block": np.arange(start, start + k),
        "random": np.sort(rng.choice(h, size=k, replace=False)),
        "bootstrap": rng.integers(0, h, size=h),
    }
    stream = torch.cuda.current_stream().cuda_stream
    report = {"snps": n, "haps": h, "subset": k, "lib": str(_lib.LIB_PATH),
              "timing": f"median of {a.regions} interleaved regions of {a.reps} calls (HIP events), ms per call",
              "selections": {}}
    for name, cols in selections.items():
        m = int(cols.size)
        idx32 = torch.from_numpy(cols.astype(np.uint32).view(np.int32)).to(dev)
        idx64 = torch.from_numpy(cols.astype(np.int64)).to(dev)
        out_sel, out_ref = PackedPanel.empty(n, m, dev), PackedPanel.empty(n, m, dev)
        gathered = torch.empty((n, m), dtype=torch.int8, device=dev)

        def select():
            _lib.check(L.ldx_panel_select_dev(p.alt.data_ptr(), p.ref.data_ptr(), n, h, None, n, idx32.data_ptr(), m,
                                              out_sel.alt.data_ptr(), out_sel.ref.data_ptr(), out_sel.acnt.data_ptr(),
                                              out_sel.rcnt.data_ptr(), stream), "ldx_panel_select_dev")
            out_sel.refresh_stats()

        def repack():
            torch.index_select(codes, 1, idx64, out=gathered)
            out_ref.pack_from(gathered)

        calls = {"select": select, "gather_repack": repack}
        for f in calls.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        same = all(torch.equal(getattr(out_sel, f), getattr(out_ref, f)) for f in ("alt", "ref", "acnt", "rcnt", "fa", "fr", "q"))
        via_method = p.select(haplotypes=cols)
        same = same and torch.equal(via_method.alt, out_ref.alt) and torch.equal(via_method.rcnt, out_ref.rcnt)
        times = {c: [] for c in calls}
        for _ in range(a.regions):
            for c, f in calls.items():
                times[c].append(region_ms(f, a.reps))
        med = {c: statistics.median(v) for c, v in times.items()}
        pb_src, pb_dst = L.ldx_plane_bytes(n, h), L.ldx_plane_bytes(n, m)
        sel_bytes = 2 * (pb_src + pb_dst)
        ref_bytes = 3 * n * m + 2 * pb_dst
        report["selections"][name] = {
            "n_hap_dst": m, "identical_to_repack": bool(same), "median_ms": med, "regions_ms": times,
            "select_bytes": sel_bytes, "select_GBps": sel_bytes / med["select"] / 1e6,
            "gather_repack_bytes": ref_bytes, "gather_repack_GBps": ref_bytes / med["gather_repack"] / 1e6,
            "select_over_gather_repack": med["select"] / med["gather_repack"],
        }
        del out_sel, out_ref, gathered
    report["resident_bytes"] = {"planes": 2 * L.ldx_plane_bytes(n, h), "codes": n * h}
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

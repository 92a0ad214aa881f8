"""Time of the genotype QC operators (ops.geno_group_counts, ld_hardy, ld_model) on one card:

    python tools/ld_qc_timing.py [--inds 2504] [--snps 100000] [--miss 0.03] [--groups 1,3,8,32] [--reps 9] [--warmup 2] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  The panel is synthetic (synth.synth_codes_device, seeded).
  (a) geno_group_counts with 1, 3, 8 and 32 random groups -- one launch of ldx_geno_group_counts_dev between two device events --
      against the only way to get those integers without it: one PackedPanel.select of the group's haplotypes plus one
      geno_snp_counts per group (``select_loop``; both timed end to end with their host-side index checks, which is what a user
      pays), interleaved rep by rep.  The 1-group case (everybody) is also timed against geno_snp_counts alone.  Before timing,
      the two routes are compared for equality.  ``group_counts_launch`` is the launch alone, its member table and output already
      on the device; with that time: the bytes the kernel must move (both planes once, the counts
      once) and their share of the HBM rate (8 TB/s datasheet, 6.29 TB/s measured copy rate: MI355X figures), and the AND + popcount
      pairs it executes.
  (b) ld_hardy for 3 groups (all, cases, controls): the counts launch plus the exact-test launch on n_snps x 3 tuples.
  (c) ld_model: the counts launch for cases and controls, the chi-square launch and Fisher's exact test on the allele counts.
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

from ld_tools_amd import PackedPanel, geno_group_counts, geno_snp_counts, ld_hardy, ld_model, synth  # noqa: E402
from ld_tools_amd._lib import check, lib  # noqa: E402
from ld_tools_amd.ops import _groups_member  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12      # bytes / s: datasheet, and the measured float4 copy rate


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def group_matrix(n_groups, n_ind, seed):
    rng = np.random.default_rng(seed)
    g = rng.random((n_groups, n_ind)) < rng.uniform(0.2, 0.8, size=(n_groups, 1))
    g[0] = True
    return g


def select_loop(panel, groups):
    out = []
    for g in groups:
        rows = np.flatnonzero(g)
        out.append(geno_snp_counts(panel.select(haplotypes=np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1))))
    return torch.stack(out, dim=1)


def counts_scan(panel, n_groups, a):
    groups = group_matrix(n_groups, panel.n_ind, n_groups)
    one = geno_group_counts(panel, groups)[0]
    if not torch.equal(one, select_loop(panel, groups)):
        raise SystemExit(f"{n_groups} groups: the one-pass counts differ from the select + count loop")
    for _ in range(a.warmup):
        geno_group_counts(panel, groups)
        select_loop(panel, groups)
    torch.cuda.synchronize()
    # the launch alone, on a member table and an output that are already on the device
    member = torch.from_numpy(_groups_member("ld_qc_timing", groups, panel.n_ind)[0].view(np.int32)).to(panel.device)
    raw = torch.empty_like(one)

    def launch():
        check(lib.ldx_geno_group_counts_dev(panel.alt.data_ptr(), panel.ref.data_ptr(), panel.n_snps, panel.n_hap, None,
                                            member.data_ptr(), n_groups, raw.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "ldx_geno_group_counts_dev")

    launch()
    if not torch.equal(raw, one):
        raise SystemExit("the raw launch differs from the operator")
    times = {"group_counts": [], "group_counts_launch": [], "select_loop": [], "snp_counts": []}
    for _ in range(a.reps):   # interleaved
        times["group_counts"].append(event_ms(lambda: geno_group_counts(panel, groups)))
        times["group_counts_launch"].append(event_ms(launch))
        times["select_loop"].append(event_ms(lambda: select_loop(panel, groups)))
        if n_groups == 1:
            times["snp_counts"].append(event_ms(lambda: geno_snp_counts(panel)))
    out = {"measurement": "geno_group_counts", "n_groups": n_groups, "n_ind": panel.n_ind, "n_snps": panel.n_snps}
    out.update({k: stats(ms) for k, ms in times.items() if ms})
    ms, call_ms = out["group_counts_launch"]["median_ms"], out["group_counts"]["median_ms"]
    plane = lib.ldx_plane_bytes(panel.n_snps, panel.n_hap)
    moved = 2 * plane + panel.n_snps * n_groups * 16
    words = 2 * plane // 8                                    # 32-bit words of one plane pair = genotype words
    out.update(bytes_moved=moved, bytes_per_s=moved / (ms * 1e-3), share_of_hbm_spec=moved / (ms * 1e-3) / HBM_SPEC,
               share_of_hbm_copy_rate=moved / (ms * 1e-3) / HBM_COPY, and_popcount_pairs=3 * words * n_groups,
               and_popcount_pairs_per_s=3 * words * n_groups / (ms * 1e-3), ratio_select_loop_over_group_counts=out["select_loop"]["median_ms"] / call_ms)
    if n_groups == 1:
        out["ratio_group_counts_over_snp_counts"] = call_ms / out["snp_counts"]["median_ms"]
    return out


def operator_scan(name, fn, a, **more):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    out = {"measurement": name, **more}
    out.update(stats([event_ms(fn) for _ in range(a.reps)]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inds", type=int, default=2504)
    ap.add_argument("--snps", type=int, default=100000)
    ap.add_argument("--miss", type=float, default=0.03)
    ap.add_argument("--groups", default="1,3,8,32")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 3:
        raise SystemExit("--reps must be at least 3")
    if not torch.cuda.is_available():
        raise SystemExit("ld_qc_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    codes = synth.synth_codes_device(a.snps, 2 * a.inds, seed=synth.BENCH_SEED, miss=a.miss, device=dev)[:, :2 * a.inds].contiguous()
    panel = PackedPanel.from_codes(codes, dev)
    del codes
    report = {"timing": "one HIP event pair around each call, ms, medians of --reps calls after --warmup calls", "miss": a.miss,
              "lib": str(lib._name), "results": []}

    def add(item):
        report["results"].append(item)
        print(json.dumps(item), flush=True)

    for n_groups in (int(v) for v in a.groups.split(",")):
        add(counts_scan(panel, n_groups, a))
    rng = np.random.default_rng(5)
    case = (rng.random(a.inds) < 0.5).astype(np.float64)
    three = np.stack([np.ones(a.inds, dtype=bool), case == 1.0, case == 0.0])
    add(operator_scan("ld_hardy", lambda: ld_hardy(panel, three), a, n_groups=3, tuples=3 * a.snps))
    add(operator_scan("ld_hardy_counts_only", lambda: geno_group_counts(panel, three), a, n_groups=3))
    add(operator_scan("ld_model", lambda: ld_model(panel, case), a, tuples=a.snps))
    add(operator_scan("ld_model_without_fisher", lambda: ld_model(panel, case, fisher=False), a, tuples=a.snps))
    text = json.dumps(report)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

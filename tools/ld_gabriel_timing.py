"""Time of the Gabriel operators (ops.ld_dprime_ci, ops.ld_gabriel_blocks; ldx_emband.hip Op kCi, ldx_gabriel.hip) against
ops.ld_em_band on the same panel and window: the band that already carries the maximum-likelihood D' is the yardstick for
what the 101-point likelihood surface per pair adds.

    python tools/ld_gabriel_timing.py [--snps 20000] [--haps 5008] [--window-snps 500] [--reps 10] [--warmup 2] [--miss 0.02]
                                      [--out FILE]

tools/ld_emband_timing.py's protocol and panels: no_holes in the plain form, all_holes (--miss of the codes missing in every
SNP) with missing="pairwise".  Runs on a GPU only.  One process, one device; each operator and ld_em_band are ALTERNATED call
by call, every call between two device events of its own, so the times are those of the whole ops call (layout, plan,
allocations, the per-SNP stats, the one host read of the layout's total; ld_gabriel_blocks: also the candidates, the sort and
the pick, but not the fetch of the result).  Before timing, a second ld_dprime_ci call must give the same bytes and the blocks
must be disjoint runs of kept SNPs; the cells themselves are the tests' business (tests/test_gpu_ld_gabriel.py).  Reported
per panel: ms, quartiles and the ratios to ld_em_band.  No threshold is applied to the times: one JSON object is printed (and
written to --out).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ld_emband_timing import PW, alternated, tiles_walked  # noqa: E402
from ld_tools_amd import PackedPanel, ops, synth  # noqa: E402


def one_panel(kind, missing, n, h, w, miss, reps, warmup, dev):
    codes = synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, miss=miss, device=dev)
    panel = PackedPanel.from_codes(codes, dev)
    del codes

    def band():
        return ops.ld_em_band(panel, window_snps=w, missing=missing)

    def ci():
        return ops.ld_dprime_ci(panel, window_snps=w, missing=missing)

    def blocks():
        return ops.ld_gabriel_blocks(panel, window_snps=w, missing=missing)

    a, b = ci(), ci()
    if not (torch.equal(a.lo, b.lo) and torch.equal(a.hi, b.hi)):
        raise SystemExit(f"{kind}: two ld_dprime_ci calls differ")
    with_interval = int((a.lo != ops.NO_CI).sum())
    if not bool((a.lo[a.lo != ops.NO_CI] <= a.hi[a.lo != ops.NO_CI]).all()):
        raise SystemExit(f"{kind}: a lower bound above its upper bound")
    n_cells, kept = a.n_cells, int(a.kept.sum())
    strong, recombinant = int(a.strong(70).sum()), int(a.recombinant().sum())
    del a, b
    res = blocks()
    block_of = res.block_of
    member = block_of < ops.NO_BLOCK
    if res.n_blocks and not (np.diff(block_of[member].astype(np.int64)) >= 0).all():
        raise SystemExit(f"{kind}: the blocks are not numbered in position order")
    report = {"panel": kind, "missing": missing, "n_snps": n, "n_hap": h, "window_snps": w, "miss": miss, "band_cells": n_cells,
              "kept_snps": kept, "cells_with_interval": with_interval, "strong_pairs_70": strong, "recombinant_pairs": recombinant,
              "tiles_walked": tiles_walked(n, w), "n_blocks": res.n_blocks, "n_candidates": res.n_candidates,
              "snps_in_blocks": int(member.sum()), "largest_block": int(res.sizes.max()) if res.n_blocks else 0}
    del res
    torch.cuda.empty_cache()
    for name, f in (("ld_dprime_ci", ci), ("ld_gabriel_blocks", blocks)):
        t_op, t_band, q_op, q_band = alternated(f, band, reps, warmup)
        report[name] = {"ms": t_op, "em_band_ms": t_band, "quartiles_ms": q_op, "em_band_quartiles_ms": q_band,
                        "ratio_to_em_band": t_op / t_band, "ns_per_cell": 1e6 * t_op / n_cells}
        torch.cuda.empty_cache()
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=20_000)
    ap.add_argument("--haps", type=int, default=5008)
    ap.add_argument("--window-snps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--miss", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 4:
        raise SystemExit("--reps must be at least 4")
    if a.haps % 2:
        raise SystemExit("--haps must be even: the EM pairs haplotypes into individuals")
    if not torch.cuda.is_available():
        raise SystemExit("ld_gabriel_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    report = {"timing": "one HIP event pair per ops call, the operator and ld_em_band alternated call by call, medians, ms",
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

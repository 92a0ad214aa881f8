"""Time of sample relatedness (ops.sample_counts: ldx_sample_planes_dev + ldx_sample_counts_dev) against the same products as
torch.matmul on fp16 0/1 matrices, on one card, on two kinds of synthetic panel:

    no_holes    a panel without a missing call: every tile takes the shortcut (3 MFMAs per 32 x 32 tile and 64 SNPs)
    holes       missing calls (--miss, default 3 %) in every individual: every tile runs the general loop (6 MFMAs)

    python tools/king_timing.py [--inds 2504] [--snps 100000,1000000] [--reps 20] [--warmup 2] [--miss 0.03] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  Three regions, each between two device events of its own and
INTERLEAVED rep by rep so that clock drift hits all alike: `planes` (the transposition of the whole panel, one store per
SAMPLE_STORE_SNPS SNPs), `counts` (the count kernel over those stores, accumulating) and `torch` (the baseline: the individual x
SNP indicator matrices called c, het t, hom-REF n, hom-ALT z as fp16, built before the clock starts, and five matmuls with an
fp32 result -- c c', t t', t c', n z', z n'; c t' is the transpose of t c'; torch.mm's out_dtype, or where this torch has none,
K blocks of 2048 summed in fp32: the report says which).  Before timing, the four count planes are
compared with the baseline's products, every cell (both are exact integers below 2^24).  No threshold is applied to the times:
one JSON object with the medians, the ratio torch / (planes + counts) and the count kernel's MFMA rate (2 ops per MAC of the
instructions it issues on lower tiles, for comparison with what tools/probes/fp4rate.hip prints) is printed (and written to
--out)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from ld_tools_amd import PackedPanel, ops, synth  # noqa: E402
from ld_tools_amd._lib import check, lib  # noqa: E402
from ld_tools_amd.panel import _stream_ptr  # noqa: E402

CHUNK = 65536   # SNPs per step while the fp16 matrices are built


def region_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def indicator_matrices(codes, n_ind, dev):
    """fp16 [n_ind, n_snps] x 4: called, het, hom-REF, hom-ALT of every individual, from the int8 codes [n_snps, n_hap]."""
    n_snps = codes.shape[0]
    out = [torch.empty((n_ind, n_snps), dtype=torch.float16, device=dev) for _ in range(4)]
    for s in range(0, n_snps, CHUNK):
        c = codes[s:s + CHUNK, :2 * n_ind]
        h0, h1 = c[:, 0::2], c[:, 1::2]
        called = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1))
        g = (h0 == 1).to(torch.int8) + (h1 == 1).to(torch.int8)
        for m, x in zip(out, (called, called & (g == 1), called & (g == 0), called & (g == 2))):
            m[:, s:s + CHUNK] = x.T.to(torch.float16)
    return out


def one_panel(kind, n_ind, n_snps, miss, reps, warmup, dev):
    codes = synth.synth_codes_device(n_snps, 2 * n_ind, seed=synth.BENCH_SEED, miss=miss, device=dev)[:, :2 * n_ind]
    panel = PackedPanel.from_codes(codes, dev)
    c, t, n, z = indicator_matrices(codes, n_ind, dev)
    del codes
    step = ops.SAMPLE_STORE_SNPS
    spans = [(b, min(step, n_snps - b)) for b in range(0, n_snps, step)]
    stores = [torch.empty(lib.ldx_sample_planes_bytes(n_ind, cnt), dtype=torch.uint8, device=dev) for _, cnt in spans]
    tables = [torch.empty(lib.ldx_sample_tables_bytes(n_ind) // 4, dtype=torch.int32, device=dev) for _ in spans]
    counts = torch.empty((4, n_ind, n_ind), dtype=torch.int32, device=dev)

    def planes():
        for (begin, cnt), st, tb in zip(spans, stores, tables):
            check(lib.ldx_sample_planes_dev(panel.alt.data_ptr(), panel.ref.data_ptr(), n_snps, panel.n_hap, None, begin, cnt,
                                            st.data_ptr(), tb.data_ptr(), _stream_ptr()), "ldx_sample_planes_dev")

    def count():
        done = 0
        for (_, cnt), st, tb in zip(spans, stores, tables):
            check(lib.ldx_sample_counts_dev(st.data_ptr(), tb.data_ptr(), n_ind, cnt, counts.data_ptr(), n_ind, int(done > 0), done, 0,
                                            _stream_ptr()), "ldx_sample_counts_dev")
            done += cnt

    prods = [None] * 5
    pairs = ((c, c), (t, t), (t, c), (n, z), (z, n))

    def mm_f32():       # fp16 operands, fp32 result: a plain fp16 result would round the counts (and overflow past 65504)
        for k, (x, y) in enumerate(pairs):
            prods[k] = torch.mm(x, y.T, out_dtype=torch.float32)

    def mm_blocked():   # where mm has no fp32 result: K blocks of 2048 (an fp16 result is exact up to 2048), summed in fp32
        for k, (x, y) in enumerate(pairs):
            acc = torch.zeros((n_ind, n_ind), dtype=torch.float32, device=dev)
            for s in range(0, n_snps, 2048):
                acc += x[:, s:s + 2048] @ y[:, s:s + 2048].T
            prods[k] = acc

    try:
        mm_f32()
        baseline, form = mm_f32, "torch.mm(fp16, fp16, out_dtype=float32)"
    except (RuntimeError, TypeError):
        baseline, form = mm_blocked, "fp16 matmuls over K blocks of 2048, summed in fp32"
    planes(), count(), baseline()
    torch.cuda.synchronize()
    want = [prods[0], prods[1], prods[3] + prods[4], prods[2]]
    for k, (name, w) in enumerate(zip(ops.SAMPLE_COUNTS, want)):
        differ = int((counts[k].to(torch.float32) != w.to(torch.float32)).sum())
        if differ:
            raise SystemExit(f"{kind} {n_ind} x {n_snps}: {differ} cells of {name} differ from the torch products")
    holes = int((tables[0][:n_ind] != tables[0][tables[0].numel() - 4]).sum())   # called kept SNPs against the kept SNPs
    for _ in range(warmup):
        planes(), count(), baseline()
    torch.cuda.synchronize()
    t_planes, t_counts, t_torch = [], [], []
    for _ in range(reps):   # interleaved
        t_planes.append(region_ms(planes))
        t_counts.append(region_ms(count))
        t_torch.append(region_ms(baseline))
    sp, sc, st = stats(t_planes), stats(t_counts), stats(t_torch)
    tiles = (n_ind + 127) // 128
    mfma_per_step = 6 if holes else 3
    steps = sum((cnt + 255) // 256 * 4 for _, cnt in spans)
    ops_issued = tiles * (tiles + 1) // 2 * 16 * steps * mfma_per_step * (32 * 32 * 64 * 2)
    return {"panel": kind, "n_ind": n_ind, "n_snps": n_snps, "miss": miss, "individuals_with_holes_in_first_store": holes,
            "stores": len(spans), "planes": sp, "counts": sc, "torch_fp16_5_matmuls": st, "torch_form": form,
            "ratio_torch_over_planes_plus_counts": st["median_ms"] / (sp["median_ms"] + sc["median_ms"]),
            "ratio_torch_over_counts": st["median_ms"] / sc["median_ms"],
            "counts_mfma_tops": ops_issued / (sc["median_ms"] * 1e-3) / 1e12, "mfma_per_tile_step": mfma_per_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inds", type=int, default=2504)
    ap.add_argument("--snps", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--miss", type=float, default=0.03)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("king_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    report = {"timing": "one HIP event pair per region, the three regions interleaved rep by rep, ms", "panels": []}
    for n_snps in (int(x) for x in a.snps.split(",")):
        for kind, miss in (("no_holes", 0.0), ("holes", a.miss)):
            report["panels"].append(one_panel(kind, a.inds, n_snps, miss, a.reps, max(1, a.warmup), dev))
            torch.cuda.empty_cache()
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

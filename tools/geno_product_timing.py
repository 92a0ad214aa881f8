"""Time of the genotype products (ops.GenoOperator: ldx_geno_matmul_dev, ldx_geno_rmatmul_dev) and of what is built on them, against
torch.mm on float32 dosage and called matrices, on one card, on two kinds of synthetic panel (no missing call / --miss, default 3 %):

    python tools/geno_product_timing.py [--inds 2504] [--snps 100000,1000000] [--k 20] [--reps 10] [--warmup 2] [--miss 0.03]
                                        [--no-pca] [--out FILE]

Runs on a GPU only (there is nothing to fall back to).  Regions, each between two device events of its own and INTERLEAVED rep by
rep so that clock drift hits all alike:
    store      the transposed store of the whole panel (ldx_sample_planes_dev), which GenoOperator builds once
    forward    matmul_q(q_w, q_wc): k columns of random int32 weights          torch: G32 @ W + C32 @ Wc  (float32, built beforehand)
    reverse    rmatmul_q(q_u)                                                torch: G32.T @ U and C32.T @ U
    kq         one application K Q of sample_pca (quantise, reverse, elementwise fp64, quantise, forward, read back), k columns
and, once per panel (a host clock around work that ends in a synchronise), sample_pca at its defaults.  Before timing the integer
products are compared with float64 products of the same matrices on the first 20 000 SNPs (exact there: every sum is below 2^53).  The float32 baseline is NOT exact
(its sums round); it is the speed yardstick tools/king_timing.py uses for its products.  No threshold is applied: one JSON object
with the medians, the ratios torch / ours, and the achieved shares of the HBM bandwidth (the bytes of the planes each product
has to read, once) and of the int8 MFMA rate (2 ops per MAC of the instructions issued) is printed (and written to --out)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ld_tools_amd import GenoOperator, PackedPanel, geno_quantize, ops, sample_pca, synth  # noqa: E402

HBM_BYTES_PER_S = 8.0e12       # MI355X datasheet
INT8_MFMA_OPS_PER_S = 5.0e15   # MI355X datasheet, dense int8
CHUNK = 65536


def region_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def float_matrices(codes, n_ind, dev):
    """float32 [n_snps, n_ind] x 2: the dosage of the called genotypes and the called flag."""
    n_snps = codes.shape[0]
    g32 = torch.empty((n_snps, n_ind), dtype=torch.float32, device=dev)
    c32 = torch.empty((n_snps, n_ind), dtype=torch.float32, device=dev)
    for s in range(0, n_snps, CHUNK):
        c = codes[s:s + CHUNK, :2 * n_ind]
        h0, h1 = c[:, 0::2], c[:, 1::2]
        called = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1))
        g32[s:s + CHUNK] = ((h0 == 1).to(torch.float32) + (h1 == 1).to(torch.float32)) * called
        c32[s:s + CHUNK] = called.to(torch.float32)
    return g32, c32


def one_panel(kind, n_ind, n_snps, k, miss, reps, warmup, with_pca, dev):
    codes = synth.synth_codes_device(n_snps, 2 * n_ind, seed=synth.BENCH_SEED, miss=miss, device=dev)[:, :2 * n_ind]
    panel = PackedPanel.from_codes(codes, dev)
    g32, c32 = float_matrices(codes, n_ind, dev)
    del codes
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda n: torch.randint(-(1 << 30), (1 << 30) + 1, (n, k), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)  # noqa: E731
    q_w, q_wc, q_u = rnd(n_snps), rnd(n_snps), rnd(n_ind)
    w32, wc32, u32 = (x.to(torch.float32) for x in (q_w, q_wc, q_u))
    op = GenoOperator(panel)

    def store():
        GenoOperator(panel)

    # exactness against float64 products of the same matrices on the first SNPs: every term is an integer below 2^31 and every
    # sum below 3 x 2^30 x 20000 < 2^53, so float64 is exact there
    head = min(n_snps, 20000)
    f64 = lambda x: x.to(torch.float64)  # noqa: E731
    z, zc = op.rmatmul_q(q_u)
    for got, m in ((z, g32), (zc, c32)):
        if not torch.equal(got[:head], (f64(m[:head]) @ f64(q_u)).to(torch.int64)):
            raise SystemExit(f"{kind} {n_ind} x {n_snps}: the reverse product differs from the float64 product")
    small = GenoOperator(panel.select(snps=np.arange(head))) if head < n_snps else op
    want = (f64(g32[:head]).T @ f64(q_w[:head]) + f64(c32[:head]).T @ f64(q_wc[:head])).to(torch.int64)
    if not torch.equal(small.matmul_q(q_w[:head].contiguous(), q_wc[:head].contiguous()), want):
        raise SystemExit(f"{kind} {n_ind} x {n_snps}: the forward product differs from the float64 product")
    del small

    Q = np.linalg.qr(np.random.default_rng(0).standard_normal((n_ind, k)))[0]
    n_i, a_i = (x.to(torch.float64) for x in op.stats())
    tp = torch.where(n_i > 0, a_i / torch.clamp(n_i, min=1.0), torch.zeros_like(n_i))[:, None]
    v = tp * (1.0 - tp / 2.0)
    w_d = torch.where(v > 0, 1.0 / torch.clamp(v, min=1e-300), torch.zeros_like(v))

    def kq():   # the steps of sample_pca's K Q (ops._pca), without the division by M
        (q,), e = geno_quantize(Q, device=dev)
        Z, Zc = op.rmatmul_q(q)
        s = ops._pow2(e - 30)[None, :]
        T = (Z.to(torch.float64) * s - tp * (Zc.to(torch.float64) * s)) * w_d
        (q_t, q_c), _ = geno_quantize(T, -(tp * T), device=dev)
        return op.matmul_q(q_t, q_c).cpu()

    regions = {
        "store": store,
        "forward": lambda: op.matmul_q(q_w, q_wc),
        "reverse": lambda: op.rmatmul_q(q_u),
        "kq": kq,
        "torch_forward": lambda: torch.mm(g32.T, w32) + torch.mm(c32.T, wc32),
        "torch_reverse": lambda: (torch.mm(g32, u32), torch.mm(c32, u32)),
    }
    for _ in range(warmup):
        for fn in regions.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in regions}
    for _ in range(reps):   # interleaved
        for name, fn in regions.items():
            times[name].append(region_ms(fn))
    out = {name: stats(ms) for name, ms in times.items()}
    med = {name: s["median_ms"] * 1e-3 for name, s in out.items()}
    slabs, blocks, groups = (n_ind + 127) // 128, (n_snps + 255) // 256, (k + 31) // 32
    tiles = (k + 7) // 8                                                    # 32-column MFMA tiles: 8 real columns x 4 limbs
    fwd_bytes = 3 * slabs * 128 * blocks * 32 + 2 * n_snps * k * 4          # the three planes once, w and wc once
    rev_bytes = 2 * ((n_snps + 127) // 128) * 128 * ((2 * n_ind + 255) // 256) * 32 * groups + 2 * n_snps * k * 8
    fwd_ops = slabs * 4 * blocks * 8 * tiles * 2 * (32 * 32 * 32 * 2)
    rev_ops = ((n_snps + 127) // 128) * 4 * ((2 * n_ind + 255) // 256) * 4 * tiles * 2 * (32 * 32 * 32 * 2)
    res = {"panel": kind, "n_ind": n_ind, "n_snps": n_snps, "k": k, "miss": miss, "stores": len(op._stores), **out,
           "ratio_torch_over_forward": med["torch_forward"] / med["forward"],
           "ratio_torch_over_reverse": med["torch_reverse"] / med["reverse"],
           "forward_hbm_share": fwd_bytes / med["forward"] / HBM_BYTES_PER_S,
           "reverse_hbm_share": rev_bytes / med["reverse"] / HBM_BYTES_PER_S,
           "forward_mfma_share": fwd_ops / med["forward"] / INT8_MFMA_OPS_PER_S,
           "reverse_mfma_share": rev_ops / med["reverse"] / INT8_MFMA_OPS_PER_S}
    if with_pca:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pca = sample_pca(panel)
        torch.cuda.synchronize()
        res["sample_pca_defaults_s"] = time.perf_counter() - t0
        res["sample_pca_top_eigenvalues"] = pca.eigenvalues[:3].tolist()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inds", type=int, default=2504)
    ap.add_argument("--snps", default="100000,1000000")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--miss", type=float, default=0.03)
    ap.add_argument("--no-pca", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("geno_product_timing needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", 0)
    report = {"timing": "one HIP event pair per region, the regions interleaved rep by rep, ms; sample_pca: host clock, s",
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "int8_mfma_ops_per_s": INT8_MFMA_OPS_PER_S, "panels": []}
    for n_snps in (int(x) for x in a.snps.split(",")):
        for kind, miss in (("no_holes", 0.0), ("holes", a.miss)):
            report["panels"].append(one_panel(kind, a.inds, n_snps, a.k, miss, a.reps, max(1, a.warmup), not a.no_pca, dev))
            torch.cuda.empty_cache()
            print(json.dumps(report["panels"][-1]), flush=True)
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

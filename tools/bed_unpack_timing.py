"""Time of the .bed unpack against what a user does without it: keep the int8 code matrix resident and pack it
(PackedPanel.pack_from), with and without a subset of half the individuals; and the time of the .bed pack.

    python tools/bed_unpack_timing.py [--shapes 100000x2504,20000x5120] [--regions 7] [--reps 100] [--out FILE]

Per shape (SNPs x individuals) the panel is synthetic: codes with LD blocks brought to the canonical form of a .bed (hets as
(1, 0), missing calls as whole genotypes), packed once; its .bed bytes come from ldx_bed_pack_dev and sit in device memory
behind a 3-byte header, so the unpack reads at base + 3 as it would from a whole file.  Timed calls, all from resident data
into panels made once, each ending with the per-SNP statistics:
    unpack        ldx_bed_unpack_dev, identity                      bytes: the rows once + both planes once
    pack_from     ldx_pack_codes_dev of the int8 codes              bytes: the codes once + both planes once
    unpack_keep   ldx_bed_unpack_dev with an index of N / 2         bytes: the rows once + both planes of the subset once
    gather_pack   index_select of the codes' columns + pack_from    bytes: the gathered codes read, written, read + planes
    bed_pack      ldx_bed_pack_dev                                  bytes: both planes once + the rows once
The calls are timed INTERLEAVED (clock drift hits all alike): a region is `reps` calls between two device events, the median
region over `regions` is reported per call, after two warm-up calls each.  GB/s is bytes / median time; `hbm_fraction` is that
over the 8.0 TB/s of the MI355X's HBM3E.  The unpacked panels are compared with the packed ones before anything is timed.
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

from ld_tools_amd import PackedPanel, _lib, synth  # noqa: E402

HBM_PEAK = 8.0e12
FIELDS = ("alt", "ref", "acnt", "rcnt", "fa", "fr", "q")


def region_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def canonical(codes):
    """The codes a .bed can hold, on the device: a het as (1, 0), a call with any other code as (2, 2)."""
    x, y = codes[:, 0::2], codes[:, 1::2]
    ok = (x >= 0) & (x < 2) & (y >= 0) & (y < 2)
    het = ok & (x != y)
    out = torch.empty_like(codes)
    out[:, 0::2] = torch.where(ok, torch.where(het, torch.ones_like(x), x), torch.full_like(x, 2))
    out[:, 1::2] = torch.where(ok, torch.where(het, torch.zeros_like(y), y), torch.full_like(y, 2))
    return out


def same(p, q):
    return all(torch.equal(getattr(p, f), getattr(q, f)) for f in FIELDS)


def shape_report(n, n_ind, a, dev):
    L = _lib.lib
    stream = torch.cuda.current_stream().cuda_stream
    h, nb = 2 * n_ind, (n_ind + 3) // 4
    codes = canonical(synth.synth_codes_device(n, h, seed=synth.BENCH_SEED, miss=0.01, device=dev))
    ref = PackedPanel.from_codes(codes, dev)
    flat = torch.zeros(3 + n * nb, dtype=torch.uint8, device=dev)
    bed = flat[3:].view(n, nb)

    def bed_pack():
        _lib.check(L.ldx_bed_pack_dev(ref.alt.data_ptr(), ref.ref.data_ptr(), n, h, 0, n, bed.data_ptr(), nb, 0, stream),
                   "ldx_bed_pack_dev")

    bed_pack()
    keep = np.sort(np.random.default_rng(1).choice(n_ind, size=n_ind // 2, replace=False))
    m = int(keep.size)
    idx32 = torch.from_numpy(keep.astype(np.uint32).view(np.int32)).to(dev)
    cols = np.stack([2 * keep, 2 * keep + 1], axis=1).reshape(-1)
    idx64 = torch.from_numpy(cols.astype(np.int64)).to(dev)
    out_u, out_p = PackedPanel.empty(n, h, dev), PackedPanel.empty(n, h, dev)
    out_uk, out_pk = PackedPanel.empty(n, 2 * m, dev), PackedPanel.empty(n, 2 * m, dev)
    gathered = torch.empty((n, 2 * m), dtype=torch.int8, device=dev)

    def unpack_into(out, idx, n_dst):
        _lib.check(L.ldx_bed_unpack_dev(bed.data_ptr(), nb, n_ind, n, None if idx is None else idx.data_ptr(), n_dst, 0, 0, n,
                                        out.alt.data_ptr(), out.ref.data_ptr(), out.acnt.data_ptr(), out.rcnt.data_ptr(),
                                        stream), "ldx_bed_unpack_dev")
        out.refresh_stats()

    def gather_pack():
        torch.index_select(codes, 1, idx64, out=gathered)
        out_pk.pack_from(gathered)

    calls = {"unpack": lambda: unpack_into(out_u, None, n_ind), "pack_from": lambda: out_p.pack_from(codes),
             "unpack_keep": lambda: unpack_into(out_uk, idx32, m), "gather_pack": gather_pack, "bed_pack": bed_pack}
    for f in calls.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    identical = {"unpack_vs_pack_from": same(out_u, out_p) and same(out_u, ref), "unpack_keep_vs_gather_pack": same(out_uk, out_pk),
                 "via_from_bed": same(PackedPanel.from_bed((bed, n_ind), keep=keep), out_pk)}
    times = {c: [] for c in calls}
    for _ in range(a.regions):
        for c, f in calls.items():
            times[c].append(region_ms(f, a.reps))
    med = {c: statistics.median(v) for c, v in times.items()}
    pb, pbk = L.ldx_plane_bytes(n, h), L.ldx_plane_bytes(n, 2 * m)
    nbytes = {"unpack": n * nb + 2 * pb, "pack_from": n * h + 2 * pb, "unpack_keep": n * nb + 2 * pbk,
              "gather_pack": 3 * n * 2 * m + 2 * pbk, "bed_pack": 2 * pb + n * nb}
    rep = {"snps": n, "individuals": n_ind, "kept": m, "identical": identical, "median_ms": med, "regions_ms": times,
           "bytes": nbytes, "GBps": {c: nbytes[c] / med[c] / 1e6 for c in calls},
           "hbm_fraction": {c: nbytes[c] / (med[c] * 1e-3) / HBM_PEAK for c in calls},
           "unpack_over_pack_from": med["unpack"] / med["pack_from"],
           "unpack_keep_over_gather_pack": med["unpack_keep"] / med["gather_pack"],
           "unpack_keep_over_unpack": med["unpack_keep"] / med["unpack"]}
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x2504,20000x5120")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    report = {"lib": str(_lib.LIB_PATH), "hbm_peak_Bps": HBM_PEAK,
              "timing": f"median of {a.regions} interleaved regions of {a.reps} calls (HIP events), ms per call", "shapes": []}
    for shape in a.shapes.split(","):
        n, n_ind = (int(v) for v in shape.split("x"))
        report["shapes"].append(shape_report(n, n_ind, a, dev))
        torch.cuda.empty_cache()
    text = json.dumps(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

"""Panels and a brute-force definition for the Gabriel block tests (tests/test_ld_gabriel_host.py, tests/test_gpu_ld_gabriel.py,
tests/test_gpu_gabriel_drivers.py) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/ld_emband_cases.py.  numpy only;
everything is seeded.

gabriel_panel: SNPs at 0.5 - 6 kb spacing in planted haplotype blocks with free SNPs between them.  Inside a block every
haplotype copies one of 6 founders (drawn per block, so blocks are independent of each other) and SNP s is ALT in the founders
below its depth: nested ALT sets, |D'| = 1 for every pair of the block; about 0.3 % of the codes are then flipped.  Planted on
top: a pair of SNPs 25 kb apart (a two-SNP candidate lost to the span), a sandwich A, X, A' with X free (lost to the 95 % rule),
a rare SNP inside a block (dropped by the MAF rule: between the block's ends and no member), two SNPs at one position, and
missing codes in some rows for the pairwise form.

brute_candidates / brute_pick are sections 3 and 4 of the definition as plain loops over every (first, last) and every pair
inside -- no suffix counts, no sorting tricks.
"""
from __future__ import annotations

import numpy as np

N_PANEL = 300                     # three slabs of 128, the last ragged (44 rows)
WINDOW = 500_000                  # about 150 SNPs each side at the mean spacing: tiles are cut by the window
N_FOUNDERS = 6
FLIP = 0.003
MISS = 0.02
GAP = 25_000
PLAN = (("free", 3), ("block", 2), ("free", 2), ("block", 3), ("free", 2), ("block", 4), ("free", 3), ("block", 5), ("free", 2),
        ("gap", 2), ("free", 2), ("sandwich", 3), ("free", 2), ("rare", 7), ("free", 3), ("dup", 5), ("free", 2), ("block", 9),
        ("free", 3), ("block", 12), ("free", 2))
NOT_KEPT, NO_BLOCK, NO_CI = 0xFFFFFFFF, 0xFFFFFFFE, 0xFF

_CACHE = {}


def gabriel_panel(n_hap: int, n: int = N_PANEL, seed: int = 2002):
    """(codes int8 [n, n_hap], positions int64 [n], planted): ``planted`` maps a kind of PLAN to the list of (first, last) SNP
    ranges it was planted at, and "rare_snp" / "dup_snp" to SNP numbers.  Read-only, built once per process."""
    key = (n_hap, n, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    codes = np.zeros((n, n_hap), dtype=np.int8)
    gaps = rng.integers(500, 6001, size=n).astype(np.int64)
    planted = {"rare_snp": [], "dup_snp": []}
    at, step = 0, 0
    while at < n:
        kind, m = PLAN[step % len(PLAN)]
        if step >= len(PLAN) and kind not in ("free", "block"):
            kind = "block"
        if step >= len(PLAN) and kind == "block":
            m = int(rng.integers(2, 13))
        step += 1
        m = min(m, n - at)
        rows = slice(at, at + m)
        planted.setdefault(kind, []).append((at, at + m - 1))
        if kind == "free":
            freq = rng.uniform(0.08, 0.5, size=m)
            codes[rows] = rng.random((m, n_hap)) < freq[:, None]
        else:
            founder = rng.integers(0, N_FOUNDERS, size=n_hap)
            depth = rng.integers(1, N_FOUNDERS, size=m)
            if kind in ("gap", "sandwich"):
                depth[:] = 3
            codes[rows] = founder[None, :] < depth[:, None]
            if kind == "gap" and m == 2:
                gaps[at + 1] = GAP
            if kind == "sandwich" and m == 3:
                codes[at + 1] = rng.random(n_hap) < 0.4
            if kind == "rare" and m >= 3:
                rare = at + m // 2
                codes[rare] = (founder == 0) & (rng.random(n_hap) < 0.12)   # about 2 % ALT, inside founder 0's carriers
                planted["rare_snp"].append(rare)
            if kind == "dup" and m >= 3:
                gaps[at + 2] = 0
                planted["dup_snp"].append(at + 2)
        at += m
    flips = rng.random(codes.shape) < FLIP
    codes[flips] ^= 1
    holes = rng.random(codes.shape) < MISS
    holes[rng.random(n) < 0.6] = False          # four rows in ten carry missing codes
    for r in planted["rare_snp"] + planted["dup_snp"]:
        holes[r] = False
    codes[holes] = 2
    gaps[0] = 1000
    positions = np.cumsum(gaps)
    codes.setflags(write=False)
    positions.setflags(write=False)
    _CACHE[key] = (codes, positions, planted)
    return _CACHE[key]


def random_panel(n: int, n_hap: int, seed: int = 5):
    """Independent SNPs at 1 kb spacing, no missing codes: few or no blocks expected."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.02, 0.5, size=n)
    codes = (rng.random((n, n_hap)) < freq[:, None]).astype(np.int8)
    return codes, 1000 * np.arange(1, n + 1, dtype=np.int64)


# ---- sections 3 and 4 as plain loops -------------------------------------------------------------------------------------------
DEFAULTS = dict(cand_cut=70, strong_hi=98, recomb_hi=90, cuts=(80, 50, 50, 70), max_spans=(20_000, 30_000, None, None),
                min_informative=(1, 3, 6, 6), strong_share=(19, 20))


def brute_candidates(lo_dense, hi_dense, positions, kept, window: int, **params):
    """(valid, lost): ``valid`` the list of (first, last, span) in (first, last) order, ``lost`` {reason: [(first, last)]} with the
    FIRST rule of section 3 a candidate misses, in the order span, informative, share.  ``lo_dense`` / ``hi_dense``: [n, n]
    bounds (NO_CI where there is none)."""
    p = dict(DEFAULTS, **params)
    pos = np.asarray(positions, dtype=np.int64)
    n = pos.shape[0]
    valid, lost = [], {"span": [], "informative": [], "share": []}

    def strong(i, j, cut):
        return lo_dense[i, j] != NO_CI and lo_dense[i, j] >= cut and hi_dense[i, j] >= p["strong_hi"]

    for first in range(n):
        for last in range(first + 1, n):
            if pos[last] - pos[first] > window:
                break
            if not (kept[first] and kept[last] and strong(last, first, p["cand_cut"])):
                continue
            snps = [s for s in range(first, last + 1) if kept[s]]
            row = min(len(snps), 5) - 2
            n_s = n_r = 0
            for a in range(len(snps)):
                for b in range(a + 1, len(snps)):
                    n_s += bool(strong(snps[b], snps[a], p["cuts"][row]))
                    n_r += bool(hi_dense[snps[b], snps[a]] < p["recomb_hi"])
            span = int(pos[last] - pos[first])
            cap = window if p["max_spans"][row] is None else p["max_spans"][row]
            if span > cap:
                lost["span"].append((first, last))
            elif n_s + n_r < p["min_informative"][row]:
                lost["informative"].append((first, last))
            elif not p["strong_share"][1] * n_s > p["strong_share"][0] * (n_s + n_r):
                lost["share"].append((first, last))
            else:
                valid.append((first, last, span))
    return valid, lost


def brute_pick(valid, n: int, kept):
    """(block_of uint32 [n], accepted [(first, last)] in position order, overlapped [(first, last)])."""
    order = sorted(valid, key=lambda c: (-c[2], c[0], c[1]))
    owner = [None] * n
    accepted, overlapped = [], []
    for first, last, _ in order:
        if any(owner[s] is not None for s in range(first, last + 1)):
            overlapped.append((first, last))
            continue
        for s in range(first, last + 1):
            owner[s] = first
        accepted.append((first, last))
    accepted.sort()
    number = {first: k for k, (first, _) in enumerate(accepted)}
    block_of = np.full(n, NOT_KEPT, dtype=np.uint32)
    for s in range(n):
        if kept[s]:
            block_of[s] = NO_BLOCK if owner[s] is None else number[owner[s]]
    return block_of, accepted, overlapped


def dense_from_band(values, band_lo, offsets, n: int) -> np.ndarray:
    """A band of bytes as a symmetric [n, n] array, NO_CI elsewhere."""
    out = np.full((n, n), NO_CI, dtype=np.uint8)
    off = np.asarray(offsets).astype(np.int64)
    blo = np.asarray(band_lo).astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(off))
    cols = np.arange(off[-1]) - off[rows] + blo[rows]
    out[rows, cols] = values
    out[cols, rows] = values
    return out


def host_bounds(codes, positions, window: int, pairwise: bool, keep=None, maf_min: float = 0.05):
    """(lo band, hi band, kept, band_lo, offsets, rows, cols) by the HOST definition: ops.dprime_ci_host on the exact pair
    counts (ld_em_pairwise_exact.pair_counts) of every in-window pair of kept SNPs, NO_CI elsewhere."""
    import ld_em_pairwise_exact as epx
    import ld_emband_cases as emb
    from ld_tools_amd import ops

    codes = np.asarray(codes)
    if not pairwise:
        codes = np.where(codes == 1, 1, 0).astype(np.int8)
    N, A = emb.own_counts(codes, True)
    kept = ops.gabriel_kept_host(N, A, keep, maf_min)
    band_lo, off, rows, cols = emb.band_cells(positions, window)
    counts = epx.pair_counts(codes, codes)[:, rows, cols]
    run = kept[rows] & kept[cols]
    lo = np.full(rows.shape[0], NO_CI, dtype=np.uint8)
    hi = np.full(rows.shape[0], NO_CI, dtype=np.uint8)
    if run.any():
        lo[run], hi[run] = ops.dprime_ci_host(*counts[:, run])
    return lo, hi, kept, band_lo, off, rows, cols

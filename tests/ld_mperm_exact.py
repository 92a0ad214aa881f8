"""Helpers of the permutation-test suites (test_mperm_host.py, test_gpu_mperm.py): per-individual loops for the two integers of
every (SNP, permutation) cell, the statistic as exact rationals, an independent rank count for the labels, and the panels.

Nothing here calls the code under test, except synth.key64 -- the definition of the keys itself."""
from fractions import Fraction

import numpy as np


def genotypes(codes) -> np.ndarray:
    """int8 [n_snps, n_ind]: 0 / 1 / 2, or -1 where either code of the individual is not 0 or 1."""
    c = np.asarray(codes)
    h0, h1 = c[:, 0::2], c[:, 1::2]
    ok = ((h0 == 0) | (h0 == 1)) & ((h1 == 0) | (h1 == 1))
    return np.where(ok, (h0 == 1).astype(np.int8) + (h1 == 1).astype(np.int8), -1).astype(np.int8)


def counts_brute(codes, case, labels) -> np.ndarray:
    """int64 [2, n_snps, R]: a then R of every cell, one individual after the other.  ``labels`` bool [R, individuals with a
    phenotype], in panel order."""
    g = genotypes(codes)
    case = np.asarray(case, dtype=np.float64)
    ind = np.nonzero(~np.isnan(case))[0]
    labels = np.asarray(labels, dtype=bool)
    assert labels.shape[1] == ind.size
    out = np.zeros((2, g.shape[0], labels.shape[0]), dtype=np.int64)
    for k, who in enumerate(ind):
        gk = g[:, who].astype(np.int64)
        called = gk >= 0
        lk = labels[:, k].astype(np.int64)
        out[0] += np.where(called, gk, 0)[:, None] * lk[None, :]
        out[1] += called.astype(np.int64)[:, None] * lk[None, :]
    return out


def snp_margins(codes, case, keep=None):
    """(N, n1, n2, R, a) int64 [n_snps] over the individuals with a phenotype, R and a of the observed labels."""
    g = genotypes(codes)
    case = np.asarray(case, dtype=np.float64)
    has = ~np.isnan(case)
    g = g[:, has]
    obs = case[has] == 1.0
    called = g >= 0
    if keep is not None:
        called = called & np.asarray(keep, dtype=bool)[:, None]
    gz = np.where(called, g, 0).astype(np.int64)
    return (called.sum(axis=1), (called & (g == 1)).sum(axis=1), (called & (g == 2)).sum(axis=1), called[:, obs].sum(axis=1),
            gz[:, obs].sum(axis=1))


def stat_fraction(test: str, N: int, n1: int, n2: int, R: int, a: int):
    """The exact statistic of one tuple, or None where its denominator is 0."""
    N, n1, n2, R, a = int(N), int(n1), int(n2), int(R), int(a)
    G, Q2, S = n1 + 2 * n2, n1 + 4 * n2, N - R
    if test == "allelic":
        b, c = 2 * R - a, G - a
        d = 2 * S - c
        den = (a + b) * (c + d) * (a + c) * (b + d)
        return Fraction(2 * N * (a * d - b * c) ** 2, den) if den else None
    den = R * S * (N * Q2 - G * G)
    return Fraction(N * (N * a - R * G) ** 2, den) if den else None


def rank_labels(seed: int, p: int, n: int, n_case: int) -> np.ndarray:
    """bool [n]: k is a case iff fewer than n_case individuals k' have (key(p, k'), k') < (key(p, k), k) -- counted pair by pair
    in Python integers."""
    from ld_tools_amd import synth

    keys = [int(x) for x in synth.key64(seed, np.uint64(p), np.arange(n, dtype=np.uint64))]
    return np.array([sum((keys[j], j) < (keys[k], k) for j in range(n)) < n_case for k in range(n)], dtype=bool)


def random_tables(rng, m: int, n_max: int):
    """(case n, het, hom, control n, het, hom) int64 [m]: random genotype tables, a few with empty cells and empty groups."""
    out = np.zeros((6, m), dtype=np.int64)
    for k in range(m):
        for g in range(2):
            n = int(rng.integers(0, n_max + 1)) if k % 7 else int(rng.integers(0, 3))
            p = rng.dirichlet((1.0, 1.0, 1.0)) if k % 5 else np.array([1.0, 0.0, 0.0])
            r = rng.multinomial(n, p)
            out[3 * g:3 * g + 3, k] = (n, r[1], r[2])
    return out


# ---- panels --------------------------------------------------------------------------------------------------------------------
def mperm_codes(n_snps: int, n_ind: int, seed: int, miss: float = 0.0, miss_from: int = 0) -> np.ndarray:
    """int8 [n_snps, 2 n_ind]: independent SNPs with ALT frequencies in [0.2, 0.5]; ``miss`` of the haplotype codes of the SNPs
    ``miss_from`` and above missing (2)."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.2, 0.5, n_snps)
    codes = (rng.random((n_snps, 2 * n_ind)) < f[:, None]).astype(np.int8)
    if miss:
        hole = rng.random(codes.shape) < miss
        hole[:miss_from] = False
        codes[hole] = 2
    return codes


def case_vector(n_ind: int, n_case: int, n_ctrl: int, seed: int) -> np.ndarray:
    """float64 [n_ind]: n_case ones, n_ctrl zeros and NaN for the rest, shuffled."""
    v = np.full(n_ind, np.nan)
    v[:n_case] = 1.0
    v[n_case:n_case + n_ctrl] = 0.0
    np.random.default_rng(seed).shuffle(v)
    return v

"""Helper of the GRM tests (no test in here): the case panels, the weights that walk the digit edges, and an exact oracle that
shares nothing with the library's host mirror -- S by Python integers in a plain loop over (SNP, individual, individual), the
GRM cell by fractions.Fraction from the UNQUANTISED rational weights.

Definitions (include/ldx.h, "weighted sample products"): individual a owns haplotypes 2a, 2a + 1; it is called at a SNP when
both codes are 0 or 1; g = its ALT dosage (0 when missing), c = 1 when called.
    S[a][b] = sum_i ( q2 g_a g_b + q1 (g_a c_b + c_a g_b) + q0 c_a c_b )
    exact grm[a][b] = (1 / N_ab) sum over the live SNPs called in both of (g_a - 2 p)(g_b - 2 p) / (2 p (1 - p)),  p = s / (2 n)"""
from fractions import Fraction

import numpy as np

# one tile; a ragged slab; an off-diagonal tile with its mirror write; three slabs
N_IND = (1, 127, 130, 257)
# one SNP; just under a K-block; past the 256-SNP K-block and the 128-SNP chunk
N_SNPS = (1, 255, 700)
HOLES = ("none", "3%", "50%")
N_SLICES = (None, 1, 3)
MAX_W = 1 << 28

# The kernel splits u = g q2 + q1 and v = g q1 + q0 into four balanced BASE-256 digits in [-128, 127]: a digit carries into the
# next one between 127 and 128 and borrows between -128 and -129, at every digit position (2^8, 2^16, 2^24).  The values of the
# issue's list (edges of a base-128 split) stay in, next to the edges of the base chosen.
EDGES = [0, 1, -1, 63, 64, -64, -65, 127, 128, -128, -129, 255, 256, -256, -257,
         (1 << 14) - 1, -(1 << 14) + 1, 1 << 14, -(1 << 14), (1 << 15) - 1, 1 << 15, -(1 << 15), -(1 << 15) - 1,
         1 << 21, -(1 << 21), (1 << 23) - 1, 1 << 23, -(1 << 23), -(1 << 23) - 1, 127 * 0x010101, 128 * 0x010101, -128 * 0x010101,
         -129 * 0x010101, MAX_W - 1, -(MAX_W - 1), MAX_W, -MAX_W]


def panel_codes(n_ind, n_snps, seed, holes="none"):
    """int8 [n_snps, 2 n_ind]: ALT frequencies uniform in [0.05, 0.95], independent haplotypes.  holes: "none"; "3%" / "50%": that
    share of the genotypes missing (code 2 on both haplotypes), a further 1 % half-missing and 1 % with a second-ALT code (3), and
    -- from three individuals on -- individual 1 without any call."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.95, size=n_snps)
    codes = (rng.random((n_snps, 2 * n_ind)) < f[:, None]).astype(np.int8)
    if holes == "none":
        return codes
    share = {"3%": 0.03, "50%": 0.5}[holes]
    u = rng.random((n_snps, n_ind))
    codes[np.repeat(u < share, 2, axis=1)] = 2
    codes[:, 0::2][(u >= share) & (u < share + 0.01)] = 2
    codes[:, 1::2][(u >= share + 0.01) & (u < share + 0.02)] = 3
    if n_ind >= 3:
        codes[:, 2:4] = 2
    return codes


def edge_weights(n_snps, seed):
    """int32 [n_snps, 3]: first every edge value alone in each of the three columns (so that u = g q2 + q1 and v = g q1 + q0 sit
    ON the digit edges for g = 1 and for a called g = 0), then rows of three edge values, then random values in range -- shuffled,
    so that a short panel still sees a mixture."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(3):
        for e in EDGES:
            r = [0, 0, 0]
            r[k] = e
            rows.append(r)
    alone = np.array(rows, dtype=np.int64)
    mixed = rng.choice(np.array(EDGES, dtype=np.int64), size=(max(n_snps, 64), 3))
    rand = rng.integers(-MAX_W, MAX_W + 1, size=(max(n_snps, 64), 3))
    q = np.concatenate([alone, mixed, rand])
    q = q[rng.permutation(q.shape[0])]
    if n_snps > q.shape[0]:
        q = np.concatenate([q, rng.integers(-MAX_W, MAX_W + 1, size=(n_snps - q.shape[0], 3))])
    return np.ascontiguousarray(q[:n_snps].astype(np.int32))


def genotypes(codes, keep=None):
    """Per SNP the list of dosages (None = missing); None for a SNP that is not kept."""
    c = np.asarray(codes)
    out = []
    for s in range(c.shape[0]):
        if keep is not None and not keep[s]:
            out.append(None)
            continue
        row = []
        for a in range(c.shape[1] // 2):
            x, y = int(c[s, 2 * a]), int(c[s, 2 * a + 1])
            row.append(x + y if x in (0, 1) and y in (0, 1) else None)
        out.append(row)
    return out


def loop_wprod(codes, q, keep=None):
    """S as a list of lists of Python integers, by the definition: for small panels."""
    n_ind = np.asarray(codes).shape[1] // 2
    S = [[0] * n_ind for _ in range(n_ind)]
    for s, g in enumerate(genotypes(codes, keep)):
        if g is None:
            continue
        q2, q1, q0 = (int(x) for x in q[s])
        for a in range(n_ind):
            if g[a] is None:
                continue
            for b in range(n_ind):
                if g[b] is not None:
                    S[a][b] += q2 * g[a] * g[b] + q1 * (g[a] + g[b]) + q0
    return S


def exact_grm(codes, keep=None, maf_min=None):
    """(grm as Fractions (None where N = 0), N, n_live) by the definition, nothing quantised.  maf_min: a Fraction or None."""
    n_ind = np.asarray(codes).shape[1] // 2
    num = [[Fraction(0)] * n_ind for _ in range(n_ind)]
    N = [[0] * n_ind for _ in range(n_ind)]
    n_live = 0
    for g in genotypes(codes, keep):
        if g is None:
            continue
        called = [x for x in g if x is not None]
        n, s = len(called), sum(called)
        if not 0 < s < 2 * n:
            continue
        if maf_min is not None and Fraction(min(s, 2 * n - s), 2 * n) < maf_min:
            continue
        n_live += 1
        p = Fraction(s, 2 * n)
        w = 1 / (2 * p * (1 - p))
        for a in range(n_ind):
            if g[a] is None:
                continue
            for b in range(n_ind):
                if g[b] is not None:
                    num[a][b] += w * (g[a] - 2 * p) * (g[b] - 2 * p)
                    N[a][b] += 1
    grm = [[num[a][b] / N[a][b] if N[a][b] else None for b in range(n_ind)] for a in range(n_ind)]
    return grm, N, n_live

"""Helper of the sample-relatedness tests (no test in here): an integer oracle that shares nothing with the library's host
mirror -- a plain triple loop over (SNP, individual, individual) -- the panel builders and the case table.

Definitions (include/ldx.h, "sample relatedness"): individual a owns haplotypes 2a, 2a + 1; it is called at a SNP when both
codes are 0 or 1; g = its ALT dosage.  Over the kept SNPs called in both: N, HH = #{g_a = g_b = 1}, IBS0 = #{(0, 2), (2, 0)},
HET[a][b] = #{g_a = 1, b called}."""
import numpy as np

# the shapes of the exactness cases: across a 32-row accumulator tile, a wave, one and two workgroup tiles ...
N_IND = (1, 2, 3, 64, 127, 128, 129, 257)
# ... across one MFMA K-step (64), one chunk (128), one K-block (256)
N_SNPS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
# the kernel's minimum slice length +-1, and the K-block count from which the automatic choice makes a second slice
# (2 * 65536 / 256 = 512 K-blocks: 130 817 SNPs is the first panel with 512)
N_SNPS_LONG = (65535, 65536, 65537, 130816, 130817, 131073)
HOLES = ("none", "3%", "single")
N_SLICES = (None, 1, 2, 3, 7)


def loop_counts(codes, keep=None):
    """int64 [4, n_ind, n_ind] (N, HH, IBS0, HET) by a plain loop: for small panels."""
    c = np.asarray(codes)
    n_snps, n_hap = c.shape
    n_ind = n_hap // 2
    out = np.zeros((4, n_ind, n_ind), dtype=np.int64)
    for s in range(n_snps):
        if keep is not None and not keep[s]:
            continue
        g = []
        for a in range(n_ind):
            x, y = int(c[s, 2 * a]), int(c[s, 2 * a + 1])
            g.append(x + y if x in (0, 1) and y in (0, 1) else None)
        for a in range(n_ind):
            if g[a] is None:
                continue
            for b in range(n_ind):
                if g[b] is None:
                    continue
                out[0, a, b] += 1
                out[1, a, b] += g[a] == 1 and g[b] == 1
                out[2, a, b] += {g[a], g[b]} == {0, 2}
                out[3, a, b] += g[a] == 1
    return out


def panel_codes(n_ind, n_snps, seed, holes="none"):
    """int8 [n_snps, 2 n_ind]: ALT frequencies uniform in [0.05, 0.5], independent haplotypes.  holes: "none"; "3%": 3 % of the
    genotypes missing (code 2 on both haplotypes), a further 0.5 % half-missing and 0.5 % with a second-ALT code (3);
    "single": one missing genotype, of individual n_ind // 2 at SNP n_snps // 2."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.5, size=n_snps)
    codes = (rng.random((n_snps, 2 * n_ind)) < f[:, None]).astype(np.int8)
    if holes == "3%":
        u = rng.random((n_snps, n_ind))
        codes[np.repeat(u < 0.03, 2, axis=1)] = 2
        half = (u >= 0.03) & (u < 0.035)
        codes[:, 0::2][half] = 2
        alt2 = (u >= 0.035) & (u < 0.04)
        codes[:, 1::2][alt2] = 3
    elif holes == "single":
        codes[n_snps // 2, 2 * (n_ind // 2): 2 * (n_ind // 2) + 2] = 2
    elif holes != "none":
        raise ValueError(holes)
    return codes


def hand_table():
    """3 individuals x 6 SNPs, counted by hand.  Genotypes (g, . = missing):
         SNP   ind 0   ind 1   ind 2
          0    0|1 1   1|0 1   1|1 2
          1    0|0 0   1|1 2   0|0 0
          2    1|2 .   0|1 1   0|0 0      (ind 0: a second-ALT code)
          3    0|? .   1|1 2   0|0 0      (ind 0: half-missing)
          4    1|1 2   0|1 1   1|0 1      (masked: not kept)
          5    1|1 2   0|0 0   0|0 0
    Kept SNPs 0 1 2 3 5.  Individual 0 is heterozygous at SNP 0, individual 1 at SNPs 0 and 2, individual 2 at no kept SNP: every
    pair with it has m = 0.  Returns (codes, keep, counts [4, 3, 3], kin [3, 3], ibs [3, 3])."""
    codes = np.array([[0, 1, 1, 0, 1, 1],
                      [0, 0, 1, 1, 0, 0],
                      [1, 2, 0, 1, 0, 0],
                      [0, -1, 1, 1, 0, 0],
                      [1, 1, 0, 1, 1, 0],
                      [1, 1, 0, 0, 0, 0]], dtype=np.int8)
    keep = np.array([1, 1, 1, 1, 0, 1], dtype=bool)
    # ind 0 called at 0 1 5 (g 1 0 2); ind 1 at 0 1 2 3 5 (g 1 2 1 2 0); ind 2 at 0 1 2 3 5 (g 2 0 0 0 0)
    N = [[3, 3, 3], [3, 5, 5], [3, 5, 5]]
    HH = [[1, 1, 0], [1, 2, 0], [0, 0, 0]]      # (0,0), (0,1): SNP 0; (1,1): SNPs 0, 2
    # (0,1): SNP 1 (0,2), SNP 5 (2,0);  (0,2): SNP 5 (2,0);  (1,2): SNPs 1 and 3 (2,0)
    IBS0 = [[0, 2, 1], [2, 0, 2], [1, 2, 0]]
    # HET[a][b]: a heterozygous and b called.  ind 0 at SNP 0; ind 1 at SNPs 0 and 2 (ind 0 is not called at 2); ind 2 never
    HET = [[1, 1, 1], [1, 2, 2], [0, 0, 0]]
    # (0,1): IBS1 = 1 + 1 - 2 = 0, m = 1: 0.5 - 8 / 4;  every pair with ind 2: m = 0;  diagonal: 0.5 where the individual has a het
    z = np.float32(-0.0)
    kin = np.array([[0.5, -1.5, z], [-1.5, 0.5, z], [z, z, z]], dtype=np.float32)
    # (0,1): IBS2 = 3 - 0 - 2 = 1: 2 / 6;  (0,2): IBS1 = 1, IBS2 = 1: 3 / 6;  (1,2): IBS1 = 2, IBS2 = 1: 4 / 10
    t, f = np.float32(2.0 / 6.0), np.float32(4.0 / 10.0)
    ibs = np.array([[1.0, t, 0.5], [t, 1.0, f], [0.5, f, 1.0]], dtype=np.float32)
    return codes, keep, np.array([N, HH, IBS0, HET], dtype=np.int64), kin, ibs

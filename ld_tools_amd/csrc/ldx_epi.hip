// Epistasis scans (include/ldx.h, "epistasis scan"): for every row of SNP set I against every row of SNP set J
// the 3 x 3 genotype table of the pair in the cases and in the controls -- 18 exact integers -- and from them one of two
// SNP x SNP interaction tests, `allelic` (PLINK --fast-epistasis) or `boost` (the likelihood-ratio test of BOOST).  ONE kernel
// template (epi_kernel) for the counts, the dense cells and the hit list with its per-SNP summary; ONE device function
// (epi_cell) from the 18 integers to the cell, which the epilogue-alone entry calls too.
//   * operands: those of the pairwise-complete EM tile (ldx_em_pw_tile.h), on the individuals' EVEN haplotype slots.  With
//     q = ind_called(alt, ref) and w = alt masked by both slots of q:
//         I side (0.5 / 1):  G = expand32_a4_dosage(w)  g / 2      T = het_a4(het_bits(w))  0.5 where g = 1      Q = even_a4(q)  0.5 where called
//         J side (2 / 4):    U = expand32_b4_dosage(w)  2 g        V = het_b4(het_bits(w))  2 where g = 1        C = het_b4(q)   2 where called
//     and the nine products GG = G.U, TT = T.V, GT = G.V, TG = T.U, GQ = G.C, QG = Q.U, TQ = T.C, QT = Q.V, QQ = Q.C.  Every
//     product is g_i g_j, g or 1 and every sum at most 4 N <= 20 480 < 2^16 < 2^24: the fp32 accumulators are exact in any
//     order, and a set fits half a word.  table_of turns the nine sets into the nine cells n_ab.
//   * the two groups are two panels (cases, controls) with their own planes and haplotype counts; a pass runs the K loop over
//     the cases' planes, packs the nine sets two to a register, runs the K loop over the controls' planes into the same
//     accumulators, and then holds all 18 sets of its cells.
//   * tile: a workgroup (4 waves as 2 x 2) owns 128 rows of I x 128 rows of J, a wave 64 x 64 cells.  Nine sets of a 32 x 32
//     accumulator tile are 144 registers and the packed cases another 80, so the wave covers its cells in FOUR passes, each over
//     one 32 x 32 tile, and the kernel asks for one workgroup per CU (launch bound 1 wave per SIMD: up to 512 registers).
//   * shortcut: per GROUP, a tile none of whose 256 SNPs has an uncalled individual of that group (called == n_ind in the
//     group's per-SNP table {called, het, hom ALT, 0}, ldx_geno_snp_counts_dev's) forms the four joint sets GG TT GT TG alone;
//     the five margins come from the tables: GQ = het_i + 2 hom_i, QG likewise of j, TQ = het_i, QT = het_j, QQ = n_ind.  The
//     integers are the same either way, so a cell cannot tell the path.
//   * K loop: the general loop of ldx_em_pw_tile.h -- per K-block of 256 haplotypes the workgroup expands the J slab's bits
//     once into LDS images [4 steps][2 halves][128 rows][8 B] (U, V and, for nine sets, C), double-buffered, one block_sync
//     per K-block; a lane loads the 16 bytes of its own I row from each plane and expands them in registers.
//   * epilogue of a pass: the accumulator of a 32 x 32 tile has the column on the lane and the rows in the 16 registers; a wave
//     stages its cells a quarter (8 rows) at a time as nine words per cell in the LDS the images no longer need (4 x 9 KiB), and a
//     rolled loop reads them back one cell per lane (lane = column, half-wave = rows r and r + 4): epi_cell per lane and trip,
//     128-byte row-major stores per half-wave.  The 18 integers never go to HBM except in the counts form.
//   * summary (hits form): per row the valid tests, the tests at or above a second bound and the best partner.  The 32 lanes of
//     a half-wave share a row: they meet in a ballot and five shuffles, so a row costs three integer atomics per trip; in the
//     self scan a lane keeps its column's three values in registers over the pass and adds them once at its end.
//   * walk: tile_of (ldx_fp4.h) as the EM rectangle; the self scan walks the tiles tj <= ti by their triangular number.
#include "ldx_em_pw_tile.h"
#include "ldx_tail.h"

namespace ldx {
namespace epi {

using em::v2i;
using em::kThreads;
using em_pw::kOpBytes;
using em_pw::mfma2;

constexpr uint32_t kImage = 3u * kOpBytes;       // one buffer of the K loop: U, V, C (24 KiB)
constexpr uint32_t kLdsBytes = 2u * kImage;      // 48 KiB
constexpr uint32_t kQuarter = 8u * 32u;          // cells of a wave's staged quarter: 8 rows x 32 columns
constexpr uint32_t kStageWords = 9u;             // 18 sets, two to a word
static_assert(em::kWaves * kStageWords * kQuarter * 4u <= kLdsBytes, "the staged quarter lives in the images' LDS");

enum Set : int { GG = 0, TT, GT, TG, GQ, QG, TQ, QT, QQ, kSets };
enum Mode : int { kDense = 0, kHits = 1, kCounts = 2 };
constexpr uint32_t kFlagEmpty = 1, kFlagAllele0 = 2, kFlagCap = 4, kFlagMargin0 = 8, kFlagNoTable = 16;

struct Group {
    const uint4 *alt, *ref;   // tiled bit planes of the group's panel
    const uint4 *cnt;         // [n] {called, het, hom ALT, 0}
};
struct Side {
    Group g[2];               // cases, controls
    uint32_t n;               // SNPs
};

struct Args {
    Side si, sj;
    uint32_t nblocks[2];      // K-blocks of 256 haplotypes per group
    uint32_t n_ind[2];
    int test, self;
    float *out_x, *out_dir;   // dense
    uint8_t *out_flags;
    uint32_t *counts;         // counts: [18][n_i][ld]
    size_t ld;
    float bound, bound_sig;   // hits
    ldx_hit *hits;
    uint64_t hit_cap;
    unsigned long long *n_hits;
    uint32_t *n_tot, *n_sig;  // summary (all null or all given)
    unsigned long long *best;
};

struct Smem {
    __attribute__((aligned(16))) unsigned char lds[kLdsBytes];   // K loops: two image buffers; epilogue: the staged quarter
    uint32_t rdos[2][kSlab], rhet[2][kSlab];   // per group: het + 2 hom and het of the workgroup's 128 rows
    uint32_t cdos[2][kSlab], chet[2][kSlab];   // ... and of its 128 columns
    uint32_t wflag[2][em::kWaves];
};

// ---- the epilogue: 18 integers -> the cell (include/ldx.h has the definitions).  fp64, -ffp-contract=off, fixed order ----------
struct Cell {
    double chisq, dir;
    uint32_t flags, cycles;
};

// the nine cells n[3 a + b] of one group from its nine sets
__device__ __forceinline__ void table_of(const uint32_t (&s)[kSets], uint32_t *n)
{
    const uint32_t n11 = s[TT], n21 = (s[GT] - s[TT]) / 2u, n12 = (s[TG] - s[TT]) / 2u;
    const uint32_t n22 = (s[GG] - n11 - 2u * n12 - 2u * n21) / 4u;
    const uint32_t r1 = s[TQ], r2 = (s[GQ] - s[TQ]) / 2u, c1 = s[QT], c2 = (s[QG] - s[QT]) / 2u;
    const uint32_t n10 = r1 - n11 - n12, n20 = r2 - n21 - n22, n01 = c1 - n11 - n21, n02 = c2 - n12 - n22;
    n[0] = s[QQ] - r1 - r2 - n01 - n02;
    n[1] = n01, n[2] = n02, n[3] = n10, n[4] = n11, n[5] = n12, n[6] = n20, n[7] = n21, n[8] = n22;
}

// one group's log odds ratio and its variance on the 2 x 2 allele table; false where a cell is 0
__device__ __forceinline__ bool allele_log(const uint32_t *n, double &L, double &V)
{
    const int64_t N = (int64_t)n[0] + n[1] + n[2] + n[3] + n[4] + n[5] + n[6] + n[7] + n[8];
    const int64_t A = (int64_t)n[3] + n[4] + n[5] + 2 * ((int64_t)n[6] + n[7] + n[8]);
    const int64_t B = (int64_t)n[1] + n[4] + n[7] + 2 * ((int64_t)n[2] + n[5] + n[8]);
    const int64_t S = (int64_t)n[4] + 2 * ((int64_t)n[5] + n[7]) + 4 * (int64_t)n[8];
    const int64_t a = S, b = 2 * A - S, c = 2 * B - S, d = 4 * N - 2 * A - 2 * B + S;
    if (a == 0 || b == 0 || c == 0 || d == 0) return false;
    L = log(((double)a * (double)d) / ((double)b * (double)c));
    V = (1.0 / (double)a + 1.0 / (double)d) + (1.0 / (double)b + 1.0 / (double)c);   // symmetric under b <-> c
    return true;
}

__device__ __forceinline__ constexpr int tr18(int k) { return (k / 9) * 9 + (k % 3) * 3 + (k % 9) / 3; }   // the SNPs swapped

// mu (18 doubles in the caller's orientation) is written where kMu and the test is boost and flag 1 is not set
template <bool kMu>
__device__ __forceinline__ Cell epi_cell(int test, const uint32_t (&n)[18], double *mu_out)
{
    const double nan = __builtin_nan("");
    Cell c{nan, nan, 0u, 0u};
    double L1 = 0.0, V1 = 0.0, L0 = 0.0, V0 = 0.0;
    const bool ok1 = allele_log(n, L1, V1), ok0 = allele_log(n + 9, L0, V0);
    if (ok1 && ok0) c.dir = L1 - L0;
    else c.flags |= kFlagAllele0;
    if (test == LDX_EPI_ALLELIC) {
        if (c.flags == 0u) {
            const double z = c.dir / __builtin_sqrt(V1 + V0);
            c.chisq = z * z;
        }
        return c;
    }
    // boost.  The table is fitted in the orientation that comes first in the order of the 18 integers, so that the two
    // orientations of a pair run the same arithmetic.
    bool swap = false, decided = false;
#pragma unroll
    for (int k = 0; k < 18; ++k) {
        if (!decided && n[tr18(k)] != n[k]) {
            swap = n[tr18(k)] < n[k];
            decided = true;
        }
    }
    double o[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) o[k] = (double)(swap ? n[tr18(k)] : n[k]);
    double m_ab[9], m_ac[2][3], m_bc[2][3];
#pragma unroll
    for (int k = 0; k < 9; ++k) m_ab[k] = o[k] + o[9 + k];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            m_ac[g][x] = (o[9 * g + 3 * x] + o[9 * g + 3 * x + 1]) + o[9 * g + 3 * x + 2];
            m_bc[g][x] = (o[9 * g + x] + o[9 * g + 3 + x]) + o[9 * g + 6 + x];
        }
    const double n_case = (m_ac[0][0] + m_ac[0][1]) + m_ac[0][2], n_ctrl = (m_ac[1][0] + m_ac[1][1]) + m_ac[1][2];
    if (n_case == 0.0 || n_ctrl == 0.0) {
        c.flags |= kFlagEmpty;
        return c;
    }
    bool zero = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) zero = zero || m_ab[k] == 0.0;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int x = 0; x < 3; ++x) zero = zero || m_ac[g][x] == 0.0 || m_bc[g][x] == 0.0;
    if (zero) c.flags |= kFlagMargin0;

    const double tol = 0x1p-40 * (n_case + n_ctrl);
    double mu[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) mu[k] = 1.0;
    bool conv = false;
    uint32_t cyc = 0;
    while (cyc < LDX_EPI_MAX_CYCLES && !conv) {
        ++cyc;
        double old[18];
#pragma unroll
        for (int k = 0; k < 18; ++k) old[k] = mu[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) {   // SNP i x SNP j
            const double s = mu[k] + mu[9 + k];
            const double f = s == 0.0 ? 0.0 : m_ab[k] / s;
            mu[k] = mu[k] * f;
            mu[9 + k] = mu[9 + k] * f;
        }
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int x = 0; x < 3; ++x) {   // SNP i x group
                const int at = 9 * g + 3 * x;
                const double s = (mu[at] + mu[at + 1]) + mu[at + 2];
                const double f = s == 0.0 ? 0.0 : m_ac[g][x] / s;
                mu[at] = mu[at] * f;
                mu[at + 1] = mu[at + 1] * f;
                mu[at + 2] = mu[at + 2] * f;
            }
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int x = 0; x < 3; ++x) {   // SNP j x group
                const int at = 9 * g + x;
                const double s = (mu[at] + mu[at + 3]) + mu[at + 6];
                const double f = s == 0.0 ? 0.0 : m_bc[g][x] / s;
                mu[at] = mu[at] * f;
                mu[at + 3] = mu[at + 3] * f;
                mu[at + 6] = mu[at + 6] * f;
            }
        double moved = 0.0;
#pragma unroll
        for (int k = 0; k < 18; ++k) {
            const double d = __builtin_fabs(mu[k] - old[k]);
            moved = d > moved ? d : moved;
        }
        conv = moved <= tol;
    }
    c.cycles = cyc;
    if (!conv) c.flags |= kFlagCap;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 18; ++k)
        if (o[k] > 0.0) acc = acc + o[k] * log(o[k] / mu[k]);
    const double g2 = 2.0 * acc;
    c.chisq = g2 > 0.0 ? g2 : 0.0;   // (the exact statistic is >= 0; a rounded sum just below it is 0)
    if constexpr (kMu) {
#pragma unroll
        for (int k = 0; k < 18; ++k) mu_out[k] = swap ? mu[tr18(k)] : mu[k];
    }
    return c;
}

// ln p of a cell's chi-square: 1 df through the two-sided normal tail of sqrt(chisq) (ldx_tail.h), 4 df in closed form
__device__ __forceinline__ double ln_p(int test, double chisq)
{
    if (chisq != chisq) return chisq;
    if (test == LDX_EPI_ALLELIC) {
        double pv, nlp;
        normal_tail(__builtin_sqrt(chisq), pv, nlp);
        return -(nlp * kTailLn10);
    }
    const double x = 0.5 * chisq;
    return -x + log1p(x);
}

// ---- one cell from its 18 integers: dense cells, hits with the summary, counts.  Called by the whole wave ------------------
template <int kMode>
struct Emit {
    const Args &p;
    HitAppender hit;
    uint32_t lane;
    uint32_t c_tot = 0, c_sig = 0;   // self scan: what the lane's column has gathered in this pass
    unsigned long long c_best = 0;

    __device__ __forceinline__ void operator()(uint32_t i, uint32_t j, const uint32_t (&n)[18])
    {
        const bool inside = i < p.si.n && j < p.sj.n && (!p.self || i > j);
        if constexpr (kMode == kCounts) {
            if (inside) {
#pragma unroll
                for (int s = 0; s < 18; ++s)
                    __builtin_nontemporal_store(n[s], p.counts + ((size_t)s * p.si.n + i) * p.ld + j);
            }
        } else {
            Cell c{__builtin_nan(""), __builtin_nan(""), 0u, 0u};
            if (inside) c = epi_cell<false>(p.test, n, nullptr);
            const float x = (float)c.chisq, dir = (float)c.dir;
            if constexpr (kMode == kDense) {
                if (inside) {
                    if (p.out_x) __builtin_nontemporal_store(x, p.out_x + (size_t)i * p.ld + j);
                    if (p.out_dir) __builtin_nontemporal_store(dir, p.out_dir + (size_t)i * p.ld + j);
                    if (p.out_flags) p.out_flags[(size_t)i * p.ld + j] = (uint8_t)c.flags;
                }
            } else {
                const bool valid = inside && x == x;
                hit.append(valid && x >= p.bound, i, j, x, dir);   // ONE float32 compare; a NaN is never a hit
                if (p.n_tot) {
                    const bool sig = valid && x >= p.bound_sig;
                    const uint32_t sh = lane & 32u;
                    const uint32_t tot = __builtin_popcount((uint32_t)(__ballot(valid) >> sh));
                    const uint32_t nsig = __builtin_popcount((uint32_t)(__ballot(sig) >> sh));
                    const uint32_t bits = __float_as_uint(x);   // x >= +0: the bits order as the values
                    unsigned long long key = valid ? ((unsigned long long)bits << 32) | (0xFFFFFFFFu - j) : 0ull;
#pragma unroll
                    for (int d = 16; d >= 1; d >>= 1) {
                        const uint32_t hi = __shfl_xor((uint32_t)(key >> 32), d), lo = __shfl_xor((uint32_t)key, d);
                        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
                        key = other > key ? other : key;
                    }
                    if ((lane & 31u) == 0u && tot != 0u) {   // a half-wave's lanes share the row
                        atomicAdd(p.n_tot + i, tot);
                        if (nsig != 0u) atomicAdd(p.n_sig + i, nsig);
                        atomicMax(p.best + i, key);
                    }
                    if (p.self && valid) {   // the column is the pair's other SNP: its partner is i
                        c_tot += 1u;
                        c_sig += sig ? 1u : 0u;
                        const unsigned long long ck = ((unsigned long long)bits << 32) | (0xFFFFFFFFu - i);
                        c_best = ck > c_best ? ck : c_best;
                    }
                }
            }
        }
    }
    // end of a pass: the lane's column j
    __device__ __forceinline__ void flush(uint32_t j)
    {
        if constexpr (kMode == kHits) {
            if (c_tot != 0u) {
                atomicAdd(p.n_tot + j, c_tot);
                if (c_sig != 0u) atomicAdd(p.n_sig + j, c_sig);
                atomicMax(p.best + j, c_best);
            }
            c_tot = 0u, c_sig = 0u, c_best = 0ull;
        }
    }
};

// ---- the K loop of one group over one 32 x 32 tile of the wave: acc += the group's sets (four, or all nine) ----------------
template <bool kNine>
__device__ __forceinline__ void count_group(unsigned char *lds, const Group &gi, const Group &gj, uint32_t nblocks, uint32_t ti,
                                            uint32_t tj, uint32_t tid, uint32_t m0, uint32_t t0, v16f (&acc)[kSets])
{
    const uint32_t lane = tid & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wr = wave >> 1, wc = wave & 1u;
    const uint32_t nchunks = 2u * nblocks;
    // thread's share of the J images: row tid % 128, chunk 2 blk + tid / 128
    const uint32_t b_row = tid & (kSlab - 1u), b_half = tid >> 7;
    const uint32_t b_off = (tj * nchunks + b_half) * kSlab + b_row;
    const uint32_t b_dst = b_half * kSlab + b_row;   // + step * 256
    auto load = [&](const uint4 *plane, uint32_t off, uint32_t blk) { return plane[off + (size_t)blk * em::kBlockVecs]; };
    auto expand_b = [&](unsigned char *buf, const uint4 &alt, const uint4 &ref) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t wa = word_of(alt, q), wf = word_of(ref, q);
            const uint32_t qc = ind_called(wa, wf), w = wa & (qc | (qc << 1));
            const v4i u = expand32_b4_dosage(w);
            v2i *const dst = reinterpret_cast<v2i *>(buf) + b_dst + (uint32_t)q * em::kBlockVecs;
            dst[0] = v2i{u.x, u.z};                                  // U: the even slots' 2 g
            dst[kOpBytes / 8u] = em::het_b4(em::het_bits(w));       // V
            if constexpr (kNine) dst[2u * (kOpBytes / 8u)] = em::het_b4(qc);   // C
        }
    };
    // lane's A source: row 64 wr + 32 m0 + l32 of slab ti, chunk 2 blk + half; planes are < 4 GiB: 32-bit indices
    const uint32_t a_off = (ti * nchunks + half) * kSlab + wr * em::kWaveRows + 32u * m0 + l32;
    const uint32_t col = wc * em::kWaveCols + 32u * t0 + l32;   // lane's column of the slab
    uint4 a_alt = load(gi.alt, a_off, 0u), a_ref = load(gi.ref, a_off, 0u);
    // (the first buffer is free: every wave left what came before through a barrier)
    expand_b(lds, load(gj.alt, b_off, 0u), load(gj.ref, b_off, 0u));
    block_sync();
    for (uint32_t blk = 0; blk < nblocks; ++blk) {
        const uint32_t nb = blk + 1u < nblocks ? blk + 1u : blk;
        const uint4 b_alt = load(gj.alt, b_off, nb), b_ref = load(gj.ref, b_off, nb);
        const uint4 n_alt = load(gi.alt, a_off, nb), n_ref = load(gi.ref, a_off, nb);
        __builtin_amdgcn_sched_barrier(0);   // the global loads stay at the top of the block
        const v2i *const rd = reinterpret_cast<const v2i *>(lds + (blk & 1u) * kImage);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const v2i *const at = rd + ((uint32_t)w * 2u + half) * kSlab + col;
            const v2i bu = at[0], bv = at[kOpBytes / 8u];
            const uint32_t wa = word_of(a_alt, w), wf = word_of(a_ref, w);
            const uint32_t qc = ind_called(wa, wf), ww = wa & (qc | (qc << 1));
            const v4i g4 = expand32_a4_dosage(ww);
            const v2i xg = {g4.x, g4.z}, xt = em::het_a4(em::het_bits(ww));
            acc[GG] = mfma2(xg, bu, acc[GG]);
            acc[TT] = mfma2(xt, bv, acc[TT]);
            acc[GT] = mfma2(xg, bv, acc[GT]);
            acc[TG] = mfma2(xt, bu, acc[TG]);
            if constexpr (kNine) {
                const v2i bc = at[2u * (kOpBytes / 8u)];
                const v4i q4 = even_a4(qc);
                const v2i xq = {q4.x, q4.z};
                acc[GQ] = mfma2(xg, bc, acc[GQ]);
                acc[QG] = mfma2(xq, bu, acc[QG]);
                acc[TQ] = mfma2(xt, bc, acc[TQ]);
                acc[QT] = mfma2(xq, bv, acc[QT]);
                acc[QQ] = mfma2(xq, bc, acc[QQ]);
            }
        }
        expand_b(lds + ((blk + 1u) & 1u) * kImage, b_alt, b_ref);
        block_sync();
        a_alt = n_alt;
        a_ref = n_ref;
    }
}

// the words of element e (row (e & 3) + 4 half of its quarter) of the lane: cases 0 .. 3 and the low half of 4, controls the
// high half of 4 and 5 .. 8
template <int kQ>
__device__ __forceinline__ void stage_quarter(uint32_t *stage, uint32_t half, uint32_t l32, const uint32_t (&pk)[5][16],
                                              const v16f (&acc)[kSets])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        constexpr int e0 = 4 * kQ;
        const uint32_t at = ((uint32_t)r + 4u * half) * 32u + l32;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            stage[(uint32_t)k * kQuarter + at] = pk[k][e0 + r];
            stage[(uint32_t)(5 + k) * kQuarter + at] = (uint32_t)acc[2 * k][e0 + r] | ((uint32_t)acc[2 * k + 1][e0 + r] << 16);
        }
        stage[4u * kQuarter + at] = pk[4][e0 + r] | ((uint32_t)acc[QQ][e0 + r] << 16);
    }
}

template <typename E>
__device__ __forceinline__ void tile_body(Smem &sm, const Args &p, uint32_t ti, uint32_t tj, uint32_t tid, E &emit)
{
    unsigned char *const lds = sm.lds;
    const uint32_t lane = tid & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wr = wave >> 1, wc = wave & 1u;

    // ---- per group: the margins' tables, and does a SNP of this tile hold an uncalled individual?  Thread t < 128 owns
    // column t of the slab, thread 128 + t row t.
    bool general[2];
    {
        const bool is_col = tid < kSlab;
        const uint32_t at = tid & (kSlab - 1u);
        const uint32_t x = (is_col ? tj : ti) * kSlab + at;
        const bool live = x < (is_col ? p.sj.n : p.si.n);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint4 *const cnt = is_col ? p.sj.g[g].cnt : p.si.g[g].cnt;
            const uint4 k = live ? cnt[x] : uint4{0u, 0u, 0u, 0u};
            (is_col ? sm.cdos : sm.rdos)[g][at] = k.y + 2u * k.z;
            (is_col ? sm.chet : sm.rhet)[g][at] = k.y;
            const bool wave_hole = __any(live && k.x != p.n_ind[g]);
            if (lane == 0) sm.wflag[g][wave] = wave_hole ? 1u : 0u;
        }
        block_sync();
#pragma unroll
        for (int g = 0; g < 2; ++g)
            general[g] = __builtin_amdgcn_readfirstlane(sm.wflag[g][0] | sm.wflag[g][1] | sm.wflag[g][2] | sm.wflag[g][3]) != 0u;
    }

    uint32_t *const stage = reinterpret_cast<uint32_t *>(lds) + wave * (kStageWords * kQuarter);
    for (uint32_t ps = 0; ps < 4u; ++ps) {
        const uint32_t m0 = ps >> 1, t0 = ps & 1u;   // the pass's tile of the wave's 2 x 2
        v16f acc[kSets];
        uint32_t pk[5][16];   // the cases' sets, two to a register
#pragma unroll
        for (int g = 0; g < 2; ++g) {
#pragma unroll
            for (int s = 0; s < kSets; ++s)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[s][e] = 0.0f;
            if (general[g]) count_group<true>(lds, p.si.g[g], p.sj.g[g], p.nblocks[g], ti, tj, tid, m0, t0, acc);
            else count_group<false>(lds, p.si.g[g], p.sj.g[g], p.nblocks[g], ti, tj, tid, m0, t0, acc);
            if (g == 0) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) pk[k][e] = (uint32_t)acc[2 * k][e] | ((uint32_t)acc[2 * k + 1][e] << 16);
                    pk[4][e] = (uint32_t)acc[QQ][e];
                }
            }
        }
        // the pass's epilogue.  Every wave is past the last block's barrier, so nobody reads the images any more.  A lane reads
        // back the words it staged itself: the LDS only turns the static register index into a loop.
        const uint32_t row_w = wr * em::kWaveRows + 32u * m0, col_w = wc * em::kWaveCols + 32u * t0 + l32;
        const uint32_t j = tj * kSlab + col_w;
#pragma unroll 1
        for (uint32_t q = 0; q < 4u; ++q) {
            if (q == 0u) stage_quarter<0>(stage, half, l32, pk, acc);
            else if (q == 1u) stage_quarter<1>(stage, half, l32, pk, acc);
            else if (q == 2u) stage_quarter<2>(stage, half, l32, pk, acc);
            else stage_quarter<3>(stage, half, l32, pk, acc);
#pragma unroll 1
            for (uint32_t rr = 0; rr < 4u; ++rr) {
                const uint32_t at = (rr + 4u * half) * 32u + l32;
                const uint32_t row = row_w + 8u * q + rr + 4u * half;   // of the slab
                uint32_t w9[kStageWords];
#pragma unroll
                for (int k = 0; k < (int)kStageWords; ++k) w9[k] = stage[(uint32_t)k * kQuarter + at];
                uint32_t s[2][kSets];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s[0][2 * k] = w9[k] & 0xFFFFu, s[0][2 * k + 1] = w9[k] >> 16;
                    s[1][2 * k] = w9[5 + k] & 0xFFFFu, s[1][2 * k + 1] = w9[5 + k] >> 16;
                }
                s[0][QQ] = w9[4] & 0xFFFFu, s[1][QQ] = w9[4] >> 16;
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    if (!general[g]) {   // the shortcut's margins, from the tables
                        s[g][GQ] = sm.rdos[g][row], s[g][TQ] = sm.rhet[g][row];
                        s[g][QG] = sm.cdos[g][col_w], s[g][QT] = sm.chet[g][col_w];
                        s[g][QQ] = p.n_ind[g];
                    }
                }
                uint32_t n[18];
                table_of(s[0], n);
                table_of(s[1], n + 9);
                emit(ti * kSlab + row, j, n);
            }
        }
        emit.flush(j);
        block_sync();   // the next pass's first image overwrites what was staged
    }
}

// the self scan's walk: workgroup b -> the tile (ti, tj <= ti) with triangular number b
__device__ __forceinline__ void tri_tile(uint32_t b, uint32_t &ti, uint32_t &tj)
{
    uint32_t t = (uint32_t)((__builtin_sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while ((uint64_t)(t + 1u) * (t + 2u) / 2u <= b) ++t;
    while ((uint64_t)t * (t + 1u) / 2u > b) --t;
    ti = t;
    tj = b - (uint32_t)((uint64_t)t * (t + 1u) / 2u);
}

template <int kMode>
__global__ void __launch_bounds__(kThreads, 1) epi_kernel(Args p)
{
    __shared__ Smem sm;
    uint32_t ti, tj;
    if (p.self) tri_tile(blockIdx.x, ti, tj);
    else tile_of<em::kBandTiles>(blockIdx.x, n_slabs(p.si.n), n_slabs(p.sj.n), ti, tj);
    Emit<kMode> emit{p, HitAppender{p.hits, p.hit_cap, p.n_hits, threadIdx.x & 63u}, threadIdx.x & 63u};
    tile_body(sm, p, ti, tj, threadIdx.x, emit);
    if constexpr (kMode == kHits) emit.hit.close();   // what is left of the wave's last batch
}

// the epilogue alone: one thread per tuple of 18 integers
__global__ void __launch_bounds__(256) from_counts_kernel(size_t m, int test, const uint32_t *tuples, double *chisq, float *chisq32,
                                                          double *dir, double *lnp, uint8_t *flags, double *mu, uint32_t *cycles)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    const double nan = __builtin_nan("");
    uint32_t n[18];
    uint32_t tot[2] = {0u, 0u};
    bool fits = true;
#pragma unroll
    for (int s = 0; s < 18; ++s) {
        n[s] = tuples[k * 18u + s];
        fits = fits && n[s] <= LDX_MAX_HAPS / 2u;
        tot[s / 9] += fits ? n[s] : 0u;
    }
    fits = fits && tot[0] <= LDX_MAX_HAPS / 2u && tot[1] <= LDX_MAX_HAPS / 2u;
    double fit[18];
#pragma unroll
    for (int s = 0; s < 18; ++s) fit[s] = nan;
    Cell c{nan, nan, kFlagNoTable, 0u};
    if (fits) c = epi_cell<true>(test, n, fit);
    if (chisq) chisq[k] = c.chisq;
    if (chisq32) chisq32[k] = (float)c.chisq;
    if (dir) dir[k] = c.dir;
    if (lnp) lnp[k] = ln_p(test, c.chisq);
    if (flags) flags[k] = (uint8_t)c.flags;
    if (cycles) cycles[k] = c.cycles;
    if (mu) {
#pragma unroll
        for (int s = 0; s < 18; ++s) mu[k * 18u + s] = fit[s];
    }
}

template <int kMode>
static int launch(const Args &p, hipStream_t s)
{
    const uint32_t ti = n_slabs(p.si.n), tj = n_slabs(p.sj.n);
    const uint32_t grid = p.self ? (uint32_t)((uint64_t)ti * (ti + 1u) / 2u) : ti * tj;
    epi_kernel<kMode><<<grid, kThreads, 0, s>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

}  // namespace epi
}  // namespace ldx

using namespace ldx;

// one side's pointers; everything returns before any HIP call
static int side_ok(const char *who, const char *name, const ldx_epi_side *s)
{
    LDX_ARG_REQUIRE(s != nullptr, "%s: %s is a null pointer", who, name);
    LDX_ARG_REQUIRE(s->alt_case != nullptr && s->ref_case != nullptr && s->cnt_case != nullptr && s->alt_ctrl != nullptr &&
                        s->ref_ctrl != nullptr && s->cnt_ctrl != nullptr,
                    "%s: %s holds a null pointer", who, name);
    LDX_ARG_REQUIRE(((uintptr_t)s->cnt_case | (uintptr_t)s->cnt_ctrl) % 16u == 0u, "%s: %s: cnt_case and cnt_ctrl must be 16-byte aligned",
                    who, name);
    return LDX_OK;
}

// the scan entries' rules: both sides, the test, and rect_args_ok (ldx_common.h) for each group's haplotype count
static int scan_args_ok(const char *who, const ldx_epi_side *si, const ldx_epi_side *sj, uint32_t n_hap_case, uint32_t n_hap_ctrl,
                        int test)
{
    if (const int rc = side_ok(who, "side_i", si)) return rc;
    if (const int rc = side_ok(who, "side_j", sj)) return rc;
    LDX_ARG_REQUIRE(test == LDX_EPI_ALLELIC || test == LDX_EPI_BOOST, "%s: test %d is neither LDX_EPI_ALLELIC nor LDX_EPI_BOOST", who,
                    test);
    const char *const why = "haplotypes 2k and 2k + 1 are the two alleles of individual k";
    if (const int rc = rect_args_ok(who, si->n_snps, sj->n_snps, n_hap_case, why, kSlab)) return rc;
    return rect_args_ok(who, si->n_snps, sj->n_snps, n_hap_ctrl, why, kSlab);
}

static epi::Args make_args(const ldx_epi_side *si, const ldx_epi_side *sj, uint32_t n_hap_case, uint32_t n_hap_ctrl, int test)
{
    epi::Args p{};
    auto side = [](const ldx_epi_side *s) {
        return epi::Side{{epi::Group{(const uint4 *)s->alt_case, (const uint4 *)s->ref_case, (const uint4 *)s->cnt_case},
                          epi::Group{(const uint4 *)s->alt_ctrl, (const uint4 *)s->ref_ctrl, (const uint4 *)s->cnt_ctrl}},
                         s->n_snps};
    };
    p.si = side(si), p.sj = side(sj);
    p.nblocks[0] = n_chunks(n_hap_case) / 2u, p.nblocks[1] = n_chunks(n_hap_ctrl) / 2u;
    p.n_ind[0] = n_hap_case / 2u, p.n_ind[1] = n_hap_ctrl / 2u;
    p.test = test;
    return p;
}

extern "C" int ldx_epi_counts_dev(const ldx_epi_side *side_i, const ldx_epi_side *side_j, uint32_t n_hap_case, uint32_t n_hap_ctrl,
                                  uint32_t *counts, size_t ld, void *stream)
{
    const char *const who = "ldx_epi_counts_dev";
    if (const int rc = scan_args_ok(who, side_i, side_j, n_hap_case, n_hap_ctrl, LDX_EPI_BOOST)) return rc;
    LDX_ARG_PTR(who, counts);
    LDX_ARG_REQUIRE(ld >= side_j->n_snps, "%s: ld %zu < n_j %u", who, ld, side_j->n_snps);
    epi::Args p = make_args(side_i, side_j, n_hap_case, n_hap_ctrl, LDX_EPI_BOOST);
    p.counts = counts, p.ld = ld;
    return epi::launch<epi::kCounts>(p, (hipStream_t)stream);
}

extern "C" int ldx_epi_rect_dev(const ldx_epi_side *side_i, const ldx_epi_side *side_j, uint32_t n_hap_case, uint32_t n_hap_ctrl,
                                int test, float *chisq, float *dir, uint8_t *flags, size_t ld, void *stream)
{
    const char *const who = "ldx_epi_rect_dev";
    if (const int rc = scan_args_ok(who, side_i, side_j, n_hap_case, n_hap_ctrl, test)) return rc;
    LDX_ARG_PTR(who, chisq);
    LDX_ARG_REQUIRE(ld >= side_j->n_snps, "%s: ld %zu < n_j %u", who, ld, side_j->n_snps);
    epi::Args p = make_args(side_i, side_j, n_hap_case, n_hap_ctrl, test);
    p.out_x = chisq, p.out_dir = dir, p.out_flags = flags, p.ld = ld;
    return epi::launch<epi::kDense>(p, (hipStream_t)stream);
}

extern "C" int ldx_epi_hits_dev(const ldx_epi_side *side_i, const ldx_epi_side *side_j, uint32_t n_hap_case, uint32_t n_hap_ctrl,
                                int test, int self, float bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, float bound_sig,
                                uint32_t *n_tot, uint32_t *n_sig, uint64_t *best, void *stream)
{
    const char *const who = "ldx_epi_hits_dev";
    if (const int rc = scan_args_ok(who, side_i, side_j, n_hap_case, n_hap_ctrl, test)) return rc;
    LDX_ARG_REQUIRE(self == 0 || self == 1, "%s: self must be 0 or 1 (got %d)", who, self);
    LDX_ARG_REQUIRE(!self || (side_i->n_snps == side_j->n_snps && side_i->alt_case == side_j->alt_case &&
                              side_i->ref_case == side_j->ref_case && side_i->alt_ctrl == side_j->alt_ctrl &&
                              side_i->ref_ctrl == side_j->ref_ctrl),
                    "%s: self = 1 needs side_j to be side_i's panels", who);
    if (const int rc = hit_args_ok(who, bound, hits, hit_cap, n_hits)) return rc;
    const bool any = n_tot != nullptr || n_sig != nullptr || best != nullptr;
    LDX_ARG_REQUIRE(!any || (n_tot != nullptr && n_sig != nullptr && best != nullptr),
                    "%s: n_tot, n_sig and best are given together or not at all", who);
    LDX_ARG_REQUIRE(!any || bound_sig > 0.0f, "%s: bound_sig must be a float32 > 0 (got %g)", who, (double)bound_sig);
    epi::Args p = make_args(side_i, side_j, n_hap_case, n_hap_ctrl, test);
    p.self = self, p.bound = bound, p.bound_sig = bound_sig, p.hits = hits, p.hit_cap = hit_cap;
    p.n_hits = (unsigned long long *)n_hits, p.n_tot = n_tot, p.n_sig = n_sig, p.best = (unsigned long long *)best;
    LDX_HIP(hipMemsetAsync(n_hits, 0, sizeof(uint64_t), (hipStream_t)stream));   // the slot counter starts at 0
    return epi::launch<epi::kHits>(p, (hipStream_t)stream);
}

extern "C" int ldx_epi_from_counts_dev(size_t m, int test, const uint32_t *tuples, double *chisq, float *chisq32, double *dir,
                                       double *ln_p, uint8_t *flags, double *mu, uint32_t *cycles, void *stream)
{
    const char *const who = "ldx_epi_from_counts_dev";
    LDX_ARG_PTR(who, tuples);
    LDX_ARG_REQUIRE(m > 0u, "%s: m is 0", who);
    LDX_ARG_REQUIRE(test == LDX_EPI_ALLELIC || test == LDX_EPI_BOOST, "%s: test %d is neither LDX_EPI_ALLELIC nor LDX_EPI_BOOST", who,
                    test);
    if ((m + 255u) / 256u >= (1ull << 31)) {
        set_error("%s: m = %zu needs 2^31 or more workgroups", who, m);
        return LDX_E_UNSUPPORTED;
    }
    epi::from_counts_kernel<<<(uint32_t)((m + 255u) / 256u), 256, 0, (hipStream_t)stream>>>(m, test, tuples, chisq, chisq32, dir, ln_p,
                                                                                           flags, mu, cycles);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

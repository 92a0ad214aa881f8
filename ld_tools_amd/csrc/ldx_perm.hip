// max(T) permutation tests (include/ldx.h, "permutation tests"): for every SNP of a panel against every one of R
// permutations of the case/control labels the two exact integers a (ALT alleles among the permutation's cases) and R (the
// permutation's cases called at the SNP), from them the allelic or the trend chi-square of ldx_model_tests_dev, and of that
// rectangle only n counters (permutations at or above the SNP's observed statistic) and R maxima (the largest statistic of each
// permutation) -- nothing of the rectangle itself reaches memory, except in the counts form.
//   * labels_kernel: one workgroup per permutation.  Individual k is a case iff fewer than n_case individuals come before it in
//     the order of (key(p, k), k); the n_case-th element of that order is found by a radix select, a byte at a time, on the
//     composite (key, index) -- 8 + 2 digits, all composites distinct, so the select ends on ONE element, usually after two or
//     three digits -- and a ballot per 64 individuals writes the 16 bytes of a chunk.  Every byte of the plane is written.
//   * perm_kernel: the tile of the pairwise-complete EM rectangle (ldx_em_pw_tile.h) with the SNPs on I and the permutations on J.
//     I side (0.5 / 1): G = expand32_a4_dosage(w), g / 2, and Q = even_a4(q), 0.5 where called; J side: L = het_b4(label word), 2
//     where the individual is a case.  a = G.L and R = Q.L: every product is g or 1 and every sum at most 2 N <= 10 240 < 2^16 <
//     2^24, so the fp32 accumulators are exact in any order and a cell's two integers fit one word.
//   * a workgroup (4 waves as 2 x 2) owns 128 SNPs x 128 permutations, a wave 64 x 64 cells as 2 x 2 accumulator tiles of
//     32 x 32, twice (a and R): 128 accumulator registers, one pass.
//   * shortcut: a tile none of whose 128 SNPs has an uncalled individual (called == n_ind in the per-SNP table) runs the a set
//     alone and reads no REF plane: R = n_case.  The integers are the same either way, so a cell cannot tell the path.
//   * K loop: per K-block of 256 haplotypes (128 individuals) the workgroup expands the J slab's label bits once into an LDS
//     image [4 steps][2 halves][128 rows][8 B], double-buffered, one block_sync per K-block; a lane loads the 16 bytes of its two
//     I rows from each plane and expands them in registers.
//   * epilogue: a wave stages its 64 x 64 cells, a | R << 16, in the LDS the images no longer need, then walks the rows with one
//     column per lane: perm_cell per lane and row -- ONE function of (test, N, G, Q2, R, a), which the epilogue-alone entry calls
//     too --, a ballot and a popcount per row and one integer atomicAdd for it, the column's maximum in a register over the 64
//     rows and one atomicMax on its bits (a non-negative double orders as its bits do).  No floating-point atomics: the results
//     do not depend on the order of arrival.
//   * walk: tile_of (ldx_fp4.h), as the EM rectangle.
#include "ldx_em_pw_tile.h"

namespace ldx {
namespace perm {

using em::v2i;
using em::kThreads;
using em_pw::kOpBytes;
using em_pw::mfma2;

constexpr uint32_t kImage = kOpBytes;                                      // one buffer of the K loop: L (8 KiB)
constexpr uint32_t kStage = em::kWaves * em::kWaveRows * em::kWaveCols * 4u;   // the staged cells: 64 KiB
constexpr uint32_t kLdsBytes = kStage;
static_assert(2u * kImage <= kLdsBytes, "the staged cells live in the images' LDS");
constexpr uint32_t kMaxInd = LDX_MAX_HAPS / 2u;
static_assert(2u * kMaxInd < (1u << 16), "a and R of a cell share a word");
// det^2 and den of the allelic test are at most N^4 (|ad - bc| <= 2R 2S <= N^2; (2R)(2S) <= N^2 and G (2N - G) <= N^2), U^2 and
// den of the trend test at most N^4 / 4 (U = S a - R c, |U| <= 2 R S; N Q2 - G^2 <= N^2): exact in int64 and in a double.
static_assert((uint64_t)kMaxInd * kMaxInd * kMaxInd * kMaxInd < (1ull << 53), "det^2 and den are exact doubles for N <= LDX_MAX_HAPS / 2");

constexpr uint32_t kFlagOk = 0, kFlagEmpty = 1, kFlagDen0 = 2, kFlagNoTable = 4;

// ---- the statistic: (test, N, G, Q2, R, a) -> chisq; false where den = 0.  fp64, -ffp-contract=off, each operation once --------
// The integers are carried as doubles: every operand, product, sum and difference up to det^2, U^2 and den is an integer below
// 2^53 in magnitude (the bounds above; a, b, c, d >= 0 for the margins of a table), so each fp64 operation on them IS the int64
// one, at a fraction of the instructions of a 64-bit integer multiply.  The two operations that round are the definition's: the
// product with T and the quotient.
__device__ __forceinline__ bool perm_cell(int test, uint32_t n_called, uint32_t g_sum, uint32_t q2_sum, uint32_t r_called, uint32_t a_alt,
                                          double &chisq)
{
    const double N = (double)n_called, G = (double)g_sum, R = (double)r_called, a = (double)a_alt, S = N - R;
    if (test == LDX_PERM_ALLELIC) {
        const double b = 2.0 * R - a, c = G - a, d = 2.0 * S - c;
        const double den = ((a + b) * (c + d)) * ((a + c) * (b + d));
        if (den == 0.0) return false;
        const double det = a * d - b * c;
        chisq = ((2.0 * N) * (det * det)) / den;
        return true;
    }
    const double U = N * a - R * G;
    const double den = (R * S) * (N * (double)q2_sum - G * G);
    if (den == 0.0) return false;
    chisq = (N * (U * U)) / den;
    return true;
}

// ---- labels ---------------------------------------------------------------------------------------------------------------------
// key(p, k) = key64(seed, i = p, h = k) of ldx_common.h: the synthetic panels' key (ldx_synth.hip, ld_tools_amd/synth.py)
constexpr uint32_t kLabThreads = 256;
constexpr uint32_t kLabPer = kMaxInd / kLabThreads;   // individuals per thread: 20
static_assert(kLabPer * kLabThreads == kMaxInd && kLabPer <= 32u, "a thread's individuals fit a 32-bit mask");
static_assert(kMaxInd <= (1u << 16), "the index is two digits of the composite");

// digit d of the composite (key, k): the key's bytes from the top, then the index's two
__device__ __forceinline__ uint32_t digit_of(uint32_t d, uint64_t key, uint32_t k)
{
    return d < 8u ? (uint32_t)(key >> (56u - 8u * d)) & 255u : (d == 8u ? (k >> 8) & 255u : k & 255u);
}

__global__ void __launch_bounds__(kLabThreads) labels_kernel(uint64_t seed, uint64_t first, uint32_t n_perm, uint32_t n, uint32_t n_case,
                                                             uint32_t nchunks, uint4 *plane)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[3];      // the digit chosen, the rank inside it, its elements
    __shared__ uint64_t t_key;       // the n_case-th composite
    __shared__ uint32_t t_idx;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t row = blockIdx.x;   // of the padded plane: n_slabs(n_perm) * 128 rows
    uint4 *const dst = plane + ((size_t)(row / kSlab) * nchunks * kSlab + row % kSlab);   // + chunk * kSlab
    if (row >= n_perm) {   // a pad row: zero bits
        for (uint32_t c = tid; c < nchunks; c += kLabThreads) dst[(size_t)c * kSlab] = uint4{0u, 0u, 0u, 0u};
        return;
    }
    const uint64_t p = first + row;
    uint64_t key[kLabPer];
    uint32_t alive = 0u;             // bit s: individual s * 256 + tid is still a candidate
#pragma unroll
    for (uint32_t s = 0; s < kLabPer; ++s) {
        const uint32_t k = s * kLabThreads + tid;
        key[s] = key64(seed, p, k);
        alive |= (k < n ? 1u : 0u) << s;
    }
    uint32_t want = n_case - 1u;     // the rank, among the candidates, of the element looked for
#pragma unroll 1
    for (uint32_t d = 0; d < 10u; ++d) {
        hist[tid] = 0u;
        block_sync();
#pragma unroll
        for (uint32_t s = 0; s < kLabPer; ++s)
            if ((alive >> s) & 1u) atomicAdd(&hist[digit_of(d, key[s], s * kLabThreads + tid)], 1u);
        block_sync();
        if (wave == 0u) {   // lane l owns the digits 4 l .. 4 l + 3
            const uint32_t c0 = hist[4u * lane], c1 = hist[4u * lane + 1u], c2 = hist[4u * lane + 2u], c3 = hist[4u * lane + 3u];
            const uint32_t tot = c0 + c1 + c2 + c3;
            uint32_t incl = tot;
#pragma unroll
            for (uint32_t o = 1; o < 64u; o <<= 1) {
                const uint32_t up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            const uint32_t excl = incl - tot;
            if (want >= excl && want < incl) {   // exactly one lane: want < the candidates
                uint32_t r = want - excl, b = 0u, c = c0;
                if (r >= c0) { r -= c0, b = 1u, c = c1;
                    if (r >= c1) { r -= c1, b = 2u, c = c2;
                        if (r >= c2) { r -= c2, b = 3u, c = c3; } } }
                sel[0] = 4u * lane + b, sel[1] = r, sel[2] = c;
            }
        }
        block_sync();
        const uint32_t bin = sel[0], cnt = sel[2];
        want = sel[1];
#pragma unroll
        for (uint32_t s = 0; s < kLabPer; ++s)
            if (((alive >> s) & 1u) && digit_of(d, key[s], s * kLabThreads + tid) != bin) alive &= ~(1u << s);
        if (cnt == 1u) break;   // workgroup-uniform; the composites are distinct, so the tenth digit ends here at the latest
    }
#pragma unroll
    for (uint32_t s = 0; s < kLabPer; ++s)
        if ((alive >> s) & 1u) t_key = key[s], t_idx = s * kLabThreads + tid;   // ONE candidate is left
    block_sync();
    const uint64_t tk = t_key;
    const uint32_t ti = t_idx;
#pragma unroll
    for (uint32_t s = 0; s < kLabPer; ++s) {
        const uint32_t k = s * kLabThreads + tid;
        const bool is_case = k < n && (key[s] < tk || (key[s] == tk && k <= ti));
        const unsigned long long m = __ballot(is_case);   // the wave's 64 individuals: one chunk of 128 haplotypes
        const uint32_t chunk = 4u * s + wave;
        if (lane == 0u && chunk < nchunks)
            dst[(size_t)chunk * kSlab] = uint4{spread16((uint32_t)m & 0xFFFFu), spread16((uint32_t)(m >> 16) & 0xFFFFu),
                                               spread16((uint32_t)(m >> 32) & 0xFFFFu), spread16((uint32_t)(m >> 48))};
    }
}

// ---- the scan -------------------------------------------------------------------------------------------------------------------
struct Args {
    const uint4 *alt, *ref;   // the panel's tiled bit planes
    const uint4 *cnt;         // [n_snps] {called, het, hom ALT, 0}
    const uint4 *lab;         // the label plane
    uint32_t n_snps, n_perm, nblocks, n_ind, n_case;
    int test;
    const double *stat;       // scan: the observed statistic, NaN = the SNP takes no part
    uint32_t *n_ge;
    unsigned long long *max;
    uint32_t *counts;         // counts: [2][n_snps][ld]
    size_t ld;
};

struct Smem {
    __attribute__((aligned(16))) unsigned char lds[kLdsBytes];   // K loop: two image buffers; epilogue: the staged cells
    uint32_t rN[kSlab], rG[kSlab], rQ2[kSlab];                    // the workgroup's 128 rows: called, het + 2 hom, het + 4 hom
    double rstat[kSlab];
    uint32_t wflag[em::kWaves];
};

// the K loop: acc_a += G.L and, where kGeneral, acc_r += Q.L of I slab ti x J slab tj.  Called by the whole workgroup; on return
// every wave is past the last block's barrier.  Accumulator (m, tt, e) is row 32 m + (e & 3) + 8 (e >> 2) + 4 half of the wave's
// 64, column 32 tt + l32.
template <bool kGeneral>
__device__ __forceinline__ void count_sets(unsigned char *lds, const Args &p, uint32_t ti, uint32_t tj, uint32_t tid, v16f (&acc_a)[2][2],
                                           v16f (&acc_r)[2][2])
{
    const uint32_t lane = tid & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wr = wave >> 1, wc = wave & 1u;
    const uint32_t nchunks = 2u * p.nblocks;
    // lane's A source: rows 64 wr + l32 and + 32 of slab ti, chunk 2 blk + half; planes are < 4 GiB: 32-bit indices
    const uint32_t a_off = (ti * nchunks + half) * kSlab + wr * em::kWaveRows + l32;
    // thread's share of the J image: row tid % 128, chunk 2 blk + tid / 128
    const uint32_t b_row = tid & (kSlab - 1u), b_half = tid >> 7;
    const uint32_t b_off = (tj * nchunks + b_half) * kSlab + b_row;
    const uint32_t b_dst = b_half * kSlab + b_row;   // + step * 256
    auto load_a = [&](uint4 (&a)[2], uint4 (&r)[2], uint32_t blk) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            a[m] = p.alt[a_off + 32u * (uint32_t)m + (size_t)blk * em::kBlockVecs];
            if constexpr (kGeneral) r[m] = p.ref[a_off + 32u * (uint32_t)m + (size_t)blk * em::kBlockVecs];
        }
    };
    auto load_b = [&](uint32_t blk) { return p.lab[b_off + (size_t)blk * em::kBlockVecs]; };
    auto expand_b = [&](unsigned char *buf, const uint4 &bits) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            reinterpret_cast<v2i *>(buf)[b_dst + (uint32_t)q * em::kBlockVecs] = em::het_b4(word_of(bits, q));
    };
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc_a[m][tt][e] = 0.0f, acc_r[m][tt][e] = 0.0f;

    uint4 a_alt[2], a_ref[2] = {}, n_alt[2], n_ref[2] = {};
    load_a(a_alt, a_ref, 0u);
    // (the first buffer is free: the caller's barrier is behind every wave)
    expand_b(lds, load_b(0u));
    block_sync();
    for (uint32_t blk = 0; blk < p.nblocks; ++blk) {
        const uint32_t nb = blk + 1u < p.nblocks ? blk + 1u : blk;   // (beyond the last block the loads repeat it: discarded)
        const uint4 bits = load_b(nb);
        load_a(n_alt, n_ref, nb);
        __builtin_amdgcn_sched_barrier(0);   // the global loads stay at the top of the block
        const v2i *const rd = reinterpret_cast<const v2i *>(lds + (blk & 1u) * kImage);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            v2i bl[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) bl[tt] = rd[((uint32_t)w * 2u + half) * kSlab + wc * em::kWaveCols + 32u * (uint32_t)tt + l32];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const uint32_t wa = word_of(a_alt[m], w);
                uint32_t qc = 0u, ww = wa;
                if constexpr (kGeneral) {
                    qc = ind_called(wa, word_of(a_ref[m], w));
                    ww = wa & (qc | (qc << 1));   // a half-missing genotype is missing
                }
                const v4i g4 = expand32_a4_dosage(ww);
                const v2i xg = {g4.x, g4.z};
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) acc_a[m][tt] = mfma2(xg, bl[tt], acc_a[m][tt]);
                if constexpr (kGeneral) {
                    const v4i q4 = even_a4(qc);
                    const v2i xq = {q4.x, q4.z};
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) acc_r[m][tt] = mfma2(xq, bl[tt], acc_r[m][tt]);
                }
            }
        }
        expand_b(lds + ((blk + 1u) & 1u) * kImage, bits);
        block_sync();
#pragma unroll
        for (int m = 0; m < 2; ++m) a_alt[m] = n_alt[m], a_ref[m] = n_ref[m];
    }
}

template <bool kCounts>
__global__ void __launch_bounds__(kThreads, 2) perm_kernel(Args p)   // two workgroups per CU: 256 registers, 2 x 66.5 KiB of LDS
{
    __shared__ Smem sm;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wr = wave >> 1, wc = wave & 1u;
    uint32_t ti, tj;
    tile_of<em::kBandTiles>(blockIdx.x, n_slabs(p.n_snps), n_slabs(p.n_perm), ti, tj);

    // ---- the rows' tables, and does a SNP of this tile hold an uncalled individual?  Thread t < 128 owns row t of the slab.
    {
        const uint32_t x = ti * kSlab + tid;
        const bool live = tid < kSlab && x < p.n_snps;
        const uint4 k = live ? p.cnt[x] : uint4{0u, 0u, 0u, 0u};
        if (tid < kSlab) {
            sm.rN[tid] = k.x, sm.rG[tid] = k.y + 2u * k.z, sm.rQ2[tid] = k.y + 4u * k.z;
            sm.rstat[tid] = live && p.stat ? p.stat[x] : __builtin_nan("");
        }
        const bool wave_hole = __any(live && k.x != p.n_ind);
        if (lane == 0) sm.wflag[wave] = wave_hole ? 1u : 0u;
    }
    block_sync();
    const bool general = __builtin_amdgcn_readfirstlane(sm.wflag[0] | sm.wflag[1] | sm.wflag[2] | sm.wflag[3]) != 0u;

    v16f acc_a[2][2], acc_r[2][2];
    if (general) count_sets<true>(sm.lds, p, ti, tj, tid, acc_a, acc_r);
    else count_sets<false>(sm.lds, p, ti, tj, tid, acc_a, acc_r);

    // ---- the wave's 64 x 64 cells, [row][column] words a | R << 16 (both are exact integers below 2^16)
    uint32_t *const stage = reinterpret_cast<uint32_t *>(sm.lds) + wave * (em::kWaveRows * em::kWaveCols);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t row = 32u * (uint32_t)m + (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * half;
                stage[row * em::kWaveCols + 32u * (uint32_t)tt + l32] = (uint32_t)acc_a[m][tt][e] | ((uint32_t)acc_r[m][tt][e] << 16);
            }
    block_sync();   // the lanes of a wave read each other's words

    // ---- the epilogue: one column per lane, the rows one after the other
    const uint32_t j = tj * kSlab + wc * em::kWaveCols + lane;
    const bool col_ok = j < p.n_perm;
    const uint32_t row0 = ti * kSlab + wr * em::kWaveRows;
    const uint32_t rows = row0 < p.n_snps ? (p.n_snps - row0 < em::kWaveRows ? p.n_snps - row0 : em::kWaveRows) : 0u;   // wave-uniform
    double cmax = 0.0;
    for (uint32_t rr = 0; rr < rows; ++rr) {
        const uint32_t word = stage[rr * em::kWaveCols + lane];
        const uint32_t a = word & 0xFFFFu, R = general ? word >> 16 : p.n_case;
        const uint32_t i = row0 + rr, r = wr * em::kWaveRows + rr;
        if constexpr (kCounts) {
            if (col_ok) {
                __builtin_nontemporal_store(a, p.counts + (size_t)i * p.ld + j);
                __builtin_nontemporal_store(R, p.counts + ((size_t)p.n_snps + i) * p.ld + j);
            }
        } else {
            const double stat = sm.rstat[r];   // one address per wave: broadcast
            if (stat != stat) continue;        // a flagged SNP: no counter, no maximum (wave-uniform)
            double chisq = 0.0;
            const bool valid = perm_cell(p.test, sm.rN[r], sm.rG[r], sm.rQ2[r], R, a, chisq) && col_ok;
            const uint32_t n_ge = (uint32_t)__builtin_popcountll(__ballot(valid && chisq >= stat));
            if (lane == 0u && n_ge != 0u) atomicAdd(p.n_ge + i, n_ge);
            if (valid && chisq > cmax) cmax = chisq;
        }
    }
    if constexpr (!kCounts) {
        // chisq >= +0: the bits order as the values, and +0.0 is "none"
        if (cmax > 0.0) atomicMax(p.max + j, (unsigned long long)__double_as_longlong(cmax));
    }
}

// the epilogue alone: one thread per tuple (N, het, hom, R, a)
__global__ void __launch_bounds__(256) from_counts_kernel(size_t m, int test, const uint32_t *n_, const uint32_t *het_, const uint32_t *hom_,
                                                          const uint32_t *r_, const uint32_t *a_, double *chisq, uint8_t *flags)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    const int64_t N = n_[k], het = het_[k], hom = hom_[k], R = r_[k], a = a_[k];
    const int64_t G = het + 2 * hom, Q2 = het + 4 * hom, S = N - R;
    double x = __builtin_nan("");
    uint32_t flag = kFlagOk;
    // no table with these margins: the cases' and the controls' ALT alleles do not fit their called individuals
    if (N > (int64_t)kMaxInd || het + hom > N || R > N || a > 2 * R || a > G || G - a > 2 * S) flag = kFlagNoTable;
    else if (R == 0 || S == 0) flag = kFlagEmpty;
    else if (!perm_cell(test, (uint32_t)N, (uint32_t)G, (uint32_t)Q2, (uint32_t)R, (uint32_t)a, x)) flag = kFlagDen0;
    chisq[k] = flag == kFlagOk ? x : __builtin_nan("");
    flags[k] = (uint8_t)flag;
}

}  // namespace perm
}  // namespace ldx

using namespace ldx;

// the shape rules the entries share, in this order; everything returns before any HIP call
static int shape_ok(const char *who, uint32_t n_rows, const char *rows_name, uint32_t n_perm, uint32_t n_hap, uint32_t n_case)
{
    LDX_ARG_REQUIRE(n_rows != 0u && n_perm != 0u, "%s: %s is 0", who, n_rows == 0u ? rows_name : "n_perm");
    LDX_ARG_REQUIRE(n_hap != 0u && n_hap % 2u == 0u, "%s: n_hap %u must be even and non-zero (haplotypes 2k and 2k + 1 are individual k)",
                    who, n_hap);
    if (n_hap > LDX_MAX_HAPS) {
        set_error("%s: n_hap %u > LDX_MAX_HAPS %u", who, n_hap, LDX_MAX_HAPS);
        return LDX_E_UNSUPPORTED;
    }
    LDX_ARG_REQUIRE(n_case >= 1u && n_case < n_hap / 2u, "%s: n_case %u outside 1 .. n - 1 = %u", who, n_case, n_hap / 2u - 1u);
    if (const int rc = plane_check(who, "labels", n_perm, n_hap)) return rc;
    return LDX_OK;
}

static int scan_args_ok(const char *who, const void *alt, const void *ref, const uint32_t *cnt, uint32_t n_snps, uint32_t n_hap,
                        const void *labels, uint32_t n_perm, uint32_t n_case)
{
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, ref); LDX_ARG_PTR(who, cnt); LDX_ARG_PTR(who, labels);
    LDX_ARG_REQUIRE(((uintptr_t)cnt & 15u) == 0u, "%s: cnt must be 16-byte aligned", who);
    if (const int rc = shape_ok(who, n_snps, "n_snps", n_perm, n_hap, n_case)) return rc;
    if (const int rc = plane_check(who, "alt", n_snps, n_hap)) return rc;
    if ((uint64_t)n_slabs(n_snps) * n_slabs(n_perm) >= (1ull << 31)) {
        set_error("%s: n_snps x n_perm = %u x %u needs 2^31 or more tiles", who, n_snps, n_perm);
        return LDX_E_UNSUPPORTED;
    }
    return LDX_OK;
}

static perm::Args make_args(const void *alt, const void *ref, const uint32_t *cnt, uint32_t n_snps, uint32_t n_hap, const void *labels,
                            uint32_t n_perm, uint32_t n_case, int test)
{
    perm::Args p{};
    p.alt = (const uint4 *)alt, p.ref = (const uint4 *)ref, p.cnt = (const uint4 *)cnt, p.lab = (const uint4 *)labels;
    p.n_snps = n_snps, p.n_perm = n_perm, p.nblocks = n_chunks(n_hap) / 2u, p.n_ind = n_hap / 2u, p.n_case = n_case, p.test = test;
    return p;
}

extern "C" int ldx_perm_labels_dev(uint64_t seed, uint64_t first, uint32_t n_perm, uint32_t n_hap, uint32_t n_case, void *labels,
                                   void *stream)
{
    const char *const who = "ldx_perm_labels_dev";
    LDX_ARG_PTR(who, labels);
    if (const int rc = shape_ok(who, n_perm, "n_perm", n_perm, n_hap, n_case)) return rc;
    perm::labels_kernel<<<n_slabs(n_perm) * kSlab, perm::kLabThreads, 0, (hipStream_t)stream>>>(seed, first, n_perm, n_hap / 2u, n_case,
                                                                                                  n_chunks(n_hap), (uint4 *)labels);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_perm_scan_dev(const void *alt, const void *ref, const uint32_t *cnt, uint32_t n_snps, uint32_t n_hap,
                                 const void *labels, uint32_t n_perm, uint32_t n_case, int test, const double *stat, uint32_t *n_ge,
                                 uint64_t *max, void *stream)
{
    const char *const who = "ldx_perm_scan_dev";
    LDX_ARG_PTR(who, stat); LDX_ARG_PTR(who, n_ge); LDX_ARG_PTR(who, max);
    LDX_ARG_REQUIRE(test == LDX_PERM_ALLELIC || test == LDX_PERM_TREND, "%s: test %d is neither LDX_PERM_ALLELIC nor LDX_PERM_TREND", who,
                    test);
    if (const int rc = scan_args_ok(who, alt, ref, cnt, n_snps, n_hap, labels, n_perm, n_case)) return rc;
    perm::Args p = make_args(alt, ref, cnt, n_snps, n_hap, labels, n_perm, n_case, test);
    p.stat = stat, p.n_ge = n_ge, p.max = (unsigned long long *)max;
    perm::perm_kernel<false><<<n_slabs(n_snps) * n_slabs(n_perm), perm::kThreads, 0, (hipStream_t)stream>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_perm_counts_dev(const void *alt, const void *ref, const uint32_t *cnt, uint32_t n_snps, uint32_t n_hap,
                                   const void *labels, uint32_t n_perm, uint32_t n_case, uint32_t *counts, size_t ld, void *stream)
{
    const char *const who = "ldx_perm_counts_dev";
    LDX_ARG_PTR(who, counts);
    if (const int rc = scan_args_ok(who, alt, ref, cnt, n_snps, n_hap, labels, n_perm, n_case)) return rc;
    LDX_ARG_REQUIRE(ld >= n_perm, "%s: ld %zu < n_perm %u", who, ld, n_perm);
    perm::Args p = make_args(alt, ref, cnt, n_snps, n_hap, labels, n_perm, n_case, LDX_PERM_ALLELIC);
    p.counts = counts, p.ld = ld;
    perm::perm_kernel<true><<<n_slabs(n_snps) * n_slabs(n_perm), perm::kThreads, 0, (hipStream_t)stream>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_perm_from_counts_dev(size_t m, int test, const uint32_t *n, const uint32_t *het, const uint32_t *hom, const uint32_t *r,
                                        const uint32_t *a, double *chisq, uint8_t *flags, void *stream)
{
    const char *const who = "ldx_perm_from_counts_dev";
    LDX_ARG_PTR(who, n); LDX_ARG_PTR(who, het); LDX_ARG_PTR(who, hom); LDX_ARG_PTR(who, r); LDX_ARG_PTR(who, a);
    LDX_ARG_PTR(who, chisq); LDX_ARG_PTR(who, flags);
    LDX_ARG_REQUIRE(m != 0u && m <= (size_t)1 << 38, "%s: m %zu must lie in 1 .. 2^38", who, m);
    LDX_ARG_REQUIRE(test == LDX_PERM_ALLELIC || test == LDX_PERM_TREND, "%s: test %d is neither LDX_PERM_ALLELIC nor LDX_PERM_TREND", who,
                    test);
    perm::from_counts_kernel<<<(uint32_t)((m + 255u) / 256u), 256, 0, (hipStream_t)stream>>>(m, test, n, het, hom, r, a, chisq, flags);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

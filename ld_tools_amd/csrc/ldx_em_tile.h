// What the EM kernels share (em_rect_kernel of ldx_em.hip and emband_kernel of ldx_emband.hip, both through tile_body of
// ldx_em_pw_tile.h): the tile's
// geometry, the het operands, the two-set K loop (S and H of a 128 x 128 tile without missing codes) with its packed LDS
// staging, and the epilogue em_cell -- ONE function of (N, a_i, a_j, S, H), so that a cell cannot depend on the kernel, the
// tile or the path it came from.
#pragma once

#include "ldx_fp4.h"

namespace ldx {
namespace em {

typedef int v2i __attribute__((ext_vector_type(2)));

constexpr uint32_t kWaves = 4, kThreads = kWaves * 64u;
constexpr uint32_t kWaveRows = 64, kWaveCols = 64;    // a wave's cells: 2 x 2 accumulator tiles of 32 x 32, twice (S and H)
constexpr uint32_t kBandTiles = 32;                   // I blocks per band of the walk: 4096 rows, as the rectangle's
constexpr uint32_t kBlockVecs = 2u * kSlab;           // 16-byte vectors of one K-block of a slab in the plane (two chunks)
constexpr uint32_t kImageS = 4u * 2u * kSlab * 16u;   // bytes of one S image: [4 steps][2 halves][128 rows][16 B]
constexpr uint32_t kImageH = 4u * 2u * kSlab * 8u;    // bytes of one H image: [4 steps][2 halves][128 rows][8 B]
constexpr uint32_t kImage = kImageS + kImageH;        // one buffer of the K loop: 24 KiB
constexpr uint32_t kStage = kWaves * kWaveRows * kWaveCols * 4u;   // the epilogue's packed counts: 64 KiB
constexpr uint32_t kLdsBytes = kStage > 2u * kImage ? kStage : 2u * kImage;
constexpr uint32_t kPackShift = 13;                   // packed cell = S << 13 | H  (H <= 5120 < 2^13, S <= 20480 < 2^15)
constexpr int kRootTrips = 128;                       // bound of the root search (bisection alone needs ~70 from [0, 5120])

// the het bits of a word's 16 individuals, on their even haplotype slots
__device__ __forceinline__ uint32_t het_bits(uint32_t w) { return (w ^ (w >> 1)) & 0x55555555u; }
// expand32_a4 / expand32_b4 of a het word: the odd slots are empty, so registers 1 and 3 are zero and only 0 and 2 are kept
__device__ __forceinline__ v2i het_a4(uint32_t x) { return v2i{(int)(x & 0x11111111u), (int)((x >> 2) & 0x11111111u)}; }   // 0.5, 0.5
__device__ __forceinline__ v2i het_b4(uint32_t x) { return v2i{(int)((x << 2) & 0x44444444u), (int)(x & 0x44444444u)}; }   // 2, 2

// ---- the epilogue: (N, a_i, a_j, S, H) -> x*, r, D' in fp64 (include/ldx.h has the definitions) ------------------------------
// Everything that enters is an integer below 2^53, every expression is symmetric in the two SNPs (n2 <-> n3 under the swap:
// they meet only in commutative sums and products), and -ffp-contract=off keeps each operation as written.
struct Table {
    double n1, n4;      // ALT.ALT, REF.REF haplotypes of known phase
    double m2, m3;      // n2 + H, n3 + H: h2 = m2 - x, h3 = m3 - x
    double n2, n3;
    double H;
};
// g(x) = x h2 h3 - (H - x) h1 h4 in the product form: two non-negative terms and one subtraction
__device__ __forceinline__ double em_g(const Table &t, double x)
{
    const double h1 = t.n1 + x, h4 = t.n4 + x, h2 = t.m2 - x, h3 = t.m3 - x;
    return x * (h2 * h3) - (t.H - x) * (h1 * h4);
}
__device__ __forceinline__ double em_dg(const Table &t, double x)
{
    const double h1 = t.n1 + x, h4 = t.n4 + x, h2 = t.m2 - x, h3 = t.m3 - x;
    return (h2 * h3 - x * (h2 + h3)) + (h1 * h4 - (t.H - x) * (h1 + h4));
}
// l(x) up to the constant T ln T; 0 ln 0 = 0 (n > 0 implies h >= n > 0, and H > 0 implies h1 h4 + h2 h3 > 0)
__device__ __forceinline__ double em_loglik(const Table &t, double x)
{
    const double h1 = t.n1 + x, h4 = t.n4 + x, h2 = t.m2 - x, h3 = t.m3 - x;
    const double l14 = (t.n1 > 0.0 ? t.n1 * log(h1) : 0.0) + (t.n4 > 0.0 ? t.n4 * log(h4) : 0.0);
    const double l23 = (t.n2 > 0.0 ? t.n2 * log(h2) : 0.0) + (t.n3 > 0.0 ? t.n3 * log(h3) : 0.0);
    return (l14 + l23) + t.H * log(h1 * h4 + h2 * h3);
}
// the root of g in [lo, hi] with g(lo) <= 0 <= g(hi): Newton steps kept inside the bracket, bisection where a step leaves
// it or gains too little.  An end that is a root is returned as it is (lo first).
__device__ __forceinline__ double em_root(const Table &t, double lo, double hi, double glo, double ghi)
{
    if (glo == 0.0) return lo;
    if (ghi == 0.0) return hi;
    double x = 0.5 * (lo + hi), dxold = hi - lo, dx = dxold;
    double g = em_g(t, x), dg = em_dg(t, x);
    for (int it = 0; it < kRootTrips && g != 0.0; ++it) {
        if (g < 0.0) lo = x; else hi = x;
        const bool bisect = ((x - hi) * dg - g) * ((x - lo) * dg - g) > 0.0 || __builtin_fabs(2.0 * g) > __builtin_fabs(dxold * dg);
        dxold = dx;
        double xn;
        if (bisect) {
            dx = 0.5 * (hi - lo);
            xn = lo + dx;
        } else {
            dx = g / dg;
            xn = x - dx;
        }
        if (xn == x) break;
        x = xn;
        g = em_g(t, x);
        dg = em_dg(t, x);
    }
    return x;
}

struct Cell {
    float r, dprime;
    double x;
};
// Tie rule: where two local maxima have the same l in this fp64 evaluation, the smaller x wins.
__device__ __forceinline__ Cell em_cell(uint32_t n_ind, uint32_t a_i, uint32_t a_j, uint32_t S, uint32_t H)
{
    const double nan = __builtin_nan("");
    const int64_t T = 2 * (int64_t)n_ind, ai = a_i, aj = a_j, h = H;
    const int64_t n1 = ((int64_t)S - h) / 2, n2 = ai - n1 - h, n3 = aj - n1 - h, n4 = T - ai - aj + n1;
    // no genotype table: NaN everywhere
    if (ai > T || aj > T || h > (int64_t)n_ind || (int64_t)S < h || (((int64_t)S - h) & 1) != 0 || n2 < 0 || n3 < 0 || n4 < 0)
        return Cell{(float)nan, (float)nan, nan};
    if (ai == 0 || ai == T || aj == 0 || aj == T) return Cell{-0.0f, -0.0f, 0.0};   // degenerate (H is 0 there)

    double x = 0.0;
    if (h > 0) {   // H = 0: fully phased, x* = 0
        Table t;
        t.n1 = (double)n1, t.n4 = (double)n4, t.n2 = (double)n2, t.n3 = (double)n3;
        t.m2 = (double)(n2 + h), t.m3 = (double)(n3 + h), t.H = (double)h;
        const double g0 = -(t.H * (t.n1 * t.n4)), gH = t.H * (t.n2 * t.n3);   // g(0) <= 0 <= g(H), exact
        // g' = 6 x^2 + 2 c2 x + c1: its discriminant / 4 is c2^2 - 6 c1, an exact integer
        const double c2 = (double)(n1 + n4 - n2 - n3 - 3 * h);
        const double c1 = (double)((n2 + h) * (n3 + h) - h * (n1 + n4) + n1 * n4);
        const double disc = c2 * c2 - 6.0 * c1;
        if (disc <= 0.0) {
            x = em_root(t, 0.0, t.H, g0, gH);   // g is monotone on [0, H]
        } else {
            // g rises on (-inf, xa] and on [xb, inf): at most one local maximum of l on each
            const double sq = __builtin_sqrt(disc);
            const double xa = (-c2 - sq) / 6.0, xb = (-c2 + sq) / 6.0;
            bool have1 = false, have2 = false;
            double hi1 = 0.0, ghi1 = 0.0, lo2 = 0.0, glo2 = 0.0;
            if (xa > 0.0) {
                hi1 = xa < t.H ? xa : t.H;
                ghi1 = xa < t.H ? em_g(t, hi1) : gH;
                have1 = ghi1 >= 0.0;
            }
            if (xb < t.H) {
                lo2 = xb > 0.0 ? xb : 0.0;
                glo2 = xb > 0.0 ? em_g(t, lo2) : g0;
                have2 = glo2 <= 0.0;
            }
            if (have1 && have2) {
                const double x1 = em_root(t, 0.0, hi1, g0, ghi1), x2 = em_root(t, lo2, t.H, glo2, gH);
                x = em_loglik(t, x2) > em_loglik(t, x1) ? x2 : x1;
            } else if (have1) {
                x = em_root(t, 0.0, hi1, g0, ghi1);
            } else if (have2) {
                x = em_root(t, lo2, t.H, glo2, gH);
            } else {
                x = em_root(t, 0.0, t.H, g0, gH);   // a rounded g at a critical point hid both brackets: the whole interval
            }
        }
    }
    // D in units of 1 / T^2: Dn = T (n1 + x) - a_i a_j, the integer part exact
    const double Td = (double)T;
    const double dn = __builtin_fma(Td, x, (double)(T * n1 - ai * aj));
    const double vi = (double)(ai * (T - ai)), vj = (double)(aj * (T - aj));
    const double r = dn / __builtin_sqrt(vi * vj);
    const int64_t u = ai * (T - aj), v = (T - ai) * aj, p = ai * aj, q = (T - ai) * (T - aj);
    const double dmax = dn >= 0.0 ? (double)(u < v ? u : v) : (double)(p < q ? p : q);
    return Cell{(float)r, (float)(__builtin_fabs(dn) / dmax), x};
}

// ---- the D' confidence bounds of a pair (include/ldx.h, "Gabriel blocks"): (N, a_i, a_j, S, H) -> lo, hi in percent -----------
// ONE function of the five integers, like em_cell, which it calls for the sign: the likelihood of the table on the 101 grid
// points D' = k / 100 of the sign's side, L_k = em_loglik's function at h1 = (a_i a_j + s k Dm / 100) / T (every h clamped below
// at 2^-20; a term with count 0 skipped), the weights exp(L_k - max L) summed ascending, and the two 5 % tails.  The 101
// values live in a per-lane array (scratch): one pass of logarithms, one of exponentials, two of sums.
constexpr int kCiGrid = 100;
constexpr uint8_t kNoCi = 0xFF;       // no interval: no genotype table, or a degenerate pair
struct Ci {
    uint8_t lo, hi;
};
__device__ __forceinline__ Ci ci_cell(uint32_t n_ind, uint32_t a_i, uint32_t a_j, uint32_t S, uint32_t H)
{
    const Cell c = em_cell(n_ind, a_i, a_j, S, H);
    const int64_t T = 2 * (int64_t)n_ind, ai = a_i, aj = a_j, h = H;
    if (c.r != c.r || ai == 0 || ai == T || aj == 0 || aj == T) return Ci{kNoCi, kNoCi};
    const int64_t n1 = ((int64_t)S - h) / 2, n2 = ai - n1 - h, n3 = aj - n1 - h, n4 = T - ai - aj + n1;
    const bool neg = c.r < 0.0f;   // the r CELL decides the side, its tie rule included
    const int64_t u = ai * (T - aj), v = (T - ai) * aj, p = ai * aj, q = (T - ai) * (T - aj);
    const int64_t dm = neg ? (p < q ? p : q) : (u < v ? u : v);
    const double Td = (double)T, base = (double)p, eps = 0x1p-20;
    const double f1 = (double)n1, f2 = (double)n2, f3 = (double)n3, f4 = (double)n4, fh = (double)h;
    const double di = (double)ai, dj = (double)aj, d4 = (double)(T - ai - aj);
    double w[kCiGrid + 1];
    double top = -__builtin_inf();
    for (int k = 0; k <= kCiGrid; ++k) {
        const double step = (double)((int64_t)k * dm) / 100.0;   // k Dm < 2^36: exact before the division
        double h1 = (neg ? base - step : base + step) / Td;
        double h2 = di - h1, h3 = dj - h1, h4 = d4 + h1;
        h1 = h1 < eps ? eps : h1, h2 = h2 < eps ? eps : h2, h3 = h3 < eps ? eps : h3, h4 = h4 < eps ? eps : h4;
        const double l14 = (n1 > 0 ? f1 * log(h1) : 0.0) + (n4 > 0 ? f4 * log(h4) : 0.0);
        const double l23 = (n2 > 0 ? f2 * log(h2) : 0.0) + (n3 > 0 ? f3 * log(h3) : 0.0);
        const double l = (l14 + l23) + (h > 0 ? fh * log(h1 * h4 + h2 * h3) : 0.0);
        w[k] = l;
        top = l > top ? l : top;
    }
    double W = 0.0;
    for (int k = 0; k <= kCiGrid; ++k) {
        const double e = exp(w[k] - top);
        w[k] = e;
        W += e;
    }
    const double tail = 0.05 * W;
    int klo = kCiGrid, khi = 0;   // (the whole sum is W > tail: both loops stop)
    double cum = 0.0;
    for (int k = 0; k <= kCiGrid; ++k) {
        cum += w[k];
        if (cum > tail) {
            klo = k;
            break;
        }
    }
    cum = 0.0;
    for (int k = kCiGrid; k >= 0; --k) {
        cum += w[k];
        if (cum > tail) {
            khi = k;
            break;
        }
    }
    return Ci{(uint8_t)(klo > 0 ? klo - 1 : 0), (uint8_t)(khi < kCiGrid ? khi + 1 : kCiGrid)};
}

// ---- the two-set K loop: S and H of I slab ti x J slab tj, no missing code read --------------------------------------------------
// Called by the whole workgroup.  `lds` holds two {S image, H image} buffers (2 x kImage); the first barrier inside also
// publishes what the caller wrote to LDS of its own before the call.  On return every wave is past the last block's barrier:
// nobody reads the images any more.  Accumulator (m, tt, e) is row 32 m + (e & 3) + 8 (e >> 2) + 4 half of the wave's 64,
// column 32 tt + l32.
__device__ __forceinline__ void count_two_sets(unsigned char *lds, const uint4 *alt_i, const uint4 *alt_j, uint32_t ti, uint32_t tj,
                                               uint32_t nblocks, uint32_t tid, v16f (&acc_s)[2][2], v16f (&acc_h)[2][2])
{
    const uint32_t lane = tid & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wr = wave >> 1, wc = wave & 1u;   // the wave's 64 rows / 64 columns inside the 128 x 128 tile
    const uint32_t nchunks = 2u * nblocks;
    // lane's A source: row 64 wr + l32 (+ 32 for the second tile) of slab ti, chunk 2 blk + half; planes are < 4 GiB
    const uint4 *const a_src = alt_i + ((ti * nchunks + half) * kSlab + wr * kWaveRows + l32);
    // thread's share of the J images: row tid % 128, chunk 2 blk + tid / 128
    const uint32_t b_row = tid & (kSlab - 1u), b_half = tid >> 7;
    const uint4 *const b_src = alt_j + ((tj * nchunks + b_half) * kSlab + b_row);
    const uint32_t b_dst = b_half * kSlab + b_row;   // + step * 256

    auto load_a = [&](uint4 (&dst)[2], uint32_t blk) {
        const uint4 *const s = a_src + (size_t)blk * kBlockVecs;
        dst[0] = s[0];
        dst[1] = s[32];
    };
    auto load_b = [&](uint32_t blk) { return b_src[(size_t)blk * kBlockVecs]; };
    auto expand_b = [&](unsigned char *buf, const uint4 &bits) {
        uint4 *const img_s = reinterpret_cast<uint4 *>(buf);
        uint2 *const img_h = reinterpret_cast<uint2 *>(buf + kImageS);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t w = word_of(bits, q);
            *reinterpret_cast<v4i *>(img_s + b_dst + (uint32_t)q * kBlockVecs) = expand32_b4_dosage(w);
            *reinterpret_cast<v2i *>(img_h + b_dst + (uint32_t)q * kBlockVecs) = het_b4(het_bits(w));
        }
    };

#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc_s[m][tt][e] = 0.0f, acc_h[m][tt][e] = 0.0f;

    // One K-block per trip, as in rect_kernel: the next block's loads first, then the 4 x 8 MFMAs of this one, then the next
    // block's J bits become the other buffer -- last read in block blk - 1, which every wave left through the barrier at its
    // end -- and the barrier publishes it.  (Beyond the last block the loads repeat it: discarded.)
    uint4 acur[2], anxt[2];
    load_a(acur, 0u);
    expand_b(lds, load_b(0u));
    block_sync();   // (also publishes the caller's tables)
    auto read_bf = [&](v4i (&bs)[2], v2i (&bh)[2], const unsigned char *rd, int w) {
        const uint4 *const img_s = reinterpret_cast<const uint4 *>(rd);
        const uint2 *const img_h = reinterpret_cast<const uint2 *>(rd + kImageS);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const uint32_t at = ((uint32_t)w * 2u + half) * kSlab + wc * kWaveCols + 32u * tt + l32;
            bs[tt] = *reinterpret_cast<const v4i *>(img_s + at);
            bh[tt] = *reinterpret_cast<const v2i *>(img_h + at);
        }
    };
    for (uint32_t blk = 0; blk < nblocks; ++blk) {
        const uint32_t nb = blk + 1u < nblocks ? blk + 1u : blk;
        const uint4 bits = load_b(nb);
        load_a(anxt, nb);
        const unsigned char *const rd = lds + (blk & 1u) * kImage;
        v4i bs[2][2], as[2][2];
        v2i bh[2][2], ah[2][2];
        read_bf(bs[0], bh[0], rd, 0);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            as[0][m] = expand32_a4(acur[m].x);
            ah[0][m] = het_a4(het_bits(acur[m].x));
        }
        // the scheduling barriers keep the order as written (rect_kernel): the global loads at the top of the block, and step
        // w + 1's fragment reads and A expansion in front of step w's eight MFMAs
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < 3) {
                read_bf(bs[(w + 1) & 1], bh[(w + 1) & 1], rd, w + 1);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const uint32_t word = word_of(acur[m], w + 1);
                    as[(w + 1) & 1][m] = expand32_a4(word);
                    ah[(w + 1) & 1][m] = het_a4(het_bits(word));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const v4i a = as[w & 1][m], bb = bs[w & 1][tt];
                    const v2i ha = ah[w & 1][m], hb = bh[w & 1][tt];
                    const v8i a8 = {a.x, a.y, a.z, a.w, 0, 0, 0, 0};
                    const v8i b8 = {bb.x, bb.y, bb.z, bb.w, 0, 0, 0, 0};
                    const v8i ha8 = {ha.x, 0, ha.y, 0, 0, 0, 0, 0};
                    const v8i hb8 = {hb.x, 0, hb.y, 0, 0, 0, 0, 0};
                    // cbsz = blgp = 4: FP4 operands (4 registers each); scale operands 0 = the unscaled instruction
                    acc_s[m][tt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc_s[m][tt], 4, 4, 0, 0, 0, 0);
                    acc_h[m][tt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ha8, hb8, acc_h[m][tt], 4, 4, 0, 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        expand_b(lds + ((blk + 1u) & 1u) * kImage, bits);
        block_sync();
        acur[0] = anxt[0];
        acur[1] = anxt[1];
    }
}

// The accumulators do not stay in registers under the epilogue's data-dependent root search: each wave packs (S, H) of its 64 x
// 64 cells into one word each, [64 rows][64 columns], in the LDS the images no longer need (4 x 16 KiB); the barrier lets the
// lanes of a wave read each other's words.  Returns the wave's words.
__device__ __forceinline__ const uint32_t *stage_two_sets(unsigned char *lds, uint32_t tid, const v16f (&acc_s)[2][2],
                                                          const v16f (&acc_h)[2][2])
{
    const uint32_t lane = tid & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t *const stage = reinterpret_cast<uint32_t *>(lds) + wave * (kWaveRows * kWaveCols);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t row = 32u * m + (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * half;
                stage[row * kWaveCols + 32u * tt + l32] = ((uint32_t)acc_s[m][tt][e] << kPackShift) | (uint32_t)acc_h[m][tt][e];
            }
    block_sync();
    return stage;
}

}  // namespace em
}  // namespace ldx

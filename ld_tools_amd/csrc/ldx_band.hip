// Stored LD bands (include/ldx.h, "Stored bands"): the lower-band layout of a window over sorted positions
// (ldx_ld_band_layout_dev) and the two consumers of bands that ldx_ld_band_dev stored -- cross-panel scores
// (ldx_band_score_dev) and matrix-vector products (ldx_band_matvec_dev).  The store itself is an epilogue of the band
// kernel (ldx_mfma.hip, BandOp::Store).  Plain HIP: the consumers stream the band's 4 bytes per stored pair.
#include "ldx_common.h"

namespace ldx {

constexpr uint32_t kLayoutThreads = 1024u, kLayoutPer = 4u;   // one tile of the scan: 4096 SNPs, four consecutive ones per thread

// lo[i] = the first j <= i with pos_i - pos_j <= window (a binary search: positions are non-decreasing; the comparison in
// doubles, as the band kernel's epilogues make it), offsets = the exclusive prefix sum of i - lo[i] with the total at
// offsets[n].  ONE workgroup walks the array tile by tile, the running total carried in a register every thread holds
// (cross_scan_kernel's scheme, ldx_area.hip): any n_snps, no second launch, no workspace; every word of both arrays is written.
__global__ void __launch_bounds__(kLayoutThreads) band_layout_kernel(const int64_t *__restrict__ pos, uint32_t n_snps, double window,
                                                                     uint32_t *__restrict__ lo, uint64_t *__restrict__ offsets)
{
    __shared__ uint64_t wave_tot[kLayoutThreads / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t carry = 0;   // offsets[base]
    if (tid == 0u) offsets[0] = 0u;
    for (uint64_t base = 0; base < n_snps; base += kLayoutThreads * kLayoutPer) {
        uint64_t d[kLayoutPer], s = 0;
#pragma unroll
        for (uint32_t e = 0; e < kLayoutPer; ++e) {
            const uint64_t m = base + (uint64_t)tid * kLayoutPer + e;
            if (m < n_snps) {
                const double pi = (double)pos[m];
                uint32_t a = 0, b = (uint32_t)m;   // the first j in [0, m] inside the window (j = m always is)
                while (a < b) {
                    const uint32_t mid = a + (b - a) / 2u;
                    if (pi - (double)pos[mid] <= window) b = mid; else a = mid + 1u;
                }
                lo[m] = a;
                s += (uint32_t)m - a;
            }
            d[e] = s;   // inclusive inside the thread
        }
        uint64_t x = s;   // inclusive over the wave
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint64_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63u) wave_tot[wave] = x;
        block_sync();
        uint64_t before = carry, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kLayoutThreads / 64u; ++w) {
            const uint64_t t = wave_tot[w];
            before += w < wave ? t : 0u;
            total += t;
        }
        before += x - s;   // the wave's lanes in front of this one
#pragma unroll
        for (uint32_t e = 0; e < kLayoutPer; ++e) {
            const uint64_t m = base + (uint64_t)tid * kLayoutPer + e;
            if (m < n_snps) offsets[m + 1u] = before + d[e];
        }
        carry += total;
        block_sync();   // wave_tot is free again
    }
}

// Cross-score term of two cells (ldx_band_score_dev): rint(2^32 (a *f32 b)) as a two's-complement word -- score_term with two
// factors, so T(c, c) IS score_term(c); -0.0f (a degenerate SNP) gives 0.
__device__ __forceinline__ uint64_t cross_term(float a, float b)
{
    const float p = a * b;
    return (uint64_t)(int64_t)__builtin_rint((double)p * 0x1p32);
}

// every SNP's own term WRITES its words: the calls need no memset of `sums`.  kScore: T(diag1, diag2); else the product's
// prod_term(prod_value(diag), x) per right-hand side (st of them).  A null diagonal: no own term.
template <bool kScore>
__global__ void band_init_kernel(const float *__restrict__ diag1, const float *__restrict__ diag2, const float *__restrict__ x,
                                 uint32_t st, bool square, uint32_t n_snps, uint64_t *__restrict__ sums)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_snps) return;
    if constexpr (kScore) {
        sums[i] = (diag1 && diag2) ? cross_term(diag1[i], diag2[i]) : 0u;
    } else {
        for (uint32_t c = 0; c < st; ++c)
            sums[(size_t)i * st + c] = diag1 ? prod_term(prod_value(diag1[i], square), x[(size_t)i * st + c]) : 0u;
    }
}

#ifndef LDX_SWEEP_ROWS   // tuning: -DLDX_SWEEP_ROWS=n builds the sweep with another number of rows per workgroup
#define LDX_SWEEP_ROWS 16
#endif
constexpr uint32_t kSweepThreads = 256u, kSweepRows = LDX_SWEEP_ROWS;   // a workgroup owns this many consecutive band rows

// ---- the sweep's accumulators.  A term is an integer t = rint(.) with |t| <= 2^62, and the contract adds terms as 64-bit
// words.  The conversion of a double to int64 is a dozen instructions on this hardware, and with eight right-hand sides the
// sweep would pay for it per cell and weight (as the band kernel's epilogue does).  So a thread keeps each sum as TWO
// doubles and converts once at the end:  h = rint(t 2^-31)  (an integer, |h| <= 2^31),  l = t - h 2^31  (one fma: the exact
// difference is an integer multiple of t's last place with |l| <= 2^30, hence representable),  hi += h,  lo += l.  Both sums
// stay exact while they are below 2^53, i.e. for 2^20 terms (the sweep folds after 512 at most), and
//     (int64) hi 2^31 + (int64) lo  =  sum of (int64) t   modulo 2^64:
// the same word the term-by-term integer additions give.
constexpr double kSplit = 0x1p31;
__device__ __forceinline__ void acc_add(double &hi, double &lo, double t)
{
    const double h = __builtin_rint(t * (1.0 / kSplit));
    hi += h;
    lo += __builtin_fma(h, -kSplit, t);
}
__device__ __forceinline__ uint64_t acc_fold(double hi, double lo)
{
    return ((uint64_t)(int64_t)hi << 31) + (uint64_t)(int64_t)lo;
}
__device__ __forceinline__ double min_raw(double a, double b)   // v_min_f64 as is (max_raw's sibling, ldx_common.h)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// prod_term's integer as a double, from the value ALREADY scaled by 2^40 (exact: a power of two): the fp64 product of two
// float32 is exact with or without the scale, the clamp to +-2^62 is prod_term's to +-2^22, rint is the same rounding
__device__ __forceinline__ double prod_term_f64(double v_scaled, float x)
{
    return __builtin_rint(min_raw(max_raw(v_scaled * (double)x, -0x1p62), 0x1p62));
}
// cross_term's integer as a double
__device__ __forceinline__ double cross_term_f64(float a, float b)
{
    const float p = a * b;
    return __builtin_rint((double)p * 0x1p32);
}

// One sweep over a stored band.  A workgroup owns the rows [i0, i0 + 16) and walks the columns they reach, [min lo, last
// row), in spans of 2048: thread t holds the columns jbase + t + 256 c, c < 8, so that the threads of a wave read consecutive
// words of a band row.  Cell (i, j) feeds row i with the other side's value at j and column j with the value at i:
//   * the weights of the thread's OWN columns stay in registers for the 16 rows (fetching them per cell made the sweep
//     eight times heavier on the caches than the cells themselves), the row's weights are the same for every thread;
//   * a row's sum is reduced over the wave once per row and span (shuffles), then one atomic per wave and word;
//   * a column's sums stay in registers over the 16 rows: one atomic per column, word and workgroup.
// More than two right-hand sides go in passes of two (the band kernel's kProdSweep): the column sums of eight would not
// fit the registers; the cells of the later passes come out of the cache.  kScore: the term is cross_term(values[idx],
// values2[idx]) (kW = 1); else prod_term(prod_value(values[idx]), x[other][k]).  Integer addition makes the result
// independent of the order.  Reads are guarded by the layout test and by idx < offsets[n_snps] (a cell that fails them
// counts as +0.0f: its terms are 0); atomics go to rows and columns below n_snps only.
template <bool kScore, int kW>
__global__ void __launch_bounds__(kSweepThreads) band_sweep_kernel(const float *__restrict__ values, const float *__restrict__ values2,
                                                                  const uint32_t *__restrict__ lo, const uint64_t *__restrict__ offsets,
                                                                  uint32_t n_snps, const float *__restrict__ x, bool square,
                                                                  uint64_t *__restrict__ sums)
{
    constexpr uint32_t kCols = 8u;                 // columns per thread and span
    constexpr int kP = kW >= 2 ? 2 : 1;            // right-hand sides per pass
    __shared__ uint32_t s_lo[kSweepRows];
    __shared__ uint64_t s_off[kSweepRows];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t i0 = blockIdx.x * kSweepRows;
    const uint32_t rows = n_snps - i0 < kSweepRows ? n_snps - i0 : kSweepRows;   // (the grid covers [0, n_snps): >= 1)
    const uint64_t n_cells = offsets[n_snps];
    if (tid < kSweepRows) {
        s_lo[tid] = tid < rows ? lo[i0 + tid] : 0xFFFFFFFFu;   // (a row beyond the panel: no column reaches it)
        s_off[tid] = tid < rows ? offsets[i0 + tid] : 0u;
    }
    block_sync();
    uint32_t jmin = 0xFFFFFFFFu;
    for (uint32_t rr = 0; rr < rows; ++rr) jmin = s_lo[rr] < jmin ? s_lo[rr] : jmin;
    const uint32_t i_last = i0 + rows - 1u;   // columns end in front of the last row
    for (uint64_t jbase = jmin; jbase < i_last; jbase += kSweepThreads * kCols) {   // block-uniform
#pragma unroll 1
        for (int k0 = 0; k0 < kW; k0 += kP) {
            uint32_t jc[kCols];
            float xj[kCols][kP];          // the own columns' weights
            double chi[kCols][kP], clo[kCols][kP];
#pragma unroll
            for (uint32_t c = 0; c < kCols; ++c) {
                const uint64_t j = jbase + tid + kSweepThreads * c;
                jc[c] = j < i_last ? (uint32_t)j : 0xFFFFFFFFu;   // (no row's lo reaches 2^32 - 1: the column takes no part)
#pragma unroll
                for (int k = 0; k < kP; ++k) {
                    xj[c][k] = (!kScore && j < i_last && k0 + k < kW) ? x[(size_t)j * kW + k0 + k] : 0.0f;
                    chi[c][k] = 0.0;
                    clo[c][k] = 0.0;
                }
            }
            // a row's cells are fetched one row AHEAD of their use (the row beyond the last: its last row again, unused): the
            // loads of row rr + 1 are in flight while the terms of row rr are computed
            auto load_row = [&](uint32_t rr, float (&v)[kCols], float (&v2)[kCols]) {
                const uint32_t i = i0 + rr, lo_r = s_lo[rr];
                const uint64_t off_r = s_off[rr];
#pragma unroll
                for (uint32_t c = 0; c < kCols; ++c) {
                    const uint64_t idx = off_r + (jc[c] - lo_r);
                    const bool ok = jc[c] >= lo_r && jc[c] < i && idx < n_cells;
                    v[c] = ok ? values[idx] : 0.0f;
                    v2[c] = (kScore && ok) ? values2[idx] : 0.0f;
                }
            };
            float v[kCols], v2[kCols];
            load_row(0u, v, v2);
            for (uint32_t rr = 0; rr < rows; ++rr) {
                const uint32_t i = i0 + rr;
                float xi[kP];             // the row's weights: the same for every thread
#pragma unroll
                for (int k = 0; k < kP; ++k) xi[k] = (!kScore && k0 + k < kW) ? x[(size_t)i * kW + k0 + k] : 0.0f;
                float nv[kCols], nv2[kCols];
                load_row(rr + 1u < rows ? rr + 1u : rr, nv, nv2);
                double rhi[kP], rlo[kP];
#pragma unroll
                for (int k = 0; k < kP; ++k) { rhi[k] = 0.0; rlo[k] = 0.0; }
#pragma unroll
                for (uint32_t c = 0; c < kCols; ++c) {
                    if constexpr (kScore) {
                        const double t = cross_term_f64(v[c], v2[c]);   // the pair's one term, to both of its SNPs
                        acc_add(rhi[0], rlo[0], t);
                        acc_add(chi[c][0], clo[c][0], t);
                    } else {
                        const double pv = (double)prod_value(v[c], square) * 0x1p40;
#pragma unroll
                        for (int k = 0; k < kP; ++k) {
                            acc_add(rhi[k], rlo[k], prod_term_f64(pv, xj[c][k]));
                            acc_add(chi[c][k], clo[c][k], prod_term_f64(pv, xi[k]));
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < kP; ++k) {   // (at most 8 terms per thread and 512 per wave: the doubles stay exact)
#pragma unroll
                    for (uint32_t o = 32u; o >= 1u; o >>= 1) {
                        rhi[k] += __shfl_down(rhi[k], o);
                        rlo[k] += __shfl_down(rlo[k], o);
                    }
                    const uint64_t tot = acc_fold(rhi[k], rlo[k]);
                    if (lane == 0u && k0 + k < kW && tot != 0u)
                        atomicAdd(reinterpret_cast<unsigned long long *>(sums) + (size_t)i * kW + k0 + k, (unsigned long long)tot);
                }
#pragma unroll
                for (uint32_t c = 0; c < kCols; ++c) { v[c] = nv[c]; v2[c] = nv2[c]; }
            }
#pragma unroll
            for (uint32_t c = 0; c < kCols; ++c)
#pragma unroll
                for (int k = 0; k < kP; ++k) {   // (at most 16 terms each)
                    const uint64_t tot = acc_fold(chi[c][k], clo[c][k]);
                    if (jc[c] != 0xFFFFFFFFu && k0 + k < kW && tot != 0u)
                        atomicAdd(reinterpret_cast<unsigned long long *>(sums) + (size_t)jc[c] * kW + k0 + k, (unsigned long long)tot);
                }
        }
    }
}

}  // namespace ldx

extern "C" int ldx_ld_band_layout_dev(const int64_t *positions, uint32_t n_snps, int64_t window, uint32_t *lo, uint64_t *offsets,
                                      void *stream)
{
    LDX_REQUIRE(positions && lo && offsets, "null pointer");
    LDX_REQUIRE(n_snps >= 1 && window >= 0, "bad shape");
    const int64_t wmax = (int64_t)1 << 52;   // the band entries' clamp: positions and window travel as doubles
    if (window > wmax) window = wmax;
    ldx::band_layout_kernel<<<1, ldx::kLayoutThreads, 0, (hipStream_t)stream>>>(positions, n_snps, (double)window, lo, offsets);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_band_score_dev(const float *values1, const float *values2, const float *diag1, const float *diag2,
                                  const uint32_t *lo, const uint64_t *offsets, uint32_t n_snps, int64_t *sums, void *stream)
{
    LDX_REQUIRE(lo && offsets && sums, "null pointer");
    LDX_REQUIRE((values1 == nullptr) == (values2 == nullptr), "one band is null (both may be when the layout holds no cell)");
    LDX_REQUIRE((diag1 == nullptr) == (diag2 == nullptr), "one diagonal is null (both null: no own term)");
    LDX_REQUIRE(n_snps >= 1, "bad shape");
    hipStream_t s = (hipStream_t)stream;
    ldx::band_init_kernel<true><<<(n_snps + 255u) / 256u, 256, 0, s>>>(diag1, diag2, nullptr, 1u, false, n_snps, (uint64_t *)sums);
    LDX_HIP(hipGetLastError());
    if (n_snps < 2 || !values1) return LDX_OK;   // no pairs
    ldx::band_sweep_kernel<true, 1><<<(n_snps + ldx::kSweepRows - 1u) / ldx::kSweepRows, ldx::kSweepThreads, 0, s>>>(
        values1, values2, lo, offsets, n_snps, nullptr, false, (uint64_t *)sums);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_band_matvec_dev(const float *values, const float *diag, const uint32_t *lo, const uint64_t *offsets,
                                   uint32_t n_snps, const float *x, uint32_t n_rhs, int power, int64_t *sums, void *stream)
{
    LDX_REQUIRE(n_rhs >= 1u && n_rhs <= 8u, "n_rhs must be 1 .. 8");
    LDX_REQUIRE(power == 1 || power == 2, "power must be 1 or 2");
    LDX_REQUIRE(lo && offsets && x && sums, "null pointer");
    LDX_REQUIRE(n_snps >= 1, "bad shape");
    hipStream_t s = (hipStream_t)stream;
    const bool square = power == 2;
    ldx::band_init_kernel<false><<<(n_snps + 255u) / 256u, 256, 0, s>>>(diag, nullptr, x, n_rhs, square, n_snps, (uint64_t *)sums);
    LDX_HIP(hipGetLastError());
    if (n_snps < 2 || !values) return LDX_OK;   // no pairs
    const uint32_t grid = (n_snps + ldx::kSweepRows - 1u) / ldx::kSweepRows;
#define LDX_GO(W)                                                                                                              \
    case W:                                                                                                                    \
        ldx::band_sweep_kernel<false, W><<<grid, ldx::kSweepThreads, 0, s>>>(values, nullptr, lo, offsets, n_snps, x, square, \
                                                                             (uint64_t *)sums);                                \
        break;
    switch (n_rhs) {   // one instantiation per count: a SNP's weights are kW contiguous floats
        LDX_GO(1) LDX_GO(2) LDX_GO(3) LDX_GO(4) LDX_GO(5) LDX_GO(6) LDX_GO(7) LDX_GO(8)
    }
#undef LDX_GO
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

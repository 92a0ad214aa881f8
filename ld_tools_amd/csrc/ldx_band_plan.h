// What the lower-band walks share (pwband_kernel of ldx_pwband.hip, emband_kernel of ldx_emband.hip).
// The device-side plan: low[i], the window's first column of every row, and the exclusive prefix of the tiles each I block of
// kRows rows meets, both into the caller's workspace, in stream order -- the host reads nothing back.
//   * low[i] = the first j with (double)pos_i - (double)pos_j <= window (band_layout_kernel's comparison, ldx_band.hip).
//     Positions are non-decreasing, so "j < i and pos_i - pos_j <= window" IS low[i] <= j < i.
//   * I block ti (rows [kRows ti, r1), r1 = min(kRows (ti + 1), n)) meets the slabs low[kRows ti] / 128 .. (r1 - 1) / 128: low is
//     non-decreasing, so these cover every in-window j < i of the block.  prefix[ti] = the tiles in front of I block ti,
//     prefix[Ti] = all of them; tile t is (ti, tj) with prefix[ti] <= t < prefix[ti + 1] (tile_at's binary search) and
//     tj = first slab + t - prefix[ti].
// And around it, once for both kernels:
//   * walk<kRows>: the tile loop of a workgroup of a fixed grid, striding over the tile numbers, with a per-tile callable.
//   * RowTables<kRows>: r_low, r_lo, r_off of a tile's rows in LDS, their fill, the `inside` predicate and the store guard.
//   * launch<kRows>: make_plan, grid = min(the caller's tile bound, 2 x CUs), the kernel launch left to a callable.
//   * shape_ok / band_args_ok<kRows>: the entries' argument rules, the parity rule and its words the caller's.
//   * called_sums: N, A and, where asked, HA of one SNP over its own called individuals, reduced over a wavefront.
#pragma once

#include "ldx_fp4.h"

namespace ldx {
namespace bandplan {

constexpr uint32_t kNoRow = 0xFFFFFFFFu;   // `low` of a row beyond the panel: no column reaches it

// low[m]: one thread per SNP.  (A template only so that the header may be included by several sources.)
template <int kUnused = 0>
__global__ void __launch_bounds__(256) low_kernel(const int64_t *__restrict__ pos, uint32_t n_snps, double window,
                                                  uint32_t *__restrict__ low)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_snps) return;
    const double pi = (double)pos[m];
    uint32_t a = 0, b = m;   // the first j in [0, m] inside the window (j = m always is)
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2u;
        if (pi - (double)pos[mid] <= window) b = mid; else a = mid + 1u;
    }
    low[m] = a;
}

// prefix[ti] = tiles of the I blocks in front of ti, prefix[Ti] = all: one workgroup, 256 I blocks per trip, the running
// total carried in a register every thread holds
template <uint32_t kRows>
__global__ void __launch_bounds__(256) plan_kernel(const uint32_t *__restrict__ low, uint32_t n_snps, uint64_t *__restrict__ prefix)
{
    __shared__ uint32_t cnt[256];
    __shared__ uint64_t pre[257];
    const uint32_t tid = threadIdx.x, Ti = (n_snps + kRows - 1u) / kRows;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < Ti; base += 256u) {
        const uint32_t ti = base + tid;
        uint32_t c = 0;
        if (ti < Ti) {
            const uint32_t r1 = n_snps - ti * kRows < kRows ? n_snps : (ti + 1u) * kRows;
            const uint32_t first = low[ti * kRows] / kSlab, last = (r1 - 1u) / kSlab;
            c = last >= first ? last - first + 1u : 0u;
        }
        cnt[tid] = c;
        block_sync();
        if (tid == 0u) {
            uint64_t s = carry;
            for (uint32_t k = 0; k < 256u; ++k) {
                pre[k] = s;
                s += cnt[k];
            }
            pre[256] = s;
        }
        block_sync();
        if (ti < Ti) prefix[ti] = pre[tid];
        carry = pre[256];
        block_sync();   // cnt and pre are free again
    }
    if (tid == 0u) prefix[Ti] = carry;
}

// tile number t of the plan: its I block and slab (workgroup-uniform)
template <uint32_t kRows>
__device__ __forceinline__ void tile_at(const uint64_t *prefix, const uint32_t *low, uint32_t Ti, uint64_t t, uint32_t &ti, uint32_t &tj)
{
    uint32_t a = 0, b = Ti - 1u;   // the last I block with prefix[ti] <= t: prefix[a] <= t < prefix[b + 1]
    while (a < b) {
        const uint32_t mid = a + (b - a + 1u) / 2u;
        if (prefix[mid] <= t) a = mid; else b = mid - 1u;
    }
    ti = a;
    tj = low[ti * kRows] / kSlab + (uint32_t)(t - prefix[ti]);
}

// the workspace: prefix [Ti + 1] uint64, then low [n] uint32, each part a multiple of 256 bytes
template <uint32_t kRows>
inline size_t prefix_bytes(uint32_t n_snps)
{
    return (((size_t)(n_snps + kRows - 1u) / kRows + 1u) * sizeof(uint64_t) + 255u) / 256u * 256u;
}
template <uint32_t kRows>
inline size_t workspace_bytes(uint32_t n_snps)
{
    return prefix_bytes<kRows>(n_snps) + ((size_t)n_snps * sizeof(uint32_t) + 255u) / 256u * 256u;
}

struct Plan {
    const uint64_t *prefix;   // [Ti + 1] tiles in front of each I block, the total last (workspace)
    const uint32_t *low;      // [n] the window's first column per row (workspace)
};

// low, then the plan, into `workspace`, in stream order
template <uint32_t kRows>
inline int make_plan(const int64_t *positions, uint32_t n, int64_t window, void *workspace, hipStream_t s, Plan &plan)
{
    uint64_t *const prefix = (uint64_t *)workspace;
    uint32_t *const low = (uint32_t *)((char *)workspace + prefix_bytes<kRows>(n));
    const int64_t wmax = (int64_t)1 << 52;   // positions and window travel as doubles
    low_kernel<><<<(n + 255u) / 256u, 256, 0, s>>>(positions, n, (double)(window > wmax ? wmax : window), low);
    LDX_HIP(hipGetLastError());
    plan_kernel<kRows><<<1, 256, 0, s>>>(low, n, prefix);
    LDX_HIP(hipGetLastError());
    plan = Plan{prefix, low};
    return LDX_OK;
}

// ---- the walk: a workgroup of a fixed grid strides over the plan's tile numbers -----------------------------------------------
// tile(ti, tj, tid) is called by the whole workgroup (kBandThreads threads), once per tile; a block_sync() separates two
// tiles of one workgroup (the last tile's tables, images and staged words are free).  tid is the thread's number as a value
// of THIS trip: what the tile's body derives from it -- a few dozen lane offsets -- would otherwise be made once in front of
// the loop and held in registers across every K loop, which does not fit.
constexpr uint32_t kBandThreads = 256;

template <uint32_t kRows, typename Tile>
__device__ __forceinline__ void walk(const Plan &plan, uint32_t n, Tile &&tile)
{
    const uint32_t Ti = (n + kRows - 1u) / kRows;
    const uint64_t total = plan.prefix[Ti];
    for (uint64_t t = blockIdx.x; t < total; t += gridDim.x) {   // workgroup-uniform
        uint32_t ti, tj;
        tile_at<kRows>(plan.prefix, plan.low, Ti, t, ti, tj);
        if (t != blockIdx.x) block_sync();
        uint32_t tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        tile(ti, tj, tid);
    }
}

// the per-tile tables of I block ti's rows, in LDS beside the tile body's; the tile body's first barrier publishes them
template <uint32_t kRows>
struct RowTables {
    uint64_t r_off[kRows];   // store: offsets[i]
    uint32_t r_low[kRows];   // the window's first column of row i (kNoRow beyond the panel)
    uint32_t r_lo[kRows];    // store: the caller's lo[i]
};

template <bool kStore, uint32_t kRows>
__device__ __forceinline__ void fill_rows(RowTables<kRows> &rt, const Plan &plan, const uint32_t *lo, const uint64_t *offsets,
                                          uint32_t n, uint32_t ti, uint32_t tid)
{
    static_assert(kRows <= kBandThreads, "a thread fills at most one row");
    if (kRows == kBandThreads || tid < kRows) {
        const uint32_t x_r = ti * kRows + tid;
        rt.r_low[tid] = x_r < n ? plan.low[x_r] : kNoRow;
        if constexpr (kStore) {
            rt.r_lo[tid] = x_r < n ? lo[x_r] : kNoRow;
            rt.r_off[tid] = x_r < n ? offsets[x_r] : 0u;
        }
    }
}

// is cell (i, j), row li of the tile, a pair of the band?  (i < n: r_low is kNoRow otherwise; j < i < n)
template <uint32_t kRows>
__device__ __forceinline__ bool inside(const RowTables<kRows> &rt, uint32_t li, uint32_t i, uint32_t j)
{
    return j < i && j >= rt.r_low[li];
}

// where a cell inside goes in the caller's layout, and whether it goes there at all: ldx_ld_band_dev's guard
template <uint32_t kRows>
__device__ __forceinline__ bool store_at(const RowTables<kRows> &rt, uint32_t li, uint32_t j, bool inside, uint64_t n_cells,
                                         uint64_t &idx)
{
    const uint32_t lo_i = rt.r_lo[li];
    idx = rt.r_off[li] + (uint64_t)(j - lo_i);
    return inside && j >= lo_i && idx < n_cells;
}

// ---- one SNP over its OWN called individuals: a wavefront per row, a lane per 32-bit word of both planes ----------------------
// N = the individuals with both codes called, A = the sum of their dosages, HA (kHom) = the homozygous ALT among them; every
// lane returns the wave's sums.
struct CalledSums {
    uint32_t N, A, HA;
};
template <bool kHom>
__device__ __forceinline__ CalledSums called_sums(const uint32_t *__restrict__ alt, const uint32_t *__restrict__ ref,
                                                  uint32_t row, uint32_t nchunks, uint32_t lane)
{
    const uint32_t slab = row / kSlab, rin = row % kSlab;
    CalledSums c{0u, 0u, 0u};
    for (uint32_t w = lane; w < nchunks * 4u; w += 64u) {
        const size_t at = (((size_t)slab * nchunks + (w >> 2)) * kSlab + rin) * 4u + (w & 3u);
        const uint32_t wa = alt[at], q = ind_called(wa, ref[at]), g = wa & (q | (q << 1));
        c.N += __builtin_popcount(q);
        c.A += __builtin_popcount(g);
        if constexpr (kHom) c.HA += __builtin_popcount(g & (g >> 1) & 0x55555555u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c.N += __shfl_xor(c.N, off);
        c.A += __shfl_xor(c.A, off);
        if constexpr (kHom) c.HA += __shfl_xor(c.HA, off);
    }
    return c;
}

// ---- the host side -----------------------------------------------------------------------------------------------------------
// low, the plan, then the band: everything in stream order, nothing read back.  `tile_bound` is the caller's upper bound of
// the plan's total: only a cap on a grid that strides.  go(plan, grid) launches the kernel(s) and returns the code.
template <uint32_t kRows, typename Go>
inline int launch(const int64_t *positions, uint32_t n, int64_t window, void *workspace, hipStream_t s, uint64_t tile_bound,
                  Go &&go)
{
    Plan plan;
    if (const int rc = make_plan<kRows>(positions, n, window, workspace, s, plan)) return rc;
    const uint64_t cap = 2u * (uint64_t)device_cus();   // two workgroups per CU are resident
    return go(plan, (uint32_t)(tile_bound < cap ? tile_bound : cap));
}

// the panel's shape rules; n_hap must be even where `odd_reason` (the words in the message's brackets) is non-null
inline int shape_ok(const char *who, uint32_t n_snps, uint32_t n_hap, const char *odd_reason)
{
    LDX_ARG_REQUIRE(n_snps != 0u, "%s: n_snps is 0", who);
    LDX_ARG_REQUIRE(n_hap != 0u, "%s: n_hap is 0", who);
    LDX_ARG_REQUIRE(!odd_reason || n_hap % 2u == 0u, "%s: n_hap %u is odd (%s)", who, n_hap, odd_reason);
    if (n_hap > LDX_MAX_HAPS) {
        set_error("%s: n_hap %u > LDX_MAX_HAPS %u", who, n_hap, LDX_MAX_HAPS);
        return LDX_E_UNSUPPORTED;
    }
    return plane_check(who, "alt", n_snps, n_hap);
}

// a band entry's rules after its own pointers: positions, workspace, window, shape, workspace size
template <uint32_t kRows>
inline int band_args_ok(const char *who, uint32_t n_snps, uint32_t n_hap, const char *odd_reason, const int64_t *positions,
                        int64_t window, const void *workspace, size_t workspace_bytes)
{
    LDX_ARG_PTR(who, positions);
    LDX_ARG_PTR(who, workspace);
    LDX_ARG_REQUIRE(window >= 0, "%s: window %lld is negative", who, (long long)window);
    if (const int rc = shape_ok(who, n_snps, n_hap, odd_reason)) return rc;
    LDX_ARG_REQUIRE(workspace_bytes >= bandplan::workspace_bytes<kRows>(n_snps), "%s: workspace_bytes %zu < %zu", who,
                    workspace_bytes, bandplan::workspace_bytes<kRows>(n_snps));
    return LDX_OK;
}

}  // namespace bandplan
}  // namespace ldx

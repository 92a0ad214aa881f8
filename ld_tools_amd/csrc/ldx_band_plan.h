// The device-side plan of the lower-band walks (pwband_kernel of ldx_pwband.hip, emband_kernel of ldx_emband.hip; DESIGN.md 3.9
// and 3.11): low[i], the window's first column of every row, and the exclusive prefix of the tiles each I block of kRows rows
// meets, both into the caller's workspace, in stream order -- the host reads nothing back.
//   * low[i] = the first j with (double)pos_i - (double)pos_j <= window (band_layout_kernel's comparison, ldx_band.hip).
//     Positions are non-decreasing, so "j < i and pos_i - pos_j <= window" IS low[i] <= j < i.
//   * I block ti (rows [kRows ti, r1), r1 = min(kRows (ti + 1), n)) meets the slabs low[kRows ti] / 128 .. (r1 - 1) / 128: low is
//     non-decreasing, so these cover every in-window j < i of the block.  prefix[ti] = the tiles in front of I block ti,
//     prefix[Ti] = all of them; tile t is (ti, tj) with prefix[ti] <= t < prefix[ti + 1] (tile_at's binary search) and
//     tj = first slab + t - prefix[ti].
#pragma once

#include "ldx_common.h"

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
    const uint64_t *prefix;
    const uint32_t *low;
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

}  // namespace bandplan
}  // namespace ldx

// Gabriel haplotype blocks on stored D' confidence bounds (include/ldx.h, "Gabriel blocks").
//   * ldx_ld_ci_from_counts_dev: ci_cell (ldx_em_tile.h) alone on a list of count tuples -- the function the band kernel of
//     ldx_emband.hip runs per pair (ldx_ld_em_ci_band_dev).
//   * ldx_gabriel_candidates_dev: everything from here on is integer logic on the two bytes of a pair.
//       suffix_kernel      one thread per row i: for every column j of the row, the kept j' in [j, i) whose pair (i, j') is
//                          strong at the cuts of the rows m = 3, 4, >= 5 or recombinant -- four counts, one 16-byte store.
//       columns_kernel     the cells of column f: the first l > f with lo[l] > f (lo is non-decreasing), minus f + 1.
//       scan_kernel        their exclusive prefix: the candidate list is column-major, so that equal spans stay ordered by
//                          (first, last) under a stable sort.
//       candidates_kernel  one thread per column `first`, `last` walking upward: the triangle counts of [first, last] are
//                          the running sums of the suffix counts at (last, first), O(1) per candidate.  Every slot of the
//                          list is written: the span of a valid candidate, -1 otherwise.
//   * ldx_gabriel_pick_dev: one workgroup takes the list, sorted by span descending (stable) by the caller, 256 candidates
//     at a time: each thread tests its candidate against the `used` bytes of the blocks accepted so far, the survivors of the
//     chunk settle among themselves in list order -- parallel rounds over their states in LDS --, the accepted ones mark
//     their SNPs.  Then the blocks are numbered in position order by a scan over the start flags.
#include "ldx_em_tile.h"

namespace ldx {
namespace gabriel {

constexpr uint32_t kNotKept = 0xFFFFFFFFu, kNoBlock = 0xFFFFFFFEu;

__global__ void __launch_bounds__(256) ci_from_counts_kernel(size_t m, const uint32_t *N, const uint32_t *a1, const uint32_t *a2,
                                                             const uint32_t *S, const uint32_t *H, uint8_t *lo, uint8_t *hi)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    const em::Ci c = em::ci_cell(N[k], a1[k], a2[k], S[k], H[k]);
    lo[k] = c.lo;
    hi[k] = c.hi;
}

__device__ __forceinline__ bool strong(uint32_t lo, uint32_t hi, uint32_t cut, uint32_t strong_hi)
{
    return lo != em::kNoCi && lo >= cut && hi >= strong_hi;
}

struct Band {
    const uint8_t *ci_lo, *ci_hi;
    const uint32_t *lo;
    const uint64_t *offsets;
    uint64_t n_cells;
    const uint8_t *keep;
    uint32_t n;
};
__device__ __forceinline__ bool kept(const Band &b, uint32_t i) { return !b.keep || b.keep[i] != 0u; }

// suf[cell(i, j)] = {strong at cut[1], at cut[2], at cut[3], recombinant} over the kept j' in [j, i); zeros where i is not kept
__global__ void __launch_bounds__(256) suffix_kernel(Band b, ldx_gabriel_params prm, uint4 *__restrict__ suf)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= b.n) return;
    const uint32_t lo_i = b.lo[i];
    const uint64_t off = b.offsets[i];
    const bool ki = kept(b, i);
    uint4 c{0u, 0u, 0u, 0u};
    for (uint32_t j = i; j-- > lo_i;) {
        const uint64_t at = off + (j - lo_i);
        if (at >= b.n_cells) continue;   // (a layout that does not belong to n_cells: nothing is touched beyond it)
        if (ki && kept(b, j)) {
            const uint32_t l = b.ci_lo[at], h = b.ci_hi[at];
            c.x += strong(l, h, prm.cut[1], prm.strong_hi);
            c.y += strong(l, h, prm.cut[2], prm.strong_hi);
            c.z += strong(l, h, prm.cut[3], prm.strong_hi);
            c.w += h < prm.recomb_hi;
        }
        suf[at] = c;
    }
}

// the first row past f whose window no longer reaches column f
__device__ __forceinline__ uint32_t column_end(const uint32_t *lo, uint32_t n, uint32_t f)
{
    uint32_t a = f + 1u, e = n;
    while (a < e) {
        const uint32_t mid = a + (e - a) / 2u;
        if (lo[mid] > f) e = mid; else a = mid + 1u;
    }
    return a;
}

__global__ void __launch_bounds__(256) columns_kernel(const uint32_t *__restrict__ lo, uint32_t n, uint32_t *__restrict__ count)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < n) count[f] = column_end(lo, n, f) - f - 1u;
}

// The inclusive prefix sum of v over a workgroup of 256 threads, and the workgroup's total: shuffles inside a wave, the four
// wave totals through `waves` (LDS, free again on return).
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint32_t tid, uint64_t (&waves)[4], uint64_t &total)
{
    const uint32_t lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)v, off);
        if (lane >= off) v += up;
    }
    if (lane == 63u) waves[wave] = v;
    block_sync();
    uint64_t add = 0;
    for (uint32_t k = 0; k < wave; ++k) add += waves[k];
    total = waves[0] + waves[1] + waves[2] + waves[3];
    block_sync();
    return v + add;
}

// col_off[f] = the cells of the columns in front of f, col_off[n] = all: one workgroup, 256 columns per trip
__global__ void __launch_bounds__(256) scan_kernel(const uint32_t *__restrict__ count, uint32_t n, uint64_t *__restrict__ col_off)
{
    __shared__ uint64_t waves[4];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n; base += 256u) {   // workgroup-uniform
        const uint32_t f = base + tid;
        const uint64_t c = f < n ? count[f] : 0u;
        uint64_t total;
        const uint64_t incl = block_scan(c, tid, waves, total);
        if (f < n) col_off[f] = carry + incl - c;
        carry += total;
    }
    if (tid == 0u) col_off[n] = carry;
}

__global__ void __launch_bounds__(256) candidates_kernel(Band b, ldx_gabriel_params prm, const int64_t *__restrict__ pos,
                                                         int64_t window, const uint4 *__restrict__ suf,
                                                         const uint64_t *__restrict__ col_off, int64_t *__restrict__ span_out,
                                                         uint32_t *__restrict__ first_out, uint32_t *__restrict__ last_out)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= b.n) return;
    const uint64_t slot0 = col_off[f];
    const uint32_t cells = (uint32_t)(col_off[f + 1u] - slot0);
    const bool kf = kept(b, f);
    const int64_t pf = pos[f];
    uint64_t tri[4] = {0u, 0u, 0u, 0u};   // pairs inside [f, l]: strong at cut[1], cut[2], cut[3]; recombinant
    uint64_t m = 1;                        // kept SNPs in [f, l]
    for (uint32_t q = 0; q < cells; ++q) {
        const uint32_t l = f + 1u + q;
        const uint64_t slot = slot0 + q;
        if (slot >= b.n_cells) break;
        int64_t out = -1;
        const uint64_t at = b.offsets[l] + (f - b.lo[l]);
        if (kf && at < b.n_cells) {
            const uint4 s = suf[at];
            tri[0] += s.x, tri[1] += s.y, tri[2] += s.z, tri[3] += s.w;
            if (kept(b, l)) {
                ++m;
                const uint32_t cl = b.ci_lo[at], ch = b.ci_hi[at];
                if (strong(cl, ch, prm.cand_cut, prm.strong_hi)) {
                    const int row = m == 2u ? 0 : m == 3u ? 1 : m == 4u ? 2 : 3;
                    const uint64_t nS = row == 0 ? (uint64_t)strong(cl, ch, prm.cut[0], prm.strong_hi) : tri[row - 1];
                    const uint64_t nR = row == 0 ? (uint64_t)(ch < prm.recomb_hi) : tri[3];
                    const int64_t span = pos[l] - pf;
                    const int64_t cap = prm.max_span[row] < 0 ? window : prm.max_span[row];
                    if (span <= window && span <= cap && nS + nR >= prm.min_informative[row] &&
                        (uint64_t)prm.frac_den * nS > (uint64_t)prm.frac_num * (nS + nR))
                        out = span;
                }
            }
        }
        span_out[slot] = out;
        first_out[slot] = f;
        last_out[slot] = l;
    }
}

__global__ void __launch_bounds__(256) pick_kernel(const int64_t *__restrict__ span, const int64_t *__restrict__ order,
                                                   const uint32_t *__restrict__ first, const uint32_t *__restrict__ last,
                                                   uint64_t n_cells, const uint8_t *__restrict__ keep, uint32_t n,
                                                   uint8_t *used, uint8_t *start, uint32_t *__restrict__ block_of,
                                                   uint32_t *__restrict__ n_out)
{
    // a candidate of the chunk: dead (overlaps a block of an earlier chunk, or lost to an earlier candidate of this one),
    // undecided, or accepted
    enum : uint8_t { kDead = 0, kOpen = 1, kTaken = 2 };
    __shared__ uint32_t s_f[256], s_l[256];
    __shared__ uint8_t s_state[256];
    __shared__ uint32_t s_open[3];   // is anybody undecided after round r: slot r % 3, reset one round ahead
    __shared__ uint64_t waves[4];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < n; i += 256u) used[i] = 0u, start[i] = 0u;
    __threadfence_block();
    block_sync();
    uint32_t n_valid = 0;   // this thread's share
    for (uint64_t base = 0; base < n_cells; base += 256u) {
        if (span[base] < 0) break;   // workgroup-uniform: the valid candidates are in front
        const uint64_t k = base + tid;
        bool ok = k < n_cells && span[k] >= 0;
        uint32_t f = 0, l = 0;
        if (ok) {
            ++n_valid;
            const int64_t c = order[k];
            f = first[c], l = last[c];
            ok = used[f] == 0u && used[l] == 0u;
            for (uint32_t i = f + 1u; ok && i < l; ++i) ok = used[i] == 0u;
        }
        s_f[tid] = f, s_l[tid] = l, s_state[tid] = ok ? kOpen : kDead;
        if (tid == 0u) s_open[0] = 0u;
        block_sync();
        // The list order decides inside the chunk: a candidate dies with an accepted earlier one that overlaps it, is accepted
        // once no earlier overlapping one is undecided, and waits otherwise.  Every round settles at least the first
        // undecided candidate; everybody reads the states of the round before (a barrier between the reads and the writes).
        uint8_t mine = ok ? kOpen : kDead;
        for (uint32_t round = 0;; ++round) {   // workgroup-uniform
            if (mine == kOpen) {
                bool dead = false, wait = false;
                for (uint32_t t = 0; t < tid && !dead; ++t) {
                    const uint8_t st = s_state[t];
                    if (st == kDead || f > s_l[t] || s_f[t] > l) continue;
                    dead = st == kTaken;
                    wait = true;
                }
                mine = dead ? kDead : wait ? kOpen : kTaken;
            }
            if (tid == 0u) s_open[(round + 1u) % 3u] = 0u;
            block_sync();
            s_state[tid] = mine;
            if (mine == kOpen) s_open[round % 3u] = 1u;
            block_sync();
            if (s_open[round % 3u] == 0u) break;
        }
        if (mine == kTaken) {
            for (uint32_t i = f; i <= l; ++i) used[i] = 1u;
            start[f] = 1u;
        }
        __threadfence_block();
        block_sync();
    }
    // the blocks in position order: block of SNP i = the starts in [0, i], minus one
    uint64_t carry = 0, total;
    for (uint32_t base = 0; base < n; base += 256u) {   // workgroup-uniform
        const uint32_t i = base + tid;
        const uint64_t incl = block_scan(i < n ? start[i] : 0u, tid, waves, total);
        if (i < n) {
            const bool k = !keep || keep[i] != 0u;
            block_of[i] = !k ? kNotKept : used[i] ? (uint32_t)(carry + incl) - 1u : kNoBlock;
        }
        carry += total;
    }
    block_scan(n_valid, tid, waves, total);   // the valid candidates: a sum over the workgroup
    if (tid == 0u) {
        n_out[0] = (uint32_t)carry;
        n_out[1] = (uint32_t)total;
    }
}

static size_t round256(size_t v) { return (v + 255u) / 256u * 256u; }
static size_t suffix_bytes(uint64_t n_cells) { return round256((size_t)n_cells * sizeof(uint4)); }
static size_t col_off_bytes(uint32_t n) { return round256(((size_t)n + 1u) * sizeof(uint64_t)); }
static size_t col_count_bytes(uint32_t n) { return round256((size_t)n * sizeof(uint32_t)); }

}  // namespace gabriel
}  // namespace ldx

using namespace ldx;

static const ldx_gabriel_params kDefaults = {70u, 98u, 90u, {80u, 50u, 50u, 70u}, {20000, 30000, -1, -1}, {1u, 3u, 6u, 6u}, 19u, 20u};

extern "C" void ldx_gabriel_default_params(ldx_gabriel_params *params)
{
    if (params) *params = kDefaults;
}

extern "C" int ldx_ld_ci_from_counts_dev(size_t m, const uint32_t *N, const uint32_t *a1, const uint32_t *a2, const uint32_t *S,
                                         const uint32_t *H, uint8_t *lo, uint8_t *hi, void *stream)
{
    const char *const who = "ldx_ld_ci_from_counts_dev";
    LDX_ARG_PTR(who, N); LDX_ARG_PTR(who, a1); LDX_ARG_PTR(who, a2); LDX_ARG_PTR(who, S); LDX_ARG_PTR(who, H);
    LDX_ARG_PTR(who, lo); LDX_ARG_PTR(who, hi);
    LDX_ARG_REQUIRE(m > 0u, "%s: m is 0", who);
    if ((m + 255u) / 256u >= (1ull << 31)) {
        set_error("%s: m = %zu needs 2^31 or more workgroups", who, m);
        return LDX_E_UNSUPPORTED;
    }
    gabriel::ci_from_counts_kernel<<<(uint32_t)((m + 255u) / 256u), 256, 0, (hipStream_t)stream>>>(m, N, a1, a2, S, H, lo, hi);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" size_t ldx_gabriel_candidates_workspace_bytes(uint32_t n_snps, uint64_t n_cells)
{
    return gabriel::suffix_bytes(n_cells) + gabriel::col_off_bytes(n_snps) + gabriel::col_count_bytes(n_snps);
}

extern "C" size_t ldx_gabriel_pick_workspace_bytes(uint32_t n_snps) { return 2u * gabriel::round256(n_snps); }

extern "C" int ldx_gabriel_candidates_dev(const uint8_t *ci_lo, const uint8_t *ci_hi, const uint32_t *lo, const uint64_t *offsets,
                                          uint64_t n_cells, const int64_t *positions, const uint8_t *keep, uint32_t n_snps,
                                          int64_t window, const ldx_gabriel_params *params, int64_t *cand_span,
                                          uint32_t *cand_first, uint32_t *cand_last, void *workspace, size_t workspace_bytes,
                                          void *stream)
{
    const char *const who = "ldx_gabriel_candidates_dev";
    LDX_ARG_PTR(who, lo); LDX_ARG_PTR(who, offsets); LDX_ARG_PTR(who, positions); LDX_ARG_PTR(who, workspace);
    LDX_ARG_REQUIRE(n_snps != 0u, "%s: n_snps is 0", who);
    LDX_ARG_REQUIRE(window >= 0, "%s: window %lld is negative", who, (long long)window);
    LDX_ARG_REQUIRE(n_cells == 0u || (ci_lo && ci_hi && cand_span && cand_first && cand_last),
                    "%s: a null pointer among ci_lo, ci_hi, cand_span, cand_first, cand_last but n_cells is %llu", who,
                    (unsigned long long)n_cells);
    const ldx_gabriel_params prm = params ? *params : kDefaults;
    LDX_ARG_REQUIRE(prm.frac_den != 0u && prm.frac_num <= prm.frac_den, "%s: the strong share %u / %u is no fraction", who,
                    prm.frac_num, prm.frac_den);
    LDX_ARG_REQUIRE(workspace_bytes >= ldx_gabriel_candidates_workspace_bytes(n_snps, n_cells), "%s: workspace_bytes %zu < %zu", who,
                    workspace_bytes, ldx_gabriel_candidates_workspace_bytes(n_snps, n_cells));
    if (n_cells == 0u) return LDX_OK;   // no pair in any window: no candidate slot
    hipStream_t s = (hipStream_t)stream;
    uint4 *const suf = (uint4 *)workspace;
    uint64_t *const col_off = (uint64_t *)((char *)workspace + gabriel::suffix_bytes(n_cells));
    uint32_t *const col_count = (uint32_t *)((char *)col_off + gabriel::col_off_bytes(n_snps));
    const gabriel::Band b{ci_lo, ci_hi, lo, offsets, n_cells, keep, n_snps};
    const uint32_t grid = (n_snps + 255u) / 256u;
    gabriel::suffix_kernel<<<grid, 256, 0, s>>>(b, prm, suf);
    LDX_HIP(hipGetLastError());
    gabriel::columns_kernel<<<grid, 256, 0, s>>>(lo, n_snps, col_count);
    LDX_HIP(hipGetLastError());
    gabriel::scan_kernel<<<1, 256, 0, s>>>(col_count, n_snps, col_off);
    LDX_HIP(hipGetLastError());
    gabriel::candidates_kernel<<<grid, 256, 0, s>>>(b, prm, positions, window, suf, col_off, cand_span, cand_first, cand_last);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_gabriel_pick_dev(const int64_t *sorted_span, const int64_t *order, const uint32_t *cand_first,
                                    const uint32_t *cand_last, uint64_t n_cells, const uint8_t *keep, uint32_t n_snps,
                                    uint32_t *block_of, uint32_t *n_out, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *const who = "ldx_gabriel_pick_dev";
    LDX_ARG_PTR(who, block_of); LDX_ARG_PTR(who, n_out); LDX_ARG_PTR(who, workspace);
    LDX_ARG_REQUIRE(n_snps != 0u, "%s: n_snps is 0", who);
    LDX_ARG_REQUIRE(n_cells == 0u || (sorted_span && order && cand_first && cand_last),
                    "%s: a null pointer among sorted_span, order, cand_first, cand_last but n_cells is %llu", who,
                    (unsigned long long)n_cells);
    LDX_ARG_REQUIRE(workspace_bytes >= ldx_gabriel_pick_workspace_bytes(n_snps), "%s: workspace_bytes %zu < %zu", who,
                    workspace_bytes, ldx_gabriel_pick_workspace_bytes(n_snps));
    uint8_t *const used = (uint8_t *)workspace;
    gabriel::pick_kernel<<<1, 256, 0, (hipStream_t)stream>>>(sorted_span, order, cand_first, cand_last, n_cells, keep, n_snps, used,
                                                             used + gabriel::round256(n_snps), block_of, n_out);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

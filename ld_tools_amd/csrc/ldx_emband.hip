// EM LD on the band (include/ldx.h, "EM on the band"): the in-window pairs i > j of ONE panel with the cell of
// ldx_ld_em_rect_dev (pairwise: ldx_ld_em_rect_pw_dev) -- the maximum-likelihood r and D' of the pair's genotype table --
// stored in the band layout (ldx_ld_em_band_dev) or filtered into neighbour records that carry D' (ldx_ld_em_neighbors_dev);
// and the per-SNP N, A, diagonal and `live` such a band goes with (ldx_em_snp_stats_dev).
//   * cell: tile_body (ldx_em_pw_tile.h), the tile of em_pw_kernel with both of its K loops, panel x panel; every cell goes
//     through the ONE em_cell(N, A, B, S, H) of ldx_em_tile.h.  A cell is a function of the pair's five integers alone, so it
//     is the rectangle's cell at (i, j) bit for bit, whichever tile computes it.  kPairwise = false is em_kernel's path: always
//     two sets, N = n_hap / 2, A / B from acnt; ref and rcnt are not read.
//   * tile: one workgroup (2 x 2 waves of 64 x 64 cells, two workgroups per CU) owns I slab ti x J slab tj of the panel.
//   * window, walk and plan: ldx_band_plan.h with I blocks of 128 rows -- low[i] per SNP, the exclusive prefix of the slabs
//     low[128 ti] / 128 .. (r1 - 1) / 128 per I block, both into the workspace; the grid is fixed at min(tile bound, 2 x CUs),
//     a workgroup strides over the tile numbers and finds (ti, tj) by binary search.  The host reads nothing back.
//   * per-tile tables: r_low, r_lo, r_off of the tile's 128 rows, 2 KiB of LDS beside tile_body's 65 KiB; tile_body's first
//     barrier publishes them.  A cell is inside iff r_low[li] <= j < i; em_cell -- the fp64 root search -- runs for the cells
//     inside only, so a tile that the window cuts pays for its share.
//   * epilogues: Store writes values_r / values_d[offsets[i] + j - lo[i]] under ldx_ld_pw_band_dev's guard; Nbr appends both
//     orientations of a pair in one HitAppender call, D' in the record's fourth word (as ldx_ld_em_rect_hits_dev).
#include "ldx_band_plan.h"
#include "ldx_em_pw_tile.h"

namespace ldx {
namespace emband {

using bandplan::kNoRow;
using em::kThreads;

enum Op : int { kStore = 0, kNbr = 1 };

struct Args {
    em_pw::Side s;             // the panel: both sides of every tile
    uint32_t nblocks;          // K-blocks of 256 haplotypes
    uint32_t n_hap;
    const uint64_t *prefix;    // [Ti + 1] tiles in front of each I block, the total last (workspace)
    const uint32_t *low;       // [n] the window's first column per row (workspace)
    const uint32_t *lo;        // store: the caller's layout
    const uint64_t *offsets;
    float *values_r, *values_d;   // store: either may be null
    uint64_t n_cells;
    float bound;               // neighbours: kept iff r *f32 r >= bound
    ldx_hit *hits;
    uint64_t hit_cap;
    unsigned long long *n_hits;
};

// the band's own per-tile tables, beside tile_body's: 2 KiB
struct BandLds {
    uint64_t r_off[kSlab];   // store: offsets[i]
    uint32_t r_low[kSlab];   // the window's first column of row i (kNoRow beyond the panel)
    uint32_t r_lo[kSlab];    // store: the caller's lo[i]
};

template <int kOp>
struct BandEmit {
    const Args &p;
    const BandLds &bl;
    HitAppender hit;
    uint32_t ti = 0;   // the tile's I slab

    __device__ __forceinline__ void operator()(uint32_t i, uint32_t j, uint32_t N, uint32_t A, uint32_t B, uint32_t S, uint32_t H)
    {
        const uint32_t li = i - ti * kSlab;
        const bool inside = j < i && j >= bl.r_low[li];   // (i < n: r_low is kNoRow otherwise; j < i < n)
        em::Cell c{-0.0f, -0.0f, 0.0};
        if (inside) c = em::em_cell(N, A, B, S, H);
        if constexpr (kOp == kStore) {
            const uint32_t lo_i = bl.r_lo[li];
            const uint64_t idx = bl.r_off[li] + (uint64_t)(j - lo_i);
            if (inside && j >= lo_i && idx < p.n_cells) {   // ldx_ld_pw_band_dev's guard
                if (p.values_r) p.values_r[idx] = c.r;
                if (p.values_d) p.values_d[idx] = c.dprime;
            }
        } else {
            hit.append_both(inside && c.r * c.r >= p.bound, i, j, c.r, c.dprime);   // ONE float32 multiply; -0.0f gives 0 < bound
        }
    }
};

template <int kOp, bool kPairwise>
__global__ void __launch_bounds__(kThreads, 2) emband_kernel(Args p)
{
    __shared__ em_pw::Smem sm;
    __shared__ BandLds bl;
    const uint32_t n = p.s.n, Ti = n_slabs(n);
    const uint64_t total = p.prefix[Ti];
    BandEmit<kOp> emit{p, bl, HitAppender{p.hits, p.hit_cap, p.n_hits, threadIdx.x & 63u}};
    for (uint64_t t = blockIdx.x; t < total; t += gridDim.x) {   // workgroup-uniform
        uint32_t ti, tj;
        bandplan::tile_at<kSlab>(p.prefix, p.low, Ti, t, ti, tj);
        if (t != blockIdx.x) block_sync();   // the last tile's tables, image and staged words are free
        // (the thread's number as a value of THIS trip, as in pwband_kernel: what tile_body derives from it would otherwise be
        // made once in front of the loop and held in registers across every K loop)
        uint32_t tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        if (tid < kSlab) {
            const uint32_t x_r = ti * kSlab + tid;
            bl.r_low[tid] = x_r < n ? p.low[x_r] : kNoRow;
            if constexpr (kOp == kStore) {
                bl.r_lo[tid] = x_r < n ? p.lo[x_r] : kNoRow;
                bl.r_off[tid] = x_r < n ? p.offsets[x_r] : 0u;
            }
        }
        emit.ti = ti;
        em_pw::tile_body<kPairwise>(sm, p.s, p.s, p.nblocks, p.n_hap, ti, tj, tid, emit);   // (its first barrier publishes the tables)
    }
    if constexpr (kOp == kNbr) emit.hit.close();   // what is left of the wave's last batch
}

// N, A, diag and live of one SNP over its OWN called individuals: one wavefront per row (pwband's snp_stats_kernel).  Plain
// form: N = n_hap / 2, A = acnt.  Pairwise form: the individuals with both codes called and the sum of their dosages, from
// both planes (a lane per 32-bit word).  live iff 0 < A < 2 N: the SNP has both alleles among them -- an all-heterozygous SNP,
// whose dosage does not vary, is live here.  The diagonal is DEFINED as +1 / -0.0f (em_cell(i, i) is -1 for such a SNP under
// the tie rule).
template <bool kPairwise>
__global__ void __launch_bounds__(256) snp_stats_kernel(const uint32_t *__restrict__ alt, const uint32_t *__restrict__ ref,
                                                        const uint32_t *__restrict__ acnt, uint32_t n_snps, uint32_t n_hap,
                                                        uint32_t *__restrict__ out_n, uint32_t *__restrict__ out_a,
                                                        float *__restrict__ diag, uint8_t *__restrict__ live)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= n_snps) return;   // wave-uniform
    uint32_t N = n_hap / 2u, A = 0;
    if constexpr (!kPairwise) {
        A = acnt[row];
    } else {
        const uint32_t nchunks = n_chunks(n_hap), slab = row / kSlab, rin = row % kSlab;
        N = 0;
        for (uint32_t w = lane; w < nchunks * 4u; w += 64u) {
            const size_t at = (((size_t)slab * nchunks + (w >> 2)) * kSlab + rin) * 4u + (w & 3u);
            const uint32_t wa = alt[at], q = ind_called(wa, ref[at]), g = wa & (q | (q << 1));
            N += __builtin_popcount(q);
            A += __builtin_popcount(g);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            N += __shfl_xor(N, off);
            A += __shfl_xor(A, off);
        }
    }
    if (lane != 0u) return;
    const bool lv = A > 0u && A < 2u * N;
    out_n[row] = N;
    out_a[row] = A;
    diag[row] = lv ? 1.0f : -0.0f;
    if (live) live[row] = lv ? 1u : 0u;
}

static size_t workspace_bytes(uint32_t n_snps) { return bandplan::workspace_bytes<kSlab>(n_snps); }

// low, the plan, then the band: everything in stream order, nothing read back
template <int kOp>
static int launch(Args &p, bool pairwise, const int64_t *positions, int64_t window, void *workspace, hipStream_t s)
{
    const uint32_t n = p.s.n;
    bandplan::Plan plan;
    if (const int rc = bandplan::make_plan<kSlab>(positions, n, window, workspace, s, plan)) return rc;
    p.prefix = plan.prefix, p.low = plan.low;
    const uint64_t Ti = n_slabs(n), tiles = Ti * (Ti + 1u) / 2u;   // (the lower triangle: an upper bound of the plan's total)
    const uint64_t cap = 2u * (uint64_t)device_cus();              // two workgroups per CU are resident
    const uint32_t grid = (uint32_t)(tiles < cap ? tiles : cap);
    if (pairwise) emband_kernel<kOp, true><<<grid, kThreads, 0, s>>>(p);
    else emband_kernel<kOp, false><<<grid, kThreads, 0, s>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

}  // namespace emband
}  // namespace ldx

using namespace ldx;

// the panel's pointers: ref and rcnt may be null only in the plain form; everything returns before any HIP call
#define LDX_EMB_PANEL(who)                                                                                         \
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, acnt);                                                                 \
    LDX_ARG_REQUIRE(ref != nullptr || !pairwise, "%s: ref is a null pointer (the pairwise form reads both planes)", who); \
    LDX_ARG_REQUIRE(rcnt != nullptr || !pairwise, "%s: rcnt is a null pointer (the pairwise form reads both count tables)", who)

static int shape_ok(const char *who, uint32_t n_snps, uint32_t n_hap)
{
    LDX_ARG_REQUIRE(n_snps != 0u, "%s: n_snps is 0", who);
    LDX_ARG_REQUIRE(n_hap != 0u, "%s: n_hap is 0", who);
    LDX_ARG_REQUIRE(n_hap % 2u == 0u, "%s: n_hap %u is odd (haplotypes 2k and 2k + 1 are the two alleles of individual k)", who, n_hap);
    if (n_hap > LDX_MAX_HAPS) {
        set_error("%s: n_hap %u > LDX_MAX_HAPS %u", who, n_hap, LDX_MAX_HAPS);
        return LDX_E_UNSUPPORTED;
    }
    return plane_check(who, "alt", n_snps, n_hap);
}

static int band_ok(const char *who, uint32_t n_snps, uint32_t n_hap, const int64_t *positions, int64_t window, const void *workspace,
                   size_t workspace_bytes)
{
    LDX_ARG_PTR(who, positions);
    LDX_ARG_PTR(who, workspace);
    LDX_ARG_REQUIRE(window >= 0, "%s: window %lld is negative", who, (long long)window);
    if (const int rc = shape_ok(who, n_snps, n_hap)) return rc;
    LDX_ARG_REQUIRE(workspace_bytes >= emband::workspace_bytes(n_snps), "%s: workspace_bytes %zu < %zu", who, workspace_bytes,
                    emband::workspace_bytes(n_snps));
    return LDX_OK;
}

static emband::Args make_args(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                              uint32_t n_hap)
{
    emband::Args p{};
    p.s = em_pw::Side{(const uint4 *)alt, (const uint4 *)ref, acnt, rcnt, n_snps};
    p.nblocks = n_chunks(n_hap) / 2u;
    p.n_hap = n_hap;
    return p;
}

extern "C" size_t ldx_ld_em_band_workspace_bytes(uint32_t n_snps) { return emband::workspace_bytes(n_snps); }

extern "C" int ldx_em_snp_stats_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                                    uint32_t n_hap, int pairwise, uint32_t *N, uint32_t *A, float *diag, uint8_t *live, void *stream)
{
    const char *const who = "ldx_em_snp_stats_dev";
    LDX_EMB_PANEL(who);
    LDX_ARG_PTR(who, N); LDX_ARG_PTR(who, A); LDX_ARG_PTR(who, diag);
    if (const int rc = shape_ok(who, n_snps, n_hap)) return rc;
    const uint32_t grid = (n_snps + 3u) / 4u;
    if (pairwise)
        emband::snp_stats_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>((const uint32_t *)alt, (const uint32_t *)ref, acnt,
                                                                               n_snps, n_hap, N, A, diag, live);
    else
        emband::snp_stats_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>((const uint32_t *)alt, nullptr, acnt, n_snps, n_hap,
                                                                                N, A, diag, live);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_ld_em_band_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                                  uint32_t n_hap, int pairwise, const int64_t *positions, int64_t window, const uint32_t *lo,
                                  const uint64_t *offsets, float *values_r, float *values_dprime, uint64_t n_cells, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    const char *const who = "ldx_ld_em_band_dev";
    LDX_EMB_PANEL(who);
    LDX_ARG_PTR(who, lo);
    LDX_ARG_PTR(who, offsets);
    LDX_ARG_REQUIRE(values_r != nullptr || values_dprime != nullptr || n_cells == 0u,
                    "%s: values_r and values_dprime are both null pointers but n_cells is %llu", who, (unsigned long long)n_cells);
    if (const int rc = band_ok(who, n_snps, n_hap, positions, window, workspace, workspace_bytes)) return rc;
    if (n_cells == 0u) return LDX_OK;   // no pair in any window: nothing to write
    emband::Args p = make_args(alt, ref, acnt, rcnt, n_snps, n_hap);
    p.lo = lo, p.offsets = offsets, p.values_r = values_r, p.values_d = values_dprime, p.n_cells = n_cells;
    return emband::launch<emband::kStore>(p, pairwise != 0, positions, window, workspace, (hipStream_t)stream);
}

extern "C" int ldx_ld_em_neighbors_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                                       uint32_t n_hap, int pairwise, const int64_t *positions, int64_t window, float r2_bound,
                                       ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    const char *const who = "ldx_ld_em_neighbors_dev";
    LDX_EMB_PANEL(who);
    if (const int rc = hit_args_ok(who, r2_bound, hits, hit_cap, n_hits)) return rc;
    if (const int rc = band_ok(who, n_snps, n_hap, positions, window, workspace, workspace_bytes)) return rc;
    emband::Args p = make_args(alt, ref, acnt, rcnt, n_snps, n_hap);
    p.bound = r2_bound, p.hits = hits, p.hit_cap = hit_cap, p.n_hits = (unsigned long long *)n_hits;
    LDX_HIP(hipMemsetAsync(n_hits, 0, sizeof(uint64_t), (hipStream_t)stream));   // the slot counter starts at 0
    return emband::launch<emband::kNbr>(p, pairwise != 0, positions, window, workspace, (hipStream_t)stream);
}

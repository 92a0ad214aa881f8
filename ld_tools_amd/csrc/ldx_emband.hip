// EM LD on the band (include/ldx.h, "EM on the band"): the in-window pairs i > j of ONE panel with the cell of
// ldx_ld_em_rect_dev (pairwise: ldx_ld_em_rect_pw_dev) -- the maximum-likelihood r and D' of the pair's genotype table --
// stored in the band layout (ldx_ld_em_band_dev) or filtered into neighbour records that carry D' (ldx_ld_em_neighbors_dev);
// and the per-SNP N, A, diagonal and `live` such a band goes with (ldx_em_snp_stats_dev).
//   * cell: tile_body (ldx_em_pw_tile.h), the tile of em_rect_kernel (ldx_em.hip) with both of its K loops, panel x panel;
//     every cell goes through the ONE em_cell(N, A, B, S, H) of ldx_em_tile.h.  A cell is a function of the pair's five integers
//     alone, so it is the rectangle's cell at (i, j) bit for bit, whichever tile computes it.  kPairwise = false is the plain
//     form: always two sets, N = n_hap / 2, A / B from acnt; ref and rcnt are not read.
//   * tile: one workgroup (2 x 2 waves of 64 x 64 cells, two workgroups per CU) owns I slab ti x J slab tj of the panel.
//   * window, walk, plan, tables and argument rules: ldx_band_plan.h, shared with pwband_kernel, with I blocks of 128 rows --
//     low[i] per SNP, the exclusive prefix of the slabs low[128 ti] / 128 .. (r1 - 1) / 128 per I block, both into the
//     workspace; the grid is fixed at min(tile bound, 2 x CUs), a workgroup strides over the tile numbers and finds (ti, tj)
//     by binary search.  The host reads nothing back.
//   * per-tile tables: r_low, r_lo, r_off of the tile's 128 rows, 2 KiB of LDS beside tile_body's 65 KiB; tile_body's first
//     barrier publishes them.  A cell is inside iff r_low[li] <= j < i; em_cell -- the fp64 root search -- runs for the cells
//     inside only, so a tile that the window cuts pays for its share.
//   * epilogues: Ci (ldx_ld_em_ci_band_dev) writes the D' confidence bounds of ci_cell for the pairs of kept SNPs into a layout
//     that fill_no_ci_kernel set to 0xFF in front of the band; Store writes values_r / values_d[offsets[i] + j - lo[i]] under ldx_ld_band_dev's guard; Nbr appends both
//     orientations of a pair in one HitAppender call, D' in the record's fourth word (as ldx_ld_em_rect_hits_dev).
#include "ldx_band_plan.h"
#include "ldx_em_pw_tile.h"

namespace ldx {
namespace emband {

using em::kThreads;
static_assert(kThreads == bandplan::kBandThreads, "the walk's workgroup");
using BandLds = bandplan::RowTables<kSlab>;   // the band's own per-tile tables, beside tile_body's: 2 KiB

enum Op : int { kStore = 0, kNbr = 1, kCi = 2 };

struct Args {
    em_pw::Side s;             // the panel: both sides of every tile
    uint32_t nblocks;          // K-blocks of 256 haplotypes
    uint32_t n_hap;
    bandplan::Plan plan;
    const uint32_t *lo;        // store: the caller's layout
    const uint64_t *offsets;
    float *values_r, *values_d;   // store: either may be null
    uint64_t n_cells;
    float bound;               // neighbours: kept iff r *f32 r >= bound
    ldx_hit *hits;
    uint64_t hit_cap;
    unsigned long long *n_hits;
    const uint8_t *keep;       // bounds: the SNPs whose pairs get an interval (null: all)
    uint8_t *ci_lo, *ci_hi;    // bounds: the caller's layout, filled with kNoCi in front of the band
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
        const bool inside = bandplan::inside(bl, li, i, j);
        if constexpr (kOp == kCi) {
            // the likelihood surface runs for the pairs of kept SNPs inside only; every other cell keeps the fill's kNoCi
            uint64_t idx;
            if (bandplan::store_at(bl, li, j, inside && (!p.keep || (p.keep[i] != 0u && p.keep[j] != 0u)), p.n_cells, idx)) {
                const em::Ci ci = em::ci_cell(N, A, B, S, H);
                p.ci_lo[idx] = ci.lo;
                p.ci_hi[idx] = ci.hi;
            }
            return;
        }
        em::Cell c{-0.0f, -0.0f, 0.0};
        if (inside) c = em::em_cell(N, A, B, S, H);
        if constexpr (kOp == kStore) {
            uint64_t idx;
            if (bandplan::store_at(bl, li, j, inside, p.n_cells, idx)) {
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
    BandEmit<kOp> emit{p, bl, HitAppender{p.hits, p.hit_cap, p.n_hits, threadIdx.x & 63u}};
    bandplan::walk<kSlab>(p.plan, p.s.n, [&](uint32_t ti, uint32_t tj, uint32_t tid) {
        bandplan::fill_rows<kOp != kNbr>(bl, p.plan, p.lo, p.offsets, p.s.n, ti, tid);
        emit.ti = ti;
        em_pw::tile_body<kPairwise>(sm, p.s, p.s, p.nblocks, p.n_hap, ti, tj, tid, emit);   // (its first barrier publishes the tables)
    });
    if constexpr (kOp == kNbr) emit.hit.close();   // what is left of the wave's last batch
}

// N, A, diag and live of one SNP over its OWN called individuals: one wavefront per row.  Plain form: N = n_hap / 2, A = acnt.
// Pairwise form: the individuals with both codes called and the sum of their dosages, from both planes (called_sums,
// ldx_band_plan.h).  live iff 0 < A < 2 N: the SNP has both alleles among them -- an all-heterozygous SNP,
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
        const bandplan::CalledSums c = bandplan::called_sums<false>(alt, ref, row, n_chunks(n_hap), lane);
        N = c.N, A = c.A;
    }
    if (lane != 0u) return;
    const bool lv = A > 0u && A < 2u * N;
    out_n[row] = N;
    out_a[row] = A;
    diag[row] = lv ? 1.0f : -0.0f;
    if (live) live[row] = lv ? 1u : 0u;
}

// kNoCi into every cell of both bound arrays: four cells per thread, one 32-bit store where the array allows it
__global__ void __launch_bounds__(256) fill_no_ci_kernel(uint8_t *__restrict__ a, uint8_t *__restrict__ b, uint64_t n_cells)
{
    const uint64_t at = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (at >= n_cells) return;
    uint8_t *const both[2] = {a, b};
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        uint8_t *const dst = both[w] + at;
        if (((uintptr_t)dst & 3u) == 0u && at + 4u <= n_cells) {
            *reinterpret_cast<uint32_t *>(dst) = 0xFFFFFFFFu;
        } else {
            for (uint64_t q = 0; q < 4u && at + q < n_cells; ++q) dst[q] = em::kNoCi;
        }
    }
}

// low, the plan, then the band (bandplan::launch); the tile bound is the lower triangle of I blocks x slabs
template <int kOp>
static int launch(Args &p, bool pairwise, const int64_t *positions, int64_t window, void *workspace, hipStream_t s)
{
    const uint64_t Ti = n_slabs(p.s.n);
    auto go = [&](const bandplan::Plan &plan, uint32_t grid) {
        p.plan = plan;
        if (pairwise) emband_kernel<kOp, true><<<grid, kThreads, 0, s>>>(p);
        else emband_kernel<kOp, false><<<grid, kThreads, 0, s>>>(p);
        LDX_HIP(hipGetLastError());
        return (int)LDX_OK;
    };
    return bandplan::launch<kSlab>(positions, p.s.n, window, workspace, s, Ti * (Ti + 1u) / 2u, go);
}

}  // namespace emband
}  // namespace ldx

using namespace ldx;

// the panel's pointers: ref and rcnt may be null only in the plain form; everything returns before any HIP call
#define LDX_EMB_PANEL(who)                                                                                         \
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, acnt);                                                                 \
    LDX_ARG_REQUIRE(ref != nullptr || !pairwise, "%s: ref is a null pointer (the pairwise form reads both planes)", who); \
    LDX_ARG_REQUIRE(rcnt != nullptr || !pairwise, "%s: rcnt is a null pointer (the pairwise form reads both count tables)", who)

static const char *const kOddReason = "haplotypes 2k and 2k + 1 are the two alleles of individual k";

static emband::Args make_args(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                              uint32_t n_hap)
{
    emband::Args p{};
    p.s = em_pw::Side{(const uint4 *)alt, (const uint4 *)ref, acnt, rcnt, n_snps};
    p.nblocks = n_chunks(n_hap) / 2u;
    p.n_hap = n_hap;
    return p;
}

extern "C" size_t ldx_ld_em_band_workspace_bytes(uint32_t n_snps) { return bandplan::workspace_bytes<kSlab>(n_snps); }

extern "C" int ldx_em_snp_stats_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                                    uint32_t n_hap, int pairwise, uint32_t *N, uint32_t *A, float *diag, uint8_t *live, void *stream)
{
    const char *const who = "ldx_em_snp_stats_dev";
    LDX_EMB_PANEL(who);
    LDX_ARG_PTR(who, N); LDX_ARG_PTR(who, A); LDX_ARG_PTR(who, diag);
    if (const int rc = bandplan::shape_ok(who, n_snps, n_hap, kOddReason)) return rc;
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
    if (const int rc = bandplan::band_args_ok<kSlab>(who, n_snps, n_hap, kOddReason, positions, window, workspace, workspace_bytes))
        return rc;
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
    if (const int rc = bandplan::band_args_ok<kSlab>(who, n_snps, n_hap, kOddReason, positions, window, workspace, workspace_bytes))
        return rc;
    emband::Args p = make_args(alt, ref, acnt, rcnt, n_snps, n_hap);
    p.bound = r2_bound, p.hits = hits, p.hit_cap = hit_cap, p.n_hits = (unsigned long long *)n_hits;
    LDX_HIP(hipMemsetAsync(n_hits, 0, sizeof(uint64_t), (hipStream_t)stream));   // the slot counter starts at 0
    return emband::launch<emband::kNbr>(p, pairwise != 0, positions, window, workspace, (hipStream_t)stream);
}

extern "C" int ldx_ld_em_ci_band_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                                     uint32_t n_hap, int pairwise, const int64_t *positions, int64_t window, const uint8_t *keep,
                                     const uint32_t *lo, const uint64_t *offsets, uint8_t *ci_lo, uint8_t *ci_hi, uint64_t n_cells,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    const char *const who = "ldx_ld_em_ci_band_dev";
    LDX_EMB_PANEL(who);
    LDX_ARG_PTR(who, lo);
    LDX_ARG_PTR(who, offsets);
    LDX_ARG_REQUIRE((ci_lo != nullptr && ci_hi != nullptr) || n_cells == 0u,
                    "%s: ci_lo or ci_hi is a null pointer but n_cells is %llu", who, (unsigned long long)n_cells);
    if (const int rc = bandplan::band_args_ok<kSlab>(who, n_snps, n_hap, kOddReason, positions, window, workspace, workspace_bytes))
        return rc;
    if (n_cells == 0u) return LDX_OK;   // no pair in any window: nothing to write
    const uint64_t fill_grid = (n_cells + 1023u) / 1024u;
    if (fill_grid >= (1ull << 31)) {
        set_error("%s: n_cells = %llu needs 2^31 or more workgroups", who, (unsigned long long)n_cells);
        return LDX_E_UNSUPPORTED;
    }
    emband::fill_no_ci_kernel<<<(uint32_t)fill_grid, 256, 0, (hipStream_t)stream>>>(ci_lo, ci_hi, n_cells);
    LDX_HIP(hipGetLastError());
    emband::Args p = make_args(alt, ref, acnt, rcnt, n_snps, n_hap);
    p.lo = lo, p.offsets = offsets, p.n_cells = n_cells, p.keep = keep, p.ci_lo = ci_lo, p.ci_hi = ci_hi;
    return emband::launch<emband::kCi>(p, pairwise != 0, positions, window, workspace, (hipStream_t)stream);
}

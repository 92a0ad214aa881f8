// Pairwise-complete rectangular LD (include/ldx.h, "pairwise-complete LD"): the signed r of every row of panel I against every
// row of panel J over the haplotypes (dosage form: the individuals) CALLED AT BOTH SNPs -- what PLINK --r2 does with missing
// calls -- as dense float32 cells (ldx_ld_rect_pw_dev), the pairs whose float32 square reaches a bound (ldx_ld_rect_pw_hits_dev)
// or the pair's integers alone (ldx_ld_rect_pw_counts_dev).  One kernel of its own, pwc_kernel, beside rect_kernel
// (ldx_rect.hip) and em_kernel (ldx_em.hip), whose counting scheme, LDS image, walk and hit appender it follows:
//   * counting, tile, shortcut, general loop, K loop: tile_body (ldx_pwc_tile.h), shared with the band's pwband_kernel
//     (ldx_pwband.hip); this file holds the rectangle's three epilogues and its walk.  The dosage shortcut counts its homozygotes
//     in the prologue: these entries have no workspace argument to keep a per-panel table in.
//   * stores: a half-wave holds 32 consecutive cells of one output row, 128-byte row-major non-temporal stores.
//   * walk: tile_of (ldx_fp4.h) in rect_kernel's bands of 16 I blocks.  hits: HitAppender (ldx_common.h).
#include "ldx_pwc_tile.h"

namespace ldx {
namespace pwc {

constexpr uint32_t kBandTiles = 16;                   // I blocks per band of the walk

enum Mode : int { kDense = 0, kHits = 1, kCounts = 2 };

struct Args {
    Side si, sj;
    uint32_t nblocks;         // K-blocks of 256 haplotypes: n_chunks / 2
    uint32_t n_hap;
    float *out;               // dense: [n_i][ld]
    uint32_t *counts;         // counts: [sets][n_i][ld]
    size_t ld;
    float bound;              // hits: kept iff r *f32 r >= bound
    ldx_hit *hits;
    uint64_t hit_cap;
    unsigned long long *n_hits;
};

// one cell, from its integers k[] and the 1 / sqrt of its two variances: the same for both paths of tile_body
template <int kMode, bool kDosage>
struct RectEpi {
    static constexpr bool kCells = kMode != kCounts, kReduce = false;
    static constexpr uint32_t kSets = Geo<kDosage>::kSets, kLast = Geo<kDosage>::kLast;
    const Args &p;
    HitAppender hit;
    size_t plane;   // one set of the counts output

    __device__ __forceinline__ void cell(uint32_t i, uint32_t j, int, const double (&k)[kSets], double rs_x, double rs_y)
    {
        const bool inside = i < p.si.n && j < p.sj.n;
        if constexpr (kMode == kCounts) {
            if (inside)
#pragma unroll
                for (uint32_t s = 0; s < kSets; ++s)
                    __builtin_nontemporal_store((uint32_t)k[s], p.counts + s * plane + (size_t)i * p.ld + j);
        } else {
            const float c = r32_cell(k[kLast], k[0], k[1], rs_x, k[2], rs_y).r;
            if constexpr (kMode == kHits) {
                const float s2 = c * c;   // ONE float32 multiply; -0.0f (degenerate) and +0.0f give 0 < bound
                hit.append(inside && s2 >= p.bound, i, j, c, s2);
            } else if (inside) {
                __builtin_nontemporal_store(c, p.out + (size_t)i * p.ld + j);   // written once, never read back here
            }
        }
    }
};

template <int kMode, bool kDosage>
__global__ void __launch_bounds__(kThreads, 2) pwc_kernel(Args p)
{
    __shared__ Smem sm;
    const uint32_t Ti = (p.si.n + kTileRows - 1u) / kTileRows, Tj = n_slabs(p.sj.n);
    uint32_t ti, tj;
    tile_of<kBandTiles>(blockIdx.x, Ti, Tj, ti, tj);
    RectEpi<kMode, kDosage> epi{p, HitAppender{p.hits, p.hit_cap, p.n_hits, threadIdx.x & 63u}, (size_t)p.si.n * p.ld};
    tile_body<kDosage, false>(sm, p.si, p.sj, p.nblocks, p.n_hap, ti, tj, threadIdx.x, epi);
    if constexpr (kMode == kHits) epi.hit.close();   // what is left of the wave's last batch
}

template <int kMode>
static int launch(const Args &p, bool dosage, hipStream_t s)
{
    const uint32_t grid = ((p.si.n + kTileRows - 1u) / kTileRows) * n_slabs(p.sj.n);
    if (dosage) pwc_kernel<kMode, true><<<grid, kThreads, 0, s>>>(p);
    else pwc_kernel<kMode, false><<<grid, kThreads, 0, s>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

}  // namespace pwc
}  // namespace ldx

using namespace ldx;

// the three entries' pointers and shape rules: rect_args_ok (ldx_common.h) with this kernel's I block and the dosage form's
// parity rule; everything returns before any HIP call
#define LDX_PW_SIDES(who)                                                                               \
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, ref_i); LDX_ARG_PTR(who, acnt_i); LDX_ARG_PTR(who, rcnt_i); \
    LDX_ARG_PTR(who, alt_j); LDX_ARG_PTR(who, ref_j); LDX_ARG_PTR(who, acnt_j); LDX_ARG_PTR(who, rcnt_j)

static int args_ok(const char *who, uint32_t n_i, uint32_t n_j, uint32_t n_hap, bool dosage)
{
    return rect_args_ok(who, n_i, n_j, n_hap, dosage ? "dosage pairs haplotypes 2k and 2k + 1 into individuals" : nullptr,
                        pwc::kTileRows);
}

static pwc::Args make_args(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                           const void *alt_j, const void *ref_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                           uint32_t n_hap)
{
    pwc::Args p{};
    p.si = pwc::Side{(const uint4 *)alt_i, (const uint4 *)ref_i, acnt_i, rcnt_i, n_i, nullptr};
    p.sj = pwc::Side{(const uint4 *)alt_j, (const uint4 *)ref_j, acnt_j, rcnt_j, n_j, nullptr};
    p.nblocks = n_chunks(n_hap) / 2u;
    p.n_hap = n_hap;
    return p;
}

extern "C" int ldx_ld_rect_pw_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i,
                                  uint32_t n_i, const void *alt_j, const void *ref_j, const uint32_t *acnt_j,
                                  const uint32_t *rcnt_j, uint32_t n_j, uint32_t n_hap, int dosage, float *out, size_t ld_out,
                                  void *stream)
{
    const char *const who = "ldx_ld_rect_pw_dev";
    LDX_PW_SIDES(who);
    LDX_ARG_PTR(who, out);
    LDX_ARG_REQUIRE(ld_out >= n_j, "%s: ld_out %zu < n_j %u", who, ld_out, n_j);
    if (const int rc = args_ok(who, n_i, n_j, n_hap, dosage != 0)) return rc;
    pwc::Args p = make_args(alt_i, ref_i, acnt_i, rcnt_i, n_i, alt_j, ref_j, acnt_j, rcnt_j, n_j, n_hap);
    p.out = out, p.ld = ld_out;
    return pwc::launch<pwc::kDense>(p, dosage != 0, (hipStream_t)stream);
}

extern "C" int ldx_ld_rect_pw_hits_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i,
                                       uint32_t n_i, const void *alt_j, const void *ref_j, const uint32_t *acnt_j,
                                       const uint32_t *rcnt_j, uint32_t n_j, uint32_t n_hap, int dosage, float r2_bound,
                                       ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, void *stream)
{
    const char *const who = "ldx_ld_rect_pw_hits_dev";
    LDX_PW_SIDES(who);
    if (const int rc = hit_args_ok(who, r2_bound, hits, hit_cap, n_hits)) return rc;
    if (const int rc = args_ok(who, n_i, n_j, n_hap, dosage != 0)) return rc;
    pwc::Args p = make_args(alt_i, ref_i, acnt_i, rcnt_i, n_i, alt_j, ref_j, acnt_j, rcnt_j, n_j, n_hap);
    p.bound = r2_bound, p.hits = hits, p.hit_cap = hit_cap, p.n_hits = (unsigned long long *)n_hits;
    LDX_HIP(hipMemsetAsync(n_hits, 0, sizeof(uint64_t), (hipStream_t)stream));   // the slot counter starts at 0
    return pwc::launch<pwc::kHits>(p, dosage != 0, (hipStream_t)stream);
}

extern "C" int ldx_ld_rect_pw_counts_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i,
                                         uint32_t n_i, const void *alt_j, const void *ref_j, const uint32_t *acnt_j,
                                         const uint32_t *rcnt_j, uint32_t n_j, uint32_t n_hap, int dosage, uint32_t *counts,
                                         size_t ld, void *stream)
{
    const char *const who = "ldx_ld_rect_pw_counts_dev";
    LDX_PW_SIDES(who);
    LDX_ARG_PTR(who, counts);
    LDX_ARG_REQUIRE(ld >= n_j, "%s: ld %zu < n_j %u", who, ld, n_j);
    if (const int rc = args_ok(who, n_i, n_j, n_hap, dosage != 0)) return rc;
    pwc::Args p = make_args(alt_i, ref_i, acnt_i, rcnt_i, n_i, alt_j, ref_j, acnt_j, rcnt_j, n_j, n_hap);
    p.counts = counts, p.ld = ld;
    return pwc::launch<pwc::kCounts>(p, dosage != 0, (hipStream_t)stream);
}

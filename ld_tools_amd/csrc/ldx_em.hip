// Unphased LD by maximum likelihood (include/ldx.h, "unphased LD by EM"): for every row of panel I against every row of panel
// J over the same individuals, the maximum-likelihood two-locus haplotype frequency from the genotype table (Hill 1974), and
// from it r and D' -- dense float32 cells (ldx_ld_em_rect_dev), the pairs whose r *f32 r reaches a bound
// (ldx_ld_em_rect_hits_dev), the two pair counts alone (ldx_ld_em_counts_dev) and the epilogue alone on a list of count
// tuples (ldx_ld_em_from_counts_dev).  One kernel of its own, em_kernel, beside the rectangle's (ldx_rect.hip), whose
// counting scheme and LDS image it follows; the FP4 expanders and the walk are the shared ones of ldx_fp4.h, the hit appender
// HitAppender of ldx_common.h; the K loop, the staging and em_cell live in ldx_em_tile.h, which em_pw_kernel (ldx_em_pw.hip, the
// pairwise-complete form) shares:
//   * counting: with the allele counts a_i, a_j fixed, the EM needs TWO pair counts, not the nine cells of the 3 x 3 table:
//     S = sum_k g_ik g_jk (the dosage rectangle's count: expand32_a4 x expand32_b4_dosage) and H = #{k : g_ik = g_jk = 1}.
//     The het bit of individual k, x = (w ^ (w >> 1)) & 0x5555..., sits on haplotype slot 2k only: expand32_a4(x) on the I
//     side (0.5 in registers 0 and 2, registers 1 and 3 are zero) and expand32_b4(x) on the J side (2 in registers 0 and 2),
//     so every product is exactly 1.  Both fp32 accumulator sets are exact: S <= 20 480, H <= 5 120.
//   * tile: a workgroup (4 waves as 2 x 2, two workgroups per CU) owns one 128-row slab of I x one 128-row slab of J; a wave
//     64 x 64 = 2 x 2 accumulator tiles of 32 x 32 in each of the two sets: 128 accumulator registers, the rectangle's number,
//     and the rectangle's ratio of four 16-byte-equivalent LDS fragment reads to eight MFMAs per K-step.
//   * K loop: the rectangle's -- a K-block is 256 haplotypes; per K-block the workgroup expands the J slab's bits ONCE into
//     two LDS images, S's [4 steps][2 halves][128 rows][16 B] and H's [4][2][128][8 B] (its two non-zero registers),
//     double-buffered (2 x 24 KiB), one block_sync per K-block; a lane loads the 16 bytes of its own I rows and expands them
//     in registers.  Plain HIP: the compiler tracks every load.
//   * epilogue: fp64 per cell with a data-dependent root search, so the accumulators do not stay in registers under it: each
//     wave packs (S, H) of its 64 x 64 cells into one word each, in the LDS the images no longer need (4 x 16 KiB), and a
//     rolled loop over the 64 rows has lane = column: one em_cell per lane and trip, 256-byte row-major stores per wave (128
//     per half-wave).  em_cell is a function of (N, a_i, a_j, S, H) alone, in an arithmetic symmetric in the two SNPs.
//   * walk: tile_of (ldx_fp4.h) with I blocks of 128 rows, 32 to a band (the rectangle's 4096-row bands).
#include "ldx_em_tile.h"

namespace ldx {
namespace em {

enum Mode : int { kDense = 0, kHits = 1, kCounts = 2 };

struct Args {
    const uint4 *alt_i, *alt_j;        // tiled bit planes (ldx_plane_bytes)
    const uint32_t *acnt_i, *acnt_j;   // [n] ALT counts (not read by the counts form)
    uint32_t n_i, n_j;
    uint32_t nblocks;                  // K-blocks of 256 haplotypes: n_chunks / 2
    uint32_t n_ind;                    // individuals: n_hap / 2
    float *out_r, *out_d;              // dense: [n_i][ld], either may be null
    uint32_t *out_s, *out_h;           // counts: [n_i][ld]
    size_t ld;
    float bound;                       // hits: kept iff r *f32 r >= bound
    ldx_hit *hits;
    uint64_t hit_cap;
    unsigned long long *n_hits;
};

template <int kMode>
__global__ void __launch_bounds__(kThreads, 2) em_kernel(Args p)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];   // K loop: two {S image, H image}; epilogue: packed counts
    __shared__ uint32_t cstat[kSlab];    // a_j of the slab's 128 columns
    __shared__ uint32_t rstat[kSlab];    // a_i of the workgroup's 128 rows
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wr = wave >> 1, wc = wave & 1u;   // the wave's 64 rows / 64 columns inside the 128 x 128 tile
    const uint32_t Ti = n_slabs(p.n_i), Tj = n_slabs(p.n_j);
    uint32_t ti, tj;
    tile_of<kBandTiles>(blockIdx.x, Ti, Tj, ti, tj);

    if constexpr (kMode != kCounts) {
        if (tid < kSlab) {
            const uint32_t j = tj * kSlab + tid;
            cstat[tid] = j < p.n_j ? p.acnt_j[j] : 0u;
        } else {
            const uint32_t i = ti * kSlab + (tid - kSlab);
            rstat[tid - kSlab] = i < p.n_i ? p.acnt_i[i] : 0u;
        }
    }

    // the K loop and the packed staging are the shared ones (ldx_em_tile.h); the loop's first barrier also publishes cstat / rstat
    v16f acc_s[2][2], acc_h[2][2];
    count_two_sets(lds, p.alt_i, p.alt_j, ti, tj, p.nblocks, tid, acc_s, acc_h);
    const uint32_t *const stage = stage_two_sets(lds, tid, acc_s, acc_h);

    const uint32_t j = tj * kSlab + wc * kWaveCols + lane;
    const bool col_ok = j < p.n_j;
    [[maybe_unused]] const uint32_t a_j = kMode != kCounts ? cstat[wc * kWaveCols + lane] : 0u;
    [[maybe_unused]] HitAppender hit{p.hits, p.hit_cap, p.n_hits, lane};
    const uint32_t row0 = ti * kSlab + wr * kWaveRows;
    const uint32_t rows = row0 < p.n_i ? (p.n_i - row0 < kWaveRows ? p.n_i - row0 : kWaveRows) : 0u;   // wave-uniform
    for (uint32_t rr = 0; rr < rows; ++rr) {
        const uint32_t i = row0 + rr;
        const uint32_t packed = stage[rr * kWaveCols + lane];
        const uint32_t S = packed >> kPackShift, H = packed & ((1u << kPackShift) - 1u);
        if constexpr (kMode == kCounts) {
            if (col_ok) {
                __builtin_nontemporal_store(S, p.out_s + (size_t)i * p.ld + j);
                __builtin_nontemporal_store(H, p.out_h + (size_t)i * p.ld + j);
            }
        } else {
            const uint32_t a_i = rstat[wr * kWaveRows + rr];   // one address per wave: broadcast
            Cell c{-0.0f, -0.0f, 0.0};
            if (col_ok) c = em_cell(p.n_ind, a_i, a_j, S, H);
            if constexpr (kMode == kHits) {
                hit.append(col_ok && c.r * c.r >= p.bound, i, j, c.r, c.dprime);   // ONE float32 multiply; -0.0f gives 0 < bound
            } else if (col_ok) {
                if (p.out_r) __builtin_nontemporal_store(c.r, p.out_r + (size_t)i * p.ld + j);
                if (p.out_d) __builtin_nontemporal_store(c.dprime, p.out_d + (size_t)i * p.ld + j);
            }
        }
    }
    if constexpr (kMode == kHits) hit.close();   // what is left of the wave's last batch
}

// the epilogue alone: one thread per tuple
__global__ void __launch_bounds__(256) from_counts_kernel(uint32_t n_ind, size_t m, const uint32_t *a1, const uint32_t *a2,
                                                          const uint32_t *S, const uint32_t *H, float *r, float *dprime, double *x)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    const Cell c = em_cell(n_ind, a1[k], a2[k], S[k], H[k]);
    if (r) r[k] = c.r;
    if (dprime) dprime[k] = c.dprime;
    if (x) x[k] = c.x;
}

static Args make_args(const void *alt_i, const uint32_t *acnt_i, uint32_t n_i, const void *alt_j, const uint32_t *acnt_j,
                      uint32_t n_j, uint32_t n_hap)
{
    Args p{};
    p.alt_i = (const uint4 *)alt_i, p.alt_j = (const uint4 *)alt_j;
    p.acnt_i = acnt_i, p.acnt_j = acnt_j;
    p.n_i = n_i, p.n_j = n_j;
    p.nblocks = n_chunks(n_hap) / 2u;
    p.n_ind = n_hap / 2u;
    return p;
}

template <int kMode>
static int launch(const Args &p, hipStream_t s)
{
    const uint32_t grid = n_slabs(p.n_i) * n_slabs(p.n_j);
    em_kernel<kMode><<<grid, kThreads, 0, s>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

}  // namespace em
}  // namespace ldx

using namespace ldx;

// the rectangle forms' shape rules: rect_args_ok (ldx_common.h) with this kernel's I block; every form pairs haplotypes
static int args_ok(const char *who, uint32_t n_i, uint32_t n_j, uint32_t n_hap)
{
    return rect_args_ok(who, n_i, n_j, n_hap, "haplotypes 2k and 2k + 1 are the two alleles of individual k", kSlab);
}

extern "C" int ldx_ld_em_rect_dev(const void *alt_i, const uint32_t *acnt_i, uint32_t n_i, const void *alt_j,
                                  const uint32_t *acnt_j, uint32_t n_j, uint32_t n_hap, float *out_r, float *out_dprime,
                                  size_t ld_out, void *stream)
{
    const char *const who = "ldx_ld_em_rect_dev";
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, acnt_i);
    LDX_ARG_PTR(who, alt_j); LDX_ARG_PTR(who, acnt_j);
    LDX_ARG_REQUIRE(out_r != nullptr || out_dprime != nullptr, "%s: out_r and out_dprime are both null pointers", who);
    LDX_ARG_REQUIRE(ld_out >= n_j, "%s: ld_out %zu < n_j %u", who, ld_out, n_j);
    if (const int rc = args_ok(who, n_i, n_j, n_hap)) return rc;
    em::Args p = em::make_args(alt_i, acnt_i, n_i, alt_j, acnt_j, n_j, n_hap);
    p.out_r = out_r, p.out_d = out_dprime, p.ld = ld_out;
    return em::launch<em::kDense>(p, (hipStream_t)stream);
}

extern "C" int ldx_ld_em_rect_hits_dev(const void *alt_i, const uint32_t *acnt_i, uint32_t n_i, const void *alt_j,
                                       const uint32_t *acnt_j, uint32_t n_j, uint32_t n_hap, float r2_bound, ldx_hit *hits,
                                       uint64_t hit_cap, uint64_t *n_hits, void *stream)
{
    const char *const who = "ldx_ld_em_rect_hits_dev";
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, acnt_i);
    LDX_ARG_PTR(who, alt_j); LDX_ARG_PTR(who, acnt_j);
    if (const int rc = hit_args_ok(who, r2_bound, hits, hit_cap, n_hits)) return rc;
    if (const int rc = args_ok(who, n_i, n_j, n_hap)) return rc;
    em::Args p = em::make_args(alt_i, acnt_i, n_i, alt_j, acnt_j, n_j, n_hap);
    p.bound = r2_bound, p.hits = hits, p.hit_cap = hit_cap, p.n_hits = (unsigned long long *)n_hits;
    LDX_HIP(hipMemsetAsync(n_hits, 0, sizeof(uint64_t), (hipStream_t)stream));   // the slot counter starts at 0
    return em::launch<em::kHits>(p, (hipStream_t)stream);
}

extern "C" int ldx_ld_em_counts_dev(const void *alt_i, uint32_t n_i, const void *alt_j, uint32_t n_j, uint32_t n_hap,
                                    uint32_t *S, uint32_t *H, size_t ld, void *stream)
{
    const char *const who = "ldx_ld_em_counts_dev";
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, alt_j);
    LDX_ARG_PTR(who, S); LDX_ARG_PTR(who, H);
    LDX_ARG_REQUIRE(ld >= n_j, "%s: ld %zu < n_j %u", who, ld, n_j);
    if (const int rc = args_ok(who, n_i, n_j, n_hap)) return rc;
    em::Args p = em::make_args(alt_i, nullptr, n_i, alt_j, nullptr, n_j, n_hap);
    p.out_s = S, p.out_h = H, p.ld = ld;
    return em::launch<em::kCounts>(p, (hipStream_t)stream);
}

extern "C" int ldx_ld_em_from_counts_dev(uint32_t n_ind, size_t m, const uint32_t *a1, const uint32_t *a2, const uint32_t *S,
                                         const uint32_t *H, float *r, float *dprime, double *x, void *stream)
{
    const char *const who = "ldx_ld_em_from_counts_dev";
    LDX_ARG_PTR(who, a1); LDX_ARG_PTR(who, a2); LDX_ARG_PTR(who, S); LDX_ARG_PTR(who, H);
    LDX_ARG_REQUIRE(n_ind > 0u, "%s: n_ind is 0", who);
    LDX_ARG_REQUIRE(m > 0u, "%s: m is 0", who);
    if (n_ind > LDX_MAX_HAPS / 2u) {
        set_error("%s: n_ind %u > LDX_MAX_HAPS / 2 = %u", who, n_ind, LDX_MAX_HAPS / 2u);
        return LDX_E_UNSUPPORTED;
    }
    if ((m + 255u) / 256u >= (1ull << 31)) {
        set_error("%s: m = %zu needs 2^31 or more workgroups", who, m);
        return LDX_E_UNSUPPORTED;
    }
    if (r == nullptr && dprime == nullptr && x == nullptr) return LDX_OK;   // nothing asked for
    em::from_counts_kernel<<<(uint32_t)((m + 255u) / 256u), 256, 0, (hipStream_t)stream>>>(n_ind, m, a1, a2, S, H, r, dprime, x);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

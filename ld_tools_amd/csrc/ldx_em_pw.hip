// Pairwise-complete unphased LD by EM (include/ldx.h, "pairwise-complete EM"): the maximum-likelihood r and D' of every row of
// panel I against every row of panel J over the individuals CALLED AT BOTH SNPs -- what PLINK --r2 dprime / --ld and Haploview
// do with missing genotype calls -- as dense float32 cells (ldx_ld_em_rect_pw_dev), the pairs whose r *f32 r reaches a bound
// (ldx_ld_em_rect_pw_hits_dev), the pair's five integers alone (ldx_ld_em_pw_counts_dev) and the epilogue alone on a list of
// tuples with a per-tuple N (ldx_ld_em_from_counts_pw_dev).  One kernel of its own, em_pw_kernel, beside em_kernel (ldx_em.hip)
// and pwc_kernel (ldx_pwc.hip); the tile, the shortcut's K loop and the epilogue em_cell are em_kernel's (ldx_em_tile.h), the
// per-individual operands pwc_kernel's (ldx_fp4.h), walk and hit appender the shared ones.  The tile's body lives in
// ldx_em_pw_tile.h (tile_body), which emband_kernel (ldx_emband.hip, the band form) shares:
//   * tile: em_kernel's.  A workgroup (4 waves as 2 x 2, two workgroups per CU) owns one 128-row slab of I x one of J, a wave
//     64 x 64 cells.
//   * shortcut: a workgroup whose 128 rows and 128 columns hold no SNP with acnt + rcnt != n_hap (read from the tables,
//     workgroup-uniform) runs em_kernel's two-set K loop and epilogue with N = n_hap / 2, A = acnt_i, B = acnt_j: the tiles
//     without holes pay nothing for the feature, and their cells are em_kernel's because the integers and the function are.
//   * general loop: five sets, N A B S H, from three operands per side.  With q = ind_called(alt, ref) and w = alt masked by both
//     slots of q, every operand lives on the individuals' EVEN haplotype slots (registers 0 and 2 of an FP4 operand; 1 and 3
//     are zero on the I side, so the J side's are never read and only two registers per operand are kept):
//         I side (0.5 / 1):  G = expand32_a4_dosage(w)  g / 2      T = het_a4(het_bits(w))  0.5 where g = 1      Q = even_a4(q)  0.5 where called
//         J side (2 / 4):    U = expand32_b4_dosage(w)  2 g        V = het_b4(het_bits(w))  2 where g = 1        C = het_b4(q)   2 where called
//         S = G . U     H = T . V     A = G . C     B = Q . U     N = Q . C
//     Neither S nor H needs a joint mask: each side's operand is already zero where that side is not called.  Every product is
//     g_x g_y, g or 1 and every sum at most 4 N <= 20 480 < 2^24: the fp32 accumulators are exact in any order.
//     Five sets of a 64 x 64 wave tile would be 320 accumulator registers, so the wave covers its cells in 4 passes over K, each
//     holding the five sets of ONE 32 x 32 tile (80 registers) and followed by that tile's epilogue, as tile_body's general loop
//     does (ldx_pwc_tile.h).  A pass expands the J slab again: per cell the general loop costs what a 64 x 64 workgroup tile
//     with five MFMAs per K-step would.
//   * K loop of a pass: em_kernel's block structure -- per K-block of 256 haplotypes the workgroup expands the J slab's bits ONCE
//     into three LDS images [4 steps][2 halves][128 rows][8 B] (U, V, C: 24 KiB, em_kernel's buffer size), double-buffered, one
//     block_sync per K-block; a lane loads the 16 bytes of its own I row from each plane and expands them in registers.
//   * epilogue of a pass: em_cell has a data-dependent root search, so the accumulators do not stay in registers under it.  Five
//     integers are 69 bits: each wave stages its 32 x 32 cells as three words per cell (S << 13 | H, A << 14 | B, N), three
//     planes of 4 KiB, in the LDS the images no longer need after the pass's last barrier (4 x 12 KiB of the 64 KiB); 16 trips
//     with lane = column and half-wave = row parity: one em_cell per lane and trip, 128-byte row-major stores per half-wave.  A
//     barrier after the epilogue frees the LDS for the next pass's first image.
//   * walk: tile_of (ldx_fp4.h) in em_kernel's bands of 32 I blocks.  hits: HitAppender (ldx_common.h).
#include "ldx_em_pw_tile.h"

namespace ldx {
namespace em_pw {

enum Mode : int { kDense = 0, kHits = 1, kCounts = 2 };

struct Args {
    Side si, sj;
    uint32_t nblocks;                  // K-blocks of 256 haplotypes: n_chunks / 2
    uint32_t n_hap;
    float *out_r, *out_d;              // dense: [n_i][ld], either may be null
    uint32_t *counts;                  // counts: [5][n_i][ld], N A B S H
    size_t ld;
    float bound;                       // hits: kept iff r *f32 r >= bound
    ldx_hit *hits;
    uint64_t hit_cap;
    unsigned long long *n_hits;
};

// one cell from its five integers: the same for both paths.  Called by the whole wave (the hit appender ballots).
template <int kMode>
struct RectEmit {
    const Args &p;
    HitAppender hit;

    __device__ __forceinline__ void operator()(uint32_t i, uint32_t j, uint32_t N, uint32_t A, uint32_t B, uint32_t S, uint32_t H)
    {
        const bool inside = i < p.si.n && j < p.sj.n;
        if constexpr (kMode == kCounts) {
            if (inside) {
                const size_t plane = (size_t)p.si.n * p.ld;
                uint32_t *const at = p.counts + (size_t)i * p.ld + j;
                __builtin_nontemporal_store(N, at);
                __builtin_nontemporal_store(A, at + plane);
                __builtin_nontemporal_store(B, at + 2u * plane);
                __builtin_nontemporal_store(S, at + 3u * plane);
                __builtin_nontemporal_store(H, at + 4u * plane);
            }
        } else {
            em::Cell c{-0.0f, -0.0f, 0.0};
            if (inside) c = em::em_cell(N, A, B, S, H);
            if constexpr (kMode == kHits) {
                hit.append(inside && c.r * c.r >= p.bound, i, j, c.r, c.dprime);   // ONE float32 multiply; -0.0f gives 0 < bound
            } else if (inside) {
                if (p.out_r) __builtin_nontemporal_store(c.r, p.out_r + (size_t)i * p.ld + j);
                if (p.out_d) __builtin_nontemporal_store(c.dprime, p.out_d + (size_t)i * p.ld + j);
            }
        }
    }
};

// the tile -- the hole test, the shortcut, the general loop and its staged epilogue -- is tile_body's (ldx_em_pw_tile.h)
template <int kMode>
__global__ void __launch_bounds__(kThreads, 2) em_pw_kernel(Args p)
{
    __shared__ Smem sm;
    uint32_t ti, tj;
    tile_of<em::kBandTiles>(blockIdx.x, n_slabs(p.si.n), n_slabs(p.sj.n), ti, tj);
    RectEmit<kMode> emit{p, HitAppender{p.hits, p.hit_cap, p.n_hits, threadIdx.x & 63u}};
    tile_body<true>(sm, p.si, p.sj, p.nblocks, p.n_hap, ti, tj, threadIdx.x, emit);
    if constexpr (kMode == kHits) emit.hit.close();   // what is left of the wave's last batch
}

// the epilogue alone with a per-tuple N: one thread per tuple.  N beyond the library's LDX_MAX_HAPS / 2 is no table of its.
__global__ void __launch_bounds__(256) from_counts_pw_kernel(size_t m, const uint32_t *N, const uint32_t *a1, const uint32_t *a2,
                                                             const uint32_t *S, const uint32_t *H, float *r, float *dprime, double *x)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    const double nan = __builtin_nan("");
    const em::Cell c = N[k] <= LDX_MAX_HAPS / 2u ? em::em_cell(N[k], a1[k], a2[k], S[k], H[k]) : em::Cell{(float)nan, (float)nan, nan};
    if (r) r[k] = c.r;
    if (dprime) dprime[k] = c.dprime;
    if (x) x[k] = c.x;
}

template <int kMode>
static int launch(const Args &p, hipStream_t s)
{
    const uint32_t grid = n_slabs(p.si.n) * n_slabs(p.sj.n);
    em_pw_kernel<kMode><<<grid, kThreads, 0, s>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

}  // namespace em_pw
}  // namespace ldx

using namespace ldx;

// the three rectangle entries' pointers and shape rules: rect_args_ok (ldx_common.h) with this kernel's I block; every form
// pairs haplotypes into individuals; everything returns before any HIP call
#define LDX_EM_PW_SIDES(who)                                                                            \
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, ref_i); LDX_ARG_PTR(who, acnt_i); LDX_ARG_PTR(who, rcnt_i); \
    LDX_ARG_PTR(who, alt_j); LDX_ARG_PTR(who, ref_j); LDX_ARG_PTR(who, acnt_j); LDX_ARG_PTR(who, rcnt_j)

static int args_ok(const char *who, uint32_t n_i, uint32_t n_j, uint32_t n_hap)
{
    return rect_args_ok(who, n_i, n_j, n_hap, "haplotypes 2k and 2k + 1 are the two alleles of individual k", kSlab);
}

static em_pw::Args make_args(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                             const void *alt_j, const void *ref_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                             uint32_t n_hap)
{
    em_pw::Args p{};
    p.si = em_pw::Side{(const uint4 *)alt_i, (const uint4 *)ref_i, acnt_i, rcnt_i, n_i};
    p.sj = em_pw::Side{(const uint4 *)alt_j, (const uint4 *)ref_j, acnt_j, rcnt_j, n_j};
    p.nblocks = n_chunks(n_hap) / 2u;
    p.n_hap = n_hap;
    return p;
}

extern "C" int ldx_ld_em_rect_pw_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i,
                                     uint32_t n_i, const void *alt_j, const void *ref_j, const uint32_t *acnt_j,
                                     const uint32_t *rcnt_j, uint32_t n_j, uint32_t n_hap, float *out_r, float *out_dprime,
                                     size_t ld_out, void *stream)
{
    const char *const who = "ldx_ld_em_rect_pw_dev";
    LDX_EM_PW_SIDES(who);
    LDX_ARG_REQUIRE(out_r != nullptr || out_dprime != nullptr, "%s: out_r and out_dprime are both null pointers", who);
    LDX_ARG_REQUIRE(ld_out >= n_j, "%s: ld_out %zu < n_j %u", who, ld_out, n_j);
    if (const int rc = args_ok(who, n_i, n_j, n_hap)) return rc;
    em_pw::Args p = make_args(alt_i, ref_i, acnt_i, rcnt_i, n_i, alt_j, ref_j, acnt_j, rcnt_j, n_j, n_hap);
    p.out_r = out_r, p.out_d = out_dprime, p.ld = ld_out;
    return em_pw::launch<em_pw::kDense>(p, (hipStream_t)stream);
}

extern "C" int ldx_ld_em_rect_pw_hits_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i,
                                          uint32_t n_i, const void *alt_j, const void *ref_j, const uint32_t *acnt_j,
                                          const uint32_t *rcnt_j, uint32_t n_j, uint32_t n_hap, float r2_bound, ldx_hit *hits,
                                          uint64_t hit_cap, uint64_t *n_hits, void *stream)
{
    const char *const who = "ldx_ld_em_rect_pw_hits_dev";
    LDX_EM_PW_SIDES(who);
    if (const int rc = hit_args_ok(who, r2_bound, hits, hit_cap, n_hits)) return rc;
    if (const int rc = args_ok(who, n_i, n_j, n_hap)) return rc;
    em_pw::Args p = make_args(alt_i, ref_i, acnt_i, rcnt_i, n_i, alt_j, ref_j, acnt_j, rcnt_j, n_j, n_hap);
    p.bound = r2_bound, p.hits = hits, p.hit_cap = hit_cap, p.n_hits = (unsigned long long *)n_hits;
    LDX_HIP(hipMemsetAsync(n_hits, 0, sizeof(uint64_t), (hipStream_t)stream));   // the slot counter starts at 0
    return em_pw::launch<em_pw::kHits>(p, (hipStream_t)stream);
}

extern "C" int ldx_ld_em_pw_counts_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i,
                                       uint32_t n_i, const void *alt_j, const void *ref_j, const uint32_t *acnt_j,
                                       const uint32_t *rcnt_j, uint32_t n_j, uint32_t n_hap, uint32_t *counts, size_t ld,
                                       void *stream)
{
    const char *const who = "ldx_ld_em_pw_counts_dev";
    LDX_EM_PW_SIDES(who);
    LDX_ARG_PTR(who, counts);
    LDX_ARG_REQUIRE(ld >= n_j, "%s: ld %zu < n_j %u", who, ld, n_j);
    if (const int rc = args_ok(who, n_i, n_j, n_hap)) return rc;
    em_pw::Args p = make_args(alt_i, ref_i, acnt_i, rcnt_i, n_i, alt_j, ref_j, acnt_j, rcnt_j, n_j, n_hap);
    p.counts = counts, p.ld = ld;
    return em_pw::launch<em_pw::kCounts>(p, (hipStream_t)stream);
}

extern "C" int ldx_ld_em_from_counts_pw_dev(size_t m, const uint32_t *N, const uint32_t *a1, const uint32_t *a2, const uint32_t *S,
                                            const uint32_t *H, float *r, float *dprime, double *x, void *stream)
{
    const char *const who = "ldx_ld_em_from_counts_pw_dev";
    LDX_ARG_PTR(who, N); LDX_ARG_PTR(who, a1); LDX_ARG_PTR(who, a2); LDX_ARG_PTR(who, S); LDX_ARG_PTR(who, H);
    LDX_ARG_REQUIRE(m > 0u, "%s: m is 0", who);
    if ((m + 255u) / 256u >= (1ull << 31)) {
        set_error("%s: m = %zu needs 2^31 or more workgroups", who, m);
        return LDX_E_UNSUPPORTED;
    }
    if (r == nullptr && dprime == nullptr && x == nullptr) return LDX_OK;   // nothing asked for
    em_pw::from_counts_pw_kernel<<<(uint32_t)((m + 255u) / 256u), 256, 0, (hipStream_t)stream>>>(m, N, a1, a2, S, H, r, dprime, x);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

// Unphased LD by maximum likelihood between two SNP sets (include/ldx.h, "unphased LD by EM" and "pairwise-complete EM";
// DESIGN.md 3.7 and 3.10): for every row of panel I against every row of panel J over the same individuals, the
// maximum-likelihood two-locus haplotype frequency from the genotype table (Hill 1974), and from it r and D'.  Two forms of
// every entry, ONE kernel template (em_rect_kernel) for both:
//   * plain (a missing code counts as REF): dense float32 cells (ldx_ld_em_rect_dev), the pairs whose r *f32 r reaches a bound
//     (ldx_ld_em_rect_hits_dev), the two pair counts S and H alone (ldx_ld_em_counts_dev) and the epilogue alone on a list of
//     count tuples (ldx_ld_em_from_counts_dev).
//   * pairwise-complete (every pair over the individuals CALLED AT BOTH SNPs -- what PLINK --r2 dprime / --ld and Haploview do
//     with missing genotype calls): ldx_ld_em_rect_pw_dev, ldx_ld_em_rect_pw_hits_dev, the pair's five integers N A B S H
//     (ldx_ld_em_pw_counts_dev) and the epilogue with a per-tuple N (ldx_ld_em_from_counts_pw_dev).
// The tile is tile_body<kPairwise> (ldx_em_pw_tile.h, which emband_kernel of ldx_emband.hip shares): it hands the five
// integers of every cell to RectEmit, the one epilogue for dense cells, hits and counts.  The plain form is kPairwise = false:
// always the two-set K loop, N = n_hap / 2, A and B from acnt; ref and rcnt are never read, and the counts form, which has no
// acnt either, passes null tables.
//   * counting, two sets: with the allele counts a_i, a_j fixed, the EM needs TWO pair counts, not the nine cells of the 3 x 3
//     table: S = sum_k g_ik g_jk (the dosage rectangle's count: expand32_a4 x expand32_b4_dosage) and H = #{k : g_ik = g_jk = 1}.
//     The het bit of individual k, x = (w ^ (w >> 1)) & 0x5555..., sits on haplotype slot 2k only: expand32_a4(x) on the I
//     side (0.5 in registers 0 and 2, registers 1 and 3 are zero) and expand32_b4(x) on the J side (2 in registers 0 and 2),
//     so every product is exactly 1.  Both fp32 accumulator sets are exact: S <= 20 480, H <= 5 120.
//   * tile: a workgroup (4 waves as 2 x 2, two workgroups per CU) owns one 128-row slab of I x one 128-row slab of J; a wave
//     64 x 64 = 2 x 2 accumulator tiles of 32 x 32 in each of the two sets: 128 accumulator registers, the rectangle's number,
//     and the rectangle's ratio of four 16-byte-equivalent LDS fragment reads to eight MFMAs per K-step.
//   * two-set K loop (count_two_sets, ldx_em_tile.h): the rectangle's -- a K-block is 256 haplotypes; per K-block the workgroup
//     expands the J slab's bits ONCE into two LDS images, S's [4 steps][2 halves][128 rows][16 B] and H's [4][2][128][8 B] (its
//     two non-zero registers), double-buffered (2 x 24 KiB), one block_sync per K-block; a lane loads the 16 bytes of its own I
//     rows and expands them in registers.  Plain HIP: the compiler tracks every load.
//   * two-set epilogue: fp64 per cell with a data-dependent root search, so the accumulators do not stay in registers under it:
//     each wave packs (S, H) of its 64 x 64 cells into one word each, in the LDS the images no longer need (4 x 16 KiB), and a
//     rolled loop over the 64 rows has lane = column: one em_cell per lane and trip, 256-byte row-major stores per wave (128
//     per half-wave).  em_cell is a function of (N, a_i, a_j, S, H) alone, in an arithmetic symmetric in the two SNPs.
//   * pairwise shortcut: a workgroup whose 128 rows and 128 columns hold no SNP with acnt + rcnt != n_hap (read from the tables,
//     workgroup-uniform) runs the two-set K loop and epilogue with N = n_hap / 2, A = acnt_i, B = acnt_j: the tiles without
//     holes pay nothing for the feature, and their cells are the plain form's because the integers and the function are.
//   * pairwise general loop: five sets, N A B S H, from three operands per side.  With q = ind_called(alt, ref) and w = alt
//     masked by both slots of q, every operand lives on the individuals' EVEN haplotype slots (registers 0 and 2 of an FP4
//     operand; 1 and 3 are zero on the I side, so the J side's are never read and only two registers per operand are kept):
//         I side (0.5 / 1):  G = expand32_a4_dosage(w)  g / 2      T = het_a4(het_bits(w))  0.5 where g = 1      Q = even_a4(q)  0.5 where called
//         J side (2 / 4):    U = expand32_b4_dosage(w)  2 g        V = het_b4(het_bits(w))  2 where g = 1        C = het_b4(q)   2 where called
//         S = G . U     H = T . V     A = G . C     B = Q . U     N = Q . C
//     Neither S nor H needs a joint mask: each side's operand is already zero where that side is not called.  Every product is
//     g_x g_y, g or 1 and every sum at most 4 N <= 20 480 < 2^24: the fp32 accumulators are exact in any order.
//     Five sets of a 64 x 64 wave tile would be 320 accumulator registers, so the wave covers its cells in 4 passes over K, each
//     holding the five sets of ONE 32 x 32 tile (80 registers) and followed by that tile's epilogue, as tile_body's general loop
//     does (ldx_pwc_tile.h).  A pass expands the J slab again: per cell the general loop costs what a 64 x 64 workgroup tile
//     with five MFMAs per K-step would.
//   * K loop of a pass: the two-set loop's block structure -- per K-block of 256 haplotypes the workgroup expands the J slab's
//     bits ONCE into three LDS images [4 steps][2 halves][128 rows][8 B] (U, V, C: 24 KiB, the two-set buffer size),
//     double-buffered, one block_sync per K-block; a lane loads the 16 bytes of its own I row from each plane and expands them
//     in registers.
//   * epilogue of a pass: five integers are 69 bits: each wave stages its 32 x 32 cells as three words per cell (S << 13 | H,
//     A << 14 | B, N), three planes of 4 KiB, in the LDS the images no longer need after the pass's last barrier (4 x 12 KiB of
//     the 64 KiB); 16 trips with lane = column and half-wave = row parity: one em_cell per lane and trip, 128-byte row-major
//     stores per half-wave.  A barrier after the epilogue frees the LDS for the next pass's first image.
//   * walk: tile_of (ldx_fp4.h) with I blocks of 128 rows, 32 to a band (the rectangle's 4096-row bands).  hits: HitAppender
//     (ldx_common.h).
#include "ldx_em_pw_tile.h"

namespace ldx {
namespace em {

using em_pw::Side;

enum Mode : int { kDense = 0, kHits = 1, kCounts = 2 };

struct Args {
    Side si, sj;                       // plain form: ref and rcnt are null, and acnt too in the counts form
    uint32_t nblocks;                  // K-blocks of 256 haplotypes: n_chunks / 2
    uint32_t n_hap;
    float *out_r, *out_d;              // dense: [n_i][ld], either may be null
    uint32_t *counts[5];               // counts: N A B S H, [n_i][ld] each; the plain form writes S and H alone
    size_t ld;
    float bound;                       // hits: kept iff r *f32 r >= bound
    ldx_hit *hits;
    uint64_t hit_cap;
    unsigned long long *n_hits;
};

// one cell from its five integers: the same for both forms and both K loops.  Called by the whole wave (the hit appender
// ballots).
template <int kMode, bool kPairwise>
struct RectEmit {
    const Args &p;
    HitAppender hit;

    __device__ __forceinline__ void operator()(uint32_t i, uint32_t j, uint32_t N, uint32_t A, uint32_t B, uint32_t S, uint32_t H)
    {
        const bool inside = i < p.si.n && j < p.sj.n;
        if constexpr (kMode == kCounts) {
            if (inside) {
                if constexpr (kPairwise) {
                    __builtin_nontemporal_store(N, p.counts[0] + (size_t)i * p.ld + j);
                    __builtin_nontemporal_store(A, p.counts[1] + (size_t)i * p.ld + j);
                    __builtin_nontemporal_store(B, p.counts[2] + (size_t)i * p.ld + j);
                }
                __builtin_nontemporal_store(S, p.counts[3] + (size_t)i * p.ld + j);
                __builtin_nontemporal_store(H, p.counts[4] + (size_t)i * p.ld + j);
            }
        } else {
            Cell c{-0.0f, -0.0f, 0.0};
            if (inside) c = em_cell(N, A, B, S, H);
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
template <int kMode, bool kPairwise>
__global__ void __launch_bounds__(kThreads, 2) em_rect_kernel(Args p)
{
    __shared__ em_pw::Smem sm;
    uint32_t ti, tj;
    tile_of<kBandTiles>(blockIdx.x, n_slabs(p.si.n), n_slabs(p.sj.n), ti, tj);
    RectEmit<kMode, kPairwise> emit{p, HitAppender{p.hits, p.hit_cap, p.n_hits, threadIdx.x & 63u}};
    em_pw::tile_body<kPairwise>(sm, p.si, p.sj, p.nblocks, p.n_hap, ti, tj, threadIdx.x, emit);
    if constexpr (kMode == kHits) emit.hit.close();   // what is left of the wave's last batch
}

// the epilogue alone: one thread per tuple, with a per-tuple N where `N` is given and n_ind otherwise.  N beyond the library's
// LDX_MAX_HAPS / 2 is no table of its (the scalar form's entry refuses such an n_ind).
__global__ void __launch_bounds__(256) from_counts_kernel(size_t m, const uint32_t *N, uint32_t n_ind, const uint32_t *a1,
                                                          const uint32_t *a2, const uint32_t *S, const uint32_t *H, float *r,
                                                          float *dprime, double *x)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    const double nan = __builtin_nan("");
    const uint32_t n = N ? N[k] : n_ind;
    const Cell c = n <= LDX_MAX_HAPS / 2u ? em_cell(n, a1[k], a2[k], S[k], H[k]) : Cell{(float)nan, (float)nan, nan};
    if (r) r[k] = c.r;
    if (dprime) dprime[k] = c.dprime;
    if (x) x[k] = c.x;
}

static Args make_args(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                      const void *alt_j, const void *ref_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                      uint32_t n_hap)
{
    Args p{};
    p.si = Side{(const uint4 *)alt_i, (const uint4 *)ref_i, acnt_i, rcnt_i, n_i};
    p.sj = Side{(const uint4 *)alt_j, (const uint4 *)ref_j, acnt_j, rcnt_j, n_j};
    p.nblocks = n_chunks(n_hap) / 2u;
    p.n_hap = n_hap;
    return p;
}

template <int kMode>
static int launch(const Args &p, bool pairwise, hipStream_t s)
{
    const uint32_t grid = n_slabs(p.si.n) * n_slabs(p.sj.n);
    if (pairwise) em_rect_kernel<kMode, true><<<grid, kThreads, 0, s>>>(p);
    else em_rect_kernel<kMode, false><<<grid, kThreads, 0, s>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

static int from_counts(const char *who, size_t m, const uint32_t *N, uint32_t n_ind, const uint32_t *a1, const uint32_t *a2,
                       const uint32_t *S, const uint32_t *H, float *r, float *dprime, double *x, hipStream_t s)
{
    if ((m + 255u) / 256u >= (1ull << 31)) {
        set_error("%s: m = %zu needs 2^31 or more workgroups", who, m);
        return LDX_E_UNSUPPORTED;
    }
    if (r == nullptr && dprime == nullptr && x == nullptr) return LDX_OK;   // nothing asked for
    from_counts_kernel<<<(uint32_t)((m + 255u) / 256u), 256, 0, s>>>(m, N, n_ind, a1, a2, S, H, r, dprime, x);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

}  // namespace em
}  // namespace ldx

using namespace ldx;

// the pairwise rectangle entries' pointers; everything returns before any HIP call
#define LDX_EM_PW_SIDES(who)                                                                            \
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, ref_i); LDX_ARG_PTR(who, acnt_i); LDX_ARG_PTR(who, rcnt_i); \
    LDX_ARG_PTR(who, alt_j); LDX_ARG_PTR(who, ref_j); LDX_ARG_PTR(who, acnt_j); LDX_ARG_PTR(who, rcnt_j)

// the rectangle forms' shape rules: rect_args_ok (ldx_common.h) with this kernel's I block; every form pairs haplotypes
static int args_ok(const char *who, uint32_t n_i, uint32_t n_j, uint32_t n_hap)
{
    return rect_args_ok(who, n_i, n_j, n_hap, "haplotypes 2k and 2k + 1 are the two alleles of individual k", kSlab);
}

static int dense(em::Args p, bool pairwise, float *out_r, float *out_dprime, size_t ld_out, void *stream)
{
    p.out_r = out_r, p.out_d = out_dprime, p.ld = ld_out;
    return em::launch<em::kDense>(p, pairwise, (hipStream_t)stream);
}

static int hits_of(em::Args p, bool pairwise, float r2_bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, void *stream)
{
    p.bound = r2_bound, p.hits = hits, p.hit_cap = hit_cap, p.n_hits = (unsigned long long *)n_hits;
    LDX_HIP(hipMemsetAsync(n_hits, 0, sizeof(uint64_t), (hipStream_t)stream));   // the slot counter starts at 0
    return em::launch<em::kHits>(p, pairwise, (hipStream_t)stream);
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
    return dense(em::make_args(alt_i, nullptr, acnt_i, nullptr, n_i, alt_j, nullptr, acnt_j, nullptr, n_j, n_hap), false, out_r,
                 out_dprime, ld_out, stream);
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
    return dense(em::make_args(alt_i, ref_i, acnt_i, rcnt_i, n_i, alt_j, ref_j, acnt_j, rcnt_j, n_j, n_hap), true, out_r,
                 out_dprime, ld_out, stream);
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
    return hits_of(em::make_args(alt_i, nullptr, acnt_i, nullptr, n_i, alt_j, nullptr, acnt_j, nullptr, n_j, n_hap), false,
                   r2_bound, hits, hit_cap, n_hits, stream);
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
    return hits_of(em::make_args(alt_i, ref_i, acnt_i, rcnt_i, n_i, alt_j, ref_j, acnt_j, rcnt_j, n_j, n_hap), true, r2_bound,
                   hits, hit_cap, n_hits, stream);
}

extern "C" int ldx_ld_em_counts_dev(const void *alt_i, uint32_t n_i, const void *alt_j, uint32_t n_j, uint32_t n_hap,
                                    uint32_t *S, uint32_t *H, size_t ld, void *stream)
{
    const char *const who = "ldx_ld_em_counts_dev";
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, alt_j);
    LDX_ARG_PTR(who, S); LDX_ARG_PTR(who, H);
    LDX_ARG_REQUIRE(ld >= n_j, "%s: ld %zu < n_j %u", who, ld, n_j);
    if (const int rc = args_ok(who, n_i, n_j, n_hap)) return rc;
    em::Args p = em::make_args(alt_i, nullptr, nullptr, nullptr, n_i, alt_j, nullptr, nullptr, nullptr, n_j, n_hap);
    p.counts[3] = S, p.counts[4] = H, p.ld = ld;
    return em::launch<em::kCounts>(p, false, (hipStream_t)stream);
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
    em::Args p = em::make_args(alt_i, ref_i, acnt_i, rcnt_i, n_i, alt_j, ref_j, acnt_j, rcnt_j, n_j, n_hap);
    for (size_t k = 0; k < 5u; ++k) p.counts[k] = counts + k * n_i * ld;   // five planes of one array
    p.ld = ld;
    return em::launch<em::kCounts>(p, true, (hipStream_t)stream);
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
    return em::from_counts(who, m, nullptr, n_ind, a1, a2, S, H, r, dprime, x, (hipStream_t)stream);
}

extern "C" int ldx_ld_em_from_counts_pw_dev(size_t m, const uint32_t *N, const uint32_t *a1, const uint32_t *a2, const uint32_t *S,
                                            const uint32_t *H, float *r, float *dprime, double *x, void *stream)
{
    const char *const who = "ldx_ld_em_from_counts_pw_dev";
    LDX_ARG_PTR(who, N); LDX_ARG_PTR(who, a1); LDX_ARG_PTR(who, a2); LDX_ARG_PTR(who, S); LDX_ARG_PTR(who, H);
    LDX_ARG_REQUIRE(m > 0u, "%s: m is 0", who);
    return em::from_counts(who, m, N, 0u, a1, a2, S, H, r, dprime, x, (hipStream_t)stream);
}

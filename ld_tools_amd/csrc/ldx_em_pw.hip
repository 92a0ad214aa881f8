// Pairwise-complete unphased LD by EM (include/ldx.h, "pairwise-complete EM"): the maximum-likelihood r and D' of every row of
// panel I against every row of panel J over the individuals CALLED AT BOTH SNPs -- what PLINK --r2 dprime / --ld and Haploview
// do with missing genotype calls -- as dense float32 cells (ldx_ld_em_rect_pw_dev), the pairs whose r *f32 r reaches a bound
// (ldx_ld_em_rect_pw_hits_dev), the pair's five integers alone (ldx_ld_em_pw_counts_dev) and the epilogue alone on a list of
// tuples with a per-tuple N (ldx_ld_em_from_counts_pw_dev).  One kernel of its own, em_pw_kernel, beside em_kernel (ldx_em.hip)
// and pwc_kernel (ldx_pwc.hip); the tile, the shortcut's K loop and the epilogue em_cell are em_kernel's (ldx_em_tile.h), the
// per-individual operands pwc_kernel's (ldx_fp4.h), walk and hit appender the shared ones:
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
#include "ldx_em_tile.h"

namespace ldx {
namespace em_pw {

using em::v2i;
using em::kThreads;
using em::kWaveRows;
using em::kWaveCols;

constexpr uint32_t kOpBytes = 4u * 2u * kSlab * 8u;   // one J operand's image: [4 steps][2 halves][128 rows][8 B] = 8 KiB
constexpr uint32_t kImage = 3u * kOpBytes;            // one buffer of the general K loop: U, V, C
constexpr uint32_t kPlane = 32u * 32u;                // words of one plane of a wave's staged 32 x 32 tile
constexpr uint32_t kStage = em::kWaves * 3u * kPlane * 4u;   // the general epilogue's staged integers: 48 KiB
constexpr uint32_t kShiftA = 14;                      // staged word 1 = A << 14 | B  (A, B <= 10 240 < 2^14)
static_assert(kImage == em::kImage && 2u * kImage <= em::kLdsBytes && kStage <= em::kLdsBytes, "the general loop lives in em_kernel's LDS");

enum Mode : int { kDense = 0, kHits = 1, kCounts = 2 };

struct Side {
    const uint4 *alt, *ref;   // tiled bit planes (ldx_plane_bytes)
    const uint32_t *acnt;     // [n] ALT counts
    const uint32_t *rcnt;     // [n] REF counts
    uint32_t n;               // SNPs
};

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
__device__ __forceinline__ void emit(const Args &p, HitAppender &hit, uint32_t i, uint32_t j, uint32_t N, uint32_t A, uint32_t B,
                                     uint32_t S, uint32_t H)
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

__device__ __forceinline__ v16f mfma2(const v2i &a, const v2i &b, const v16f &c)
{
    const v8i a8 = {a.x, 0, a.y, 0, 0, 0, 0, 0};
    const v8i b8 = {b.x, 0, b.y, 0, 0, 0, 0, 0};
    // cbsz = blgp = 4: FP4 operands (4 registers each); scale operands 0 = the unscaled instruction
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 0, 0, 0);
}

template <int kMode>
__global__ void __launch_bounds__(kThreads, 2) em_pw_kernel(Args p)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[em::kLdsBytes];   // K loops: two image buffers; epilogues: staged counts
    __shared__ uint32_t cstat[kSlab];    // acnt of the slab's 128 columns
    __shared__ uint32_t rstat[kSlab];    // acnt of the workgroup's 128 rows
    __shared__ uint32_t wflag[em::kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wr = wave >> 1, wc = wave & 1u;   // the wave's 64 rows / 64 columns inside the 128 x 128 tile
    const uint32_t Ti = n_slabs(p.si.n), Tj = n_slabs(p.sj.n);
    uint32_t ti, tj;
    tile_of<em::kBandTiles>(blockIdx.x, Ti, Tj, ti, tj);
    const uint32_t nblocks = p.nblocks, nchunks = 2u * nblocks;

    // ---- which path: does a SNP of this tile hold a hole?  Thread t < 128 owns column t of the slab, thread 128 + t row t.
    {
        const bool is_col = tid < kSlab;
        const uint32_t *const acnt = is_col ? p.sj.acnt : p.si.acnt, *const rcnt = is_col ? p.sj.rcnt : p.si.rcnt;
        const uint32_t x = (is_col ? tj : ti) * kSlab + (tid & (kSlab - 1u));
        uint32_t a = 0;
        bool hole = false;
        if (x < (is_col ? p.sj.n : p.si.n)) {
            a = acnt[x];
            hole = a + rcnt[x] != p.n_hap;
        }
        (is_col ? cstat : rstat)[tid & (kSlab - 1u)] = a;
        const bool wave_hole = __any(hole);
        if (lane == 0) wflag[wave] = wave_hole ? 1u : 0u;
    }
    block_sync();
    const bool general = __builtin_amdgcn_readfirstlane(wflag[0] | wflag[1] | wflag[2] | wflag[3]) != 0u;
    [[maybe_unused]] HitAppender hit{p.hits, p.hit_cap, p.n_hits, lane};

    if (!general) {
        // ---- the shortcut: em_kernel's K loop and epilogue; N, A and B from the launch and the tables
        v16f acc_s[2][2], acc_h[2][2];
        em::count_two_sets(lds, p.si.alt, p.sj.alt, ti, tj, nblocks, tid, acc_s, acc_h);
        const uint32_t *const stage = em::stage_two_sets(lds, tid, acc_s, acc_h);
        const uint32_t j = tj * kSlab + wc * kWaveCols + lane;
        const uint32_t a_j = cstat[wc * kWaveCols + lane];
        const uint32_t row0 = ti * kSlab + wr * kWaveRows;
        const uint32_t rows = row0 < p.si.n ? (p.si.n - row0 < kWaveRows ? p.si.n - row0 : kWaveRows) : 0u;   // wave-uniform
        for (uint32_t rr = 0; rr < rows; ++rr) {
            const uint32_t packed = stage[rr * kWaveCols + lane];
            const uint32_t a_i = rstat[wr * kWaveRows + rr];   // one address per wave: broadcast
            emit<kMode>(p, hit, row0 + rr, j, p.n_hap / 2u, a_i, a_j, packed >> em::kPackShift, packed & ((1u << em::kPackShift) - 1u));
        }
    } else {
        // ---- the general loop.  Thread's share of the J images: row tid % 128, chunk 2 blk + tid / 128
        const uint32_t b_row = tid & (kSlab - 1u), b_half = tid >> 7;
        const uint32_t b_off = (tj * nchunks + b_half) * kSlab + b_row;
        const uint32_t b_dst = b_half * kSlab + b_row;   // + step * 256
        auto load = [&](const uint4 *plane, uint32_t off, uint32_t blk) { return plane[off + (size_t)blk * em::kBlockVecs]; };
        auto expand_b = [&](unsigned char *buf, const uint4 &alt, const uint4 &ref) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t wa = word_of(alt, q), wf = word_of(ref, q);
                const uint32_t qc = ind_called(wa, wf), w = wa & (qc | (qc << 1));
                const v4i u = expand32_b4_dosage(w);
                v2i *const dst = reinterpret_cast<v2i *>(buf) + b_dst + (uint32_t)q * em::kBlockVecs;
                dst[0] = v2i{u.x, u.z};                                  // U: the even slots' 2 g
                dst[kOpBytes / 8u] = em::het_b4(em::het_bits(w));       // V
                dst[2u * (kOpBytes / 8u)] = em::het_b4(qc);             // C
            }
        };
        uint32_t *const stage = reinterpret_cast<uint32_t *>(lds) + wave * (3u * kPlane);
        for (uint32_t ps = 0; ps < 4u; ++ps) {
            const uint32_t m0 = ps >> 1, t0 = ps & 1u;   // the pass's tile of the wave's 2 x 2
            // lane's A source: row 64 wr + 32 m0 + l32 of slab ti, chunk 2 blk + half; planes are < 4 GiB: 32-bit indices
            const uint32_t a_off = (ti * nchunks + half) * kSlab + wr * kWaveRows + 32u * m0 + l32;
            const uint32_t col = wc * kWaveCols + 32u * t0 + l32;   // lane's column of the slab
            v16f acc[5];   // N A B S H
#pragma unroll
            for (int s = 0; s < 5; ++s)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[s][e] = 0.0f;
            uint4 a_alt = load(p.si.alt, a_off, 0u), a_ref = load(p.si.ref, a_off, 0u);
            // (the first buffer is free: every wave left the last pass's epilogue through the barrier at its end)
            expand_b(lds, load(p.sj.alt, b_off, 0u), load(p.sj.ref, b_off, 0u));
            block_sync();
            for (uint32_t blk = 0; blk < nblocks; ++blk) {
                const uint32_t nb = blk + 1u < nblocks ? blk + 1u : blk;
                const uint4 b_alt = load(p.sj.alt, b_off, nb), b_ref = load(p.sj.ref, b_off, nb);
                const uint4 n_alt = load(p.si.alt, a_off, nb), n_ref = load(p.si.ref, a_off, nb);
                __builtin_amdgcn_sched_barrier(0);   // the global loads stay at the top of the block
                const v2i *const rd = reinterpret_cast<const v2i *>(lds + (blk & 1u) * kImage);
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const v2i *const at = rd + ((uint32_t)w * 2u + half) * kSlab + col;
                    const v2i bu = at[0], bv = at[kOpBytes / 8u], bc = at[2u * (kOpBytes / 8u)];
                    const uint32_t wa = word_of(a_alt, w), wf = word_of(a_ref, w);
                    const uint32_t qc = ind_called(wa, wf), ww = wa & (qc | (qc << 1));
                    const v4i g4 = expand32_a4_dosage(ww), q4 = even_a4(qc);
                    const v2i xg = {g4.x, g4.z}, xq = {q4.x, q4.z}, xt = em::het_a4(em::het_bits(ww));
                    acc[3] = mfma2(xg, bu, acc[3]);   // S
                    acc[4] = mfma2(xt, bv, acc[4]);   // H
                    acc[1] = mfma2(xg, bc, acc[1]);   // A
                    acc[2] = mfma2(xq, bu, acc[2]);   // B
                    acc[0] = mfma2(xq, bc, acc[0]);   // N
                }
                expand_b(lds + ((blk + 1u) & 1u) * kImage, b_alt, b_ref);
                block_sync();
                a_alt = n_alt;
                a_ref = n_ref;
            }
            // the pass's epilogue.  Every wave is past the last block's barrier, so nobody reads the images any more: the wave
            // stages its tile, three planes of [32 rows][32 columns] words.  Accumulator element e is row (e & 3) + 8 (e >> 2)
            // + 4 half, column l32.
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t at = ((uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * half) * 32u + l32;
                stage[at] = ((uint32_t)acc[3][e] << em::kPackShift) | (uint32_t)acc[4][e];
                stage[kPlane + at] = ((uint32_t)acc[1][e] << kShiftA) | (uint32_t)acc[2][e];
                stage[2u * kPlane + at] = (uint32_t)acc[0][e];
            }
            block_sync();   // the lanes of a wave read each other's words
            const uint32_t i0 = ti * kSlab + wr * kWaveRows + 32u * m0 + half, j = tj * kSlab + col;
            for (uint32_t rr = 0; rr < 16u; ++rr) {   // lane's row of the trip: 2 rr + half
                const uint32_t at = (2u * rr + half) * 32u + l32;
                const uint32_t sh = stage[at], ab = stage[kPlane + at], N = stage[2u * kPlane + at];
                emit<kMode>(p, hit, i0 + 2u * rr, j, N, ab >> kShiftA, ab & ((1u << kShiftA) - 1u), sh >> em::kPackShift,
                            sh & ((1u << em::kPackShift) - 1u));
            }
            block_sync();   // the next pass's first image overwrites what was staged
        }
    }
    if constexpr (kMode == kHits) hit.close();   // what is left of the wave's last batch
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

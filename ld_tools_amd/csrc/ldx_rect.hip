// Rectangular LD (include/ldx.h, "Rectangular LD"): the signed r of every row of panel I against every row of panel J over
// the same haplotypes -- dense float32 cells (ldx_ld_rect_dev) or the pairs whose float32 square reaches a bound
// (ldx_ld_rect_hits_dev), each also in the genotype-dosage form.  One kernel of its own, rect_kernel, beside the triangle's
// (ldx_mfma.hip), with which it shares the counting scheme and the cell arithmetic but no code object:
//   * counting: v_mfma_f32_32x32x64_f8f6f4 with FP4 operands (cbsz = blgp = 4, scale 0).  The A operand of a haplotype bit is
//     expand32_a4's nibble, the B operand expand32_b4's (dosage: expand32_b4_dosage's), every co-occurrence multiplies to
//     exactly 1 and the fp32 accumulators hold n11 (dosage: S = sum g_i g_j) exactly, < 2^24.  The expanders and
//     their exactness argument are the triangle's own: ldx_fp4.h.
//   * tile: a workgroup (4 waves, two workgroups per CU) owns 256 rows of I x one 128-row slab of J; a wave 64 x 128 = 2 x 4
//     accumulator tiles of 32 x 32 (128 registers).  J sits on the accumulator's COLUMN side (col = lane & 31), so a
//     half-wave holds 32 consecutive cells of one output row: 128-byte row-major stores.
//   * K loop: a K-block is 256 haplotypes (two 128-haplotype chunks, one per lane half).  Per K-block the workgroup
//     expands the J slab's bits ONCE into an LDS image [4 steps][2 halves][128 rows][16 B] (double-buffered, 2 x 16 KiB, one
//     block_sync per K-block); a lane loads the 16 bytes of its own I rows and expands them in registers.  The next
//     K-block's global loads are issued before the current block's 32 MFMAs.  Plain HIP: the compiler tracks every load.
//   * walk: workgroups are numbered so that consecutive ones share ONE J slab and differ in their I block, inside bands of
//     kBandTiles I blocks (4096 rows): tile_of (ldx_fp4.h), which em_kernel walks too; DESIGN.md, "Rectangular LD", has the
//     reasoning and the budget.
//   * hits: HitAppender (ldx_common.h), the slot protocol that ldx_area_finish_ex_dev consumes.
//   * epilogue: every cell is r32_cell(count, n, a_i, rs_i, a_j, rs_j) (ldx_common.h) with the per-SNP {a, rs} of r32_snp --
//     bit for bit the r32 triangle's cell for the same two SNPs.  The rectangle knows nothing about the identity of SNPs:
//     where row i of I and row j of J are the same variant the cell is still r32_cell, NOT r32_diag.
#include "ldx_fp4.h"

namespace ldx {
namespace rect {

typedef double d2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kWaves = 4, kThreads = kWaves * 64u;
constexpr uint32_t kWaveRows = 64;                    // I rows per wave: two 32-row accumulator tiles
constexpr uint32_t kTileRows = kWaves * kWaveRows;    // I rows per workgroup: 256 (two slabs)
constexpr uint32_t kBandTiles = 16;                   // I blocks per band of the walk
constexpr uint32_t kImageVecs = 4u * 2u * kSlab;      // 16-byte vectors of one J image: [4 steps][2 halves][128 rows]
constexpr uint32_t kBlockVecs = 2u * kSlab;           // 16-byte vectors of one K-block of a slab in the plane (two chunks)

// One side's per-SNP tables: the haplotype form reads acnt / rcnt, the dosage form gstat (ldx_dosage_stats_dev).
struct Side {
    const uint4 *alt;        // tiled bit plane (ldx_plane_bytes)
    const uint32_t *acnt;    // [n] ALT counts           (haplotype form)
    const uint32_t *rcnt;    // [n] REF counts           (haplotype form)
    const double *gstat;     // [n][2] {a, 1 / sqrt(v)}  (dosage form)
    uint32_t n;              // SNPs
};
struct Args {
    Side si, sj;
    uint32_t nblocks;        // K-blocks of 256 haplotypes: n_chunks / 2
    double n;                // observations per SNP: n_hap (dosage: n_hap / 2)
    float *out;              // dense: [n_i][ld_out]
    size_t ld_out;
    float bound;             // hits: kept iff r *f32 r >= bound
    ldx_hit *hits;
    uint64_t hit_cap;
    unsigned long long *n_hits;
};

// {a, rs} of SNP x as r32_snp makes them from the counts (a r and the counts themselves are exact in fp64); {0, 0} beyond the panel
template <bool kDosage>
__device__ __forceinline__ d2 snp_ars(const Side &s, uint32_t x)
{
    if (x >= s.n) return d2{0.0, 0.0};
    if constexpr (kDosage) {
        return d2{s.gstat[2u * (size_t)x], s.gstat[2u * (size_t)x + 1u]};
    } else {
        const double a = (double)s.acnt[x], r = (double)s.rcnt[x];
        const double ar = a * r;
        return d2{a, ar > 0.0 ? 1.0 / __builtin_sqrt(ar) : 0.0};
    }
}

template <bool kHits, bool kDosage>
__global__ void __launch_bounds__(kThreads, 2) rect_kernel(Args p)
{
    __shared__ uint4 image[2][kImageVecs];    // the J slab's expanded K-block, double-buffered: 2 x 16 KiB
    __shared__ d2 cstat[kSlab];               // {a, rs} of the slab's 128 columns
    __shared__ d2 rstat[kTileRows];           // {a, rs} of the workgroup's 256 rows
    const uint32_t tid = threadIdx.x, lane = tid & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t Ti = (p.si.n + kTileRows - 1u) / kTileRows, Tj = n_slabs(p.sj.n);
    uint32_t ti, tj;
    tile_of<kBandTiles>(blockIdx.x, Ti, Tj, ti, tj);
    const uint32_t nblocks = p.nblocks, nchunks = 2u * nblocks;

    if (tid < kSlab) cstat[tid] = snp_ars<kDosage>(p.sj, tj * kSlab + tid);
    rstat[tid] = snp_ars<kDosage>(p.si, ti * kTileRows + tid);

    // this wave's 64 rows lie in ONE slab of I (64 divides 128).  The last I block may reach past the padded plane (an odd
    // number of slabs): such a wave reads the last slab instead -- its rows are >= n_i, nothing of it is stored.
    const uint32_t row0 = ti * kTileRows + wave * kWaveRows;
    const uint32_t slabs_i = n_slabs(p.si.n);
    const uint32_t slab_i = row0 / kSlab < slabs_i ? row0 / kSlab : slabs_i - 1u;
    // lane's A source: row (row0 % 128) + l32 (+ 32 for the second tile), chunk 2 blk + half; planes are < 4 GiB: 32-bit indices
    const uint4 *const a_src = p.si.alt + ((slab_i * nchunks + half) * kSlab + (row0 & (kSlab - 1u)) + l32);
    // thread's share of the J image: row tid % 128, chunk 2 blk + tid / 128
    const uint32_t b_row = tid & (kSlab - 1u), b_half = tid >> 7;
    const uint4 *const b_src = p.sj.alt + ((tj * nchunks + b_half) * kSlab + b_row);
    const uint32_t b_dst = b_half * kSlab + b_row;   // + step * 256

    auto load_a = [&](uint4 (&dst)[2], uint32_t blk) {
        const uint4 *const s = a_src + (size_t)blk * kBlockVecs;
        dst[0] = s[0];
        dst[1] = s[32];
    };
    auto load_b = [&](uint32_t blk) { return b_src[(size_t)blk * kBlockVecs]; };
    auto expand_b = [&](uint4 *buf, const uint4 &bits) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t w = word_of(bits, q);
            const v4i e = kDosage ? expand32_b4_dosage(w) : expand32_b4(w);
            *reinterpret_cast<v4i *>(buf + b_dst + (uint32_t)q * kBlockVecs) = e;
        }
    };

    v16f acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][tt][e] = 0.0f;

    // One K-block per trip: the loads of the next block go out first, then the 4 x 8 MFMAs of this one out of `acur` and
    // image[blk & 1], then the next block's J bits become image[(blk + 1) & 1] -- last read in block blk - 1, which every wave
    // left through the barrier at its end -- and the barrier publishes it.  (Beyond the last block the loads repeat it:
    // discarded.)
    uint4 acur[2], anxt[2];
    load_a(acur, 0u);
    expand_b(image[0], load_b(0u));
    block_sync();   // (also publishes cstat / rstat)
    auto read_bf = [&](v4i (&bf)[4], const uint4 *rd, int w) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
            bf[tt] = *reinterpret_cast<const v4i *>(rd + ((uint32_t)w * 2u + half) * kSlab + 32u * tt + l32);
    };
    for (uint32_t blk = 0; blk < nblocks; ++blk) {
        const uint32_t nb = blk + 1u < nblocks ? blk + 1u : blk;
        const uint4 bits = load_b(nb);
        load_a(anxt, nb);
        const uint4 *const rd = image[blk & 1u];
        v4i bf[2][4], af[2][2];
        read_bf(bf[0], rd, 0);
#pragma unroll
        for (int m = 0; m < 2; ++m) af[0][m] = expand32_a4(acur[m].x);
        // the scheduling barriers keep the order as written: the global loads at the top of the block (left alone the compiler
        // sinks them to their first use, the end of the block, and the wave waits out their whole latency there), and step
        // w + 1's fragment reads and A expansion in front of step w's eight MFMAs
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < 3) {
                read_bf(bf[(w + 1) & 1], rd, w + 1);
#pragma unroll
                for (int m = 0; m < 2; ++m) af[(w + 1) & 1][m] = expand32_a4(word_of(acur[m], w + 1));
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const v4i a = af[w & 1][m], bb = bf[w & 1][tt];
                    const v8i a8 = {a.x, a.y, a.z, a.w, 0, 0, 0, 0};
                    const v8i b8 = {bb.x, bb.y, bb.z, bb.w, 0, 0, 0, 0};
                    // cbsz = blgp = 4: FP4 operands (4 registers each); scale operands 0 = the unscaled instruction
                    acc[m][tt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc[m][tt], 4, 4, 0, 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        expand_b(image[(blk + 1u) & 1u], bits);
        block_sync();
        acur[0] = anxt[0];
        acur[1] = anxt[1];
    }

    // ---- epilogue: accumulator (m, tt, e) is row 32 m + (e & 3) + 8 (e >> 2) + 4 half of the wave, column 32 tt + l32 of the slab
    const uint32_t j0 = tj * kSlab + l32;
    double ca[4], cs[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
        const d2 c = cstat[32u * tt + l32];
        ca[tt] = c.x;
        cs[tt] = c.y;
    }
    const double n = p.n;
    [[maybe_unused]] HitAppender hit{p.hits, p.hit_cap, p.n_hits, lane};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const uint32_t ri = wave * kWaveRows + 32u * m + (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * half;
            const d2 rw = rstat[ri];   // two addresses per wave: broadcast
            const uint32_t i = ti * kTileRows + ri;
            float c4[4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) c4[tt] = r32_cell((double)acc[m][tt][e], n, rw.x, rw.y, ca[tt], cs[tt]).r;
            if constexpr (kHits) {
                bool keep[4];
                float s4[4];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    s4[tt] = c4[tt] * c4[tt];   // ONE float32 multiply; -0.0f (degenerate) and +0.0f give 0 < bound
                    keep[tt] = i < p.si.n && j0 + 32u * tt < p.sj.n && s4[tt] >= p.bound;
                }
                if (!__any(keep[0] || keep[1] || keep[2] || keep[3])) continue;   // wave-uniform
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) hit.append(keep[tt], i, j0 + 32u * tt, c4[tt], s4[tt]);
            } else {
                if (i < p.si.n) {
                    float *const row = p.out + (size_t)i * p.ld_out;
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt)   // written once, never read back here: non-temporal, as the triangle's cells
                        if (j0 + 32u * tt < p.sj.n) __builtin_nontemporal_store(c4[tt], row + j0 + 32u * tt);
                }
            }
        }
    }
    if constexpr (kHits) hit.close();   // what is left of the wave's last batch
}

template <bool kHits, bool kDosage>
static int launch(const Args &p, hipStream_t s)
{
    const uint32_t grid = ((p.si.n + kTileRows - 1u) / kTileRows) * n_slabs(p.sj.n);
    rect_kernel<kHits, kDosage><<<grid, kThreads, 0, s>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

static Args make_args(const void *alt_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, const double *gstat_i, uint32_t n_i,
                      const void *alt_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, const double *gstat_j, uint32_t n_j,
                      uint32_t n_hap, bool dosage)
{
    Args p{};
    p.si = Side{(const uint4 *)alt_i, acnt_i, rcnt_i, gstat_i, n_i};
    p.sj = Side{(const uint4 *)alt_j, acnt_j, rcnt_j, gstat_j, n_j};
    p.nblocks = n_chunks(n_hap) / 2u;
    p.n = dosage ? (double)(n_hap / 2u) : (double)n_hap;
    return p;
}

static int dense(Args p, float *out, size_t ld_out, bool dosage, hipStream_t s)
{
    p.out = out;
    p.ld_out = ld_out;
    return dosage ? launch<false, true>(p, s) : launch<false, false>(p, s);
}

static int hits(Args p, float r2_bound, ldx_hit *hit_buf, uint64_t hit_cap, uint64_t *n_hits, bool dosage,
                hipStream_t s)
{
    p.bound = r2_bound;
    p.hits = hit_buf;
    p.hit_cap = hit_cap;
    p.n_hits = (unsigned long long *)n_hits;
    LDX_HIP(hipMemsetAsync(n_hits, 0, sizeof(uint64_t), s));   // the slot counter starts at 0
    return dosage ? launch<true, true>(p, s) : launch<true, false>(p, s);
}

}  // namespace rect
}  // namespace ldx

using namespace ldx;

// the four entries' shape rules: rect_args_ok (ldx_common.h) with this kernel's I block and the dosage form's parity rule
static int args_ok(const char *who, uint32_t n_i, uint32_t n_j, uint32_t n_hap, bool dosage)
{
    return rect_args_ok(who, n_i, n_j, n_hap, dosage ? "dosage pairs haplotypes 2k and 2k + 1 into individuals" : nullptr,
                        rect::kTileRows);
}

extern "C" int ldx_ld_rect_dev(const void *alt_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                               const void *alt_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j, uint32_t n_hap,
                               float *out, size_t ld_out, void *stream)
{
    const char *const who = "ldx_ld_rect_dev";
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, acnt_i); LDX_ARG_PTR(who, rcnt_i);
    LDX_ARG_PTR(who, alt_j); LDX_ARG_PTR(who, acnt_j); LDX_ARG_PTR(who, rcnt_j);
    LDX_ARG_PTR(who, out);
    LDX_ARG_REQUIRE(ld_out >= n_j, "%s: ld_out %zu < n_j %u", who, ld_out, n_j);
    if (const int rc = args_ok(who, n_i, n_j, n_hap, false)) return rc;
    return rect::dense(rect::make_args(alt_i, acnt_i, rcnt_i, nullptr, n_i, alt_j, acnt_j, rcnt_j, nullptr, n_j, n_hap, false),
                       out, ld_out, false, (hipStream_t)stream);
}

extern "C" int ldx_ld_rect_dosage_dev(const void *alt_i, const double *gstat_i, uint32_t n_i, const void *alt_j,
                                      const double *gstat_j, uint32_t n_j, uint32_t n_hap, float *out, size_t ld_out, void *stream)
{
    const char *const who = "ldx_ld_rect_dosage_dev";
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, gstat_i);
    LDX_ARG_PTR(who, alt_j); LDX_ARG_PTR(who, gstat_j);
    LDX_ARG_PTR(who, out);
    LDX_ARG_REQUIRE(ld_out >= n_j, "%s: ld_out %zu < n_j %u", who, ld_out, n_j);
    if (const int rc = args_ok(who, n_i, n_j, n_hap, true)) return rc;
    return rect::dense(rect::make_args(alt_i, nullptr, nullptr, gstat_i, n_i, alt_j, nullptr, nullptr, gstat_j, n_j, n_hap, true),
                       out, ld_out, true, (hipStream_t)stream);
}

extern "C" int ldx_ld_rect_hits_dev(const void *alt_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                                    const void *alt_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                                    uint32_t n_hap, float r2_bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits,
                                    void *stream)
{
    const char *const who = "ldx_ld_rect_hits_dev";
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, acnt_i); LDX_ARG_PTR(who, rcnt_i);
    LDX_ARG_PTR(who, alt_j); LDX_ARG_PTR(who, acnt_j); LDX_ARG_PTR(who, rcnt_j);
    if (const int rc = hit_args_ok(who, r2_bound, hits, hit_cap, n_hits)) return rc;
    if (const int rc = args_ok(who, n_i, n_j, n_hap, false)) return rc;
    return rect::hits(rect::make_args(alt_i, acnt_i, rcnt_i, nullptr, n_i, alt_j, acnt_j, rcnt_j, nullptr, n_j, n_hap, false),
                      r2_bound, hits, hit_cap, n_hits, false, (hipStream_t)stream);
}

extern "C" int ldx_ld_rect_hits_dosage_dev(const void *alt_i, const double *gstat_i, uint32_t n_i, const void *alt_j,
                                           const double *gstat_j, uint32_t n_j, uint32_t n_hap, float r2_bound, ldx_hit *hits,
                                           uint64_t hit_cap, uint64_t *n_hits, void *stream)
{
    const char *const who = "ldx_ld_rect_hits_dosage_dev";
    LDX_ARG_PTR(who, alt_i); LDX_ARG_PTR(who, gstat_i);
    LDX_ARG_PTR(who, alt_j); LDX_ARG_PTR(who, gstat_j);
    if (const int rc = hit_args_ok(who, r2_bound, hits, hit_cap, n_hits)) return rc;
    if (const int rc = args_ok(who, n_i, n_j, n_hap, true)) return rc;
    return rect::hits(rect::make_args(alt_i, nullptr, nullptr, gstat_i, n_i, alt_j, nullptr, nullptr, gstat_j, n_j, n_hap, true),
                      r2_bound, hits, hit_cap, n_hits, true, (hipStream_t)stream);
}

// Sample relatedness (include/ldx.h, "sample relatedness"): the co-occurrence counts N, HH, IBS0, HET between
// INDIVIDUALS over the kept SNPs, and the KING-robust kinship and IBS cells that are functions of them.  The kernels:
//   * planes_kernel: the transposed store.  From the panel's tiled ALT / REF planes (rows = SNPs, bits = haplotypes) it writes
//     three individual-major planes -- called c, heterozygous t, homozygous ALT z: rows = individuals, bits = SNPs -- in the
//     panel's own tiled layout with the two axes exchanged: slabs of 128 individuals, chunks of 128 SNPs (16 bytes), chunks in
//     pairs.  A wave owns 64 individuals x 128 SNPs: lane = SNP, one ballot per individual is a row of the 64 x 64 bit
//     transpose, and the lane whose number is the individual's keeps it, so that the wave stores 64 x 16 contiguous bytes per
//     plane.  It also counts the per-individual tables (called, het, hom-ALT over the kept SNPs) and the kept SNPs.
//   * counts_kernel: workgroup = (lower tile ti >= tj of 128 x 128 individuals, K slice).  v_mfma_f32_32x32x64_f8f6f4 on the
//     one-bit-per-nibble FP4 operands of ldx_fp4.h: every product is 1, every fp32 accumulator an exact count below 2^24 (the
//     slice bound).  General path, 6 MFMAs per 32 x 32 tile and 64 SNPs into 5 accumulators:
//         N = c.c   HH = t.t   IBS0 = n.z + z.n   HET[a][b] = t.c   HET[b][a] = c.t        (n = c & ~t & ~z: homozygous REF)
//     Shortcut (no individual of the tile misses a kept call: read from the tables, workgroup-uniform), 3 MFMAs: HH and IBS0;
//     N and HET come from the tables, added by the tile's first slice.  Operands come straight from global memory (a lane's
//     16 bytes are 128 SNPs of its row), no LDS in the K loop and no barrier.  At the end of the slice the accumulators become
//     uint32 once and are added to the output with 32-bit integer atomics: order-independent, so the counts are reproducible
//     bit for bit.  The mirrored orientation goes through a 32 x 32 LDS transpose so that both orientations add 128
//     contiguous bytes per half-wave.
//   * cells_kernel / tuples_kernel: king_cell and ibs_cell, one function each, dense or on a list of tuples.
#include "ldx_fp4.h"
#include "ldx_sample_store.h"   // pad_ind, snp_chunks, plane_vecs

namespace ldx {
namespace king {

constexpr uint32_t kTile = kSlab;             // individuals per tile side == rows per slab of the store
constexpr uint32_t kBlockSnps = 256;          // SNPs per K-block: two chunks, one per lane half
constexpr uint32_t kBlockVecs = 2u * kSlab;   // 16-byte vectors of one K-block of a slab
constexpr uint32_t kMA = 1, kMB = 2;          // 32 x 32 accumulator tiles of a wave: rows x columns
constexpr uint32_t kWavesR = kTile / (32u * kMA), kWavesC = kTile / (32u * kMB);
constexpr uint32_t kWaves = kWavesR * kWavesC, kThreads = kWaves * 64u;   // 8 waves: two per SIMD
constexpr uint32_t kSets = 5;                 // N HH IBS0 HETa HETb
constexpr uint32_t kMinSliceBlocks = LDX_KING_MIN_SLICE_SNPS / kBlockSnps;
constexpr uint32_t kMaxSliceBlocks = LDX_KING_MAX_SLICE_SNPS / kBlockSnps;
// every product is 1 (0.5 x 2 or 1 x 1) and of n.z and z.n at most one is set per SNP: an accumulator is at most the slice's SNPs
static_assert(1ull * LDX_KING_MAX_SLICE_SNPS < (1ull << 24), "a slice's counts must stay exact in fp32");
static_assert(LDX_KING_MIN_SLICE_SNPS % kBlockSnps == 0 && LDX_KING_MAX_SLICE_SNPS % kBlockSnps == 0, "slices are whole K-blocks");

// ---- the cells: functions of the pair's integers alone ----------------------------------------------------------------------
__device__ __forceinline__ float king_cell(uint32_t, uint32_t HH, uint32_t IBS0, uint32_t HETa, uint32_t HETb)
{
    const uint32_t m = HETa < HETb ? HETa : HETb;
    if (m == 0u) return -0.0f;
    const uint64_t ibs1 = (uint64_t)HETa + (uint64_t)HETb - 2ull * HH;
    return (float)(0.5 - (double)(4ull * IBS0 + ibs1) / (double)(4ull * m));
}
__device__ __forceinline__ float ibs_cell(uint32_t N, uint32_t HH, uint32_t IBS0, uint32_t HETa, uint32_t HETb)
{
    if (N == 0u) return -0.0f;
    const uint64_t ibs1 = (uint64_t)HETa + (uint64_t)HETb - 2ull * HH;
    const uint64_t ibs2 = (uint64_t)N - ibs1 - (uint64_t)IBS0;
    return (float)((double)(2ull * ibs2 + ibs1) / (double)(2ull * N));
}

// ---- the transposed store -----------------------------------------------------------------------------------------------------
constexpr uint32_t kPlaneWaves = 4, kPlaneThreads = kPlaneWaves * 64u;
constexpr uint32_t kChunksPerWave = 8;   // SNP chunks a wave walks, its table counts in registers: one atomic round per wave

struct PlaneArgs {
    const uint4 *alt, *ref;   // the panel's tiled planes
    const uint8_t *keep;      // [n_snps] of the panel, or null
    uint32_t hap_chunks;      // chunks of a panel row
    uint32_t snp_begin, snp_count;
    uint32_t n_ind, n_pad;
    uint32_t chunks;          // SNP chunks of the store
    uint4 *store;             // three planes
    size_t plane;             // vectors of one plane
    uint32_t *tables;
};

// bit 2 k of the four words x (an individual's bit on its even haplotype slot) of every lane, k = 0 .. 63: the lane whose number
// is k keeps the ballot -- the 64 SNPs of the wave as bits of individual k
__device__ __forceinline__ uint64_t transpose64(const uint32_t (&x)[4], uint32_t lane)
{
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
#pragma unroll 4   // (all 64 ballots unrolled kept every result in scalar registers at once: they spilled)
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint64_t b = __ballot((x[w] >> (2u * j)) & 1u);
            mine = lane == 16u * w + j ? b : mine;
        }
    }
    return mine;
}

__global__ void __launch_bounds__(kPlaneThreads) planes_kernel(PlaneArgs p)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t g = blockIdx.x;                       // 64 individuals: haplotype chunk g of the panel
    const uint32_t ind = g * 64u + lane;                 // this lane's individual, < n_pad
    const uint32_t c0 = (blockIdx.y * kPlaneWaves + wave) * kChunksPerWave;
    uint32_t cnt[3] = {0u, 0u, 0u}, kept_snps = 0u;
    for (uint32_t c = c0; c < c0 + kChunksPerWave && c < p.chunks; ++c) {
        uint64_t bits[3][2];
#pragma unroll
        for (uint32_t h = 0; h < 2u; ++h) {
            const uint32_t k = c * 128u + h * 64u + lane;   // SNP of the store
            const uint32_t s = p.snp_begin + (k < p.snp_count ? k : 0u);
            const bool kept = k < p.snp_count && (p.keep == nullptr || p.keep[s] != 0);
            uint4 va = {0u, 0u, 0u, 0u}, vr = {0u, 0u, 0u, 0u};
            if (kept) {
                const size_t at = ((size_t)(s / kSlab) * p.hap_chunks + g) * kSlab + (s & (kSlab - 1u));
                va = p.alt[at], vr = p.ref[at];
            }
            uint32_t q[4], t[4], z[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t wa = word_of(va, w), wr = word_of(vr, w);
                q[w] = ind_called(wa, wr);
                const uint32_t a = wa & (q[w] | (q[w] << 1));   // a half-missing genotype is missing
                z[w] = a & (a >> 1) & 0x55555555u;
                t[w] = (a ^ (a >> 1)) & q[w];
            }
            bits[0][h] = transpose64(q, lane), bits[1][h] = transpose64(t, lane), bits[2][h] = transpose64(z, lane);
            if (g == 0u) kept_snps += (uint32_t)__builtin_popcountll(__ballot(kept));
        }
        const size_t at = ((size_t)(ind / kSlab) * p.chunks + c) * kSlab + (ind & (kSlab - 1u));
#pragma unroll
        for (uint32_t s = 0; s < 3u; ++s) {
            p.store[s * p.plane + at] = uint4{(uint32_t)bits[s][0], (uint32_t)(bits[s][0] >> 32), (uint32_t)bits[s][1],
                                              (uint32_t)(bits[s][1] >> 32)};
            cnt[s] += (uint32_t)(__builtin_popcountll(bits[s][0]) + __builtin_popcountll(bits[s][1]));
        }
    }
    if (ind < p.n_ind) {
#pragma unroll
        for (uint32_t s = 0; s < 3u; ++s)
            if (cnt[s]) atomicAdd(p.tables + s * p.n_pad + ind, cnt[s]);
    }
    if (g == 0u && lane == 0u && kept_snps) atomicAdd(p.tables + 3u * p.n_pad, kept_snps);
}

// ---- the counts ---------------------------------------------------------------------------------------------------------------
struct CountArgs {
    const uint4 *store;
    size_t plane;             // vectors of one plane of the store
    const uint32_t *tables;
    uint32_t *counts;         // [4][n_ind][ld]
    size_t ld;
    uint32_t n_ind, n_pad;
    uint32_t chunks;          // SNP chunks of a row of the store
    uint32_t nblocks, slice_blocks, n_tiles;
};

struct Smem {
    uint32_t t[kWaves][32][33];   // a wave's 32 x 32 transpose
};

__device__ __forceinline__ v16f mfma4(const v4i &a, const v4i &b, const v16f &c)
{
    const v8i a8 = {a.x, a.y, a.z, a.w, 0, 0, 0, 0};
    const v8i b8 = {b.x, b.y, b.z, b.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 0, 0, 0);   // FP4 both sides, unscaled
}

template <bool kGeneral>
__device__ __forceinline__ void k_loop(const CountArgs &p, size_t a_off, const size_t (&b_off)[kMB], uint32_t blk0, uint32_t blk1,
                                       v16f (&acc)[kMA][kMB][kSets])
{
    const uint4 *const pc = p.store, *const pt = p.store + p.plane, *const pz = p.store + 2u * p.plane;
    uint4 ac[kMA], at[kMA], az[kMA], bc[kMB], bt[kMB], bz[kMB];
    auto load = [&](uint32_t blk) {
        const size_t o = (size_t)blk * kBlockVecs;
#pragma unroll
        for (uint32_t m = 0; m < kMA; ++m) ac[m] = pc[a_off + 32u * m + o], at[m] = pt[a_off + 32u * m + o], az[m] = pz[a_off + 32u * m + o];
#pragma unroll
        for (uint32_t t = 0; t < kMB; ++t) bc[t] = pc[b_off[t] + o], bt[t] = pt[b_off[t] + o], bz[t] = pz[b_off[t] + o];
    };
    for (uint32_t blk = blk0; blk < blk1; ++blk) {
        load(blk);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            v4i xc[kMA], xt[kMA], xn[kMA], xz[kMA];
#pragma unroll
            for (uint32_t m = 0; m < kMA; ++m) {
                const uint32_t c = word_of(ac[m], w), t = word_of(at[m], w), z = word_of(az[m], w);
                xt[m] = expand32_a4(t), xz[m] = expand32_a4(z), xn[m] = expand32_a4(c & ~(t | z));
                if constexpr (kGeneral) xc[m] = expand32_a4(c);
            }
#pragma unroll
            for (uint32_t tt = 0; tt < kMB; ++tt) {
                const uint32_t c = word_of(bc[tt], w), t = word_of(bt[tt], w), z = word_of(bz[tt], w);
                const v4i yt = expand32_b4(t), yz = expand32_b4(z), yn = expand32_b4(c & ~(t | z));
#pragma unroll
                for (uint32_t m = 0; m < kMA; ++m) {
                    acc[m][tt][1] = mfma4(xt[m], yt, acc[m][tt][1]);   // HH
                    acc[m][tt][2] = mfma4(xn[m], yz, acc[m][tt][2]);   // IBS0: (0, 2)
                    acc[m][tt][2] = mfma4(xz[m], yn, acc[m][tt][2]);   //       (2, 0)
                }
                if constexpr (kGeneral) {
                    const v4i yc = expand32_b4(c);
#pragma unroll
                    for (uint32_t m = 0; m < kMA; ++m) {
                        acc[m][tt][0] = mfma4(xc[m], yc, acc[m][tt][0]);   // N
                        acc[m][tt][3] = mfma4(xt[m], yc, acc[m][tt][3]);   // HET[a][b]
                        acc[m][tt][4] = mfma4(xc[m], yt, acc[m][tt][4]);   // HET[b][a]
                    }
                }
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads, 2) counts_kernel(CountArgs p)
{
    __shared__ Smem sm;
    const uint32_t lane = threadIdx.x & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wr = wave / kWavesC, wc = wave - wr * kWavesC;
    const uint32_t slice = blockIdx.x / p.n_tiles, lt = blockIdx.x - slice * p.n_tiles;
    // lower tile lt -> (ti, tj), ti >= tj: lt = ti (ti + 1) / 2 + tj
    uint32_t ti = (uint32_t)((__builtin_sqrt(8.0 * (double)lt + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1u) / 2u > lt) --ti;
    while ((ti + 1u) * (ti + 2u) / 2u <= lt) ++ti;
    const uint32_t tj = lt - ti * (ti + 1u) / 2u;
    const uint32_t blk0 = slice * p.slice_blocks;
    const uint32_t blk1 = blk0 + p.slice_blocks < p.nblocks ? blk0 + p.slice_blocks : p.nblocks;

    // which path: does an individual of this tile miss a kept call?  every wave reads all 256 entries: wave-uniform, and the same in
    // every wave and every slice of the tile
    const uint32_t *const t_called = p.tables, *const t_het = p.tables + p.n_pad;
    const uint32_t n_kept = p.tables[3u * p.n_pad];
    bool hole = false;
#pragma unroll
    for (uint32_t k = 0; k < 2u; ++k) {
        const uint32_t xi = ti * kTile + 64u * k + lane, xj = tj * kTile + 64u * k + lane;
        hole = hole || (xi < p.n_ind && t_called[xi] != n_kept) || (xj < p.n_ind && t_called[xj] != n_kept);
    }
    const bool general = __any(hole) != 0;

    // lane's operand rows: row r of a slab, chunk 2 blk + half
    const size_t a_off = ((size_t)ti * p.chunks + half) * kSlab + 32u * kMA * wr + l32;
    size_t b_off[kMB];
#pragma unroll
    for (uint32_t t = 0; t < kMB; ++t) b_off[t] = ((size_t)tj * p.chunks + half) * kSlab + 32u * (kMB * wc + t) + l32;

    v16f acc[kMA][kMB][kSets];
#pragma unroll
    for (uint32_t m = 0; m < kMA; ++m)
#pragma unroll
        for (uint32_t t = 0; t < kMB; ++t)
#pragma unroll
            for (uint32_t s = 0; s < kSets; ++s)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[m][t][s][e] = 0.0f;
    if (general) k_loop<true>(p, a_off, b_off, blk0, blk1, acc);
    else k_loop<false>(p, a_off, b_off, blk0, blk1, acc);

    // ---- the slice's counts into the output.  Accumulator element e of a tile is row (e & 3) + 8 (e >> 2) + 4 half, column l32.
    const bool tables_too = general || slice == 0u;   // N and HET of a shortcut tile: added once, by its first slice
    const bool mirror = ti != tj;                     // a diagonal tile holds both orientations itself
    const size_t plane = (size_t)p.n_ind * p.ld;
    auto tile_row = [&](int e) { return (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * half; };
#pragma unroll
    for (uint32_t m = 0; m < kMA; ++m) {
#pragma unroll
        for (uint32_t t = 0; t < kMB; ++t) {
            const uint32_t i0 = ti * kTile + 32u * (kMA * wr + m), j0 = tj * kTile + 32u * (kMB * wc + t);
            // set s of element e: the accumulator, or -- N and HET of a shortcut tile, whose every individual is called at every kept
            // SNP -- the tables' entry
            auto value = [&](uint32_t s, int e) -> uint32_t {
                if (s == 1u || s == 2u || general) return (uint32_t)acc[m][t][s][e];
                if (s == 0u) return n_kept;
                const uint32_t x = s == 3u ? i0 + tile_row(e) : j0 + l32;
                return x < p.n_ind ? t_het[x] : 0u;
            };
            // as computed: cell (i0 + tile_row(e), j0 + l32); a half-wave adds 128 contiguous bytes
#pragma unroll
            for (uint32_t s = 0; s < 4u; ++s) {
                if (s != 1u && s != 2u && !tables_too) continue;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint32_t i = i0 + tile_row(e), j = j0 + l32;
                    if (i < p.n_ind && j < p.n_ind) atomicAdd(p.counts + s * plane + (size_t)i * p.ld + j, value(s, e));
                }
            }
            if (!mirror) continue;
            // mirrored: cell (j0 + tile_row(e), i0 + l32) receives what (i0 + l32, j0 + tile_row(e)) holds; its HET is the partner's
#pragma unroll
            for (uint32_t s = 0; s < 4u; ++s) {
                if (s != 1u && s != 2u && !tables_too) continue;   // workgroup-uniform
                const uint32_t src = s == 3u ? 4u : s;
#pragma unroll
                for (int e = 0; e < 16; ++e) sm.t[wave][l32][tile_row(e)] = value(src, e);
                block_sync();
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint32_t j = j0 + tile_row(e), i = i0 + l32;
                    const uint32_t x = sm.t[wave][tile_row(e)][l32];
                    if (i < p.n_ind && j < p.n_ind) atomicAdd(p.counts + s * plane + (size_t)j * p.ld + i, x);
                }
                block_sync();
            }
        }
    }
}

// ---- the cells ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tuples_kernel(size_t m, const uint32_t *N, const uint32_t *HH, const uint32_t *IBS0,
                                                     const uint32_t *HETa, const uint32_t *HETb, float *kin, float *ibs)
{
    for (size_t k = (size_t)blockIdx.x * 256u + threadIdx.x; k < m; k += (size_t)gridDim.x * 256u) {
        if (kin) kin[k] = king_cell(N[k], HH[k], IBS0[k], HETa[k], HETb[k]);
        if (ibs) ibs[k] = ibs_cell(N[k], HH[k], IBS0[k], HETa[k], HETb[k]);
    }
}

__global__ void __launch_bounds__(256) cells_kernel(const uint32_t *counts, uint32_t n_ind, size_t ld, float *kin, float *ibs,
                                                    size_t ld_out)
{
    const size_t plane = (size_t)n_ind * ld, total = (size_t)n_ind * n_ind;
    for (size_t k = (size_t)blockIdx.x * 256u + threadIdx.x; k < total; k += (size_t)gridDim.x * 256u) {
        const uint32_t a = (uint32_t)(k / n_ind), b = (uint32_t)(k - (size_t)a * n_ind);
        const size_t ab = (size_t)a * ld + b, ba = (size_t)b * ld + a;
        const uint32_t N = counts[ab], HH = counts[plane + ab], IBS0 = counts[2u * plane + ab];
        const uint32_t HETa = counts[3u * plane + ab], HETb = counts[3u * plane + ba];
        if (kin) kin[(size_t)a * ld_out + b] = king_cell(N, HH, IBS0, HETa, HETb);
        if (ibs) ibs[(size_t)a * ld_out + b] = ibs_cell(N, HH, IBS0, HETa, HETb);
    }
}

static uint32_t grid_for(size_t items)
{
    const size_t want = (items + 255u) / 256u, cap = (size_t)device_cus() * 8u;
    return (uint32_t)(want < cap ? (want ? want : 1u) : cap);
}

}  // namespace king
}  // namespace ldx

using namespace ldx;

// the shape rules every entry of the store shares; everything returns before any HIP call
static int sample_shape_ok(const char *who, uint32_t n_ind, uint32_t n_snps)
{
    LDX_ARG_REQUIRE(n_ind != 0u && n_snps != 0u, "%s: n_ind and the SNP count must be non-zero", who);
    if (n_ind > LDX_MAX_HAPS / 2u) {
        set_error("%s: %u individuals, more than LDX_MAX_HAPS / 2 = %u", who, n_ind, LDX_MAX_HAPS / 2u);
        return LDX_E_UNSUPPORTED;
    }
    LDX_ARG_REQUIRE(n_snps <= LDX_KING_MAX_STORE_SNPS, "%s: %u SNPs in one store, more than %u: split the SNPs over several calls",
                    who, n_snps, LDX_KING_MAX_STORE_SNPS);
    return LDX_OK;
}

extern "C" size_t ldx_sample_planes_bytes(uint32_t n_ind, uint32_t n_snps)
{
    return 3u * king::plane_vecs(n_ind, n_snps) * sizeof(uint4);
}

extern "C" size_t ldx_sample_tables_bytes(uint32_t n_ind) { return ((size_t)3u * king::pad_ind(n_ind) + 4u) * sizeof(uint32_t); }

extern "C" int ldx_sample_planes_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                                     uint32_t snp_begin, uint32_t snp_count, void *store, uint32_t *tables, void *stream)
{
    const char *const who = "ldx_sample_planes_dev";
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, ref); LDX_ARG_PTR(who, store); LDX_ARG_PTR(who, tables);
    LDX_ARG_REQUIRE(n_hap != 0u && n_hap % 2u == 0u, "%s: n_hap %u must be even and non-zero (haplotypes 2a and 2a + 1 are individual a)",
                    who, n_hap);
    if (n_hap > LDX_MAX_HAPS) {
        set_error("%s: n_hap %u > LDX_MAX_HAPS", who, n_hap);
        return LDX_E_UNSUPPORTED;
    }
    if (const int rc = sample_shape_ok(who, n_hap / 2u, snp_count)) return rc;
    LDX_ARG_REQUIRE(snp_begin < n_snps && snp_count <= n_snps - snp_begin, "%s: SNPs %u .. %llu outside the panel's %u", who,
                    snp_begin, (unsigned long long)snp_begin + snp_count, n_snps);
    if (const int rc = plane_check(who, nullptr, n_snps, n_hap)) return rc;
    const uint32_t n_ind = n_hap / 2u;
    king::PlaneArgs p{};
    p.alt = (const uint4 *)alt, p.ref = (const uint4 *)ref, p.keep = keep;
    p.hap_chunks = n_chunks(n_hap);
    p.snp_begin = snp_begin, p.snp_count = snp_count;
    p.n_ind = n_ind, p.n_pad = king::pad_ind(n_ind);
    p.chunks = king::snp_chunks(snp_count);
    p.store = (uint4 *)store, p.plane = king::plane_vecs(n_ind, snp_count);
    p.tables = tables;
    hipStream_t s = (hipStream_t)stream;
    LDX_HIP(hipMemsetAsync(tables, 0, ldx_sample_tables_bytes(n_ind), s));
    const uint32_t per_block = king::kPlaneWaves * king::kChunksPerWave;
    const dim3 grid(p.n_pad / 64u, (p.chunks + per_block - 1u) / per_block);
    king::planes_kernel<<<grid, king::kPlaneThreads, 0, s>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_sample_counts_dev(const void *store, const uint32_t *tables, uint32_t n_ind, uint32_t n_snps, uint32_t *counts,
                                     size_t ld, int accumulate, uint64_t n_prior, uint32_t n_slices, void *stream)
{
    const char *const who = "ldx_sample_counts_dev";
    LDX_ARG_PTR(who, store); LDX_ARG_PTR(who, tables); LDX_ARG_PTR(who, counts);
    if (const int rc = sample_shape_ok(who, n_ind, n_snps)) return rc;
    LDX_ARG_REQUIRE(ld >= n_ind, "%s: ld %zu < n_ind %u", who, ld, n_ind);
    LDX_ARG_REQUIRE(accumulate != 0 || n_prior == 0u, "%s: n_prior %llu without accumulate", who, (unsigned long long)n_prior);
    LDX_ARG_REQUIRE(n_prior + n_snps <= 0xFFFFFFFFull, "%s: %llu SNPs already counted and %u more could pass 2^32 - 1 in a uint32 count",
                    who, (unsigned long long)n_prior, n_snps);
    const uint32_t chunks = king::snp_chunks(n_snps), nblocks = chunks / 2u;
    const uint32_t T = n_slabs(n_ind), n_tiles = T * (T + 1u) / 2u;
    if (n_slices == 0u) {   // enough workgroups for about four rounds of the card, none shorter than the minimum slice, none longer than the bound
        const uint32_t want = (4u * (uint32_t)device_cus() + n_tiles - 1u) / n_tiles, by_len = nblocks / king::kMinSliceBlocks;
        n_slices = want < by_len ? want : by_len;
        const uint32_t need = (nblocks + king::kMaxSliceBlocks - 1u) / king::kMaxSliceBlocks;
        n_slices = n_slices < need ? need : n_slices;
    }
    n_slices = n_slices > nblocks ? nblocks : n_slices;
    const uint32_t slice_blocks = (nblocks + n_slices - 1u) / n_slices;
    LDX_ARG_REQUIRE(slice_blocks <= king::kMaxSliceBlocks,
                    "%s: %u slices of %u SNPs: a slice may hold at most LDX_KING_MAX_SLICE_SNPS = %u (exact fp32 counts)", who, n_slices,
                    slice_blocks * king::kBlockSnps, LDX_KING_MAX_SLICE_SNPS);
    n_slices = (nblocks + slice_blocks - 1u) / slice_blocks;   // no empty slice
    LDX_ARG_REQUIRE((uint64_t)n_tiles * n_slices < (1ull << 31), "%s: %u tiles x %u slices: too many workgroups", who, n_tiles, n_slices);
    king::CountArgs p{};
    p.store = (const uint4 *)store, p.plane = king::plane_vecs(n_ind, n_snps);
    p.tables = tables, p.counts = counts, p.ld = ld;
    p.n_ind = n_ind, p.n_pad = king::pad_ind(n_ind);
    p.chunks = chunks, p.nblocks = nblocks, p.slice_blocks = slice_blocks, p.n_tiles = n_tiles;
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate)
        LDX_HIP(hipMemset2DAsync(counts, ld * sizeof(uint32_t), 0, (size_t)n_ind * sizeof(uint32_t), (size_t)4u * n_ind, s));
    king::counts_kernel<<<n_tiles * n_slices, king::kThreads, 0, s>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_king_from_counts_dev(size_t m, const uint32_t *N, const uint32_t *HH, const uint32_t *IBS0, const uint32_t *HETa,
                                        const uint32_t *HETb, float *kin, float *ibs, void *stream)
{
    const char *const who = "ldx_king_from_counts_dev";
    LDX_ARG_PTR(who, N); LDX_ARG_PTR(who, HH); LDX_ARG_PTR(who, IBS0); LDX_ARG_PTR(who, HETa); LDX_ARG_PTR(who, HETb);
    LDX_ARG_REQUIRE(kin != nullptr || ibs != nullptr, "%s: kin and ibs are both null pointers", who);
    if (m == 0u) return LDX_OK;
    king::tuples_kernel<<<king::grid_for(m), 256, 0, (hipStream_t)stream>>>(m, N, HH, IBS0, HETa, HETb, kin, ibs);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_sample_cells_dev(const uint32_t *counts, uint32_t n_ind, size_t ld, float *kin, float *ibs, size_t ld_out,
                                    void *stream)
{
    const char *const who = "ldx_sample_cells_dev";
    LDX_ARG_PTR(who, counts);
    LDX_ARG_REQUIRE(kin != nullptr || ibs != nullptr, "%s: kin and ibs are both null pointers", who);
    LDX_ARG_REQUIRE(n_ind != 0u, "%s: n_ind is 0", who);
    LDX_ARG_REQUIRE(ld >= n_ind && ld_out >= n_ind, "%s: ld %zu or ld_out %zu < n_ind %u", who, ld, ld_out, n_ind);
    king::cells_kernel<<<king::grid_for((size_t)n_ind * n_ind), 256, 0, (hipStream_t)stream>>>(counts, n_ind, ld, kin, ibs, ld_out);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

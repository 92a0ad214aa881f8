// Weighted sample products (include/ldx.h, "weighted sample products"): the genotype matrix against itself with
// an integer weight per SNP, the sums of the genetic relationship matrix:
//     S[a][b] = sum_i ( q2_i g_ia g_ib + q1_i (g_ia c_ib + c_ia g_ib) + q0_i c_ia c_ib )
//             = sum_i ( g_ia u_ib + c_ia v_ib ),      u_ib = q2_i g_ib + q1_i c_ib,   v_ib = q1_i g_ib + q0_i c_ib
// on v_mfma_i32_32x32x32_i8, from the transposed store of ldx_sample_planes_dev.  The kernels:
//   * wtable_kernel: per SNP the three values u and v can take for a called individual (g = 0, 1, 2; both are 0 for a missing
//     one) as four balanced base-256 digits in [-128, 127] each (x + 0x80808080 has the digits plus 128 in its bytes):
//     24 bytes per SNP, laid out as the words the product kernel ANDs with its byte masks -- byte b of word dd of
//     (K-block, step, lane half) belongs to the SNP whose bit the genotype operand carries in byte b of register dd.
//   * wprod_kernel: workgroup = (lower tile ti >= tj of 128 x 128 individuals, K slice); wave w owns the 32 columns w of the
//     tile and all four row blocks: 4 x 4 digit accumulators of 16 int32.  Per K-step of 32 SNPs (16 per lane half):
//         A operand (rows, tile ti): g = het + 2 hom-ALT and c as int8, a shift and an AND per register as in ldx_geno.hip;
//         B operand (columns, tile tj): digit l of u resp. v -- byte masks of "hom-REF", "het", "hom-ALT" made from the bit
//             planes ((x << 8) - x turns 0x01 bytes into 0xFF) select among the three table words: three bit operations per
//             register; the table of the K-block sits in LDS (double-buffered, one barrier per K-block), read as broadcasts;
//         8 MFMAs per 32 x 32 x 32: acc_l += g . digit_l(u) and acc_l += c . digit_l(v), l = 0 .. 3.
//     At the end of the slice sum_l 256^l acc_l in int64 -- the digits sit in separate accumulators of one lane: no shuffle --
//     is added to S with 64-bit integer atomics; the mirrored tile goes through a 32 x 32 LDS transpose so that both
//     orientations add 256 contiguous bytes per half-wave.  No floating point anywhere: order-independent, bit-reproducible.
//   * cells_kernel: the GRM cell, a function of the pair's two integers.
// Exactness: |u|, |v| <= 3 x 2^28 < 2^30 have four balanced digits; an accumulator takes |g d| + |c d'| <= 2 x 128 + 128 per SNP:
// see the static_asserts below.
#include "ldx_fp4.h"
#include "ldx_sample_store.h"   // pad_ind, snp_chunks, plane_vecs

namespace ldx {
namespace grm {

typedef int v16i __attribute__((ext_vector_type(16)));

constexpr uint32_t kTile = kSlab;             // individuals per tile side == rows per slab of the store
constexpr uint32_t kWaves = 4, kThreads = kWaves * 64u;   // one wave per SIMD: the 256 accumulator registers leave room for no second
constexpr uint32_t kMA = kTile / 32u;         // row blocks of a wave: all four
constexpr uint32_t kDigits = 4;               // balanced base-256 digits of u and v
constexpr uint32_t kSteps = 8;                // MFMA K-steps of a K-block: 256 SNPs, 16 per lane half each
constexpr uint32_t kBlockSnps = 256, kBlockVecs = 2u * kSlab;
constexpr uint32_t kGroupVecs = 2u * 3u * kDigits;        // 16-byte vectors of one (step, lane half): [u, v][g = 0, 1, 2][digit], 4 registers each
constexpr uint32_t kTabVecs = kSteps * 2u * kGroupVecs;   // of one K-block: 384 = 6 KiB = 24 bytes per SNP
constexpr uint32_t kMinSliceBlocks = LDX_WPROD_MIN_SLICE_SNPS / kBlockSnps;
constexpr uint32_t kMaxSliceBlocks = LDX_WPROD_MAX_SLICE_SNPS / kBlockSnps;
constexpr uint32_t kByteMask = 0x01010101u;
static_assert(3ll * LDX_WPROD_MAX_WEIGHT < (1ll << 30), "u = 2 q2 + q1 and v = 2 q1 + q0 must have four balanced base-256 digits");
static_assert((2ull * 128ull + 128ull) * LDX_WPROD_MAX_SLICE_SNPS < (1ull << 31), "a slice's int32 accumulators must not overflow");
static_assert(9ull * LDX_WPROD_MAX_WEIGHT * LDX_KING_MAX_STORE_SNPS < (1ull << 59),
              "|term| <= (4 + 2 + 2 + 1) 2^28 per SNP: every partial sum over 2^27 SNPs stays below 2^59");
static_assert(LDX_WPROD_MIN_SLICE_SNPS % kBlockSnps == 0 && LDX_WPROD_MAX_SLICE_SNPS % kBlockSnps == 0, "slices are whole K-blocks");
static_assert(kTabVecs > kThreads && kTabVecs <= 2u * kThreads, "a thread stages one or two vectors of a K-block's table");

// the four balanced base-256 digits of x as the bytes of one word: x = sum_l 256^l (int8)byte_l, for every |x| <= 2^30
__device__ __forceinline__ uint32_t limbs_of(int32_t x) { return ((uint32_t)x + 0x80808080u) ^ 0x80808080u; }

// byte l of x0 .. x3 as one word
__device__ __forceinline__ uint32_t gather_byte(const uint32_t (&x)[4], uint32_t l)
{
    const uint32_t s = 8u * l;
    return ((x[0] >> s) & 0xFFu) | (((x[1] >> s) & 0xFFu) << 8) | (((x[2] >> s) & 0xFFu) << 16) | (((x[3] >> s) & 0xFFu) << 24);
}

// the SNP (of the store) behind byte b of register dd of a lane half in a K-step: bit 8 b + 4 (step & 1) + dd of word step >> 1
__device__ __forceinline__ uint32_t snp_of(uint32_t blk, uint32_t step, uint32_t half, uint32_t dd, uint32_t b)
{
    return blk * kBlockSnps + 128u * half + 32u * (step >> 1) + 8u * b + 4u * (step & 1u) + dd;
}

// ---- the digit table ------------------------------------------------------------------------------------------------------------
// a thread per (K-block, step, lane half, register): 4 SNPs, 24 words
__global__ void __launch_bounds__(256) wtable_kernel(const int32_t *q, uint32_t n_snps, uint32_t nblocks, uint32_t *tab)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= nblocks * kSteps * 8u) return;
    const uint32_t dd = idx & 3u, half = (idx >> 2) & 1u, step = (idx >> 3) & 7u, blk = idx >> 6;
    uint32_t u[3][4], v[3][4];
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t snp = snp_of(blk, step, half, dd, b);
        int32_t q2 = 0, q1 = 0, q0 = 0;
        if (snp < n_snps) q2 = q[3u * (size_t)snp], q1 = q[3u * (size_t)snp + 1u], q0 = q[3u * (size_t)snp + 2u];
#pragma unroll
        for (int g = 0; g < 3; ++g) u[g][b] = limbs_of(g * q2 + q1), v[g][b] = limbs_of(g * q1 + q0);
    }
    uint32_t *const grp = tab + (size_t)(idx >> 2) * (kGroupVecs * 4u);   // (blk, step, half)
#pragma unroll
    for (uint32_t g = 0; g < 3u; ++g)
#pragma unroll
        for (uint32_t l = 0; l < kDigits; ++l) {
            grp[((0u * 3u + g) * kDigits + l) * 4u + dd] = gather_byte(u[g], l);
            grp[((1u * 3u + g) * kDigits + l) * 4u + dd] = gather_byte(v[g], l);
        }
}

// ---- the products ---------------------------------------------------------------------------------------------------------------
struct ProdArgs {
    const uint4 *store;
    size_t plane;             // vectors of one plane of the store
    const uint4 *tab;         // the digit table: kTabVecs per K-block
    long long *S;
    size_t ld;
    uint32_t n_ind;
    uint32_t chunks;          // SNP chunks of a row of the store
    uint32_t nblocks, slice_blocks, n_tiles;
};

struct Smem {
    uint4 tab[2][kTabVecs];           // the current and the next K-block's table
    long long t[kWaves][32][33];      // a wave's 32 x 32 transpose
};

// accumulator element e of a lane: row (e & 3) + 8 (e >> 2) + 4 (lane >> 5) of the 32 x 32 tile, column lane & 31
__device__ __forceinline__ uint32_t tile_row(int e, uint32_t half) { return (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * half; }

// 0x01 bytes of x to 0xFF
__device__ __forceinline__ uint32_t byte_mask(uint32_t x) { return (x << 8) - x; }

__global__ void __launch_bounds__(kThreads) wprod_kernel(ProdArgs p)
{
    __shared__ Smem sm;
    const uint32_t lane = threadIdx.x & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t slice = blockIdx.x / p.n_tiles, lt = blockIdx.x - slice * p.n_tiles;
    // lower tile lt -> (ti, tj), ti >= tj: lt = ti (ti + 1) / 2 + tj
    uint32_t ti = (uint32_t)((__builtin_sqrt(8.0 * (double)lt + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1u) / 2u > lt) --ti;
    while ((ti + 1u) * (ti + 2u) / 2u <= lt) ++ti;
    const uint32_t tj = lt - ti * (ti + 1u) / 2u;
    const uint32_t blk0 = slice * p.slice_blocks;
    const uint32_t blk1 = blk0 + p.slice_blocks < p.nblocks ? blk0 + p.slice_blocks : p.nblocks;
    const uint4 *const pc = p.store, *const pt = p.store + p.plane, *const pz = p.store + 2u * p.plane;
    // lane's operand rows: row r of a slab, chunk 2 blk + half
    const size_t a_off = ((size_t)ti * p.chunks + half) * kSlab + l32;
    const size_t b_off = ((size_t)tj * p.chunks + half) * kSlab + 32u * wave + l32;

    v16i acc[kMA][kDigits];
#pragma unroll
    for (uint32_t m = 0; m < kMA; ++m)
#pragma unroll
        for (uint32_t l = 0; l < kDigits; ++l)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][l][e] = 0;

    uint4 nat[kMA], naz[kMA], nac[kMA], nbt, nbz, nbc, ntab0, ntab1 = {0u, 0u, 0u, 0u};
    // a K-block's operands into registers, in two parts so that the rows' vectors of the next K-block replace the half of the current
    // ones that is already used up (all at once they would not fit beside the 256 accumulator registers)
    auto fetch_rows = [&](uint32_t blk) {
        const size_t o = (size_t)blk * kBlockVecs;
#pragma unroll
        for (uint32_t m = 0; m < kMA; ++m) nat[m] = pt[a_off + 32u * m + o], naz[m] = pz[a_off + 32u * m + o], nac[m] = pc[a_off + 32u * m + o];
    };
    auto fetch_cols = [&](uint32_t blk) {   // the columns' vectors and this thread's share of the K-block's table
        const size_t o = (size_t)blk * kBlockVecs;
        nbt = pt[b_off + o], nbz = pz[b_off + o], nbc = pc[b_off + o];
        const uint4 *const g = p.tab + (size_t)blk * kTabVecs;
        ntab0 = g[threadIdx.x];
        if (threadIdx.x < kTabVecs - kThreads) ntab1 = g[kThreads + threadIdx.x];
    };
    if (blk0 < blk1) fetch_rows(blk0), fetch_cols(blk0);
    for (uint32_t blk = blk0; blk < blk1; ++blk) {
        uint4 vat[kMA], vaz[kMA], vac[kMA];
#pragma unroll
        for (uint32_t m = 0; m < kMA; ++m) vat[m] = nat[m], vaz[m] = naz[m], vac[m] = nac[m];
        const uint4 vbt = nbt, vbz = nbz, vbc = nbc;
        // buffer (blk - blk0) & 1 was last read two K-blocks ago: every wave has passed the barrier in between
        uint4 *const tab = sm.tab[(blk - blk0) & 1u];
        tab[threadIdx.x] = ntab0;
        if (threadIdx.x < kTabVecs - kThreads) tab[kThreads + threadIdx.x] = ntab1;
        block_sync();
        if (blk + 1u < blk1) fetch_cols(blk + 1u);   // in flight under this K-block's MFMAs
#pragma unroll
        for (int wd = 0; wd < 4; ++wd) {
            if (wd == 2 && blk + 1u < blk1) fetch_rows(blk + 1u);   // half a K-block ahead
#pragma unroll
            for (uint32_t sh = 0; sh < 2u; ++sh) {
                const uint32_t step = 2u * (uint32_t)wd + sh;
                const uint4 *const grp = tab + (step * 2u + half) * kGroupVecs;
                v4i ag[kMA], ac[kMA];
#pragma unroll
                for (uint32_t m = 0; m < kMA; ++m) {
                    const uint32_t t = word_of(vat[m], wd) >> (4u * sh), z = word_of(vaz[m], wd) >> (4u * sh);
                    const uint32_t c = word_of(vac[m], wd) >> (4u * sh);
#pragma unroll
                    for (int dd = 0; dd < 4; ++dd) {
                        ag[m][dd] = (int)(((t >> dd) & kByteMask) | (((z >> dd) & kByteMask) << 1));   // g = het + 2 hom-ALT
                        ac[m][dd] = (int)((c >> dd) & kByteMask);
                    }
                }
                // the column individual's genotype at the register's four SNPs, as byte masks: het, hom-ALT, hom-REF (called
                // and neither: the store's het and hom-ALT bits are disjoint subsets of its called bits)
                uint32_t mt[4], mz[4], mr[4];
                {
                    const uint32_t t = word_of(vbt, wd) >> (4u * sh), z = word_of(vbz, wd) >> (4u * sh);
                    const uint32_t c = word_of(vbc, wd) >> (4u * sh);
#pragma unroll
                    for (int dd = 0; dd < 4; ++dd) {
                        mt[dd] = byte_mask((t >> dd) & kByteMask), mz[dd] = byte_mask((z >> dd) & kByteMask);
                        mr[dd] = byte_mask((c >> dd) & kByteMask) ^ mt[dd] ^ mz[dd];
                    }
                }
#pragma unroll
                for (uint32_t uv = 0; uv < 2u; ++uv) {
#pragma unroll
                    for (uint32_t l = 0; l < kDigits; ++l) {
                        const uint4 d0 = grp[(uv * 3u + 0u) * kDigits + l], d1 = grp[(uv * 3u + 1u) * kDigits + l];
                        const uint4 d2 = grp[(uv * 3u + 2u) * kDigits + l];
                        v4i b;
#pragma unroll
                        for (int dd = 0; dd < 4; ++dd)
                            b[dd] = (int)((mr[dd] & word_of(d0, dd)) | (mt[dd] & word_of(d1, dd)) | (mz[dd] & word_of(d2, dd)));
#pragma unroll
                        for (uint32_t m = 0; m < kMA; ++m)
                            acc[m][l] = __builtin_amdgcn_mfma_i32_32x32x32_i8(uv == 0u ? ag[m] : ac[m], b, acc[m][l], 0, 0, 0);
                    }
                }
            }
        }
    }

    // ---- the slice's sums into S: cell (i0 + tile_row(e), j0 + l32); a half-wave adds 256 contiguous bytes
    const bool mirror = ti != tj;   // a diagonal tile holds both orientations itself
    const uint32_t j0 = tj * kTile + 32u * wave;
#pragma unroll
    for (uint32_t m = 0; m < kMA; ++m) {
        const uint32_t i0 = ti * kTile + 32u * m;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            long long v = 0;
#pragma unroll
            for (uint32_t l = 0; l < kDigits; ++l) v += (long long)acc[m][l][e] * (1ll << (8u * l));
            const uint32_t i = i0 + tile_row(e, half), j = j0 + l32;
            if (i < p.n_ind && j < p.n_ind && v != 0) atomicAdd((unsigned long long *)(p.S + (size_t)i * p.ld + j), (unsigned long long)v);
            if (mirror) sm.t[wave][l32][tile_row(e, half)] = v;
        }
        if (!mirror) continue;   // workgroup-uniform
        // mirrored: cell (j0 + tile_row(e), i0 + l32) receives what (i0 + l32, j0 + tile_row(e)) holds
        block_sync();
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const uint32_t j = j0 + tile_row(e, half), i = i0 + l32;
            const long long x = sm.t[wave][tile_row(e, half)][l32];
            if (i < p.n_ind && j < p.n_ind && x != 0)
                atomicAdd((unsigned long long *)(p.S + (size_t)j * p.ld + i), (unsigned long long)x);
        }
        block_sync();
    }
}

// ---- the cell: a function of the pair's integers alone ----------------------------------------------------------------------------
__device__ __forceinline__ float grm_cell(long long S, uint32_t N, double scale)
{
    if (N == 0u) return -0.0f;
    return (float)(((double)S * scale) / (double)N);
}

__global__ void __launch_bounds__(256) cells_kernel(const long long *S, size_t ld_s, const uint32_t *N, size_t ld_n, uint32_t n_ind,
                                                    double scale, float *out, size_t ld_out)
{
    const size_t total = (size_t)n_ind * n_ind;
    for (size_t k = (size_t)blockIdx.x * 256u + threadIdx.x; k < total; k += (size_t)gridDim.x * 256u) {
        const uint32_t a = (uint32_t)(k / n_ind), b = (uint32_t)(k - (size_t)a * n_ind);
        out[(size_t)a * ld_out + b] = grm_cell(S[(size_t)a * ld_s + b], N[(size_t)a * ld_n + b], scale);
    }
}

}  // namespace grm
}  // namespace ldx

using namespace ldx;

extern "C" size_t ldx_sample_wprod_workspace_bytes(uint32_t n_snps)
{
    return (size_t)(king::snp_chunks(n_snps) / 2u) * grm::kTabVecs * sizeof(uint4);
}

extern "C" int ldx_sample_wprod_dev(const void *store, const uint32_t *tables, uint32_t n_ind, uint32_t n_snps, const int32_t *q,
                                    int64_t *S, size_t ld, int accumulate, uint32_t n_slices, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    const char *const who = "ldx_sample_wprod_dev";
    LDX_ARG_PTR(who, store); LDX_ARG_PTR(who, tables); LDX_ARG_PTR(who, q); LDX_ARG_PTR(who, S); LDX_ARG_PTR(who, workspace);
    LDX_ARG_REQUIRE(n_ind != 0u && n_snps != 0u, "%s: n_ind and n_snps must be non-zero", who);
    if (n_ind > LDX_MAX_HAPS / 2u) {
        set_error("%s: %u individuals, more than LDX_MAX_HAPS / 2 = %u", who, n_ind, LDX_MAX_HAPS / 2u);
        return LDX_E_UNSUPPORTED;
    }
    LDX_ARG_REQUIRE(n_snps <= LDX_KING_MAX_STORE_SNPS, "%s: %u SNPs in one store, more than %u: split the SNPs over several calls",
                    who, n_snps, LDX_KING_MAX_STORE_SNPS);
    LDX_ARG_REQUIRE(ld >= n_ind, "%s: ld %zu < n_ind %u", who, ld, n_ind);
    LDX_ARG_REQUIRE(workspace_bytes >= ldx_sample_wprod_workspace_bytes(n_snps), "%s: workspace of %zu bytes, %zu needed", who,
                    workspace_bytes, ldx_sample_wprod_workspace_bytes(n_snps));
    LDX_ARG_REQUIRE(((uintptr_t)workspace & 15u) == 0u, "%s: workspace must be 16-byte aligned", who);
    const uint32_t chunks = king::snp_chunks(n_snps), nblocks = chunks / 2u;
    const uint32_t T = n_slabs(n_ind), n_tiles = T * (T + 1u) / 2u;
    if (n_slices == 0u) {   // enough workgroups for about four rounds of the card, none shorter than the minimum slice, none longer than the bound
        const uint32_t cus = (uint32_t)device_cus();   // one workgroup per CU at a time: 512 registers per lane
        const uint32_t want = (4u * cus + n_tiles - 1u) / n_tiles, by_len = nblocks / grm::kMinSliceBlocks;
        n_slices = want < by_len ? want : by_len;
        // of the next few slice counts the one whose last round is fullest: 210 tiles x 5 slices are 4.1 rounds of 256 CUs, x 6 are 4.9
        double best = 0.0;
        for (uint32_t s = n_slices; s >= 1u && s <= want + 3u && s <= by_len; ++s) {
            const uint64_t groups = (uint64_t)n_tiles * s, rounds = (groups + cus - 1u) / cus;
            const double fill = (double)groups / (double)(rounds * cus);
            if (fill > best + 1e-9) best = fill, n_slices = s;
        }
        const uint32_t need = (nblocks + grm::kMaxSliceBlocks - 1u) / grm::kMaxSliceBlocks;
        n_slices = n_slices < need ? need : n_slices;
    }
    n_slices = n_slices > nblocks ? nblocks : n_slices;
    const uint32_t slice_blocks = (nblocks + n_slices - 1u) / n_slices;
    LDX_ARG_REQUIRE(slice_blocks <= grm::kMaxSliceBlocks,
                    "%s: %u slices of %u SNPs: a slice may hold at most LDX_WPROD_MAX_SLICE_SNPS = %u (int32 accumulators)", who,
                    n_slices, slice_blocks * grm::kBlockSnps, LDX_WPROD_MAX_SLICE_SNPS);
    n_slices = (nblocks + slice_blocks - 1u) / slice_blocks;   // no empty slice
    LDX_ARG_REQUIRE((uint64_t)n_tiles * n_slices < (1ull << 31), "%s: %u tiles x %u slices: too many workgroups", who, n_tiles, n_slices);
    grm::ProdArgs p{};
    p.store = (const uint4 *)store, p.plane = king::plane_vecs(n_ind, n_snps);
    p.tab = (const uint4 *)workspace;
    p.S = (long long *)S, p.ld = ld, p.n_ind = n_ind;
    p.chunks = chunks, p.nblocks = nblocks, p.slice_blocks = slice_blocks, p.n_tiles = n_tiles;
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate) LDX_HIP(hipMemset2DAsync(S, ld * sizeof(int64_t), 0, (size_t)n_ind * sizeof(int64_t), n_ind, s));
    const uint32_t table_threads = nblocks * grm::kSteps * 8u;   // nblocks <= 2^19
    grm::wtable_kernel<<<(table_threads + 255u) / 256u, 256, 0, s>>>(q, n_snps, nblocks, (uint32_t *)workspace);
    LDX_HIP(hipGetLastError());
    grm::wprod_kernel<<<n_tiles * n_slices, grm::kThreads, 0, s>>>(p);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_grm_cells_dev(const int64_t *S, size_t ld_s, const uint32_t *N, size_t ld_n, uint32_t n_ind, int exp, float *grm,
                                 size_t ld_out, void *stream)
{
    const char *const who = "ldx_grm_cells_dev";
    LDX_ARG_PTR(who, S); LDX_ARG_PTR(who, N); LDX_ARG_PTR(who, grm);
    LDX_ARG_REQUIRE(n_ind != 0u, "%s: n_ind is 0", who);
    LDX_ARG_REQUIRE(ld_s >= n_ind && ld_n >= n_ind && ld_out >= n_ind, "%s: ld_s %zu, ld_n %zu or ld_out %zu < n_ind %u", who, ld_s,
                    ld_n, ld_out, n_ind);
    LDX_ARG_REQUIRE(exp >= -LDX_GRM_MAX_EXP && exp <= LDX_GRM_MAX_EXP, "%s: exp %d outside -%d .. %d", who, exp, LDX_GRM_MAX_EXP,
                    LDX_GRM_MAX_EXP);
    const size_t items = (size_t)n_ind * n_ind, want = (items + 255u) / 256u, cap = (size_t)device_cus() * 8u;
    const double scale = __builtin_ldexp(1.0, exp - LDX_WPROD_SCALE_BITS);
    grm::cells_kernel<<<(uint32_t)(want < cap ? want : cap), 256, 0, (hipStream_t)stream>>>((const long long *)S, ld_s, N, ld_n, n_ind,
                                                                                             scale, grm, ld_out);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

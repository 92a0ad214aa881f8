// Genotype products (include/ldx.h, "genotype products"): the genotype matrix times a narrow dense matrix, both
// ways, straight from the bit planes, every term an integer:
//     forward   y[a][c] += sum_i g_ia w[i][c] + c_ia wc[i][c]           (store of ldx_sample_planes_dev: rows = individuals)
//     reverse   z[i][c]  = sum_a g_ia u[a][c],  zc[i][c] = sum_a c_ia u[a][c]      (the panel's tiled planes: rows = SNPs)
// Both run on v_mfma_i32_32x32x32_i8.
//   * A operand: the genotype as int8 0 / 1 / 2 (the called bit as 0 / 1), made from the bit planes where it is used.  The K
//     order inside an instruction is free as long as both operands use the same one, so byte b of register d of a lane is
//     bit 8 b + d of its 32-bit word (forward: 32 SNPs; two instructions per word) or bit 8 b + 2 d (reverse: the even haplotype
//     slots of 16 individuals; one instruction per word): a shift and an AND per register, no byte movement.
//   * B operand: the weights as LIMBS.  x + 0x80808080 has the balanced base-256 digits of x plus 128 in its bytes, so the four
//     int8 digits d_l in [-128, 127] with x = sum_l 256^l d_l are two integer operations; a real column is four int8 columns
//     (lanes 4 q .. 4 q + 3 of a 32-column tile: 8 real columns per tile, up to 4 tiles = 32 real columns per workgroup).  The
//     workgroup's four waves share the B fragments of a K-block through LDS: each thread splits 16 weights of one column and
//     writes the four limbs' 16-byte fragments, each wave reads a fragment per MFMA with one ds_read_b128.
//   * Recombination: at the end of the K range sum_l 2^(8 l) acc_l in int64 over the four lanes of a real column (two
//     shuffles), then 64-bit integer atomics (forward: K slices and stores add into one y, order-independent) or plain
//     stores (reverse).
// Exactness: an int8 product is at most 2 x 128, and the forward accumulator takes g w + c wc <= 3 x 128 per SNP: see the
// static_asserts below.
#include "ldx_fp4.h"
#include "ldx_sample_store.h"

namespace ldx {
namespace geno {

typedef int v16i __attribute__((ext_vector_type(16)));

constexpr uint32_t kWaves = 4, kThreads = kWaves * 64u;   // a wave owns 32 rows of the slab of 128
constexpr uint32_t kTileCols = 8;                          // real columns of a 32-column tile: four limbs each
constexpr uint32_t kMaxTiles = 4;                          // tiles of a workgroup
constexpr uint32_t kGroupCols = kTileCols * kMaxTiles;     // real columns of a workgroup
constexpr uint32_t kFwdSteps = 8;                          // MFMAs along a forward K-block: 256 SNPs, 16 per lane half each
constexpr uint32_t kRevSteps = 4;                          // along a reverse K-block: 128 individuals
constexpr uint32_t kBlockSnps = 256, kBlockVecs = 2u * kSlab;
constexpr uint32_t kMinSliceBlocks = 8;                    // the automatic choice makes no slice under 2048 SNPs
constexpr uint32_t kMaxSliceBlocks = LDX_GENO_MAX_SLICE_SNPS / kBlockSnps;
constexpr uint32_t kByteMask = 0x01010101u;
// forward: |g d| <= 2 x 128 and |c d'| <= 128 meet in one accumulator, per SNP of the slice
static_assert(3ull * 128ull * LDX_GENO_MAX_SLICE_SNPS < (1ull << 31), "a slice's int32 accumulators must not overflow");
static_assert(LDX_GENO_MAX_SLICE_SNPS % kBlockSnps == 0, "slices are whole K-blocks");
// reverse: no slicing, K = all individuals
static_assert(2ull * 128ull * (LDX_MAX_HAPS / 2u) < (1ull << 31), "the reverse product's int32 accumulators must not overflow");
static_assert(LDX_GENO_MAX_COLS % kGroupCols == 0, "column groups");

// the four balanced base-256 digits of x as the bytes of one word: x = sum_l 256^l (int8)byte_l, for every |x| <= 2^30
__device__ __forceinline__ uint32_t limbs_of(int32_t x) { return ((uint32_t)x + 0x80808080u) ^ 0x80808080u; }

// byte l of x0 .. x3 as one word
__device__ __forceinline__ uint32_t gather_byte(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t l)
{
    const uint32_t s = 8u * l;
    return ((x0 >> s) & 0xFFu) | (((x1 >> s) & 0xFFu) << 8) | (((x2 >> s) & 0xFFu) << 16) | (((x3 >> s) & 0xFFu) << 24);
}

// One K-block of the weights `w` (rows of ld int32, columns col0 .. col0 + ncols - 1) into LDS as B fragments:
// frag[(step * kTiles + tile) * 64 + lane] is what lane (half h = lane >> 5, column lane & 31 = 4 (r & 7) + limb of tile
// r >> 3) feeds to the MFMA of `step`; its byte 4 dd + b is the limb of row row_of(step, h, dd, b) -- the row whose genotype
// the A operand carries in byte b of register dd.  Rows from n_rows on and columns from ncols on are zero.
// In two halves, so that the loads of the NEXT K-block are in flight under the MFMAs of the current one: load_weights issues a
// thread's loads (kSteps / 4 units of one column x 16 rows; addresses clamped into the matrix and a validity mask kept, so that
// no load hangs on a branch), store_weights splits, transposes and writes them a K-block later.
template <uint32_t kSteps>
struct Staged {
    int32_t x[kSteps / 4u][16];
    uint32_t valid[kSteps / 4u];
};

template <uint32_t kSteps, typename RowOf>
__device__ __forceinline__ void load_weights(Staged<kSteps> &s, const int32_t *w, size_t ld, uint32_t col0, uint32_t ncols,
                                             uint32_t n_tiles, uint32_t n_rows, RowOf row_of)
{
    const uint32_t r = threadIdx.x & 31u;
    if (r >= n_tiles * kTileCols) return;
    const int32_t *const col = w + col0 + (r < ncols ? r : ncols - 1u);
#pragma unroll
    for (uint32_t i = 0; i < kSteps / 4u; ++i) {
        const uint32_t u = i * (kThreads / 32u) + (threadIdx.x >> 5), step = u >> 1, h = u & 1u;
        uint32_t valid = 0;
#pragma unroll
        for (uint32_t dd = 0; dd < 4u; ++dd)
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) {
                const uint32_t row = row_of(step, h, dd, b);
                s.x[i][4u * dd + b] = col[(size_t)(row < n_rows ? row : n_rows - 1u) * ld];
                valid |= (uint32_t)(r < ncols && row < n_rows) << (4u * dd + b);
            }
        s.valid[i] = valid;
    }
}

template <uint32_t kSteps, uint32_t kTiles>
__device__ __forceinline__ void store_weights(uint4 *frag, const Staged<kSteps> &s)
{
    const uint32_t r = threadIdx.x & 31u;
    if (r >= kTiles * kTileCols) return;
#pragma unroll
    for (uint32_t i = 0; i < kSteps / 4u; ++i) {
        const uint32_t u = i * (kThreads / 32u) + (threadIdx.x >> 5), step = u >> 1, h = u & 1u;
        uint32_t x[16];
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) x[j] = (s.valid[i] >> j) & 1u ? limbs_of(s.x[i][j]) : 0u;
#pragma unroll
        for (uint32_t l = 0; l < 4u; ++l)
            frag[(step * kTiles + (r >> 3)) * 64u + 32u * h + 4u * (r & 7u) + l] =
                uint4{gather_byte(x[0], x[1], x[2], x[3], l), gather_byte(x[4], x[5], x[6], x[7], l),
                      gather_byte(x[8], x[9], x[10], x[11], l), gather_byte(x[12], x[13], x[14], x[15], l)};
    }
}

__device__ __forceinline__ v4i frag_of(const uint4 &v) { return v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w}; }

// accumulator element e of a lane: row (e & 3) + 8 (e >> 2) + 4 (lane >> 5) of the 32 x 32 tile, column lane & 31
__device__ __forceinline__ uint32_t tile_row(int e, uint32_t half) { return (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * half; }

// sum_l 2^(8 l) acc_l over the four limb lanes 4 q .. 4 q + 3 of a real column; every lane of the quad gets the sum
__device__ __forceinline__ long long recombine(int acc, uint32_t limb)
{
    long long v = (long long)acc * (1ll << (8u * limb));
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v;
}

// ---- forward: y += [G | C] [w ; wc] ---------------------------------------------------------------------------------------------
struct FwdArgs {
    const uint4 *store;       // called, het, hom-ALT planes
    size_t plane;             // vectors of one plane
    uint32_t n_ind, n_snps;
    uint32_t chunks;          // SNP chunks of a row of the store
    uint32_t nblocks, slice_blocks, slabs;
    const int32_t *w, *wc;
    size_t ld_w;
    uint32_t k, col0;         // the launch's column group: columns col0 .. col0 + 8 kTiles - 1 (those below k)
    long long *y;
    size_t ld_y;
};

template <bool kCalled, uint32_t kTiles>
__global__ void __launch_bounds__(kThreads) matmul_kernel(FwdArgs p)
{
    __shared__ uint4 sm[(kCalled ? 2u : 1u) * kFwdSteps * kTiles * 64u];
    uint4 *const fw = sm, *const fc = sm + (kCalled ? kFwdSteps * kTiles * 64u : 0u);
    const uint32_t lane = threadIdx.x & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the slab is the fast index: the workgroups that stream the same K slice of the weights run side by side and meet in L2
    const uint32_t slice = blockIdx.x / p.slabs, slab = blockIdx.x - slice * p.slabs, col0 = p.col0;
    const uint32_t ncols = p.k - col0 < kTiles * kTileCols ? p.k - col0 : kTiles * kTileCols;
    const uint32_t blk0 = slice * p.slice_blocks;
    const uint32_t blk1 = blk0 + p.slice_blocks < p.nblocks ? blk0 + p.slice_blocks : p.nblocks;
    const uint4 *const pc = p.store, *const pt = p.store + p.plane, *const pz = p.store + 2u * p.plane;
    // lane's operand row: row 32 wave + l32 of the slab, chunk 2 blk + half
    const size_t a_off = ((size_t)slab * p.chunks + half) * kSlab + 32u * wave + l32;

    v16i acc[kTiles];
#pragma unroll
    for (uint32_t t = 0; t < kTiles; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0;

    Staged<kFwdSteps> sw;
    [[maybe_unused]] Staged<kFwdSteps> sc;
    uint4 nt, nz, nc = {0u, 0u, 0u, 0u};
    auto fetch = [&](uint32_t blk) {   // a K-block's weights and plane vectors into registers
        auto row_of = [blk](uint32_t step, uint32_t h, uint32_t dd, uint32_t b) {
            return blk * kBlockSnps + 128u * h + 32u * (step >> 1) + 8u * b + 4u * (step & 1u) + dd;
        };
        load_weights<kFwdSteps>(sw, p.w, p.ld_w, col0, ncols, kTiles, p.n_snps, row_of);
        if constexpr (kCalled) load_weights<kFwdSteps>(sc, p.wc, p.ld_w, col0, ncols, kTiles, p.n_snps, row_of);
        const size_t o = a_off + (size_t)blk * kBlockVecs;
        nt = pt[o], nz = pz[o];
        if constexpr (kCalled) nc = pc[o];
    };
    if (blk0 < blk1) fetch(blk0);
    for (uint32_t blk = blk0; blk < blk1; ++blk) {
        const uint4 vt = nt, vz = nz, vc = nc;
        block_sync();   // the previous K-block's fragments are read
        store_weights<kFwdSteps, kTiles>(fw, sw);
        if constexpr (kCalled) store_weights<kFwdSteps, kTiles>(fc, sc);
        block_sync();
        if (blk + 1u < blk1) fetch(blk + 1u);   // in flight under this K-block's MFMAs
#pragma unroll
        for (int wd = 0; wd < 4; ++wd) {
#pragma unroll
            for (uint32_t sh = 0; sh < 2u; ++sh) {
                const uint32_t step = 2u * (uint32_t)wd + sh;
                const uint32_t t = word_of(vt, wd) >> (4u * sh), z = word_of(vz, wd) >> (4u * sh), c = word_of(vc, wd) >> (4u * sh);
                v4i ag, ac;
#pragma unroll
                for (int dd = 0; dd < 4; ++dd) {
                    ag[dd] = (int)(((t >> dd) & kByteMask) | (((z >> dd) & kByteMask) << 1));   // g = het + 2 hom-ALT
                    ac[dd] = (int)((c >> dd) & kByteMask);
                }
#pragma unroll
                for (uint32_t tt = 0; tt < kTiles; ++tt) {
                    const uint32_t at = (step * kTiles + tt) * 64u + lane;
                    acc[tt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ag, frag_of(fw[at]), acc[tt], 0, 0, 0);
                    if constexpr (kCalled) acc[tt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ac, frag_of(fc[at]), acc[tt], 0, 0, 0);
                }
            }
        }
    }

    const uint32_t limb = l32 & 3u;
#pragma unroll
    for (uint32_t tt = 0; tt < kTiles; ++tt) {   // every lane takes part in the shuffles
        const uint32_t col = col0 + kTileCols * tt + (l32 >> 2);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const long long v = recombine(acc[tt][e], limb);
            const uint32_t a = slab * kSlab + 32u * wave + tile_row(e, half);
            if (limb == 0u && a < p.n_ind && col < p.k && v != 0)
                atomicAdd((unsigned long long *)(p.y + (size_t)a * p.ld_y + col), (unsigned long long)v);
        }
    }
}

// ---- reverse: z = G^T u, zc = C^T u -----------------------------------------------------------------------------------------------
struct RevArgs {
    const uint4 *alt, *ref;   // the panel's tiled planes
    const uint8_t *keep;      // [n_snps], or null
    uint32_t n_snps, n_ind;
    uint32_t hap_chunks;      // chunks of a panel row
    const int32_t *u;
    size_t ld_u;
    uint32_t k, col0;         // the launch's column group
    long long *z, *zc;
    size_t ld_z;
};

template <uint32_t kTiles>
__global__ void __launch_bounds__(kThreads) rmatmul_kernel(RevArgs p)
{
    __shared__ uint4 sm[kRevSteps * kTiles * 64u];
    const uint32_t lane = threadIdx.x & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t slab = blockIdx.x, col0 = p.col0;
    const uint32_t ncols = p.k - col0 < kTiles * kTileCols ? p.k - col0 : kTiles * kTileCols;
    const uint32_t s = slab * kSlab + 32u * wave + l32;   // lane's SNP row
    const bool kept = s < p.n_snps && (p.keep == nullptr || p.keep[s] != 0);
    const size_t a_off = ((size_t)slab * p.hap_chunks + half) * kSlab + 32u * wave + l32;

    v16i accg[kTiles], accc[kTiles];
#pragma unroll
    for (uint32_t t = 0; t < kTiles; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) accg[t][e] = 0, accc[t][e] = 0;

    Staged<kRevSteps> su;
    uint4 na = {0u, 0u, 0u, 0u}, nr = {0u, 0u, 0u, 0u};
    const uint32_t n_kb = p.hap_chunks / 2u;
    auto fetch = [&](uint32_t kb) {   // a K-block's weights and plane vectors into registers
        load_weights<kRevSteps>(su, p.u, p.ld_u, col0, ncols, kTiles, p.n_ind,
                                [kb](uint32_t step, uint32_t h, uint32_t dd, uint32_t b) {
                                    return kb * 128u + 64u * h + 16u * step + dd + 4u * b;
                                });
        if (kept) {
            const size_t o = a_off + (size_t)kb * kBlockVecs;
            na = p.alt[o], nr = p.ref[o];
        }
    };
    fetch(0u);
    for (uint32_t kb = 0; kb < n_kb; ++kb) {
        const uint4 va = na, vr = nr;
        block_sync();   // the previous K-block's fragments are read
        store_weights<kRevSteps, kTiles>(sm, su);
        block_sync();
        if (kb + 1u < n_kb) fetch(kb + 1u);   // in flight under this K-block's MFMAs
#pragma unroll
        for (int wd = 0; wd < 4; ++wd) {
            const uint32_t wa = word_of(va, wd), wr = word_of(vr, wd);
            const GenoWords g = geno_words(wa, wr);   // a half-missing genotype is missing
            const uint32_t q = g.q, z = g.z, t = g.t;
            v4i ag, ac;
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                ag[dd] = (int)(((t >> (2 * dd)) & kByteMask) | (((z >> (2 * dd)) & kByteMask) << 1));
                ac[dd] = (int)((q >> (2 * dd)) & kByteMask);
            }
#pragma unroll
            for (uint32_t tt = 0; tt < kTiles; ++tt) {
                const v4i b = frag_of(sm[((uint32_t)wd * kTiles + tt) * 64u + lane]);
                accg[tt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ag, b, accg[tt], 0, 0, 0);
                accc[tt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ac, b, accc[tt], 0, 0, 0);
            }
        }
    }

    const uint32_t limb = l32 & 3u;
#pragma unroll
    for (uint32_t tt = 0; tt < kTiles; ++tt) {   // every lane takes part in the shuffles
        const uint32_t col = col0 + kTileCols * tt + (l32 >> 2);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const long long vg = recombine(accg[tt][e], limb), vc = recombine(accc[tt][e], limb);
            const uint32_t i = slab * kSlab + 32u * wave + tile_row(e, half);
            if (limb == 0u && i < p.n_snps && col < p.k) {
                p.z[(size_t)i * p.ld_z + col] = vg;    // a SNP that is not kept: its A rows were zero
                p.zc[(size_t)i * p.ld_z + col] = vc;
            }
        }
    }
}

template <bool kCalled>
static void launch_matmul(uint32_t tiles, uint32_t grid, hipStream_t s, const FwdArgs &p)
{
    switch (tiles) {
    case 1: matmul_kernel<kCalled, 1><<<grid, kThreads, 0, s>>>(p); break;
    case 2: matmul_kernel<kCalled, 2><<<grid, kThreads, 0, s>>>(p); break;
    case 3: matmul_kernel<kCalled, 3><<<grid, kThreads, 0, s>>>(p); break;
    default: matmul_kernel<kCalled, 4><<<grid, kThreads, 0, s>>>(p); break;
    }
}

static void launch_rmatmul(uint32_t tiles, uint32_t grid, hipStream_t s, const RevArgs &p)
{
    switch (tiles) {
    case 1: rmatmul_kernel<1><<<grid, kThreads, 0, s>>>(p); break;
    case 2: rmatmul_kernel<2><<<grid, kThreads, 0, s>>>(p); break;
    case 3: rmatmul_kernel<3><<<grid, kThreads, 0, s>>>(p); break;
    default: rmatmul_kernel<4><<<grid, kThreads, 0, s>>>(p); break;
    }
}

}  // namespace geno
}  // namespace ldx

using namespace ldx;

static int geno_cols_ok(const char *who, uint32_t k, size_t ld_in, const char *in_name, size_t ld_out, const char *out_name)
{
    LDX_ARG_REQUIRE(k >= 1u && k <= LDX_GENO_MAX_COLS, "%s: k %u outside 1 .. LDX_GENO_MAX_COLS = %u", who, k, LDX_GENO_MAX_COLS);
    LDX_ARG_REQUIRE(ld_in >= k, "%s: %s %zu < k %u", who, in_name, ld_in, k);
    LDX_ARG_REQUIRE(ld_out >= k, "%s: %s %zu < k %u", who, out_name, ld_out, k);
    return LDX_OK;
}

extern "C" int ldx_geno_matmul_dev(const void *store, const uint32_t *tables, uint32_t n_ind, uint32_t n_snps, const int32_t *w,
                                   const int32_t *wc, size_t ld_w, uint32_t k, int64_t *y, size_t ld_y, int accumulate,
                                   uint32_t n_slices, void *stream)
{
    const char *const who = "ldx_geno_matmul_dev";
    LDX_ARG_PTR(who, store); LDX_ARG_PTR(who, tables); LDX_ARG_PTR(who, w); LDX_ARG_PTR(who, y);
    LDX_ARG_REQUIRE(n_ind != 0u && n_snps != 0u, "%s: n_ind and n_snps must be non-zero", who);
    if (n_ind > LDX_MAX_HAPS / 2u) {
        set_error("%s: %u individuals, more than LDX_MAX_HAPS / 2 = %u", who, n_ind, LDX_MAX_HAPS / 2u);
        return LDX_E_UNSUPPORTED;
    }
    LDX_ARG_REQUIRE(n_snps <= LDX_KING_MAX_STORE_SNPS, "%s: %u SNPs in one store, more than %u", who, n_snps, LDX_KING_MAX_STORE_SNPS);
    if (const int rc = geno_cols_ok(who, k, ld_w, "ld_w", ld_y, "ld_y")) return rc;
    const uint32_t chunks = king::snp_chunks(n_snps), nblocks = chunks / 2u;
    const uint32_t slabs = n_slabs(n_ind), groups = (k + geno::kGroupCols - 1u) / geno::kGroupCols;
    if (n_slices == 0u) {   // about eight rounds of two workgroups per CU (a short tail), no slice under the minimum, none over the bound
        const uint32_t want = (16u * (uint32_t)device_cus() + slabs - 1u) / slabs, by_len = nblocks / geno::kMinSliceBlocks;
        n_slices = want < by_len ? want : by_len;
        const uint32_t need = (nblocks + geno::kMaxSliceBlocks - 1u) / geno::kMaxSliceBlocks;
        n_slices = n_slices < need ? need : n_slices;
    }
    n_slices = n_slices > nblocks ? nblocks : n_slices;
    const uint32_t slice_blocks = (nblocks + n_slices - 1u) / n_slices;
    LDX_ARG_REQUIRE(slice_blocks <= geno::kMaxSliceBlocks,
                    "%s: %u slices of %u SNPs: a slice may hold at most LDX_GENO_MAX_SLICE_SNPS = %u (int32 accumulators)", who,
                    n_slices, slice_blocks * geno::kBlockSnps, LDX_GENO_MAX_SLICE_SNPS);
    n_slices = (nblocks + slice_blocks - 1u) / slice_blocks;   // no empty slice
    geno::FwdArgs p{};
    p.store = (const uint4 *)store, p.plane = king::plane_vecs(n_ind, n_snps);
    p.n_ind = n_ind, p.n_snps = n_snps;
    p.chunks = chunks, p.nblocks = nblocks, p.slice_blocks = slice_blocks, p.slabs = slabs;
    p.w = w, p.wc = wc, p.ld_w = ld_w, p.k = k;
    p.y = (long long *)y, p.ld_y = ld_y;
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate) LDX_HIP(hipMemset2DAsync(y, ld_y * sizeof(int64_t), 0, (size_t)k * sizeof(int64_t), n_ind, s));
    for (uint32_t g = 0; g < groups; ++g) {   // one launch per group of 32 columns, instantiated for the group's tiles of 8
        p.col0 = g * geno::kGroupCols;
        const uint32_t tiles = (k - p.col0 < geno::kGroupCols ? k - p.col0 + geno::kTileCols - 1u : geno::kGroupCols) / geno::kTileCols;
        if (wc != nullptr) geno::launch_matmul<true>(tiles, n_slices * slabs, s, p);
        else geno::launch_matmul<false>(tiles, n_slices * slabs, s, p);
        LDX_HIP(hipGetLastError());
    }
    return LDX_OK;
}

extern "C" int ldx_geno_rmatmul_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                                    const int32_t *u, size_t ld_u, uint32_t k, int64_t *z, int64_t *zc, size_t ld_z, void *stream)
{
    const char *const who = "ldx_geno_rmatmul_dev";
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, ref); LDX_ARG_PTR(who, u); LDX_ARG_PTR(who, z); LDX_ARG_PTR(who, zc);
    LDX_ARG_REQUIRE(n_hap != 0u && n_hap % 2u == 0u, "%s: n_hap %u must be even and non-zero (haplotypes 2a and 2a + 1 are individual a)",
                    who, n_hap);
    if (n_hap > LDX_MAX_HAPS) {
        set_error("%s: n_hap %u > LDX_MAX_HAPS", who, n_hap);
        return LDX_E_UNSUPPORTED;
    }
    LDX_ARG_REQUIRE(n_snps != 0u, "%s: n_snps is 0", who);
    if (const int rc = geno_cols_ok(who, k, ld_u, "ld_u", ld_z, "ld_z")) return rc;
    if (const int rc = plane_check(who, nullptr, n_snps, n_hap)) return rc;
    geno::RevArgs p{};
    p.alt = (const uint4 *)alt, p.ref = (const uint4 *)ref, p.keep = keep;
    p.n_snps = n_snps, p.n_ind = n_hap / 2u, p.hap_chunks = n_chunks(n_hap);
    p.u = u, p.ld_u = ld_u, p.k = k;
    p.z = (long long *)z, p.zc = (long long *)zc, p.ld_z = ld_z;
    for (p.col0 = 0u; p.col0 < k; p.col0 += geno::kGroupCols) {   // one launch per group of 32 columns
        const uint32_t tiles = (k - p.col0 < geno::kGroupCols ? k - p.col0 + geno::kTileCols - 1u : geno::kGroupCols) / geno::kTileCols;
        geno::launch_rmatmul(tiles, n_slabs(n_snps), (hipStream_t)stream, p);
        LDX_HIP(hipGetLastError());
    }
    return LDX_OK;
}

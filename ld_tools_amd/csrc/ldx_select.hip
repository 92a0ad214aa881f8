// Sample and SNP subsets of a packed panel, on the device: dst(i, h) = src(snp_idx[i], hap_idx[h]) in both bit planes,
// straight from the tiled planes -- the allele codes never exist again.  What the reference answers by building the genotype
// lists of another sample selection from the VCF (get_sample_names.py, ld_triangle.py:160-186), and what a haplotype
// bootstrap needs (indices may repeat).
#include "ldx_common.h"

namespace ldx {

constexpr uint32_t kSelRows = 32u;                       // destination rows per workgroup
constexpr uint32_t kSelThreads = 512u;
constexpr uint32_t kSelWaves = kSelThreads / 64u;
constexpr uint32_t kSelLdsRows = 2u * kSelRows;          // (plane, row): one per lane of a wave

// words of one staged row: its chunks, then ONE zero word.  The word makes the stride odd, so the 32 rows of a plane reading
// one word column hit 32 banks; and it is where a haplotype index past the source reads its zero bit.
__host__ __device__ inline uint32_t sel_stride(uint32_t nch_src) { return nch_src * 4u + 1u; }
__host__ __device__ inline size_t sel_lds_bytes(uint32_t nch_src)
{
    return ((size_t)kSelLdsRows * sel_stride(nch_src) + kSelThreads) * sizeof(uint32_t);
}

// bit (h % 32) of a staged word: one v_bfe_u32 (its offset operand reads the low five bits of h)
__device__ __forceinline__ uint32_t sel_bit(uint32_t word, uint32_t h) { return __builtin_amdgcn_ubfe(word, h, 1u); }

// One workgroup per 32 destination rows (a quarter of a slab), all their chunks, both planes.
//   stage   the 32 source rows, 16-byte group by group, into LDS: row (plane, r) at word (32 plane + r) * stride.  An item is
//           (plane, chunk, row) with the row fastest: without a SNP selection 32 lanes read 512 contiguous bytes.  A row past
//           n_snps_dst (the slab's pad rows) or with an index past the source is staged as zero bits.
//   gather  lane = (plane, row), so the destination haplotype -- and with it the source haplotype, its word column and its
//           shift -- is the same for the 64 lanes of a wave: the indices arrive by scalar loads, a bit costs one ds_read_b32
//           (conflict-free: odd stride) and three vector instructions.  A wave builds the four words of one destination chunk
//           and stores them as ONE 16-byte group per lane; the 32 lanes of a plane store 512 contiguous bytes.
//   counts  popcounts of the words just built, summed over the workgroup's waves through LDS: the workgroup owns its rows,
//           so the counts are plain stores (pad rows: 0).
// Every group of both destination planes and every count word is written; nothing is read from the destination.
__global__ void __launch_bounds__(kSelThreads) panel_select_kernel(
    const uint4 *__restrict__ alt_src, const uint4 *__restrict__ ref_src, uint32_t n_snps_src, uint32_t n_hap_src,
    uint32_t nch_src, const uint32_t *__restrict__ snp_idx, uint32_t n_snps_dst, const uint32_t *__restrict__ hap_idx,
    uint32_t n_hap_dst, uint32_t nch_dst, uint4 *__restrict__ alt_dst, uint4 *__restrict__ ref_dst,
    uint32_t *__restrict__ acnt, uint32_t *__restrict__ rcnt)
{
    extern __shared__ uint32_t sel_lds[];
    const uint32_t stride = sel_stride(nch_src);
    uint32_t *cnts = sel_lds + kSelLdsRows * stride;     // [wave][lane]
    const uint32_t t = threadIdx.x;
    const uint32_t row0 = blockIdx.x * kSelRows;
    const uint32_t planes = ref_src ? 2u : 1u;

    {   // stage: this thread's items all belong to row r (kSelThreads is a multiple of 32)
        const uint32_t r = t & 31u, i = row0 + r;
        uint32_t si = 0xFFFFFFFFu;
        if (i < n_snps_dst) si = snp_idx ? snp_idx[i] : i;
        const bool live = si < n_snps_src;
        const size_t sbase = live ? (size_t)(si / kSlab) * nch_src * kSlab + si % kSlab : 0;
        const uint32_t n_pc = planes * nch_src;          // (plane, chunk) pairs
#pragma unroll 4
        for (uint32_t pc = t >> 5; pc < n_pc; pc += kSelThreads / 32u) {
            const uint32_t plane = pc >= nch_src ? 1u : 0u, c = pc - plane * nch_src;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (live) v = (plane ? ref_src : alt_src)[sbase + (size_t)c * kSlab];
            uint32_t *d = sel_lds + (plane * kSelRows + r) * stride + c * 4u;
            d[0] = v.x;
            d[1] = v.y;
            d[2] = v.z;
            d[3] = v.w;
        }
        if (t < kSelLdsRows) sel_lds[t * stride + nch_src * 4u] = 0u;
    }
    block_sync();

    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63u;
    const uint32_t plane = lane >> 5, r = lane & 31u;
    const bool active = plane < planes;
    const uint32_t *rowp = sel_lds + lane * stride;      // (32 plane + r) * stride
    const uint32_t zero_at = nch_src * 128u;             // bit 0 of the row's zero word
    const uint32_t slab = row0 / kSlab, rin = row0 % kSlab + r;
    uint4 *dst = plane ? ref_dst : alt_dst;
    uint32_t cnt = 0;
    if (active) {
        for (uint32_t c = wave; c < nch_dst; c += kSelWaves) {
            uint32_t w[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t d0 = c * 128u + k * 32u;
                uint32_t word = 0;
                if (!hap_idx) {                          // identity: n_hap_dst == n_hap_src, the source's pad bits are zero
                    word = rowp[c * 4u + k];
                } else if (d0 + 32u <= n_hap_dst) {
#pragma unroll
                    for (uint32_t b = 0; b < 32u; ++b) {
                        uint32_t h = hap_idx[d0 + b];
                        h = h < n_hap_src ? h : zero_at;
                        word |= sel_bit(rowp[h >> 5], h) << b;
                    }
                } else {                                 // the ragged last word; words past n_hap_dst stay zero
                    for (uint32_t b = 0; d0 + b < n_hap_dst; ++b) {
                        uint32_t h = hap_idx[d0 + b];
                        h = h < n_hap_src ? h : zero_at;
                        word |= sel_bit(rowp[h >> 5], h) << b;
                    }
                }
                w[k] = word;
                cnt += __builtin_popcount(word);
            }
            dst[((size_t)slab * nch_dst + c) * kSlab + rin] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    cnts[t] = cnt;
    block_sync();
    if (t < 64u && active) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kSelWaves; ++k) sum += cnts[k * 64u + t];
        (plane ? rcnt : acnt)[row0 + r] = sum;
    }
}

static bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}

}  // namespace ldx

using namespace ldx;

extern "C" int ldx_panel_select_dev(const void *alt_src, const void *ref_src, uint32_t n_snps_src, uint32_t n_hap_src,
                                    const uint32_t *snp_idx, uint32_t n_snps_dst, const uint32_t *hap_idx,
                                    uint32_t n_hap_dst, void *alt_dst, void *ref_dst, uint32_t *acnt_dst,
                                    uint32_t *rcnt_dst, void *stream)
{
    LDX_REQUIRE(alt_src && alt_dst && acnt_dst, "alt_src, alt_dst and acnt_dst must be non-null");
    LDX_REQUIRE((ref_src == nullptr) == (ref_dst == nullptr) && (ref_dst == nullptr) == (rcnt_dst == nullptr),
                "ref_src, ref_dst and rcnt_dst must be given together");
    LDX_REQUIRE(n_snps_src > 0 && n_snps_dst > 0, "bad shape");
    if (n_hap_src < 1 || n_hap_src > LDX_MAX_HAPS || n_hap_dst < 1 || n_hap_dst > LDX_MAX_HAPS) {
        set_error("%s: n_hap_src=%u / n_hap_dst=%u outside 1..%u", __func__, n_hap_src, n_hap_dst, LDX_MAX_HAPS);
        return LDX_E_UNSUPPORTED;
    }
    LDX_REQUIRE(snp_idx || n_snps_dst == n_snps_src, "snp_idx = NULL (identity) needs n_snps_dst == n_snps_src");
    LDX_REQUIRE(hap_idx || n_hap_dst == n_hap_src, "hap_idx = NULL (identity) needs n_hap_dst == n_hap_src");
    const size_t pb_src = ldx_plane_bytes(n_snps_src, n_hap_src), pb_dst = ldx_plane_bytes(n_snps_dst, n_hap_dst);
    const void *srcs[2] = {alt_src, ref_src};
    const void *dsts[2] = {alt_dst, ref_dst};
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            LDX_REQUIRE(!overlap(srcs[a], pb_src, dsts[b], pb_dst), "source and destination planes overlap");
    LDX_REQUIRE(!overlap(alt_dst, pb_dst, ref_dst, pb_dst), "destination planes overlap");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nch_src = n_chunks(n_hap_src), nch_dst = n_chunks(n_hap_dst);
    const size_t lds = sel_lds_bytes(nch_src);
    if (lds > 65536u)   // > 64 KiB of dynamic LDS needs the opt-in attribute
        LDX_HIP(hipFuncSetAttribute((const void *)panel_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    panel_select_kernel<<<ldx_padded_snps(n_snps_dst) / kSelRows, kSelThreads, lds, s>>>(
        (const uint4 *)alt_src, (const uint4 *)ref_src, n_snps_src, n_hap_src, nch_src, snp_idx, n_snps_dst, hap_idx,
        n_hap_dst, nch_dst, (uint4 *)alt_dst, (uint4 *)ref_dst, acnt_dst, rcnt_dst);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

// PLINK .bed rows <-> the tiled 2-plane panel, on the device (include/ldx.h, "PLINK .bed ingest and export").  A SNP-major
// .bed row holds individual k as the 2-bit field at bits 2 (k % 4), 2 (k % 4) + 1 of byte k / 4; a panel row holds the
// individual's two haplotypes at bits 2k % 32, 2k % 32 + 1 of a plane word.  So 4 source bytes ARE one destination word of
// each plane up to a few bitwise operations, and the work is the relayout from unaligned rows into the tiled planes (and back).
#include "ldx_common.h"

namespace ldx {

constexpr uint32_t kBedRows = 32u;                        // panel rows per workgroup (a quarter of a slab)
constexpr uint32_t kBedThreads = 512u;
constexpr uint32_t kBedWaves = kBedThreads / 64u;
constexpr uint32_t kEven = 0x55555555u;
constexpr uint32_t kBedMissing = 0x55555555u;             // sixteen fields 01
// The LDS / global switch of the gather: a workgroup stages its 32 source rows whole while they fit 64 KiB of LDS (the size a
// launch gets without an opt-in, two workgroups per CU), which is a source of up to kBedLdsInd individuals; a wider source --
// a biobank row is 125 KB -- is gathered from global memory through the index, one byte load per field.
constexpr uint32_t kBedLdsWords = 478u;                   // source words per staged row, at most
constexpr uint32_t kBedLdsInd = kBedLdsWords * 16u;       // 7648 individuals

enum BedMode { kBedIdentity = 0, kBedGatherLds = 1, kBedGatherGlobal = 2 };

// words of one staged row: its source words, ONE word of missing fields (where an index past the source reads), and one more
// where that sum is even: an odd stride, so that 32 rows reading one word column hit 32 banks
__host__ __device__ constexpr uint32_t bed_stride(uint32_t nwords) { return (nwords + 1u) | 1u; }
__host__ __device__ constexpr size_t bed_lds_bytes(uint32_t nwords, bool staged)
{
    return ((staged ? (size_t)kBedRows * bed_stride(nwords) : 0u) + 2u * kBedThreads) * sizeof(uint32_t);
}

// bytes 4 wd .. 4 wd + 3 of a row of nbytes bytes at ANY address, as one word: the aligned dword that holds byte 4 wd and,
// where the row has bytes in it, the next one, through one v_alignbyte_b32.  Only dwords that hold a byte of the row are
// loaded (an aligned dword never straddles a page, so its bytes beside the row are readable); what those bytes and the bytes
// past the row's end put into the word is masked by the caller.  Requires 4 wd < nbytes.
__device__ __forceinline__ uint32_t bed_load_word(const uint8_t *row, uint32_t nbytes, uint32_t wd)
{
    const uint32_t p = (uint32_t)reinterpret_cast<uintptr_t>(row) & 3u;   // the byte phase: one per row
    const uint32_t *aw = reinterpret_cast<const uint32_t *>(row - p) + wd;
    const uint32_t lo = aw[0];
    uint32_t hi = 0u;
    if (p != 0u && 4u * wd + 4u - p < nbytes) hi = aw[1];   // near the row's end: only if a byte of the row lives there
    return __builtin_amdgcn_alignbyte(hi, lo, p);
}

static_assert(bed_lds_bytes(kBedLdsWords, true) <= 65536u, "the staged rows and the count words must fit 64 KiB");
static_assert(kBedLdsWords * 16u >= LDX_MAX_HAPS / 2u, "the identity form stages every row it can be given");

// sixteen fields -> the sixteen individuals' bits of both planes.  lo / hi: the fields' low / high bits on the even positions.
//   ALT = A1:  alt = {00, 10 | 00}   ref = {11 | 10, 11}      ALT = A2:  alt = {10, 11 | 11}   ref = {00 | 00, 10}
// (haplotype 2k | haplotype 2k + 1; a het puts ALT on 2k; 01, a missing call, is in neither plane)
__device__ __forceinline__ void bed_planes(uint32_t w, bool a2, uint32_t &alt, uint32_t &ref)
{
    const uint32_t lo = w & kEven, hi = (w >> 1) & kEven;
    const uint32_t e = hi, f = lo & hi, g = ~lo & kEven, h = ~lo & ~hi & kEven;
    alt = a2 ? (e | (f << 1)) : (g | (h << 1));
    ref = a2 ? (h | (g << 1)) : (f | (e << 1));
}

// the valid haplotype bits of plane word k of a row of n_hap haplotypes
__device__ __forceinline__ uint32_t hap_mask(uint32_t n_hap, uint32_t k)
{
    const uint32_t at = k * 32u;
    if (at >= n_hap) return 0u;
    const uint32_t rem = n_hap - at;
    return rem >= 32u ? 0xFFFFFFFFu : (1u << rem) - 1u;
}

// One workgroup per 32 destination rows, all their chunks, both planes; thread t works for row t % 32 throughout.
//   stage    (identity, LDS gather) the 32 source rows into LDS word by word, a wave per row and a lane per word: 256
//            contiguous bytes per load instruction at any byte phase (bed_load_word).
//   identity a thread builds whole chunks: four LDS words -> the four words of both planes -> one 16-byte store per plane;
//            the 32 lanes of a row group store 512 contiguous bytes.
//   gather   lane = (half, row): a lane builds words 2 half, 2 half + 1 of a chunk, so the destination individual -- and with
//            it the source index, its word and its shift -- is one of two wave-uniform values: the indices arrive by scalar
//            loads.  A field costs one ds_read_b32 (conflict-free: odd stride) or, past the LDS budget, one byte load; the
//            gathered fields form a .bed word and take the identity's bit operations.  A lane stores 8 bytes per plane.
//   counts   popcounts of the words just built, summed over the threads of a row through LDS: the workgroup owns its rows,
//            so the counts are plain stores (pad rows: 0).
// Every group of both planes and every count word of the slabs the launch owns is written; the destination is never read.
template <int kMode>
__global__ void __launch_bounds__(kBedThreads) bed_unpack_kernel(
    const uint8_t *__restrict__ bed, size_t row_bytes, uint32_t n_ind_src, uint32_t n_rows, const uint32_t *__restrict__ ind_idx,
    uint32_t n_ind_dst, uint32_t a2, uint32_t row0, uint32_t nch_dst, uint4 *__restrict__ alt_dst, uint4 *__restrict__ ref_dst,
    uint32_t *__restrict__ acnt, uint32_t *__restrict__ rcnt)
{
    extern __shared__ uint32_t bed_lds[];
    const uint32_t nbytes = (n_ind_src + 3u) / 4u, nwords = (nbytes + 3u) / 4u;
    const uint32_t stride = bed_stride(nwords);
    uint32_t *cnts = bed_lds + (kMode == kBedGatherGlobal ? 0u : kBedRows * stride);   // [plane][thread]
    const uint32_t t = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63u;
    const uint32_t local0 = blockIdx.x * kBedRows;       // first row of the workgroup, counted from row0
    const uint32_t n_hap_dst = 2u * n_ind_dst;

    if (kMode != kBedGatherGlobal) {
        for (uint32_t r = wave; r < kBedRows; r += kBedWaves) {
            uint32_t *d = bed_lds + r * stride;
            if (local0 + r < n_rows) {                   // wave-uniform
                const uint8_t *src = bed + (size_t)(local0 + r) * row_bytes;
                for (uint32_t wd = lane; wd < nwords; wd += 64u) d[wd] = bed_load_word(src, nbytes, wd);
            }
            if (lane == 0) d[nwords] = kBedMissing;
        }
        block_sync();
    }

    const uint32_t r = t & 31u;
    const bool live = local0 + r < n_rows;               // else a pad row of the last slab: zero bits
    const uint32_t *rowp = bed_lds + r * stride;
    const uint32_t prow = row0 + local0 + r, slab = prow / kSlab, rin = prow % kSlab;
    uint32_t ca = 0, cr = 0;
    if (kMode == kBedIdentity) {
        for (uint32_t c = t >> 5; c < nch_dst; c += kBedThreads / 32u) {
            uint32_t a[4], b[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t wd = c * 4u + k;
                const uint32_t m = live ? hap_mask(n_hap_dst, wd) : 0u;
                const uint32_t w = wd < nwords ? rowp[wd] : 0u;
                bed_planes(w, a2 != 0u, a[k], b[k]);
                a[k] &= m;
                b[k] &= m;
                ca += __builtin_popcount(a[k]);
                cr += __builtin_popcount(b[k]);
            }
            const size_t at = ((size_t)slab * nch_dst + c) * kSlab + rin;
            alt_dst[at] = make_uint4(a[0], a[1], a[2], a[3]);
            ref_dst[at] = make_uint4(b[0], b[1], b[2], b[3]);
        }
    } else {
        const uint32_t half = lane >> 5;
        const uint32_t miss_at = nwords * 16u;           // the first field of the staged row's missing word
        const uint8_t *grow = bed + (size_t)(live ? local0 + r : 0u) * row_bytes;
        for (uint32_t c = wave; c < nch_dst; c += kBedWaves) {
            uint32_t a[2], b[2];
#pragma unroll
            for (uint32_t k = 0; k < 2u; ++k) {
                const uint32_t d0 = c * 64u + k * 16u;   // first destination individual of word k of half 0; half 1: + 32
                uint32_t w = 0u;
                if (d0 < n_ind_dst) {                    // wave-uniform (half 1's words lie further out: masked below)
#pragma unroll
                    for (uint32_t f = 0; f < 16u; ++f) {
                        const uint32_t i0 = d0 + f, i1 = d0 + 32u + f;
                        const uint32_t h0 = i0 < n_ind_dst ? ind_idx[i0] : n_ind_src;   // scalar loads
                        const uint32_t h1 = i1 < n_ind_dst ? ind_idx[i1] : n_ind_src;
                        const uint32_t h = half ? h1 : h0;
                        uint32_t field;
                        if (kMode == kBedGatherLds) {
                            const uint32_t hh = h < n_ind_src ? h : miss_at;
                            field = __builtin_amdgcn_ubfe(rowp[hh >> 4], (hh & 15u) * 2u, 2u);
                        } else {
                            field = 1u;                  // an index past the source: a missing call
                            if (h < n_ind_src && live) field = ((uint32_t)grow[h >> 2] >> ((h & 3u) * 2u)) & 3u;
                        }
                        w |= field << (2u * f);
                    }
                }
                const uint32_t m = live ? hap_mask(n_hap_dst, c * 4u + half * 2u + k) : 0u;
                bed_planes(w, a2 != 0u, a[k], b[k]);
                a[k] &= m;
                b[k] &= m;
                ca += __builtin_popcount(a[k]);
                cr += __builtin_popcount(b[k]);
            }
            const size_t at = (((size_t)slab * nch_dst + c) * kSlab + rin) * 2u + half;
            reinterpret_cast<uint2 *>(alt_dst)[at] = make_uint2(a[0], a[1]);
            reinterpret_cast<uint2 *>(ref_dst)[at] = make_uint2(b[0], b[1]);
        }
    }
    cnts[t] = ca;
    cnts[kBedThreads + t] = cr;
    block_sync();
    if (t < 64u) {
        const uint32_t plane = t >> 5;
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kBedThreads / 32u; ++k) sum += cnts[plane * kBedThreads + k * 32u + r];
        (plane ? rcnt : acnt)[prow] = sum;
    }
}

// sixteen individuals of both planes -> their sixteen fields.  AA / RR: both haplotypes ALT / REF; HET: one of each in either
// order; everything else is a missing call (01).  ALT = A1: AA -> 00, HET -> 10, RR -> 11; ALT = A2: AA and RR swapped.
__device__ __forceinline__ uint32_t bed_fields(uint32_t alt, uint32_t ref, bool a2)
{
    const uint32_t a0 = alt & kEven, a1 = (alt >> 1) & kEven, r0 = ref & kEven, r1 = (ref >> 1) & kEven;
    const uint32_t aa = a0 & a1, rr = r0 & r1, het = (a0 & r1) | (r0 & a1);
    const uint32_t zero = a2 ? rr : aa, three = a2 ? aa : rr;   // the homozygotes written 00 and 11
    const uint32_t lo = kEven & ~(zero | het), hi = het | three;
    return lo | (hi << 1);
}

constexpr uint32_t kPackChunks = 16u;                     // chunks (256 .bed bytes per row) per workgroup

// One workgroup per 32 panel rows x 16 chunks.  load: thread = (row, chunk) with the row fastest -- a 16-byte group of each
// plane per thread, 512 contiguous bytes per 32 lanes --, the four .bed words go to LDS (odd stride).  store: a wave per row, a
// lane per word: 256 contiguous bytes per row; a word inside the row at a 4-byte aligned address is one dword store, the
// others (an unaligned row, the row's last bytes) go byte by byte.  Bytes past ceil(n_ind / 4) are not touched.
__global__ void __launch_bounds__(kBedThreads) bed_pack_kernel(const uint4 *__restrict__ alt, const uint4 *__restrict__ ref,
                                                               uint32_t n_ind, uint32_t nch, uint32_t row0, uint32_t n_rows,
                                                               uint8_t *__restrict__ bed, size_t row_bytes, uint32_t a2)
{
    __shared__ uint32_t words[kBedRows][kPackChunks * 4u + 1u];
    const uint32_t t = threadIdx.x;
    const uint32_t local0 = blockIdx.x * kBedRows, c0 = blockIdx.y * kPackChunks;
    {
        const uint32_t r = t & 31u, cc = t >> 5, c = c0 + cc;
        if (local0 + r < n_rows && c < nch) {
            const uint32_t prow = row0 + local0 + r;
            const size_t at = ((size_t)(prow / kSlab) * nch + c) * kSlab + prow % kSlab;
            const uint4 va = alt[at], vr = ref[at];
            const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wr[4] = {vr.x, vr.y, vr.z, vr.w};
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t first = (c * 4u + k) * 16u;   // the word's first individual
                uint32_t w = bed_fields(wa[k], wr[k], a2 != 0u);
                if (first >= n_ind) w = 0u;
                else if (n_ind - first < 16u) w &= (1u << (2u * (n_ind - first))) - 1u;   // pad bits: zero
                words[r][cc * 4u + k] = w;
            }
        }
    }
    block_sync();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63u;
    const uint32_t nbytes = (n_ind + 3u) / 4u;
    const uint32_t b0 = c0 * 16u + lane * 4u;             // the lane's first byte in the row
    for (uint32_t r = wave; r < kBedRows; r += kBedWaves) {
        if (local0 + r >= n_rows || b0 >= nbytes) continue;
        uint8_t *dst = bed + (size_t)(local0 + r) * row_bytes + b0;
        const uint32_t w = words[r][lane];
        if (b0 + 4u <= nbytes && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0u) {
            *reinterpret_cast<uint32_t *>(dst) = w;
        } else {
            for (uint32_t k = 0; k < 4u && b0 + k < nbytes; ++k) dst[k] = (uint8_t)(w >> (8u * k));
        }
    }
}

}  // namespace ldx

using namespace ldx;

extern "C" int ldx_bed_unpack_dev(const uint8_t *bed, size_t row_bytes, uint32_t n_ind_src, uint32_t n_rows,
                                  const uint32_t *ind_idx, uint32_t n_ind_dst, int alt_is_a2, uint32_t row0,
                                  uint32_t n_snps_panel, void *alt, void *ref, uint32_t *acnt, uint32_t *rcnt, void *stream)
{
    LDX_REQUIRE(bed && alt && ref && acnt && rcnt, "bed, alt, ref, acnt and rcnt must be non-null");
    LDX_REQUIRE(n_ind_src > 0 && n_ind_dst > 0 && n_rows > 0 && n_snps_panel > 0, "bad shape");
    LDX_REQUIRE(row_bytes >= ((size_t)n_ind_src + 3u) / 4u, "row_bytes is below ceil(n_ind_src / 4)");
    LDX_REQUIRE(alt_is_a2 == 0 || alt_is_a2 == 1, "alt_is_a2 must be 0 or 1");
    if (n_ind_dst > LDX_MAX_HAPS / 2u) {
        set_error("%s: n_ind_dst=%u: more than %u haplotypes", __func__, n_ind_dst, LDX_MAX_HAPS);
        return LDX_E_UNSUPPORTED;
    }
    LDX_REQUIRE(ind_idx || n_ind_dst == n_ind_src, "ind_idx = NULL (identity) needs n_ind_dst == n_ind_src");
    LDX_REQUIRE(row0 % kSlab == 0u, "row0 must be a multiple of 128 (a call owns whole slabs)");
    LDX_REQUIRE(row0 < n_snps_panel && n_rows <= n_snps_panel - row0, "rows row0 .. row0 + n_rows - 1 leave the panel");
    LDX_REQUIRE(n_rows % kSlab == 0u || row0 + n_rows == n_snps_panel,
                "n_rows must be a multiple of 128 unless the call reaches n_snps_panel");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nch = n_chunks(2u * n_ind_dst);
    const uint32_t nwords = (n_ind_src + 15u) / 16u;
    const uint32_t grid = n_slabs(n_rows) * (kSlab / kBedRows);
    uint4 *a = (uint4 *)alt, *r = (uint4 *)ref;
    if (!ind_idx)
        bed_unpack_kernel<kBedIdentity><<<grid, kBedThreads, bed_lds_bytes(nwords, true), s>>>(
            bed, row_bytes, n_ind_src, n_rows, nullptr, n_ind_dst, (uint32_t)alt_is_a2, row0, nch, a, r, acnt, rcnt);
    else if (n_ind_src <= kBedLdsInd)
        bed_unpack_kernel<kBedGatherLds><<<grid, kBedThreads, bed_lds_bytes(nwords, true), s>>>(
            bed, row_bytes, n_ind_src, n_rows, ind_idx, n_ind_dst, (uint32_t)alt_is_a2, row0, nch, a, r, acnt, rcnt);
    else
        bed_unpack_kernel<kBedGatherGlobal><<<grid, kBedThreads, bed_lds_bytes(nwords, false), s>>>(
            bed, row_bytes, n_ind_src, n_rows, ind_idx, n_ind_dst, (uint32_t)alt_is_a2, row0, nch, a, r, acnt, rcnt);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_bed_pack_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, uint32_t row0,
                                uint32_t n_rows, uint8_t *bed, size_t row_bytes, int alt_is_a2, void *stream)
{
    LDX_REQUIRE(alt && ref && bed, "alt, ref and bed must be non-null");
    LDX_REQUIRE(n_snps > 0 && n_hap > 0 && n_rows > 0, "bad shape");
    LDX_REQUIRE(n_hap % 2u == 0u, "n_hap is odd (a .bed field is an individual: haplotypes 2k and 2k + 1)");
    if (n_hap > LDX_MAX_HAPS) {
        set_error("%s: n_hap=%u above %u", __func__, n_hap, LDX_MAX_HAPS);
        return LDX_E_UNSUPPORTED;
    }
    LDX_REQUIRE(row0 < n_snps && n_rows <= n_snps - row0, "rows row0 .. row0 + n_rows - 1 leave the panel");
    LDX_REQUIRE(row_bytes >= ((size_t)n_hap / 2u + 3u) / 4u, "row_bytes is below ceil(n_ind / 4)");
    LDX_REQUIRE(alt_is_a2 == 0 || alt_is_a2 == 1, "alt_is_a2 must be 0 or 1");
    const uint32_t nch = n_chunks(n_hap);
    const dim3 grid((n_rows + kBedRows - 1u) / kBedRows, (nch + kPackChunks - 1u) / kPackChunks);
    bed_pack_kernel<<<grid, kBedThreads, 0, (hipStream_t)stream>>>((const uint4 *)alt, (const uint4 *)ref, n_hap / 2u, nch, row0,
                                                                   n_rows, bed, row_bytes, (uint32_t)alt_is_a2);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

/*
 * ldx.h -- C ABI of the MI355X (gfx950) pairwise-LD engine.
 *
 * Drop-in boundary for the hot path of PlatonB/ld-tools: everything the reference does in
 * backend/calc_ld.py:3-99, batched over the pair loops that drive it
 * (ld_triangle.py:133-230, ld_area.py:152-276).  The reference is pure Python and has no FFI
 * of its own; the binding a maintainer adds is the ctypes stub shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ types, no exceptions cross the boundary.
 *   - every function returns 0 on success or a negative LDX_E_* code; ldx_last_error() gives
 *     the message of the last failure on the calling thread.
 *   - `_dev` entry points take DEVICE pointers (e.g. torch tensors' data_ptr()) and a
 *     hipStream_t passed as void* (NULL = the null stream).  They enqueue work and return;
 *     they never allocate, free or synchronise.  The caller owns every buffer.
 *   - `_host` entry points take HOST pointers, run the same kernels on the current device and
 *     synchronise before returning.  There is no CPU fallback anywhere in this library.
 *
 * Packed panel layout in HBM ("tiled plane")
 *   A plane holds one bit per (SNP, haplotype).  Rows are grouped into slabs of LDX_SLAB_ROWS
 *   SNPs; the haplotype axis is cut into chunks of 128 haplotypes (16 bytes), allocated in pairs
 *   (n_chunks = 2 * ceil(n_hap / 256): the matrix kernel consumes two chunks per K-block).  Element
 *   (slab s, chunk c, row r) is the 16-byte group at byte offset
 *       ((s * n_chunks + c) * LDX_SLAB_ROWS + r) * 16,
 *   bit (h % 128) of it (little-endian, 32-bit words) being haplotype h = 128*c + (h % 128) of
 *   SNP 128*s + r.  One slab is therefore a contiguous n_chunks*2 KiB image that a workgroup
 *   copies linearly into LDS, and 8 consecutive SNPs of one chunk are 128 contiguous bytes that a
 *   wavefront fetches with scalar loads.  Pad bits and pad rows are zero.
 *   The `alt` plane has bit = 1 where the allele code is 1, the `ref` plane where it is 0
 *   (calc_ld.py:37-40 counts them separately; any other code is in neither plane).
 */
#ifndef LDX_H
#define LDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDX_VERSION 102            /* 0.1.2: ldx_triangle_ex_dev takes the pass scheduler's workspace (the library keeps no per-stream
                                      state); one-measure cell formats LDX_OUT_K16_RSQ / LDX_OUT_K16_DPRIME */
#define LDX_SLAB_ROWS 128u         /* SNP rows per slab == SNP columns per j-tile */
#define LDX_GROUP_ROWS 8u          /* SNP rows a wavefront pairs against one j-tile per unit */
#define LDX_CHUNK_HAPS 128u        /* haplotypes per 16-byte chunk */
#define LDX_UNIT_PAIRS (LDX_SLAB_ROWS * LDX_GROUP_ROWS)   /* 1024 result cells per unit */
/* Cell order INSIDE a unit (8 rows x 128 columns), r8 = row % 8, c = column % 128: rows one after the other (128 cells
 * each).  Inside a row the order follows what ONE lane of the matrix kernel holds -- a 32 x 32 MFMA tile puts column l
 * of each of the four column tiles into lane l, i.e. the four columns {c0, c0 + 32, c0 + 64, c0 + 96} -- so that the lane
 * writes them with 16-byte stores and a wave's store instruction covers whole contiguous runs:
 *   4-byte cells (ldx_k16, ldx_r32):  the lane's four cells are adjacent: element 4 * (c % 32) + c / 32  (one store per row);
 *   8-byte cells (ldx_ld32): the lane's cells of column tiles (0, 1) and (2, 3) are adjacent pairs:
 *                            element 64 * (c / 64) + 2 * (c % 32) + (c / 32) % 2              (two stores per row).
 * Why: the kernel's result stream was bound by the number of store INSTRUCTIONS a CU can issue, not by bytes (round 4:
 * no stores at all -19 % kernel time at 50 000 x 1008, eight 4-byte stores -> two 16-byte stores per step -12 %;
 * tools/probes/wrbw.hip, profiles/r04/store_issue_*.log).  Side outputs of a launch (n11, unrounded values) use the order
 * of that launch's cell format.  Every producer and consumer of strip output goes through these macros
 * (ld_tools_amd/_lib.py: cell_offset).  Round 3's column-quad-major attempt (quads of ADJACENT columns, which needed the
 * MFMA operand roles swapped) was slower; this order needs no change to the arithmetic. */
#define LDX_CELL_OFFSET4(r8, c) ((r8) * LDX_SLAB_ROWS + (((c) & 31u) << 2) + ((c) >> 5))
#define LDX_CELL_OFFSET8(r8, c) ((r8) * LDX_SLAB_ROWS + (((c) >> 6) << 6) + (((c) & 31u) << 1) + (((c) >> 5) & 1u))
#define LDX_CELL_OFFSET(out_format, r8, c) ((out_format) == LDX_OUT_LD32 ? LDX_CELL_OFFSET8(r8, c) : LDX_CELL_OFFSET4(r8, c))
#define LDX_MAX_HAPS 10240u        /* one j-tile (128 rows, all chunks) must fit 160 KiB of LDS */

/* error codes */
#define LDX_OK 0
#define LDX_E_ARG (-1)             /* bad argument (null pointer, size out of range, ...) */
#define LDX_E_HIP (-2)             /* a HIP runtime call failed; see ldx_last_error() */
#define LDX_E_UNSUPPORTED (-3)     /* n_hap > LDX_MAX_HAPS, wrong device architecture, ... */
#define LDX_E_OVERFLOW (-4)        /* hit buffer too small (ldx_area_*): count is still returned */

/* per-pair flag bits: which results are the reference's *int* 0 rather than a float */
#define LDX_FLAG_DPRIME_INT0 1u    /* calc_ld.py:68-69,75-76 (ZeroDivisionError branch) */
#define LDX_FLAG_RSQ_INT0 2u       /* calc_ld.py:89-90 (unrounded d_prime == 0) */
#define LDX_FLAG_F32_SURE 0x80u     /* ldx_ld_from_counts_ex_dev only: the fp32 epilogue tier would keep this pair */

/* measures (ld_triangle -l / ld_area -l: ld_triangle_cli_en.py:52, ld_area_cli_en.py:50) */
#define LDX_MEASURE_RSQ 0
#define LDX_MEASURE_DPRIME 1

/* Result cells.  The reference returns round(r_square, 4) and round(d_prime, 4) (calc_ld.py:94-95), i.e. k / 10^4
 * for an integer k, or the *int* 0 in the degenerate branches.  Two cell formats carry (k, int-0 mark) per value:
 *   ldx_ld32 (8 bytes/pair): the float32 nearest to k / 10^4; int 0 is -0.0f (sign bit set), a float 0.0 is +0.0f.
 *            k = rint(value * 10^4) is exact while value < 1024 (float32 ulp below 10^-4).  Larger values -- they
 *            arise only with missing codes, where a + r < n lets the bound of D' vanish -- are stored as the quiet
 *            NaN LDX_LD32_BIG_BITS: fetch the exact value with ldx_ld_pairs_dev.
 *   ldx_k16  (4 bytes/pair): k itself in bits 0..14 of a uint16 (host: k / 10^4 in double IS Python's round(x, 4)),
 *            bit 15 set (LDX_K16_INT0) for the int 0; k >= 32767 (value >= 3.2767) is stored as LDX_K16_BIG: fetch
 *            the exact value with ldx_ld_pairs_dev.
 * str() of every value can be reproduced from either. */
typedef struct { float r_square; float d_prime; } ldx_ld32;
typedef struct { uint16_t r_square; uint16_t d_prime; } ldx_k16;
typedef struct { double r_square; double d_prime; } ldx_ld64;   /* unrounded, for parity checks */
#define LDX_LD32_BIG_BITS 0x7FC00B16u   /* ldx_ld32 value >= 1024: a quiet NaN with this payload */
#define LDX_K16_INT0 0x8000u
#define LDX_K16_BIG 0x7FFFu
#define LDX_OUT_LD32 0
#define LDX_OUT_K16 1
/* ONE measure per pair, 2 bytes (round 6): the r_square half or the d_prime half of ldx_k16 alone -- what a caller that writes
 * one measure needs (ld_triangle.py:223-230,344-360 fill and print ld_two_dim for the ONE measure -l names).  Same element
 * order as ldx_k16 (LDX_CELL_OFFSET4), same k / int-0 bit / escape.  The kernel skips the other value's arithmetic, margin
 * and bytes.  No side outputs (out_raw, out_n11) with these formats. */
typedef struct { uint16_t value; } ldx_k16one;
#define LDX_OUT_K16_RSQ 2
#define LDX_OUT_K16_DPRIME 3
/* Signed r, unrounded: ONE float32 per pair, the correlation of the two SNPs' ALT-allele indicators -- what fine-mapping,
 * colocalisation and summary-statistics imputation consume.  Same element order as ldx_k16 (LDX_CELL_OFFSET4).  With n = n_hap,
 * a / r = ALT / REF counts (missing codes count in n only) and n11 the exact alt/alt count:
 *     num = n * n11 - a_i * a_j                         (an exact integer, |num| < 2^31)
 *     cell = -0.0f                                      if a_i r_i == 0 or a_j r_j == 0 (the reference's degenerate SNPs:
 *                                                       its r^2 is the int 0 there, as in ldx_ld32)
 *     cell = float32 of num / sqrt(a_i r_i a_j r_j)     otherwise, within 4 float32 ulps of the exact value; +0.0f iff num == 0
 *     cell = +1.0f / -1.0f exactly                      when num^2 == a_i r_i a_j r_j (an exact duplicate / complement of a row without
 *                                                       missing codes): the fp64 arithmetic is within ~4 2^-53 of +-1, far inside half a
 *                                                       float32 ulp, so ldx_ld_neighbors_dev keeps the pair at r2_bound = 1.0f (s = 1.0f)
 *                                                       and drops it at the next float32 above 1
 * r > 0 when ALT alleles co-occur more often than independence predicts (D > 0); r^2 is the reference's unrounded r^2
 * (calc_ld.py:50,86-90), so with missing codes |r| may exceed 1.  Without missing codes r is the Pearson correlation of the
 * two 0/1 haplotype vectors.  Every kernel computes it with the same arithmetic: the cells are bit-identical across
 * paths.  No side outputs (out_raw, out_n11) with this format; ldx_triangle_r_block_dev turns the strips into a square. */
typedef struct { float r; } ldx_r32;
#define LDX_OUT_R32 4

/* one ld_area hit (ld_area.py:261-271): query/opposing SNP row indices and rounded values.  A record of
 * ldx_ld_neighbors_dev uses the same layout with other values: r_square holds the signed r cell, d_prime s = r *f32 r. */
typedef struct {
    uint32_t query;      /* row index of var_1 (the query) in the panel */
    uint32_t oppos;      /* row index of var_2 (the opposing variant) */
    float r_square;      /* as ldx_ld32 (neighbour lists: the signed r) */
    float d_prime;       /* (neighbour lists: s = r *f32 r) */
} ldx_hit;

/* ---- library / device ---------------------------------------------------------------- */
int ldx_version(void);
const char *ldx_last_error(void);
int ldx_device_count(void);                 /* number of visible HIP devices, <0 on error */
int ldx_device_arch(int device, char *buf, size_t buflen);   /* e.g. "gfx950" */

/* ---- geometry helpers (pure arithmetic, usable without a GPU) ------------------------- */
uint32_t ldx_n_slabs(uint32_t n_snps);                     /* ceil(n_snps / 128) */
uint32_t ldx_n_chunks(uint32_t n_hap);                     /* 2 * ceil(n_hap / 256): chunks come in pairs */
size_t ldx_plane_bytes(uint32_t n_snps, uint32_t n_hap);   /* bytes of one tiled plane */
uint32_t ldx_padded_snps(uint32_t n_snps);                 /* n_slabs * 128 */
/* Triangle work units.  Unit u of the strict lower triangle pairs the 8 rows of group g with the
 * 128 columns of j-tile t, u = t*G - 8*t*(t-1) + (g - 16*t), G = padded_snps/8, g >= 16*t.  Result
 * cell (row i, column j), i > j, lives at element u*1024 + LDX_CELL_OFFSET(format, i % 8, j % 128) of the strip
 * output, t = j/128, g = i/8 (ldx_triangle_cell_index does the arithmetic). */
uint64_t ldx_triangle_units(uint32_t n_snps);
uint64_t ldx_triangle_unit_of(uint32_t n_snps, uint32_t row, uint32_t col);  /* requires row > col */
uint64_t ldx_triangle_tile_base(uint32_t n_snps, uint32_t tile);             /* first unit of j-tile */
uint64_t ldx_triangle_cell_index(uint32_t n_snps, uint32_t row, uint32_t col, int out_format); /* element of cell (row > col) in the full strip output of that cell format (LDX_OUT_*) */

/* ---- packing: the genotype lists of ld_triangle.py:160-186 / ld_area.py:182-187,230-235 ---- */
/* codes: int8 [n_snps][ld_codes], 1 = ALT, 0 = REF, anything else = neither (None, 2nd ALT...).
 * alt/ref: tiled planes of ldx_plane_bytes(); ref may be NULL.  acnt/rcnt: uint32 [padded_snps]
 * = per-SNP counts of code 1 / code 0 (calc_ld.py:37-40); rcnt may be NULL iff ref is. */
int ldx_pack_codes_dev(const int8_t *codes, uint32_t n_snps, uint32_t n_hap, size_t ld_codes,
                       void *alt, void *ref, uint32_t *acnt, uint32_t *rcnt, void *stream);
/* row-major bit planes (uint32 words, W32 = ld_words per row, little-endian bit order) -> tiled */
int ldx_tile_plane_dev(const uint32_t *rowmajor, uint32_t n_snps, uint32_t n_hap, size_t ld_words,
                       void *tiled, uint32_t *cnt, void *stream);
/* per-SNP frequency vectors used by the epilogue: fa = a/n, fr = r/n, q = fa*fr (calc_ld.py:41-44,
 * and the first product of :87-88).  double [padded_snps] each. */
int ldx_snp_stats_dev(const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps, uint32_t n_hap,
                      double *fa, double *fr, double *q, void *stream);

/* round(a/n, 4) per SNP as a double: var_1/var_2_alt_freq of calc_ld.py:96-97 and the query's alt_freq of
 * ld_area.py:188-189.  freq4: double [n_snps]. */
int ldx_alt_freq4_dev(const uint32_t *acnt, uint32_t n_snps, uint32_t n_hap, double *freq4, void *stream);

/* ---- sample and SNP subsets of a packed panel: another answer to get_sample_names.py without the codes ---- */
/* dst(i, h) = src(snp_idx[i], hap_idx[h]) in both planes, i < n_snps_dst, h < n_hap_dst, written in the tiled layout of
 * ldx_plane_bytes(n_snps_dst, n_hap_dst) -- what ldx_pack_codes_dev would make of codes[snp_idx][:, hap_idx], byte for byte,
 * counts included, without the codes: a population or gender subset of a resident panel, a SNP subset, a haplotype
 * bootstrap.  Every operator works on the result as on any packed panel (ldx_snp_stats_dev gives its fa / fr / q).
 *   snp_idx: uint32 [n_snps_dst] source rows, or NULL = identity (then n_snps_dst == n_snps_src, else LDX_E_ARG);
 *   hap_idx: uint32 [n_hap_dst] source haplotypes, or NULL = identity (then n_hap_dst == n_hap_src, else LDX_E_ARG);
 *   indices come in ANY order and MAY REPEAT; n_hap_dst may exceed n_hap_src; n_hap_src and n_hap_dst both lie in
 *   1 .. LDX_MAX_HAPS (else LDX_E_UNSUPPORTED).
 * Out-of-range indices have a meaning (a _dev entry cannot report from inside the launch) and are never a stray read:
 *   a haplotype index >= n_hap_src is a MISSING CALL: zero bits in both planes at that destination haplotype (in n only);
 *   a SNP index >= n_snps_src is an ALL-MISSING ROW: zero bits in both planes, a = r = 0, a degenerate SNP.
 * The call writes EVERY byte of both destination planes (pad haplotypes and pad rows as zero bits) and EVERY word of
 * acnt_dst / rcnt_dst up to ldx_padded_snps(n_snps_dst) (pad rows 0): the caller zeroes nothing, and a launch into a used
 * buffer gives the same bytes.  The counts are popcounts of the bits just assembled, stored by the workgroup that owns the
 * rows: no atomics, no memset.
 * Source and destination must not overlap (checked on the plane extents: LDX_E_ARG).  ref_src, ref_dst and rcnt_dst are NULL
 * together (an ALT-only subset), as ref / rcnt of ldx_pack_codes_dev.  The source's pad bits must be zero, as every producer
 * in this library leaves them.  The call only enqueues ONE kernel on `stream`: no allocation, no synchronisation, no state. */
int ldx_panel_select_dev(const void *alt_src, const void *ref_src, uint32_t n_snps_src, uint32_t n_hap_src,
                         const uint32_t *snp_idx, uint32_t n_snps_dst, const uint32_t *hap_idx, uint32_t n_hap_dst,
                         void *alt_dst, void *ref_dst, uint32_t *acnt_dst, uint32_t *rcnt_dst, void *stream);

/* ---- PLINK .bed ingest and export: genotype calls straight from / to the file's own bytes ---- */
/* A SNP-major .bed row holds individual k as the 2-bit field at bits 2 (k % 4), 2 (k % 4) + 1 of byte k / 4, low bit first:
 * 00 = homozygous A1, 01 (low bit set) = missing, 10 = heterozygous, 11 = homozygous A2.  In the panel individual k owns
 * haplotypes 2k and 2k + 1.  With alt_is_a2 = 0 (ALT = A1, what PLINK and LDSC count) the codes are hom A1 -> (1, 1), het ->
 * (1, 0), hom A2 -> (0, 0), missing -> (2, 2): a het always puts the ALT allele on haplotype 2k (a .bed carries no phase);
 * alt_is_a2 = 1 swaps the two homozygotes.  ld_tools_amd/plink.py states the same on the host (bed_codes_host /
 * codes_bed_host), and both entries match it byte for byte.
 *
 * ldx_bed_unpack_dev: rows row0 .. row0 + n_rows - 1 of a panel of n_snps_panel x 2 n_ind_dst, both planes and both counts,
 * from n_rows .bed rows -- what ldx_pack_codes_dev makes of bed_codes_host(rows, n_ind_src, keep = ind_idx), without the codes.
 *   bed: device pointer to the rows, row_bytes >= ceil(n_ind_src / 4) apart (else LDX_E_ARG), at ANY alignment (a whole file
 *        copied to the device is read at base + 3); bits past n_ind_src in a row's last byte are ignored.  n_ind_src has no
 *        upper limit.
 *   ind_idx: uint32 [n_ind_dst] device array of source individuals, any order, repeats allowed, or NULL = identity (then
 *        n_ind_dst == n_ind_src, else LDX_E_ARG).  An index >= n_ind_src has a meaning, as in ldx_panel_select_dev (a _dev
 *        entry cannot report from inside the launch), and is never a stray read: a MISSING CALL at that individual.
 *        2 n_ind_dst <= LDX_MAX_HAPS, else LDX_E_UNSUPPORTED.
 *   row0: a multiple of 128; n_rows: a multiple of 128 unless row0 + n_rows == n_snps_panel; row0 + n_rows <= n_snps_panel
 *        (else LDX_E_ARG).  So a file streams into one panel chunk by chunk, and each call owns whole slabs.
 *   alt / ref / acnt / rcnt: the panel's (ldx_plane_bytes(n_snps_panel, 2 n_ind_dst), uint32 [padded_snps]), all required.
 * EVERY byte of the slabs a call owns is written: both planes, pad haplotypes and the pad rows of the last slab as zero
 * bits, acnt / rcnt including the pad rows' zeros.  The counts are plain stores by the workgroup that owns the rows: no
 * memset, no atomics, nothing read from the destination -- a call into a used or poisoned panel gives the same bytes.
 * A source of up to 7648 individuals is staged in LDS (the identity form always is); a wider one is gathered from global
 * memory through the index.  The call only enqueues ONE kernel on `stream`: no allocation, no synchronisation, no state. */
int ldx_bed_unpack_dev(const uint8_t *bed, size_t row_bytes, uint32_t n_ind_src, uint32_t n_rows,
                       const uint32_t *ind_idx, uint32_t n_ind_dst, int alt_is_a2, uint32_t row0, uint32_t n_snps_panel,
                       void *alt, void *ref, uint32_t *acnt, uint32_t *rcnt, void *stream);
/* ldx_bed_pack_dev: rows row0 .. row0 + n_rows - 1 (any range inside the panel, else LDX_E_ARG) of a panel of n_snps x n_hap
 * as n_rows .bed rows, row_bytes >= ceil(n_ind / 4) apart, at any alignment.  Per individual: both haplotypes ALT -> hom ALT,
 * both REF -> hom REF, one of each in either order -> het, anything else (a bit missing from both planes) -> missing.  n_hap
 * must be even (else LDX_E_ARG) and within LDX_MAX_HAPS (else LDX_E_UNSUPPORTED); ref is required.  Every byte of the
 * ceil(n_ind / 4) of each row is written, pad bits zero; the bytes between that and row_bytes are left alone.  One kernel on
 * `stream`. */
int ldx_bed_pack_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, uint32_t row0, uint32_t n_rows,
                     uint8_t *bed, size_t row_bytes, int alt_is_a2, void *stream);

/* ---- bit-exact contract: the alt/alt haplotype count of calc_ld.py:32 ------------------ */
/* n11[i][j] = popcount(alt_i[row i] & alt_j[row j]) for all rows of panel I against all rows of
 * panel J (may be the same plane).  n11 is dense row-major uint32 [n_i][ld]. */
int ldx_pair_counts_dev(const void *alt_i, uint32_t n_i, const void *alt_j, uint32_t n_j,
                        uint32_t n_hap, uint32_t *n11, size_t ld, void *stream);

/* ---- the epilogue alone: calc_ld.py:33-97 from the six integers ------------------------ */
/* Element k uses (n, n11[k], a1[k], r1[k], a2[k], r2[k]).  Any output may be NULL. */
int ldx_ld_from_counts_dev(uint32_t n, size_t m, const uint32_t *n11, const uint32_t *a1,
                           const uint32_t *r1, const uint32_t *a2, const uint32_t *r2,
                           ldx_ld64 *raw, ldx_ld32 *rounded, uint8_t *flags, void *stream);
/* The same with every output form: k = round(x, 4) * 10^4 as doubles [m][2] (r_square, d_prime; exact for any
 * magnitude), and the two cell formats.  The cells come from the production epilogues of the pair kernels (every tier:
 * fp32 / count-domain fp64 / op-for-op mirror), which must agree with each other bit for bit -- a disagreement poisons
 * the cell (NaN / 0xFFFF) so that the exhaustive tests fail loudly.  Any output may be NULL. */
int ldx_ld_from_counts_ex_dev(uint32_t n, size_t m, const uint32_t *n11, const uint32_t *a1,
                              const uint32_t *r1, const uint32_t *a2, const uint32_t *r2,
                              ldx_ld64 *raw, double *k, ldx_ld32 *cells32, ldx_k16 *cells16, uint8_t *flags,
                              void *stream);

/* ---- LD of an explicit list of pairs of one panel: calc_ld.py:30-97 per pair, exact for any magnitude ---- */
/* Pair p = (var_1 = rows[p], var_2 = cols[p]).  k: double [m][2] = round(x, 4) * 10^4 for (r_square, d_prime);
 * raw: unrounded; flags: LDX_FLAG_*; n11: the alt/alt haplotype counts.  Any output may be NULL.  This is how the
 * escape cells of the two formats are resolved, and what ld_lite-style single lookups use. */
int ldx_ld_pairs_dev(const void *alt, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps, uint32_t n_hap,
                     const uint32_t *rows, const uint32_t *cols, size_t m, double *k, ldx_ld64 *raw,
                     uint8_t *flags, uint32_t *n11, void *stream);

/* ---- ld_triangle: all row > col pairs (ld_triangle.py:133-230) ------------------------- */
/* Computes work units [unit_begin, unit_end) (clamped to ldx_triangle_units()).  var_1 = row,
 * var_2 = col as at ld_triangle.py:193-194.  Outputs are indexed from unit_begin:
 * out[(u - unit_begin)*1024 + ...].  Cells with row <= col or row >= n_snps are written as zero.
 * out_raw / out_n11 may be NULL.  fa/fr/q from ldx_snp_stats_dev. */
int ldx_triangle_dev(const void *alt, const double *fa, const double *fr, const double *q,
                     uint32_t n_snps, uint32_t n_hap, uint64_t unit_begin, uint64_t unit_end,
                     ldx_ld32 *out, ldx_ld64 *out_raw, uint32_t *out_n11, void *stream);
/* Which kernel ldx_triangle_dev launches.  All produce identical results (tests compare them cell for
 * cell): POPCOUNT = v_and_b32 + v_bcnt_u32_b32 on the bit-packed rows; MFMA = int8 G.G^T on the matrix
 * cores (v_mfma_i32_32x32x32_i8) with the bits expanded to bytes in registers; FP4 = the same contraction on
 * v_mfma_f32_32x32x64_f8f6f4 with the bits expanded to FP4 nibbles (twice the int8 rate; fp32 accumulation of
 * 0/1 products is exact below 2^24).  AUTO picks the one that measures fastest (FP4).
 * ldx_set_triangle_path sets the process-wide default that ldx_triangle_dev reads (atomically) at every call;
 * ldx_triangle_path_dev takes the path per call. */
#define LDX_PATH_AUTO 0
#define LDX_PATH_POPCOUNT 1
#define LDX_PATH_MFMA 2
#define LDX_PATH_FP4 3
int ldx_set_triangle_path(int path);
int ldx_get_triangle_path(void);
/* ldx_triangle_dev with the kernel path and the cell format per call.  out: ldx_ld32, ldx_k16, ldx_k16one or ldx_r32 cells
 * (out_format = LDX_OUT_LD32 / LDX_OUT_K16 / LDX_OUT_K16_RSQ / LDX_OUT_K16_DPRIME / LDX_OUT_R32), indexed as in
 * ldx_triangle_dev.  out_raw needs LDX_OUT_LD32; the one-measure formats take neither side output and run on the FP4 or the
 * popcount kernel; LDX_OUT_R32 takes neither side output and runs on all three kernels.
 * workspace (ABI 102): ldx_triangle_workspace_bytes() bytes of device memory, 256-byte aligned, that hold the matrix
 * kernel's pass scheduler (two ticket counters).  Contract:
 *   - ZERO it once before the first launch that uses it (hipMemsetAsync, torch.zeros, or ldx_triangle_workspace_init_dev);
 *     every launch leaves it zeroed again -- re-armed by its last workgroup -- so it is never touched by the host afterwards;
 *   - ONE workspace per launch that may be in flight: launches that may overlap (different streams, parallel branches of a
 *     graph, two graphs replayed at once) need different workspaces; consecutive launches of one stream, or consecutive
 *     nodes of one graph, may share one.  ld_tools_amd.ld_triangle keeps one per result buffer (TriangleResult.ws);
 *   - the library keeps NO scheduling state of its own (no per-stream slots, no limit on streams or captured launches, no
 *     allocation, nothing to leak); a launch recorded under stream capture is like any other;
 *   - workspace = NULL is allowed: the passes are then dealt round-robin instead of drawn from the counter (identical
 *     cells; measured 6.5-7.4 % slower on panels of more than one round of passes -- 10 000 x 5008, 40 000 x 5008,
 *     50 000 x 1008 -- and 3 % faster below one round, profiles/r06/round_robin_without_workspace.log) -- what
 *     ldx_triangle_dev does.
 * The popcount path ignores the workspace. */
size_t ldx_triangle_workspace_bytes(void);
int ldx_triangle_workspace_init_dev(void *workspace, size_t workspace_bytes, void *stream);   /* = hipMemsetAsync(workspace, 0, ...) */
int ldx_triangle_ex_dev(const void *alt, const double *fa, const double *fr, const double *q,
                        uint32_t n_snps, uint32_t n_hap, uint64_t unit_begin, uint64_t unit_end,
                        int path, int out_format, void *out, ldx_ld64 *out_raw, uint32_t *out_n11,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Strip output -> dense row-major float32 [n_rows][ld] matrix of one measure with the
 * ld_two_dim semantics of ld_triangle.py:114,223-230: cell = rounded measure, or 0 when
 * row <= col or (has_thres and rounded measure < thres).  Rows [row_begin, row_end). */
int ldx_triangle_dense_dev(const ldx_ld32 *strips, uint32_t n_snps, int measure, int has_thres,
                           double thres, uint32_t row_begin, uint32_t row_end, float *dense,
                           size_t ld, void *stream);
/* The same for any cell format (strips_format = LDX_OUT_*; a one-measure format holds ONE measure: `measure` must be it).
 * Escape cells (values the format cannot hold) come out as the NaN LDX_LD32_BIG_BITS whatever the threshold: resolve them
 * with ldx_ld_pairs_dev. */
int ldx_triangle_dense_ex_dev(const void *strips, int strips_format, uint32_t n_snps, int measure, int has_thres,
                              double thres, uint32_t row_begin, uint32_t row_end, float *dense,
                              size_t ld, void *stream);
/* Full (unsharded) LDX_OUT_R32 strips -> block [row_begin, row_end) x [col_begin, col_end) of the SYMMETRIC square r matrix,
 * row-major float32 with leading dimension ld_out: (i, j) = strip cell (i, j) for i > j, (j, i) for i < j; the diagonal is the
 * same formula at i = j, (n - a_i) / r_i (exactly 1.0f for a polymorphic SNP without missing codes, -0.0f for a degenerate
 * one), from acnt / rcnt (ldx_pack_codes_dev) and n_hap.  Reads and writes are coalesced (tiles staged through LDS). */
int ldx_triangle_r_block_dev(const ldx_r32 *strips, uint32_t n_snps, const uint32_t *acnt, const uint32_t *rcnt,
                             uint32_t n_hap, uint32_t row_begin, uint32_t row_end, uint32_t col_begin, uint32_t col_end,
                             float *out, size_t ld_out, void *stream);

/* ---- ld_area: windowed scan around query SNPs (ld_area.py:152-276) --------------------- */
/* positions: int64 [n_snps] ascending 1-based coordinates (VCF order).  queries: uint32 row
 * indices [n_query].  For each query q the opposing set is o != q with
 * max(0, pos_q - flank) < pos_o <= pos_q + flank (pysam fetch semantics, ld_area.py:174-177,
 * 215-217).  var_1 = query, var_2 = opposing (ld_area.py:242-243).  A hit is kept when the
 * ROUNDED measure >= thres (ld_area.py:248).  `queries` must ascend STRICTLY (distinct rows; so their positions ascend):
 * n_query == n_snps therefore means "every SNP is a query", which the matrix-pipe band takes as such.
 * hits: capacity hit_cap, written in arbitrary order (sort by (query, oppos) for VCF order).
 * Wavefronts reserve hit slots in batches of 256: *n_hits (device uint64) receives the number of
 * slots RESERVED, unused slots carry query == UINT32_MAX and must be skipped.  If *n_hits exceeds
 * hit_cap only the first hit_cap slots were stored: retry with a larger buffer.
 * workspace: ldx_area_workspace_bytes() bytes, 256-byte aligned, scratch for the gathered query
 * panel, the unit plan and the band kernel's ticket counters: one workspace per scan in flight (two scans that may run
 * at the same time -- different streams, or two graphs that hold a scan each -- need two). */
int ldx_area_dev(const void *alt, const double *fa, const double *fr, const double *q,
                 uint32_t n_snps, uint32_t n_hap, const int64_t *positions,
                 const uint32_t *queries, uint32_t n_query, int64_t flank, int measure,
                 double thres, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, void *workspace,
                 size_t workspace_bytes, void *stream);
size_t ldx_area_workspace_bytes(uint32_t n_snps, uint32_t n_hap, uint32_t n_query);
/* The same scan, which also counts the stored hits per query row as it appends them: query_counts = device uint32
 * [n_snps + 1] (zeroed here) or NULL.  With query_counts = ldx_area_finish_counts(finish workspace) the finishing step
 * below (ldx_area_finish_ex_dev, counts_ready = 1) needs neither its memset nor its pass over the slot buffer. */
int ldx_area_scan_dev(const void *alt, const double *fa, const double *fr, const double *q,
                      uint32_t n_snps, uint32_t n_hap, const int64_t *positions,
                      const uint32_t *queries, uint32_t n_query, int64_t flank, int measure,
                      double thres, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, uint32_t *query_counts,
                      void *workspace, size_t workspace_bytes, void *stream);
/* Finish a scan on the device, without a host round trip: raw slots (arbitrary order, unused slots marked) -> hits
 * sorted by (query row, opposing row) = the reference's output order (ld_area.py:152,215-217), plus the per-row index
 * offsets[n_snps + 1] (hits of query row q are sorted[offsets[q] .. offsets[q + 1])).  n_reserved: the device counter
 * ldx_area_dev filled; sorted: capacity hit_cap; summary: device uint64 [2] = {number of hits, slots reserved}.
 * If summary[1] > hit_cap the scan overflowed its buffer: run both again with hit_cap >= summary[1].
 * `raw` is CONSUMED: once its slots have been scattered it serves as the scratch the ordering of long hit lists writes to.
 * offsets must be 16-byte aligned, workspace 256-byte aligned. */
int ldx_area_finish_dev(ldx_hit *raw, const uint64_t *n_reserved, uint64_t hit_cap, uint32_t n_snps,
                        ldx_hit *sorted, uint32_t *offsets, uint64_t *summary, void *workspace,
                        size_t workspace_bytes, void *stream);
size_t ldx_area_finish_workspace_bytes(uint32_t n_snps);
int ldx_area_finish_ex_dev(ldx_hit *raw, const uint64_t *n_reserved, uint64_t hit_cap, uint32_t n_snps,
                           ldx_hit *sorted, uint32_t *offsets, uint64_t *summary, void *workspace,
                           size_t workspace_bytes, int counts_ready, void *stream);
uint32_t *ldx_area_finish_counts(void *finish_workspace);   /* where the finishing step keeps its per-query counts */
/* The caller's copy of a finished scan in ONE launch: the first n_hits sorted hits split into query rows, opposing rows
 * (int64 each) and the value pairs (float [n_hits][2]: r_square, d_prime), and -- each optional, NULL to skip -- a copy of
 * the n_offsets words of the offsets index and of one 32-bit instrumentation word.  (ld_area.py:261-276 reads exactly these
 * per query; a driver that keeps the scan's buffers for the next table needs its own copy of the result.) */
int ldx_area_results_dev(const ldx_hit *sorted, uint64_t n_hits, int64_t *query, int64_t *oppos, float *values,
                         const uint32_t *offsets_src, uint32_t *offsets_dst, uint32_t n_offsets,
                         const uint32_t *word_src, uint32_t *word_dst, void *stream);
/* instrumentation: byte offset, inside the workspace of ldx_area_dev, of the uint32 count of passes (4 units of 64 rows
 * x 128 columns) the matrix-pipe band evaluated */
size_t ldx_area_band_passes_offset(uint32_t n_snps);
/* kernel behind ldx_area_dev: LDX_PATH_AUTO (FP4 matrix-pipe band when >= 1/16 of the SNPs are queries, popcount scan
 * otherwise), LDX_PATH_POPCOUNT, LDX_PATH_MFMA (int8 band), LDX_PATH_FP4; the hit sets are identical */
int ldx_set_area_path(int path);
int ldx_get_area_path(void);

/* ---- LD scores: windowed sums of r^2 per SNP (LD score regression's l2 column) on the matrix-pipe band ---- */
/* For every SNP i, with r_ij the signed r cell of ldx_triangle_ex_dev(LDX_OUT_R32) for the pair (bit for bit the same value),
 * and the diagonal r_ii = (n - a_i) / r_i of ldx_triangle_r_block_dev (1 for a polymorphic SNP without missing codes, -0.0f
 * for a degenerate one):
 *     term(r) = rint(2^32 * (r *f32 r))        one IEEE float32 multiply, then exact scaling; a uint64.  Exact for every
 *                                              r^2 >= 2^-9; the -0.0f of a degenerate SNP gives 0
 *     sums[i][0]     = sum of term(r_ij) over j with |pos_i - pos_j| <= window      (j = i included: the window is
 *                                                                                      symmetric and inclusive)
 *     sums[i][1 + k] = the same sum over the j whose annot[j] has bit k set (j = i: if annot[i] has it), k < n_annot
 * so sums / 2^32 is the LD score L(i, C) = sum of r^2.  Every SNP is a query.  The sums are 64-bit integer atomics, so the
 * result does not depend on the order of the work: it is bit-reproducible run to run and equal to a host sum of the terms
 * of the r32 triangle.  They wrap only if one SNP's sum of r^2 reaches 2^32 (without missing codes r^2 <= 1: never).
 *   positions: int64 [n_snps], NON-DECREASING (duplicates allowed: both SNPs are then in each other's window);
 *   window >= 0 in the units of positions (values above 2^52 act as 2^52);
 *   annot: uint8 [n_snps] category bitmasks (bits >= n_annot are ignored), NULL iff n_annot == 0; n_annot <= 8;
 *   sums: uint64 [n_snps][1 + n_annot], written by the call (no need to zero it);
 *   acnt / rcnt from ldx_pack_codes_dev, fa / fr from ldx_snp_stats_dev;
 *   path: LDX_PATH_AUTO / LDX_PATH_FP4 = the FP4 band, LDX_PATH_MFMA = the int8 band (identical sums), LDX_PATH_POPCOUNT =
 *         LDX_E_UNSUPPORTED; n_hap > LDX_MAX_HAPS = LDX_E_UNSUPPORTED.
 * workspace: ldx_ld_score_workspace_bytes() bytes, 256-byte aligned, no initialisation needed (the call's first kernels set
 * what it reads): ONE workspace per launch that may be in flight, as for ldx_area_dev -- launches that may overlap (different
 * streams, parallel graph branches) need different workspaces; consecutive launches of one stream may share one.
 * The call only enqueues work on `stream`: it allocates nothing and does not synchronise. */
size_t ldx_ld_score_workspace_bytes(uint32_t n_snps, uint32_t n_hap);
int ldx_ld_score_dev(const void *alt, const uint32_t *acnt, const uint32_t *rcnt, const double *fa, const double *fr,
                     uint32_t n_snps, uint32_t n_hap, const int64_t *positions, int64_t window,
                     const uint8_t *annot, uint32_t n_annot, int path,
                     uint64_t *sums, void *workspace, size_t workspace_bytes, void *stream);

/* ---- LD decay: sums of r^2 and pair counts per distance bin (the LD decay curve) on the matrix-pipe band ---- */
/* A pair is every unordered i > j with
 *     d = pos_i - pos_j <= window        (positions are non-decreasing, so d >= 0; duplicate positions give d = 0; i = j is
 *                                         not a pair),
 *     both SNPs non-degenerate (a r > 0), and -- if keep != NULL -- keep[i] and keep[j] both non-zero.
 * For each pair, with c_ij the signed r cell of ldx_triangle_ex_dev(LDX_OUT_R32), bit for bit:
 *     term = rint(2^32 * (c_ij *f32 c_ij))    the term ldx_ld_score_dev sums
 *     b    = floor(d / bin_width)             EXACTLY (integer arithmetic on d: a pair at d = k bin_width lies in bin k,
 *                                             one at d = k bin_width - 1 in bin k - 1)
 *     sums[b] += term,  counts[b] += 1
 * so sums[b] / 2^32 / counts[b] is the mean r^2 of the pairs whose distance lies in [b bin_width, (b + 1) bin_width).  The
 * sums are 64-bit integer atomics: the result does not depend on the order of the work, it is bit-reproducible run to run,
 * identical on both paths and equal to a host histogram of the terms of the r32 triangle.  Two identities follow: the
 * counts add up to the number of in-window pairs of kept non-degenerate SNPs, and with keep = NULL
 *     2 * (sum over b of sums[b]) + (sum over i of term(c_ii)) = sum over i of ldx_ld_score_dev's sums[i][0]
 * on the same window (a degenerate SNP adds 0 on both sides).
 *   positions: int64 [n_snps], NON-DECREASING; window >= 0 in their units (values above 2^52 act as 2^52);
 *   bin_width >= 1 in the same units (else LDX_E_ARG); a width above the window gives the single bin 0;
 *   n_bins: must equal min(window, 2^52) / bin_width + 1 and be <= LDX_DECAY_MAX_BINS (else LDX_E_ARG);
 *   keep: uint8 [n_snps] or NULL (every SNP kept);
 *   sums, counts: uint64 [n_bins] each, written by the call (no need to zero them);
 *   acnt / rcnt from ldx_pack_codes_dev, fa / fr from ldx_snp_stats_dev;
 *   path: LDX_PATH_AUTO / LDX_PATH_FP4 = the FP4 band, LDX_PATH_MFMA = the int8 band (identical outputs), LDX_PATH_POPCOUNT =
 *         LDX_E_UNSUPPORTED; n_hap > LDX_MAX_HAPS and a bit plane of 4 GiB or more = LDX_E_UNSUPPORTED.
 * workspace: ldx_ld_decay_workspace_bytes() bytes, 256-byte aligned, no initialisation needed (the score band's layout; its
 * leading bytes hold the effective keep mask, kept AND non-degenerate): one per launch that may be in flight, as for
 * ldx_ld_score_dev.  The call only enqueues work on `stream`: no allocation, no synchronisation, no state in the library.
 * D' is not offered: the band's r32 family carries no D', and an unrounded D' would need a contract of its own. */
#define LDX_DECAY_MAX_BINS 1024u
size_t ldx_ld_decay_workspace_bytes(uint32_t n_snps, uint32_t n_hap);
int ldx_ld_decay_dev(const void *alt, const uint32_t *acnt, const uint32_t *rcnt, const double *fa, const double *fr,
                     uint32_t n_snps, uint32_t n_hap, const int64_t *positions, int64_t window, int64_t bin_width,
                     const uint8_t *keep, int path,
                     uint64_t *sums, uint64_t *counts, uint32_t n_bins,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- haplotype blocks by the four-gamete test (Hudson & Kaplan 1985) on the matrix-pipe band ---- */
/* Gametes of SNPs i > j, with A_x the set of haplotypes whose code is 1 (ALT) at SNP x, a_x = |A_x| and n = n_hap:
 *     g11 = |A_i n A_j|,  g10 = a_i - g11,  g01 = a_j - g11,  g00 = n - a_i - a_j + g11.
 * "Not ALT" is the other allele: a missing code or a second ALT allele counts with REF.  (The REF plane never enters the
 * band; callers who want missing codes out of the test drop such SNPs with `keep`.)
 * The pair is RECOMBINANT iff min(g11, g10, g01, g00) >= min_count, 1 <= min_count <= n_hap (else LDX_E_ARG).  It is
 * evaluated iff both SNPs are kept (keep: uint8 [n_snps] or NULL = every SNP) and d = pos_i - pos_j <= window (positions
 * int64, NON-DECREASING; duplicate positions give d = 0; values of window above 2^52 act as 2^52), as in ldx_ld_decay_dev.
 * A monomorphic SNP is compatible with everything; it is masked out only if `keep` does it.
 *     left[i] = 1 + max{ j < i : (i, j) recombinant },  0 if there is none          (uint32 [n_snps])
 * The call writes every word of `left` (no memset by the caller; a relaunch into a used buffer gives the same array).  The
 * predicate is integer arithmetic on exact counts: no rounding, identical on both paths, equal to a host count over the
 * allele codes.
 *   acnt from ldx_pack_codes_dev (the ALT counts; no frequency vector is read);
 *   path: LDX_PATH_AUTO / LDX_PATH_FP4 = the FP4 band, LDX_PATH_MFMA = the int8 band (identical outputs), LDX_PATH_POPCOUNT =
 *         LDX_E_UNSUPPORTED; n_hap > LDX_MAX_HAPS and a bit plane of 4 GiB or more = LDX_E_UNSUPPORTED.
 * workspace: ldx_ld_fgt_workspace_bytes() bytes, 256-byte aligned, no initialisation needed (the score band's layout; its
 * leading bytes hold the keep mask): one per launch that may be in flight.  The call only enqueues work on `stream`: no
 * allocation, no synchronisation, no state in the library.
 *
 * ldx_ld_blocks_dev: the greedy left-to-right partition of the kept SNPs over `left` (the Hudson-Kaplan partition; not
 * Haploview's block-picking order).  With s the current block's first SNP, kept SNP i starts a new block iff there is no
 * current block, or left[i] >= s + 1, or pos_i - pos_s > window -- the window rule keeps "no recombinant pair inside a
 * block" true, since every pair inside a block was tested.
 *     block_of[i] (uint32 [n_snps]): the 0-based block of SNP i, 0xFFFFFFFF for a SNP not kept;
 *     n_out[0]: the number of blocks;  n_out[1]: the block starts caused by the `left` rule (it outranks the window rule) --
 *               Hudson & Kaplan's lower bound Rm on the number of recombination events, restricted to the window.
 * One wave walks the SNPs (the scan is sequential in the number of blocks); the result stays on the device, so the two
 * calls can be captured together.  Gabriel's D' confidence-interval blocks -- the definition for unphased genotypes, a PLINK
 * fileset among them -- are the "Gabriel blocks" entries below (ldx_ld_em_ci_band_dev, ldx_gabriel_candidates_dev,
 * ldx_gabriel_pick_dev). */
size_t ldx_ld_fgt_workspace_bytes(uint32_t n_snps, uint32_t n_hap);
int ldx_ld_fgt_dev(const void *alt, const uint32_t *acnt, uint32_t n_snps, uint32_t n_hap, const int64_t *positions,
                   int64_t window, uint32_t min_count, const uint8_t *keep, int path,
                   uint32_t *left, void *workspace, size_t workspace_bytes, void *stream);
int ldx_ld_blocks_dev(const uint32_t *left, const int64_t *positions, const uint8_t *keep, uint32_t n_snps, int64_t window,
                      uint32_t *block_of, uint32_t *n_out, void *stream);

/* ---- LD-independent regions: the cross-LD profile of the band and the optimal cuts over it ---- */
/* ldx_ld_cross_dev: ldx_ld_score_dev's sweep -- the same pairs, window test, r cell and term -- with the two halves of every
 * SNP's score kept apart.  For every pair i > j with pos_i - pos_j <= window (positions int64, NON-DECREASING; duplicates
 * give distance 0; i = j is not a pair), with c_ij the signed r cell of ldx_triangle_ex_dev(LDX_OUT_R32), bit for bit:
 *     term = rint(2^32 * (c_ij *f32 c_ij))     the term ldx_ld_score_dev sums (0 for the -0.0f cell of a degenerate SNP)
 *     sides[i][0] += term                      i's LEFT partners   (uint64 [n_snps][2])
 *     sides[j][1] += term                      j's RIGHT partners
 * so sides[i][0] + sides[i][1] + term(c_ii) = ldx_ld_score_dev's sums[i][0] on the same window, and the sum of all left
 * halves = the sum of all right halves = the sum of ldx_ld_decay_dev's sums with keep = NULL.  The call writes every word
 * of `sides` (no memset by the caller; a relaunch into a used buffer gives the same array); the sums are 64-bit integer
 * atomics: order-independent, bit-reproducible, identical on both paths, equal to a host sum over the r32 square.
 * A scan then writes the CROSS-LD PROFILE, the LD that crosses a cut before SNP k:
 *     cross[k] = sum of term over the pairs j < k <= i inside the window          (uint64 [n_snps + 1], k = 0 .. n_snps)
 *              = cross[k - 1] + sides[k - 1][1] - sides[k - 1][0] modulo 2^64,  cross[0] = 0
 * (pair (i, j) enters at k = j + 1 and leaves at k = i + 1, so cross[n_snps] = 0 too).  The true value is non-negative, so
 * the modular sum is exact as long as it is below 2^64: cross[k] wraps only if the r^2 that straddles ONE cut reaches 2^32
 * (without missing codes r^2 <= 1: 2^32 in-window pairs across one cut).  A half of `sides` wraps like ldx_ld_score_dev's sums.
 * ldx_ld_cross_scan_dev is the scan alone (ldx_ld_cross_dev ends with it): one workgroup walks the array, any n_snps.
 *   acnt / rcnt / fa / fr, positions, window (values above 2^52 act as 2^52), n_hap: as for ldx_ld_score_dev;
 *   path: LDX_PATH_AUTO / LDX_PATH_FP4 = the FP4 band, LDX_PATH_MFMA = the int8 band (identical outputs), LDX_PATH_POPCOUNT =
 *         LDX_E_UNSUPPORTED; n_hap > LDX_MAX_HAPS and a bit plane of 4 GiB or more = LDX_E_UNSUPPORTED.
 * workspace: ldx_ld_cross_workspace_bytes() bytes, 256-byte aligned, no initialisation needed (the score band's layout): one
 * per launch that may be in flight, as for ldx_ld_score_dev.  The calls only enqueue work on `stream`: no allocation, no
 * synchronisation, no state in the library.
 *
 * ldx_ld_split_dev: the cuts of minimum total cross-LD with every region min_snps .. max_snps SNPs long (the objective of
 * ldetect, Berisa & Pickrell 2016, and of bigsnpr's snp_ldsplit, with ADDITIVE cuts: the cost of a cut set is the sum over
 * its cuts of the LD crossing each one, so a pair that straddles two cuts counts twice -- which needs a region narrower
 * than the window).  A cut c is a boundary before SNP c, 0 < c < n.  With cost[k] = cross[k] >> 16 (units of 2^-16 r^2):
 *     best[0] = 0
 *     best[k] = min over p in [max(0, k - max_snps), k - min_snps] with best[p] feasible of best[p]
 *               + (cost[k] if k < n else 0);                      infeasible if there is no such p     (k = 1 .. n)
 *     prev[k] = the LARGEST p attaining that minimum
 * and the cuts are the backtrack from n through prev, 0 excluded, written ascending:
 *     cuts (uint32, room for n / min_snps entries; at most n / min_snps - 1 are written);
 *     n_out[0] = the number of cuts;
 *     n_out[1] = 0, or 1 if best[n] is infeasible (no m with m min_snps <= n <= m max_snps), or 2 if a sum wrapped; no cut
 *                is written then and n_out[0] = 0.
 * Sums saturate at 2^64 - 2, and a saturated best[n] is what "wrapped" means: the total cost of the optimal cuts reached
 * 2^64 - 2, i.e. 2^48 of r^2 summed over the cuts (cost[k] < 2^48 always).  A saturated state that is not on the optimal
 * path does not set the flag: costs are non-negative, so it cannot lie on a path with a smaller total.
 *   cross: uint64 [n + 1] (ldx_ld_cross_dev's, or any array: only cross[1 .. n - 1] is read);
 *   1 <= min_snps <= max_snps (else LDX_E_ARG); max_snps above n acts as n.
 * ONE workgroup runs the recurrence: the min_snps states k .. k + min_snps - 1 depend only on best[p], p < k, so they are
 * computed side by side, a barrier between such chunks; the range minimum costs O(1) per state through prefix / suffix
 * arg-minima over blocks of max_snps - min_snps + 1 states (van Herk / Gil-Werman), each written once by a segmented scan.
 * One lane backtracks at the end, so everything stays on the device and the call can be captured behind ldx_ld_cross_dev.
 * workspace: ldx_ld_split_workspace_bytes(n) bytes (20 per state), 256-byte aligned, no initialisation needed. */
size_t ldx_ld_cross_workspace_bytes(uint32_t n_snps, uint32_t n_hap);
int ldx_ld_cross_dev(const void *alt, const uint32_t *acnt, const uint32_t *rcnt, const double *fa, const double *fr,
                     uint32_t n_snps, uint32_t n_hap, const int64_t *positions, int64_t window, int path,
                     uint64_t *sides, uint64_t *cross, void *workspace, size_t workspace_bytes, void *stream);
int ldx_ld_cross_scan_dev(const uint64_t *sides, uint32_t n_snps, uint64_t *cross, void *stream);
size_t ldx_ld_split_workspace_bytes(uint32_t n);
int ldx_ld_split_dev(const uint64_t *cross, uint32_t n, uint32_t min_snps, uint32_t max_snps,
                     uint32_t *cuts, uint32_t *n_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- banded LD matrix-vector products: R_w X and (R_w o R_w) X without the matrix, on the matrix-pipe band ---- */
/* For every SNP i and right-hand side k < n_rhs (1 <= n_rhs <= 8), power in {1, 2}:
 *     c_ij = the signed r cell of ldx_triangle_ex_dev(LDX_OUT_R32) for the pair, bit for bit; c_ii = (n - a_i) / r_i, the
 *            diagonal of ldx_triangle_r_block_dev (-0.0f for a degenerate SNP)
 *     v_ij = c_ij                          (power 1)
 *          = c_ij *f32 c_ij                (power 2: ONE IEEE float32 multiply, the value ldx_ld_score_dev's term scales)
 *     term = (int64) rint(2^40 * clamp((double)v_ij * (double)x[j][k], -2^22, 2^22))
 *            -- the fp64 product of two float32 is exact (24 + 24 bits), the clamp and the scaling are exact: ONE rounding
 *               (half to even), so every term is within 2^-41 of v_ij x_jk.  The clamp keeps the conversion defined; it is
 *               only reachable with |x| or |c| far above 1
 *     sums[i][k] = sum of term over j with |pos_i - pos_j| <= window      (j = i included; int64, two's-complement adds)
 * so sums * 2^-40 is (R_w X)[i][k] with R_w the windowed signed-r matrix (power 2: its elementwise square, i.e. the LD score
 * of a continuous annotation x).  The -0.0f cell of a degenerate SNP gives term 0 in both directions: its row is 0 and it
 * adds 0 to every neighbour.  The sums are 64-bit integer atomics, so the result does not depend on the order of the work:
 * bit-reproducible run to run, identical on both paths, and equal to a host sum of the terms over the r32 square.  A sum
 * wraps only if one SNP's sum of |v x| over its window reaches 2^23 (with |x| <= 1 and without missing codes, |c| <= 1:
 * 2^23 SNPs in one window -- more than a bit plane under 4 GiB holds at 5008 haplotypes).
 *   x: float32 [n_snps][n_rhs], finite;  sums: int64 [n_snps][n_rhs], written by the call (no need to zero it);
 *   positions, window, acnt / rcnt / fa / fr, path, n_hap: as for ldx_ld_score_dev (LDX_PATH_POPCOUNT and
 *   n_hap > LDX_MAX_HAPS = LDX_E_UNSUPPORTED); n_rhs outside 1 .. 8 or power outside {1, 2} = LDX_E_ARG.
 * workspace: ldx_ld_matvec_workspace_bytes() bytes, 256-byte aligned, no initialisation needed: one per launch that may be
 * in flight (as for ldx_ld_score_dev).  The call only enqueues work on `stream`: no allocation, no synchronisation, no
 * state in the library. */
size_t ldx_ld_matvec_workspace_bytes(uint32_t n_snps, uint32_t n_hap);
int ldx_ld_matvec_dev(const void *alt, const uint32_t *acnt, const uint32_t *rcnt, const double *fa, const double *fr,
                      uint32_t n_snps, uint32_t n_hap, const int64_t *positions, int64_t window,
                      const float *x, uint32_t n_rhs, int power, int path,
                      int64_t *sums, void *workspace, size_t workspace_bytes, void *stream);

/* ---- LD neighbour lists on the matrix-pipe band (clumping and pruning, with ldx_ld_select_dev) ---- */
/* Every ordered pair (i, j), i != j, with
 *     |pos_i - pos_j| <= window          (the inclusive, symmetric window of ldx_ld_score_dev; duplicate positions allowed)
 *     s_ij = c_ij *f32 c_ij >= r2_bound  (c_ij the signed r cell of ldx_triangle_ex_dev(LDX_OUT_R32), bit for bit; s ONE
 *                                         IEEE float32 multiply, as in ldx_ld_score_dev's term)
 * is stored as the record {query = i, oppos = j, r_square = c_ij, d_prime = s_ij} -- every pair in both orientations.
 * r2_bound: a float32 > 0 (so the -0.0f cell of a degenerate SNP and a cell with num == 0 never pass).  A caller with a
 * threshold t (a double) passes the smallest float32 not below t for `r^2 >= t`, and the smallest float32 above t for
 * `r^2 > t`: s is a float32, so either test is then exactly s >= r2_bound.
 *   positions: int64 [n_snps], NON-DECREASING; window >= 0 in their units (values above 2^52 act as 2^52);
 *   acnt / rcnt from ldx_pack_codes_dev (as for ldx_ld_score_dev), fa / fr from ldx_snp_stats_dev;
 *   path: LDX_PATH_AUTO / LDX_PATH_FP4 = the FP4 band, LDX_PATH_MFMA = the int8 band (identical records), LDX_PATH_POPCOUNT
 *         = LDX_E_UNSUPPORTED; n_hap > LDX_MAX_HAPS = LDX_E_UNSUPPORTED.
 * hits: capacity hit_cap (< 2^32), written in arbitrary order; *n_hits (device uint64) receives the number of slots
 * RESERVED (batches of 256 per wave; unused slots carry query == UINT32_MAX), as for ldx_area_scan_dev: if it exceeds
 * hit_cap only the first hit_cap slots were stored -- retry with a larger buffer.  row_counts: device uint32 [n_snps + 1]
 * (zeroed here) or NULL; with row_counts = ldx_area_finish_counts(finish workspace), ldx_area_finish_ex_dev(counts_ready = 1)
 * turns the slots into the per-SNP neighbour CSR: records sorted by (query, oppos), row i's at [offsets[i], offsets[i + 1]).
 * workspace: ldx_ld_neighbors_workspace_bytes() bytes, 256-byte aligned, no initialisation needed: one per launch that may
 * be in flight (as for ldx_ld_score_dev).  The call only enqueues work on `stream`. */
size_t ldx_ld_neighbors_workspace_bytes(uint32_t n_snps, uint32_t n_hap);
int ldx_ld_neighbors_dev(const void *alt, const uint32_t *acnt, const uint32_t *rcnt, const double *fa, const double *fr,
                         uint32_t n_snps, uint32_t n_hap, const int64_t *positions, int64_t window, float r2_bound, int path,
                         ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, uint32_t *row_counts,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Greedy selection over a neighbour CSR (records + offsets of ldx_area_finish_ex_dev after ldx_ld_neighbors_dev; only
 * `oppos` is read).  rank: uint32 [n_snps], distinct among the candidates, UINT32_MAX for a SNP that is not one;
 * member_ok: uint8 [n_snps], non-zero for every candidate.  The result is that of the sequential rule: take the candidates
 * in increasing rank; one not yet assigned becomes an INDEX, and each of its neighbours that is not yet assigned and has
 * member_ok set is assigned to it.  So the indices are the lexicographically-first maximal independent set of the
 * candidates' subgraph, and a SNP's owner is its neighbour index of smallest rank.  Computed in ROUNDS, one kernel launch
 * each: an undecided candidate becomes an index once every neighbour candidate of smaller rank has been removed, and is
 * removed as soon as one of them is an index.  Decisions are final, so a round may read what other workgroups wrote in it;
 * each round decides at least the undecided candidate of lowest rank: at most (number of candidates) rounds.
 * The call enqueues rounds [first_round, first_round + n_rounds) (n_rounds >= 1; first_round = 0 initialises the
 * workspace, later calls continue from where the previous one stopped: call them in order on one stream with one
 * workspace), then writes the number of candidates still undecided to *undecided (device uint32).  A round enqueued after
 * convergence returns at once.  When *undecided is 0 the call has also written
 *     state[i] (uint8) = LDX_SEL_INDEX, LDX_SEL_ASSIGNED (a candidate that is not an index) or LDX_SEL_OUT (no candidate)
 *     owner[i] (uint32) = i for an index; the index row SNP i was assigned to; UINT32_MAX for none.
 * workspace: ldx_ld_select_workspace_bytes() bytes, 256-byte aligned. */
#define LDX_SEL_INDEX 1
#define LDX_SEL_ASSIGNED 2
#define LDX_SEL_OUT 3
size_t ldx_ld_select_workspace_bytes(uint32_t n_snps);
int ldx_ld_select_dev(const ldx_hit *nbrs, const uint32_t *offsets, uint32_t n_snps, const uint32_t *rank,
                      const uint8_t *member_ok, uint32_t first_round, uint32_t n_rounds, uint8_t *state, uint32_t *owner,
                      uint32_t *undecided, void *workspace, size_t workspace_bytes, void *stream);

/* ---- genotype-dosage LD (unphased r): the r32 triangle, LD scores and neighbour lists over individuals ---- */
/* The entries above correlate haplotypes (n = n_hap phased ALT indicators).  These correlate the ALT DOSAGE of individuals,
 * which does not depend on phase: what PLINK --r2 / --indep-pairwise and ldsc.py --l2 compute.  Individual k owns haplotypes
 * 2k and 2k + 1 of the panel (n_hap even, N = n_hap / 2), and
 *     g_ik = number of code-1 alleles of individual k at SNP i  (0, 1 or 2)
 *     a_i = sum_k g_ik  (= acnt[i])     hom_i = #{k : g_ik = 2}     Q_i = sum_k g_ik^2 = a_i + 2 hom_i
 *     S_ij = sum_k g_ik g_jk            num = N S_ij - a_i a_j      v_i = N Q_i - a_i^2
 *     r_ij = num / sqrt(v_i v_j)        degenerate (cell -0.0f) iff v_i v_j == 0
 * -- all integers (below 2^28 for n_hap <= LDX_MAX_HAPS), so a cell is within 4 float32 ulps of the exact r, +0.0f exactly
 * when num == 0, and -0.0f exactly on a degenerate pair.  v_i == 0 for a SNP without variance among the DOSAGES: no ALT
 * allele, every allele ALT, and also every individual heterozygous (a_i r_i > 0 there: the haplotype entries call it live).
 * Missing data: g counts code 1 ONLY.  Every other code (REF, missing, a second ALT allele) contributes 0, so a missing call
 * acts as REF -- a documented imputation -- and a multi-allelic site gives the one-vs-rest dosage of its code-1 allele.
 *
 * ldx_dosage_stats_dev: from the tiled ALT plane and acnt (ldx_pack_codes_dev / ldx_tile_plane_dev) writes, per row of the
 * padded panel (ldx_padded_snps; pad rows: zeros -- every byte is written, no memset needed),
 *     hom[i]   uint32     popcount(w & (w >> 1) & 0x5555...) over the row's words
 *     gstat[i] double[2]  {a_i, rs_i},  rs_i = v_i > 0 ? 1 / sqrt((double)v_i) : 0
 * The cell is r32_cell(S, N, a_i, rs_i, a_j, rs_j) of the haplotype entries (num exact in fp64, then two products): the
 * same epilogue with another per-SNP table and another count.  S comes from the FP4 matrix kernel at the haplotype rate (the
 * B operand carries the individual's dosage); no other kernel counts it, so
 *     n_hap odd = LDX_E_ARG;  path LDX_PATH_MFMA / LDX_PATH_POPCOUNT = LDX_E_UNSUPPORTED (LDX_PATH_AUTO = LDX_PATH_FP4);
 *     n_hap > LDX_MAX_HAPS, or a bit plane of 4 GiB or more = LDX_E_UNSUPPORTED.
 *
 * ldx_triangle_dosage_dev: ldx_triangle_ex_dev(out_format = LDX_OUT_R32) with dosage cells -- same units, cell order,
 * workspace (ldx_triangle_workspace_bytes, or NULL) and zero cells outside the triangle.
 * ldx_triangle_r_block_dosage_dev: ldx_triangle_r_block_dev over such strips; the diagonal is +1.0f for v_i > 0, -0.0f
 * otherwise.
 * ldx_ld_score_dosage_dev: ldx_ld_score_dev over the dosage cells -- same window, annotation words, workspace
 * (ldx_ld_score_workspace_bytes) and integer terms rint(2^32 c *f32 c); a SNP's own term is 2^32 for v_i > 0 and 0 otherwise.
 * `sums` equal the host sum of those terms over the dosage r32 matrix, bit for bit, whatever the order of the launch.
 * ldx_ld_neighbors_dosage_dev: ldx_ld_neighbors_dev over the dosage cells -- same records, slots, row_counts and workspace
 * (ldx_ld_neighbors_workspace_bytes).
 * All calls only enqueue work on `stream`. */
int ldx_dosage_stats_dev(const void *alt, const uint32_t *acnt, uint32_t n_snps, uint32_t n_hap, uint32_t *hom, double *gstat,
                         void *stream);
int ldx_triangle_dosage_dev(const void *alt, const double *gstat, uint32_t n_snps, uint32_t n_hap, uint64_t unit_begin,
                            uint64_t unit_end, int path, ldx_r32 *out, void *workspace, size_t workspace_bytes, void *stream);
int ldx_triangle_r_block_dosage_dev(const ldx_r32 *strips, uint32_t n_snps, const double *gstat, uint32_t row_begin,
                                    uint32_t row_end, uint32_t col_begin, uint32_t col_end, float *out, size_t ld_out,
                                    void *stream);
int ldx_ld_score_dosage_dev(const void *alt, const double *gstat, uint32_t n_snps, uint32_t n_hap, const int64_t *positions,
                            int64_t window, const uint8_t *annot, uint32_t n_annot, int path, uint64_t *sums, void *workspace,
                            size_t workspace_bytes, void *stream);
int ldx_ld_neighbors_dosage_dev(const void *alt, const double *gstat, uint32_t n_snps, uint32_t n_hap, const int64_t *positions,
                                int64_t window, float r2_bound, int path, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits,
                                uint32_t *row_counts, void *workspace, size_t workspace_bytes, void *stream);

/* ---- stored bands: signed r of every in-window pair, kept --------------------------------------------------------------
 * The band operators above reduce the in-window r cells and drop them; these entries KEEP them, 4 bytes per unordered pair,
 * with no threshold and no sort -- the windowed LD matrix of a whole chromosome -- and consume what was kept.
 *
 * Layout.  For non-decreasing positions and window >= 0 (values above 2^52 act as 2^52):
 *     lo[i]      = min{ j <= i : pos_i - pos_j <= window }              uint32 [n_snps]
 *     offsets[0] = 0,  offsets[i + 1] = offsets[i] + (i - lo[i])        uint64 [n_snps + 1]
 *     cell (i, j), lo[i] <= j < i, lives at values[offsets[i] + (j - lo[i])]
 * Lower band only: every unordered in-window pair once, no diagonal; offsets[n_snps] is the number of cells.
 * ldx_ld_band_layout_dev writes every word of lo and offsets (one workgroup, any n_snps, no workspace).
 *
 * ldx_ld_band_dev: for every pair i > j with pos_i - pos_j <= window, values[offsets[i] + j - lo[i]] = the signed r cell of
 * ldx_triangle_ex_dev(LDX_OUT_R32), bit for bit (-0.0f for a degenerate pair); ldx_ld_band_dosage_dev: the cell of
 * ldx_triangle_dosage_dev.  Both paths (LDX_PATH_FP4 = LDX_PATH_AUTO, LDX_PATH_MFMA) store identical bytes.  The call writes
 * every one of the offsets[n_snps] cells -- no memset, a relaunch into a used buffer gives the same bytes -- and nothing
 * else: the kernel stores only where lo[i] <= j < i and the index is < n_cells (passed by value), so a lo / offsets pair
 * that is not the layout of `positions` / `window` gives wrong or missing cells, never a write outside values[0, n_cells).
 * workspace: ldx_ld_band_workspace_bytes() bytes (the LD-score band's layout), 256-byte aligned, no initialisation needed:
 * one per launch that may be in flight.  LDX_PATH_POPCOUNT, n_hap > LDX_MAX_HAPS and a bit plane of 4 GiB or more =
 * LDX_E_UNSUPPORTED; the dosage form follows the dosage entries' rules (even n_hap, FP4 only).
 *
 * ldx_band_score_dev: cross-panel LD scores of two bands that share ONE layout (same positions, same window; the panels may
 * differ in their haplotypes, and either band may be a dosage band).  With T(a, b) = (int64) rint(2^32 (a *f32 b)) -- one
 * IEEE float32 multiply, exact scaling, round-half-even -- every stored cell adds T(c1_ij, c2_ij) to sums[i] and to sums[j],
 * and SNP i's own term is T(diag1[i], diag2[i]) (both diagonals NULL: no own term).  sums is int64 [n_snps], written by the
 * call (no memset); the additions are 64-bit integer ones, so the result does not depend on their order.  values2 ==
 * values1 is allowed: with diag = the r32 diagonal of ldx_triangle_r_block_dev the sums then equal ldx_ld_score_dev's
 * sums[i][0], bit for bit.
 *
 * ldx_band_matvec_dev: ldx_ld_matvec_dev from a stored band -- the same term (fp64 product of the cell, or of its float32
 * square for power 2, and the float32 weight, clamped to +-2^22, rint(2^40 .)), cell (i, j) feeding row i with x[j] and row j
 * with x[i], SNP i's own term from diag[i] (NULL: none); 1 <= n_rhs <= 8, x and sums [n_snps][n_rhs].  With the band of
 * ldx_ld_band_dev and the r32 diagonal the sums equal ldx_ld_matvec_dev's on the same window, bit for bit.
 *
 * A band pointer may be NULL when its layout holds no cell.  All calls only enqueue work on `stream` and keep no state. */
int ldx_ld_band_layout_dev(const int64_t *positions, uint32_t n_snps, int64_t window, uint32_t *lo, uint64_t *offsets,
                           void *stream);
size_t ldx_ld_band_workspace_bytes(uint32_t n_snps, uint32_t n_hap);
int ldx_ld_band_dev(const void *alt, const uint32_t *acnt, const uint32_t *rcnt, const double *fa, const double *fr,
                    uint32_t n_snps, uint32_t n_hap, const int64_t *positions, int64_t window, int path, const uint32_t *lo,
                    const uint64_t *offsets, float *values, uint64_t n_cells, void *workspace, size_t workspace_bytes,
                    void *stream);
int ldx_ld_band_dosage_dev(const void *alt, const double *gstat, uint32_t n_snps, uint32_t n_hap, const int64_t *positions,
                           int64_t window, int path, const uint32_t *lo, const uint64_t *offsets, float *values,
                           uint64_t n_cells, void *workspace, size_t workspace_bytes, void *stream);
int ldx_band_score_dev(const float *values1, const float *values2, const float *diag1, const float *diag2, const uint32_t *lo,
                       const uint64_t *offsets, uint32_t n_snps, int64_t *sums, void *stream);
int ldx_band_matvec_dev(const float *values, const float *diag, const uint32_t *lo, const uint64_t *offsets, uint32_t n_snps,
                        const float *x, uint32_t n_rhs, int power, int64_t *sums, void *stream);

/* ---- rectangular LD: the rows of one SNP set against the rows of another, over the same haplotypes -------------------------
 * Every entry above that produces r pairs one panel with itself (the triangle, or a window of it).  These pair the n_i rows of
 * panel I with the n_j rows of panel J -- two tiled bit planes (ldx_plane_bytes) over the SAME n_hap haplotypes, for instance
 * two sub-panels of ldx_panel_select_dev: lead SNPs x a chromosome, an rsID list x itself in the caller's order, chromosome A
 * x chromosome B.  alt_i == alt_j is allowed (a panel against itself: the full square).  A kernel of its own on the FP4 matrix
 * cores (ldx_rect.hip); no workspace, no library state.
 *
 * The cell of (row i of I, row j of J) is the signed r cell of ldx_triangle_ex_dev(LDX_OUT_R32) for those two SNPs, bit for
 * bit: r32 arithmetic on the exact count, -0.0f on a degenerate pair, +0.0f iff num == 0, within 4 float32 ulps of the exact r
 * otherwise.  The rectangle knows nothing about the identity of SNPs: where row i of I and row j of J are the same variant
 * the cell is still that pair formula (n n11 - a a) / (a r) in the r32 arithmetic -- within 4 ulps of the exact diagonal
 * (n - a) / r, -0.0f for a degenerate SNP -- and NOT the one-division diagonal of ldx_triangle_r_block_dev.
 *   acnt / rcnt: uint32 [n] per side, from ldx_pack_codes_dev / ldx_panel_select_dev (only the first n words are read);
 *   dosage forms: gstat per side from ldx_dosage_stats_dev, the cell is ldx_triangle_dosage_dev's (n = n_hap / 2 individuals).
 *
 * ldx_ld_rect_dev / ldx_ld_rect_dosage_dev: out[i * ld_out + j] = the cell, float32, for i < n_i and j < n_j.  Every one of
 * these n_i x n_j words is written (no memset) and nothing else: the columns [n_j, ld_out) of a wider row keep their bytes.
 *
 * ldx_ld_rect_hits_dev / ldx_ld_rect_hits_dosage_dev: every pair with s = c *f32 c >= r2_bound (ONE IEEE float32 multiply;
 * r2_bound a float32 > 0, so a degenerate pair and a cell with num == 0 are never kept: ldx_ld_neighbors_dev's rule) is stored
 * as the record {query = i, oppos = j, r_square = c, d_prime = s} -- once per (i, j): the orientation is the rectangle's.
 * hits: capacity hit_cap, written in arbitrary order; *n_hits (device uint64, zeroed by the call) receives the number of slots
 * RESERVED (batches of 256 per wave; unused slots carry query == UINT32_MAX), as for ldx_area_scan_dev: if it exceeds hit_cap
 * only the first hit_cap slots were stored -- retry with a larger buffer.  ldx_area_finish_ex_dev(n_snps = n_i, counts_ready
 * = 0) turns the slots into a CSR over the rows of I: records sorted by (i, j), row i's at [offsets[i], offsets[i + 1]).
 *
 * Argument rules, checked before any HIP call (ldx_last_error() names the argument): a null pointer, n_i or n_j = 0, ld_out <
 * n_j, r2_bound not > 0, an odd n_hap in the dosage forms = LDX_E_ARG; n_hap > LDX_MAX_HAPS, or a bit plane of 4 GiB or more
 * on either side = LDX_E_UNSUPPORTED.  All calls only enqueue work on `stream`. */
int ldx_ld_rect_dev(const void *alt_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                    const void *alt_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                    uint32_t n_hap, float *out, size_t ld_out, void *stream);
int ldx_ld_rect_dosage_dev(const void *alt_i, const double *gstat_i, uint32_t n_i,
                           const void *alt_j, const double *gstat_j, uint32_t n_j,
                           uint32_t n_hap, float *out, size_t ld_out, void *stream);
int ldx_ld_rect_hits_dev(const void *alt_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                         const void *alt_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                         uint32_t n_hap, float r2_bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, void *stream);
int ldx_ld_rect_hits_dosage_dev(const void *alt_i, const double *gstat_i, uint32_t n_i,
                                const void *alt_j, const double *gstat_j, uint32_t n_j,
                                uint32_t n_hap, float r2_bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits,
                                void *stream);

/* ---- pairwise-complete LD: the rectangle's r over the observations called at BOTH SNPs -----------------------------------
 * The entries above keep every haplotype in n and leave a missing call out of the allele counts (the dosage forms count it as
 * REF).  PLINK --r2, Haploview and the LDpred / bigsnpr readers compute each pair's correlation over the samples called at both
 * variants instead.  These entries do that for the rectangle; they take BOTH bit planes of a panel (called = alt | ref) and its
 * acnt / rcnt tables.  For row x of I and row y of J over the same n_hap haplotypes:
 *
 * haplotype form (dosage = 0).  Haplotype h is jointly called when both codes are 0 or 1.
 *     n = #{h jointly called}    a = #{x = 1 and y called}    b = #{x called and y = 1}    c = #{x = 1 and y = 1}       (<= 10 240)
 *     num = fma(c, n, -(a b))    v_x = a (n - a)    v_y = b (n - b)
 * dosage form (dosage != 0; n_hap even, individual k owns haplotypes 2k and 2k + 1).  An individual is called at a SNP when
 * BOTH of its codes are 0 or 1 -- a half-missing genotype is missing (PLINK's rule, not the dosage entries' missing = REF);
 * g = the ALT dosage of a called individual.  Over the individuals called at both SNPs:
 *     N    A = sum g_x    B = sum g_y    HA = #{g_x = 2}    HB = #{g_y = 2}    S = sum g_x g_y
 *     num = fma(S, N, -(A B))    v_x = N (A + 2 HA) - A^2    v_y = N (B + 2 HB) - B^2
 * the cell, in fp64 with every operation rounded as written (r32_cell's arithmetic on the pair's own counts):
 *     rs = 1 / sqrt(v) (0 for v = 0);   cell = (float)(num (rs_x rs_y));   -0.0f where either variance is 0 (n = 0 and N = 0
 *     included);   +0.0f exactly where num = 0.
 * Consequences: a pair of rows without a missing code gives the ldx_ld_rect_dev (ldx_ld_rect_dosage_dev) cell bit for bit;
 * every cell is within 4 float32 ulps of the exact r of its counts; the cell is a function of the integers alone, symmetric in
 * the two SNPs: swapped sides give the transpose, permuted individuals (dosage form: rephased genotypes too) the same bits.
 * The integers come from the FP4 matrix cores (ldx_pwc.hip); a tile none of whose SNPs has a missing code counts c (S) alone
 * and reads the rest from acnt -- through the same cell functions, so a cell does not depend on its tile.  No workspace.
 *
 * ldx_ld_rect_pw_dev: out[i * ld_out + j] = the cell for i < n_i, j < n_j; exactly these words are written.
 * ldx_ld_rect_pw_hits_dev: ldx_ld_rect_hits_dev's records, rule (ONE float32 multiply against r2_bound > 0; -0.0f never a hit),
 *   slots and overflow protocol; ldx_area_finish_ex_dev(n_snps = n_i, counts_ready = 0) finishes.
 * ldx_ld_rect_pw_counts_dev: counts[(s * n_i + i) * ld + j] = integer s of the pair as uint32, s in the order n a b c (4 sets)
 *   or N A B HA HB S (6 sets): what the K loop produced, before any float.
 *
 * Argument rules and codes are ldx_ld_rect_dev's, checked before any HIP call: a null pointer, n_i or n_j = 0, ld < n_j,
 * r2_bound not > 0, an odd n_hap with dosage = LDX_E_ARG; n_hap > LDX_MAX_HAPS or a bit plane of 4 GiB or more =
 * LDX_E_UNSUPPORTED.  All calls only enqueue work on `stream`. */
int ldx_ld_rect_pw_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                       const void *alt_j, const void *ref_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                       uint32_t n_hap, int dosage, float *out, size_t ld_out, void *stream);
int ldx_ld_rect_pw_hits_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                            const void *alt_j, const void *ref_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                            uint32_t n_hap, int dosage, float r2_bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits,
                            void *stream);
int ldx_ld_rect_pw_counts_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                              const void *alt_j, const void *ref_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                              uint32_t n_hap, int dosage, uint32_t *counts, size_t ld, void *stream);

/* ---- pairwise-complete bands: the band operators over the observations called at BOTH SNPs ---------------------------------
 * The windowed operators above (ldx_ld_band_dev, ldx_ld_score_dev, ldx_ld_neighbors_dev and their dosage forms) keep every
 * haplotype in n, or count a missing call as REF.  These three are their pairwise-complete forms: for every pair i > j of ONE
 * panel with pos_i - pos_j <= window the cell is the cell of ldx_ld_rect_pw_dev for that panel against itself at (i, j), bit for
 * bit -- the same integers (n a b c / N A B HA HB S), the same cell functions, -0.0f on a degenerate pair, +0.0f iff num = 0,
 * within 4 float32 ulps of the exact r of its counts, symmetric in its two SNPs.  A kernel of its own on the FP4 matrix cores
 * (ldx_pwband.hip), which walks the 256 x 128 tiles of the lower band only.
 *
 * Every entry takes both bit planes of the panel, its acnt / rcnt tables, `dosage` (0: haplotype form; else the dosage form,
 * n_hap even), `hom` -- the uint32 table of ldx_dosage_stats_dev, read for rows without a missing code only, where it IS HA;
 * NULL unless dosage --, positions (int64 [n_snps], NON-DECREASING, duplicates allowed) and window >= 0 in their units (values
 * above 2^52 act as 2^52; the comparison is (double)pos_i - (double)pos_j <= window, ldx_ld_band_layout_dev's).
 *
 * ldx_pw_snp_stats_dev: the diagonal such a band goes with, over each SNP's OWN called set (it takes no window).  Haplotype
 *   form: live iff acnt rcnt > 0.  Dosage form: over the individuals with both codes called -- N of them, A the sum of their
 *   dosages, HA homozygous ALT -- live iff N (A + 2 HA) - A^2 > 0.  diag[i] (float32 [n_snps]) = +1.0f if live, else -0.0f;
 *   live (uint8 [n_snps], or NULL) = 1 / 0.  On a panel without missing codes diag is the diagonal of ldx_ld_band_dev.
 * ldx_ld_pw_band_dev: values[offsets[i] + j - lo[i]] = the cell, in the layout of ldx_ld_band_layout_dev for the same positions
 *   and window.  The guard is ldx_ld_band_dev's -- a store only where lo[i] <= j < i and the index is < n_cells -- so every one of
 *   the offsets[n_snps] cells is written (no memset) and nothing else.  values may be NULL when n_cells is 0.  The stored band
 *   is a band like any other: ldx_band_score_dev and ldx_band_matvec_dev take it with the diagonal above.
 * ldx_ld_pw_score_dev: ldx_ld_score_dev's sums over these cells: term = rint(2^32 (c *f32 c)) added to sums[i][0] and sums[j][0],
 *   to sums[i][1 + k] where annot[j] has bit k and to sums[j][1 + k] where annot[i] has it (n_annot <= 8; annot NULL iff
 *   n_annot = 0), as 64-bit integer atomics.  SNP i's own term, rint(2^32 diag[i]^2) -- 2^32 where it is live, else 0 --,
 *   initialises sums[i][0] and the words 1 + k whose bit annot[i] has: sums (uint64 [n_snps][1 + n_annot]) needs no memset.
 *   diag: ldx_pw_snp_stats_dev's.  The band is walked once per word: 1 + n_annot passes.
 * ldx_ld_pw_neighbors_dev: every pair with s = c *f32 c >= r2_bound (ONE float32 multiply; r2_bound a float32 > 0) as the
 *   records {i, j, c, s} and {j, i, c, s}, in the slots of ldx_ld_rect_pw_hits_dev (*n_hits is zeroed by the call and receives
 *   the slots reserved; beyond hit_cap nothing is stored).  ldx_area_finish_ex_dev(counts_ready = 0) turns the slots into the
 *   per-SNP neighbour CSR of ldx_ld_neighbors_dev.
 *
 * workspace: ldx_ld_pw_band_workspace_bytes(n_snps) bytes, 256-byte aligned, no initialisation needed (the call's first kernels
 * write what the band kernel reads: each row's first in-window column and the tiles in front of each block of 256 rows): ONE
 * workspace per launch that may be in flight.  Argument rules, checked before any HIP call (ldx_last_error() names the
 * argument): a null pointer, n_snps or n_hap = 0, a negative window, r2_bound not > 0, an odd n_hap with dosage, n_annot > 8, a
 * workspace too small = LDX_E_ARG; n_hap > LDX_MAX_HAPS or a bit plane of 4 GiB or more = LDX_E_UNSUPPORTED.  All calls only
 * enqueue work on `stream`: no allocation, no synchronisation, no library state. */
size_t ldx_ld_pw_band_workspace_bytes(uint32_t n_snps);
int ldx_pw_snp_stats_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                         uint32_t n_hap, int dosage, float *diag, uint8_t *live, void *stream);
int ldx_ld_pw_band_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, const uint32_t *hom,
                       uint32_t n_snps, uint32_t n_hap, int dosage, const int64_t *positions, int64_t window,
                       const uint32_t *lo, const uint64_t *offsets, float *values, uint64_t n_cells, void *workspace,
                       size_t workspace_bytes, void *stream);
int ldx_ld_pw_score_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, const uint32_t *hom,
                        uint32_t n_snps, uint32_t n_hap, int dosage, const int64_t *positions, int64_t window,
                        const uint8_t *annot, uint32_t n_annot, const float *diag, uint64_t *sums, void *workspace,
                        size_t workspace_bytes, void *stream);
int ldx_ld_pw_neighbors_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, const uint32_t *hom,
                            uint32_t n_snps, uint32_t n_hap, int dosage, const int64_t *positions, int64_t window,
                            float r2_bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, void *workspace,
                            size_t workspace_bytes, void *stream);

/* ---- unphased LD by EM: maximum-likelihood r and D' of every row of one SNP set against every row of another ---------------
 * The dosage entries above give Weir's composite r of the genotypes.  These give what PLINK --r2 dprime / --ld and Haploview
 * compute from unphased genotypes: the maximum-likelihood two-locus haplotype frequency, the double heterozygotes resolved by
 * EM (Hill 1974), and from it r and D'.  Panels, individuals and dosages are those of the dosage entries: n_hap even, N =
 * n_hap / 2, individual k owns haplotypes 2k and 2k + 1, g in {0, 1, 2} counts code-1 alleles only (a missing code or a second
 * ALT acts as REF), T = 2 N.  For row i of I and row j of J:
 *     a_i = sum_k g_ik (= acnt[i])    a_j likewise
 *     S   = sum_k g_ik g_jk           (the dosage entries' S, <= 4 N)
 *     H   = #{k : g_ik = 1 and g_jk = 1}      (double heterozygotes, <= N)
 *   haplotypes of known phase (integers >= 0; S - H is always even):
 *     n1 = (S - H) / 2          ALT.ALT        n2 = a_i - n1 - H         ALT.REF
 *     n3 = a_j - n1 - H         REF.ALT        n4 = T - a_i - a_j + n1   REF.REF         n1 + n2 + n3 + n4 + 2 H = T
 *   x in [0, H] = expected number of double heterozygotes in coupling phase:
 *     h1 = n1 + x, h4 = n4 + x, h2 = n2 + H - x, h3 = n3 + H - x
 *     g(x) = x h2 h3 - (H - x) h1 h4      (a cubic with leading coefficient 2, g(0) <= 0 <= g(H))
 *     l(x) = n1 ln h1 + n2 ln h2 + n3 ln h3 + n4 ln h4 + H ln(h1 h4 + h2 h3)         (0 ln 0 = 0)
 * l' has the sign of -g, so the local maxima of l on [0, H] are the roots of g on its rising branches, at most two.  x* is
 * the maximiser of l over [0, H]; where both local maxima have the same l in the kernel's own fp64 evaluation, x* is the
 * SMALLER x.  Then
 *     p = (n1 + x*) / T,  pA = a_i / T,  pB = a_j / T,  D = p - pA pB
 *     r  = D / sqrt(pA (1 - pA) pB (1 - pB))
 *     D' = |D| / Dmax,  Dmax = min(pA (1 - pB), (1 - pA) pB) if D >= 0,  min(pA pB, (1 - pA)(1 - pB)) if D < 0
 * (calc_ld.py's convention: D' >= 0, the sign lives in r).  Cells are float32:
 *   degenerate pair (a_i in {0, T} or a_j in {0, T}): both cells -0.0f.  An all-heterozygous SNP (pA = 1/2) is LIVE here,
 *     unlike in the dosage entries.
 *   H = 0: x* = 0, the pair is fully phased; r is then +0.0f iff T n1 - a_i a_j = 0.  No other exact-zero promise is made.
 *   accuracy: each cell is within 2 float32 ulps of the exact value plus 2^-40 absolute.
 *   determinism: a cell is a function of (N, a_i, a_j, S, H) only, evaluated in fp64 by an arithmetic symmetric in the two
 *     SNPs: rephasing, permuting individuals, or swapping the sides (transposed output) gives bit-identical cells.
 * S and H come from the FP4 matrix cores in one K loop (ldx_em.hip: S as the dosage rectangle counts it, H from the het bits
 * (w ^ (w >> 1)) & 0x5555...); no workspace, no library state.
 *
 * ldx_ld_em_rect_dev: out_r[i * ld_out + j] = r, out_dprime[i * ld_out + j] = D' for i < n_i, j < n_j.  Either output may be
 *   NULL, not both.  Exactly the n_i x n_j words of each given output are written: the columns [n_j, ld_out) keep their bytes.
 * ldx_ld_em_rect_hits_dev: every pair with r *f32 r >= r2_bound (ONE IEEE float32 multiply; r2_bound a float32 > 0, so a
 *   degenerate pair is never kept) as the record {query = i, oppos = j, r_square = the r cell, d_prime = the D' cell}.  Slots,
 *   batches, *n_hits and overflow are ldx_ld_rect_hits_dev's; ldx_area_finish_ex_dev(n_snps = n_i, counts_ready = 0) finishes.
 * ldx_ld_em_counts_dev: S[i * ld + j], H[i * ld + j] = the two counts as uint32 (no acnt needed): what the K loop produced.
 * ldx_ld_em_from_counts_dev: the epilogue alone on m tuples (a1[k], a2[k], S[k], H[k]) of n_ind individuals -- the device
 *   function the kernel calls: r[k], dprime[k] the cells, x[k] = x* as a double.  Any output may be NULL.  A tuple that is no
 *   genotype table (S - H odd, a negative n, a > 2 n_ind, H > n_ind) gives NaN in every output.
 *
 * Argument rules, checked before any HIP call (ldx_last_error() names the argument): a null pointer, n_i, n_j, m or n_ind = 0,
 * ld < n_j, r2_bound not > 0, an odd n_hap = LDX_E_ARG; n_hap > LDX_MAX_HAPS (n_ind > LDX_MAX_HAPS / 2), or a bit plane of
 * 4 GiB or more on either side = LDX_E_UNSUPPORTED.  All calls only enqueue work on `stream`. */
int ldx_ld_em_rect_dev(const void *alt_i, const uint32_t *acnt_i, uint32_t n_i,
                       const void *alt_j, const uint32_t *acnt_j, uint32_t n_j,
                       uint32_t n_hap, float *out_r, float *out_dprime, size_t ld_out, void *stream);
int ldx_ld_em_rect_hits_dev(const void *alt_i, const uint32_t *acnt_i, uint32_t n_i,
                            const void *alt_j, const uint32_t *acnt_j, uint32_t n_j,
                            uint32_t n_hap, float r2_bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, void *stream);
int ldx_ld_em_counts_dev(const void *alt_i, uint32_t n_i, const void *alt_j, uint32_t n_j, uint32_t n_hap,
                         uint32_t *S, uint32_t *H, size_t ld, void *stream);
int ldx_ld_em_from_counts_dev(uint32_t n_ind, size_t m, const uint32_t *a1, const uint32_t *a2, const uint32_t *S,
                              const uint32_t *H, float *r, float *dprime, double *x, void *stream);

/* ---- pairwise-complete EM: unphased LD by EM over the individuals called at BOTH SNPs -----------------------------------------
 * The EM entries above count a missing code as REF, which biases r and D' on the data they are meant for: unphased call sets
 * are the ones that carry missing calls.  PLINK --r2 dprime / --ld and Haploview estimate each pair's haplotype frequencies
 * over the individuals called at both variants; these entries do that.  Panels and individuals are those of the dosage form of
 * the pairwise-complete entries: both bit planes and the acnt / rcnt tables of each panel, n_hap even, individual k owns
 * haplotypes 2k and 2k + 1 and is CALLED at a SNP when BOTH of its codes are 0 or 1 -- a half-missing genotype is missing, a
 * second-ALT code is missing -- and g is the ALT dosage of a called individual.  For row x of I and row y of J, over the
 * individuals called at both:
 *     N    A = sum g_x    B = sum g_y    S = sum g_x g_y    H = #{g_x = 1 and g_y = 1}        (N, H <= 5120; A, B <= 10 240; S <= 20 480)
 * and the two cells are those of the section above with the pair's OWN N, A and B in the place of n_hap / 2, acnt[i] and
 * acnt[j]: T = 2 N, a_i = A, a_j = B, the same table n1 .. n4, the same x*, r and D' -- one device function, em_cell
 * (ldx_em_tile.h), shared by both kernels, so a cell cannot depend on the kernel or the tile it came from.  Consequences:
 *   a pair of rows without a missing code gives the ldx_ld_em_rect_dev cell bit for bit;
 *   both cells are -0.0f when N = 0, or when A or B is 0 or 2 N within the joint set -- a SNP that is polymorphic overall but
 *     monomorphic among the jointly called individuals included;
 *   accuracy is the section above's: each cell within 2 float32 ulps of the exact value of its integers plus 2^-40 absolute;
 *   a cell is a function of (N, A, B, S, H) alone, symmetric in the two SNPs: swapped sides give the transpose, permuted
 *     individuals and rephased genotypes identical bits.
 * The integers come from the FP4 matrix cores (ldx_em.hip, the same kernel template), five exact fp32 accumulator sets from three per-individual
 * operands on each side; a 128 x 128 tile none of whose SNPs has acnt + rcnt != n_hap runs the two-set loop of the section
 * above and reads N, A and B from n_hap / 2 and acnt.  No workspace, no library state.
 *
 * ldx_ld_em_rect_pw_dev: ldx_ld_em_rect_dev's outputs and output rules (either of out_r, out_dprime may be NULL, not both;
 *   exactly the n_i x n_j words of each given output are written).
 * ldx_ld_em_rect_pw_hits_dev: ldx_ld_em_rect_hits_dev's records {i, j, the r cell, the D' cell}, rule (ONE float32 multiply
 *   against r2_bound > 0; -0.0f never a hit), slots and overflow; ldx_area_finish_ex_dev(n_snps = n_i, counts_ready = 0) finishes.
 * ldx_ld_em_pw_counts_dev: counts[(s * n_i + i) * ld + j] = integer s of the pair as uint32, s in the order N A B S H: what
 *   the K loop produced (the shortcut: what it read from the tables), before any float.
 * ldx_ld_em_from_counts_pw_dev: the epilogue alone on m tuples (N[k], a1[k], a2[k], S[k], H[k]) -- ldx_ld_em_from_counts_dev with
 *   a per-tuple N.  A tuple that is no genotype table (or has N > LDX_MAX_HAPS / 2) gives NaN in every output; N = 0 with every
 *   other integer 0 is the degenerate pair: -0.0f, x = 0.  Any output may be NULL.
 *
 * Argument rules and codes are those of the EM and pairwise-complete entries, checked before any HIP call (ldx_last_error()
 * names the argument): a null pointer, n_i, n_j or m = 0, ld < n_j, r2_bound not > 0, an odd n_hap = LDX_E_ARG; n_hap >
 * LDX_MAX_HAPS or a bit plane of 4 GiB or more on either side = LDX_E_UNSUPPORTED.  All calls only enqueue work on `stream`. */
int ldx_ld_em_rect_pw_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                          const void *alt_j, const void *ref_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                          uint32_t n_hap, float *out_r, float *out_dprime, size_t ld_out, void *stream);
int ldx_ld_em_rect_pw_hits_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                               const void *alt_j, const void *ref_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                               uint32_t n_hap, float r2_bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, void *stream);
int ldx_ld_em_pw_counts_dev(const void *alt_i, const void *ref_i, const uint32_t *acnt_i, const uint32_t *rcnt_i, uint32_t n_i,
                            const void *alt_j, const void *ref_j, const uint32_t *acnt_j, const uint32_t *rcnt_j, uint32_t n_j,
                            uint32_t n_hap, uint32_t *counts, size_t ld, void *stream);
int ldx_ld_em_from_counts_pw_dev(size_t m, const uint32_t *N, const uint32_t *a1, const uint32_t *a2, const uint32_t *S,
                                 const uint32_t *H, float *r, float *dprime, double *x, void *stream);

/* ---- EM on the band: the EM r and D' of the in-window pairs of one panel, stored or as neighbour lists -----------------------
 * The EM entries above give a rectangle; the standard request -- PLINK --r2 dprime --ld-window-kb over a chromosome -- is the
 * band of ONE panel.  For every pair i > j with pos_i - pos_j <= window the two cells are those of ldx_ld_em_rect_dev
 * (pairwise != 0: ldx_ld_em_rect_pw_dev) for that panel against itself at (i, j), bit for bit: the same integers through the
 * same device function em_cell.  A kernel of its own on the FP4 matrix cores (ldx_emband.hip), which walks the 128 x 128
 * tiles of the lower band only and runs the fp64 root search for the cells inside the window only.
 *
 * Every entry takes the panel's ALT plane and acnt table; `pairwise` (0: a missing code counts as REF, N = n_hap / 2; else
 * every pair over the individuals called at both SNPs) and then also the REF plane and the rcnt table, which may be NULL
 * only when pairwise is 0; n_hap even; positions (int64 [n_snps], NON-DECREASING, duplicates allowed) and window >= 0 in
 * their units (values above 2^52 act as 2^52; the comparison is (double)pos_i - (double)pos_j <= window).
 *
 * ldx_em_snp_stats_dev: per SNP, over its OWN called individuals (it takes no window): N[i] of them and A[i] the sum of their
 *   dosages (pairwise = 0: n_hap / 2 and acnt[i]); live iff 0 < A < 2 N -- the SNP has both alleles among them.  This is not
 *   ldx_pw_snp_stats_dev's dosage `live`: an all-heterozygous SNP has no dosage variance but is a live EM SNP.  diag[i]
 *   (float32 [n_snps]) = +1.0f if live, else -0.0f: the band's diagonal is DEFINED, not computed by em_cell (whose tie rule
 *   gives -1 for an all-heterozygous SNP against itself).  N, A uint32 [n_snps]; live uint8 [n_snps] or NULL.
 * ldx_ld_em_band_dev: values_r[offsets[i] + j - lo[i]] = r, values_dprime[the same] = D', in the layout of
 *   ldx_ld_band_layout_dev for the same positions and window.  Either output may be NULL, not both (both only when n_cells is
 *   0, which returns LDX_OK and launches nothing).  The guard is ldx_ld_pw_band_dev's -- a store only where lo[i] <= j < i and
 *   the index is < n_cells -- so every one of the offsets[n_snps] cells is written (no memset) and nothing else.  values_r with
 *   the diagonal above is a band like any other: ldx_band_score_dev and ldx_band_matvec_dev take it.
 * ldx_ld_em_neighbors_dev: every pair with r *f32 r >= r2_bound (ONE float32 multiply; r2_bound a float32 > 0, so -0.0f is
 *   never kept) as the records {i, j, r, D'} and {j, i, r, D'} -- the fourth word carries the D' cell, as in
 *   ldx_ld_em_rect_hits_dev, not r^2 -- in the slots of ldx_ld_rect_hits_dev (*n_hits is zeroed by the call and receives the slots
 *   reserved; beyond hit_cap nothing is stored).  ldx_area_finish_ex_dev(counts_ready = 0) turns the slots into the per-SNP
 *   neighbour CSR of ldx_ld_neighbors_dev.
 *
 * workspace: ldx_ld_em_band_workspace_bytes(n_snps) bytes, 256-byte aligned, no initialisation needed (the call's first
 * kernels write what the band kernel reads: each row's first in-window column and the tiles in front of each block of 128
 * rows): ONE workspace per launch that may be in flight.  Argument rules, checked before any HIP call (ldx_last_error() names
 * the argument): a null pointer (ref, rcnt: only with pairwise), n_snps or n_hap = 0, an odd n_hap, a negative window, r2_bound
 * not > 0, both value pointers NULL with n_cells > 0, a workspace too small = LDX_E_ARG; n_hap > LDX_MAX_HAPS or a bit plane of
 * 4 GiB or more = LDX_E_UNSUPPORTED.  All calls only enqueue work on `stream`: no allocation, no synchronisation, no library
 * state. */
size_t ldx_ld_em_band_workspace_bytes(uint32_t n_snps);
int ldx_em_snp_stats_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                         uint32_t n_hap, int pairwise, uint32_t *N, uint32_t *A, float *diag, uint8_t *live, void *stream);
int ldx_ld_em_band_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                       uint32_t n_hap, int pairwise, const int64_t *positions, int64_t window, const uint32_t *lo,
                       const uint64_t *offsets, float *values_r, float *values_dprime, uint64_t n_cells, void *workspace,
                       size_t workspace_bytes, void *stream);
int ldx_ld_em_neighbors_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                            uint32_t n_hap, int pairwise, const int64_t *positions, int64_t window, float r2_bound,
                            ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, void *workspace, size_t workspace_bytes,
                            void *stream);

/* ---- Gabriel blocks: D' confidence bounds on the EM band, candidates and block picking ----------------------------------------
 * This project's own definition, written after Gabriel et al. 2002 and Haploview's defaults; NOT validated against PLINK
 * --blocks or Haploview.  All thresholds are integers in percent, so everything behind the two bounds is integer logic.
 *
 * The bounds of a pair (device function ci_cell, ONE function of N, a_i, a_j, S, H; T, n1..n4, H as in the EM section):
 *   no genotype table, or a_i or a_j in {0, T}: lo = hi = 0xFF, "no interval" (neither strong nor recombinant).
 *   s = -1 iff the pair's em_cell r cell is < 0, else +1; Dm = min(a_i (T - a_j), (T - a_i) a_j) for s = +1,
 *   min(a_i a_j, (T - a_i)(T - a_j)) for s = -1.  For k = 0 .. 100: h1 = (a_i a_j + s k Dm / 100) / T, h2 = a_i - h1,
 *   h3 = a_j - h1, h4 = T - a_i - a_j + h1, each clamped below at 2^-20;
 *   L_k = n1 ln h1 + n2 ln h2 + n3 ln h3 + n4 ln h4 + H ln(h1 h4 + h2 h3), a term with count 0 skipped;
 *   w_k = exp(L_k - max L), W = sum w_k ascending.  lo = (the smallest k with sum_{m <= k} w_m > 0.05 W) - 1, floored at 0;
 *   hi = (the largest k with sum_{m >= k} w_m > 0.05 W) + 1, capped at 100; the sums run from their own end.  fp64.
 * ldx_ld_ci_from_counts_dev: that function alone on m tuples (N per tuple, as ldx_ld_em_from_counts_pw_dev).
 * ldx_ld_em_ci_band_dev: ldx_ld_em_band_dev's arguments and rules, with `keep` (uint8 [n_snps], NULL = all) and the two bound
 *   arrays (uint8 [n_cells]) in place of the float values: ci_lo / ci_hi[offsets[i] + j - lo[i]] for every in-window pair
 *   i > j of kept SNPs; every other cell of the layout is 0xFF and runs no likelihood surface.  Every one of the n_cells cells
 *   is written by the call (a fill in front of the band): no memset by the caller.
 *
 * Candidates (ldx_gabriel_candidates_dev), on the stored bounds and `keep` -- the caller folds MAF and `live` into it:
 *   a pair of kept SNPs is strong at cut c iff lo != 0xFF, lo >= c and hi >= strong_hi (98); recombinant iff hi < recomb_hi (90).
 *   A candidate is first < last, both kept, in each other's window (a cell of the layout), the pair strong at cand_cut (70).
 *   m = the kept SNPs in [first, last], span = pos_last - pos_first, row = m - 2 capped at 3:
 *       m      cut[row]   max_span[row]      min_informative[row]
 *       2      80         20 000             1
 *       3      50         30 000             3
 *       4      50         window (-1)        6
 *       >= 5   70         window (-1)        6
 *   nS = the strong pairs at cut[row], nR = the recombinant pairs, over all pairs of kept SNPs inside [first, last].  Valid iff
 *   span <= max_span[row], nS + nR >= min_informative[row] and frac_den nS > frac_num (nS + nR) (20, 19: more than 95 %).
 *   The list has one slot per cell of the layout, column-major (first ascending, then last): cand_span[slot] = the span of a
 *   valid candidate, -1 otherwise; cand_first / cand_last[slot] always.  params NULL = the defaults above
 *   (ldx_gabriel_default_params writes them).
 * Pick (ldx_gabriel_pick_dev): the caller sorts cand_span descending with a STABLE sort -- ties stay ordered by smaller first,
 *   then smaller last -- and passes the sorted spans and the permutation (order[k] = the slot at rank k).  Going down the valid
 *   candidates, one is accepted iff no SNP in [first, last] lies in an accepted block.
 *     block_of[i] (uint32 [n_snps]): the 0-based block, in position order, of SNP i; 0xFFFFFFFF for a SNP not kept (it may lie
 *                 between a block's ends and is no member); 0xFFFFFFFE for a kept SNP in no block;
 *     n_out[0]: the blocks;  n_out[1]: the valid candidates.
 * Workspaces (256-byte aligned, no initialisation needed, one per launch in flight): ldx_gabriel_candidates_workspace_bytes
 * (16 bytes per cell and 12 per SNP) and ldx_gabriel_pick_workspace_bytes.  n_cells = 0 (no pair in any window) is valid: the
 * candidates call does nothing and the pick call marks every kept SNP 0xFFFFFFFE.  Argument rules as for the EM band, checked
 * before any HIP call; the calls only enqueue work on `stream`. */
typedef struct ldx_gabriel_params {
    uint32_t cand_cut, strong_hi, recomb_hi;
    uint32_t cut[4];
    int64_t max_span[4];           /* negative: the window */
    uint32_t min_informative[4];
    uint32_t frac_num, frac_den;
} ldx_gabriel_params;
void ldx_gabriel_default_params(ldx_gabriel_params *params);
int ldx_ld_ci_from_counts_dev(size_t m, const uint32_t *N, const uint32_t *a1, const uint32_t *a2, const uint32_t *S,
                              const uint32_t *H, uint8_t *lo, uint8_t *hi, void *stream);
int ldx_ld_em_ci_band_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                          uint32_t n_hap, int pairwise, const int64_t *positions, int64_t window, const uint8_t *keep,
                          const uint32_t *lo, const uint64_t *offsets, uint8_t *ci_lo, uint8_t *ci_hi, uint64_t n_cells,
                          void *workspace, size_t workspace_bytes, void *stream);
size_t ldx_gabriel_candidates_workspace_bytes(uint32_t n_snps, uint64_t n_cells);
size_t ldx_gabriel_pick_workspace_bytes(uint32_t n_snps);
int ldx_gabriel_candidates_dev(const uint8_t *ci_lo, const uint8_t *ci_hi, const uint32_t *lo, const uint64_t *offsets,
                               uint64_t n_cells, const int64_t *positions, const uint8_t *keep, uint32_t n_snps, int64_t window,
                               const ldx_gabriel_params *params, int64_t *cand_span, uint32_t *cand_first, uint32_t *cand_last,
                               void *workspace, size_t workspace_bytes, void *stream);
int ldx_gabriel_pick_dev(const int64_t *sorted_span, const int64_t *order, const uint32_t *cand_first, const uint32_t *cand_last,
                         uint64_t n_cells, const uint8_t *keep, uint32_t n_snps, uint32_t *block_of, uint32_t *n_out,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- sample relatedness: IBS counts and KING-robust kinship between the INDIVIDUALS of a panel -------------------------------
 * This project's own definitions, written after Manichaikul et al. 2010 (the between-family estimator); NOT validated against
 * PLINK 2 (--make-king-table, --king-cutoff, --distance ibs) or KING.
 *
 * Individual a owns haplotypes 2a and 2a + 1 (n_hap even).  At a SNP it is CALLED when both codes are 0 or 1 -- a half-missing
 * or second-ALT genotype is missing -- and then has the ALT dosage g in {0, 1, 2}.  A SNP is KEPT when it passes the optional
 * mask keep (uint8 [n_snps] of the panel, NULL = all); a SNP that is not kept counts as missing for everybody.
 * Counts of individuals a, b over the kept SNPs called in both, uint32:
 *     N[a][b]     SNPs jointly called                 HH[a][b]    #{g_a = 1 and g_b = 1}
 *     IBS0[a][b]  #{(g_a, g_b) = (0, 2) or (2, 0)}    HET[a][b]   #{g_a = 1 and b called}   (not symmetric: HET[b][a] is the partner's)
 * Derived, exact:  IBS1 = HET[a][b] + HET[b][a] - 2 HH,  IBS2 = N - IBS1 - IBS0,  sum (g_a - g_b)^2 = 4 IBS0 + IBS1.
 * Cells, each operation in fp64 rounded once, then one conversion (numpy reproduces them bit for bit), m = min(HET[a][b], HET[b][a]):
 *     kin = (float)(0.5 - (double)(4 IBS0 + IBS1) / (double)(4 m));    -0.0f where m == 0
 *     ibs = (float)((double)(2 IBS2 + IBS1) / (double)(2 N));          -0.0f where N == 0
 * On the diagonal kin[a][a] is 0.5f when a has a heterozygous kept call, else -0.0f.  Both are functions of the integers alone:
 * symmetric, and identical under permuted SNPs, rephased genotypes and a split of the SNPs over several calls.
 *
 * The transposed store (ldx_sample_planes_dev): three bit planes, in this order -- called, heterozygous, homozygous ALT -- each
 * a tiled plane as above with the axes exchanged: rows = individuals in slabs of 128, bits = the SNPs snp_begin .. snp_begin +
 * snp_count - 1 of the panel in chunks of 128 (16 bytes), n_chunks = 2 * ceil(snp_count / 256); element (slab s, chunk c, row r)
 * of a plane is the 16-byte group at ((s * n_chunks + c) * 128 + r) * 16, bit k % 128 of it SNP snp_begin + 128 c + k % 128 of
 * individual 128 s + r: a row's consecutive SNPs are 16-byte loads that consecutive rows coalesce.  A bit of a SNP that is not
 * kept, of a pad SNP or of a pad row is 0.  ldx_sample_planes_bytes(n_ind, snp_count) is the size of the three planes; the call
 * writes every byte of it and the tables: no memset by the caller.  tables (ldx_sample_tables_bytes, uint32): the called, the
 * heterozygous and the homozygous-ALT kept calls per individual -- [3][128 * ceil(n_ind / 128)] -- then the number of kept SNPs.
 * At most LDX_KING_MAX_STORE_SNPS SNPs per store; a longer panel is counted in several calls (accumulate).
 *
 * ldx_sample_counts_dev: counts[(k * n_ind + a) * ld + b], k in the order N, HH, IBS0, HET, the full square, from a store and its
 * tables.  accumulate = 0: the call first defines every word [a][b < n_ind]; accumulate = 1: it adds to what is there (chromosomes,
 * .bed chunks), n_prior being the SNPs already counted into `counts`: n_prior + n_snps may not pass 2^32 - 1 (LDX_E_ARG).
 * Work: (lower tile of 128 x 128 individuals) x (K slice); a slice's sums are exact fp32 integers -- every FP4 product is 1, so
 * slice SNPs <= LDX_KING_MAX_SLICE_SNPS < 2^24 -- converted to uint32 once and added with 32-bit integer atomics: bit-reproducible.
 * n_slices = 0 lets the library choose (about four rounds of workgroups, no slice under LDX_KING_MIN_SLICE_SNPS); a value of the
 * caller's is used as given (capped at the K-blocks of 256 SNPs) and refused with LDX_E_ARG when a slice would pass the bound.
 * A tile none of whose individuals misses a kept call takes N and HET from the tables; both paths end in the same integers.
 * ldx_king_from_counts_dev: the two cells on m tuples; ldx_sample_cells_dev: dense float32 [n_ind][ld_out] from the four count
 * planes.  Either of kin, ibs may be NULL, not both.  n_ind <= LDX_MAX_HAPS / 2.  Argument rules are checked before any HIP call. */
#define LDX_KING_MIN_SLICE_SNPS 65536u      /* the automatic choice makes no shorter slice: its atomics stay small beside its MFMAs */
#define LDX_KING_MAX_SLICE_SNPS 8388608u    /* 2^23: (largest product, 1) x (slice SNPs) < 2^24 */
#define LDX_KING_MAX_STORE_SNPS 134217728u  /* 2^27 SNPs in one store */
size_t ldx_sample_planes_bytes(uint32_t n_ind, uint32_t n_snps);
size_t ldx_sample_tables_bytes(uint32_t n_ind);
int ldx_sample_planes_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                          uint32_t snp_begin, uint32_t snp_count, void *store, uint32_t *tables, void *stream);
int ldx_sample_counts_dev(const void *store, const uint32_t *tables, uint32_t n_ind, uint32_t n_snps, uint32_t *counts,
                          size_t ld, int accumulate, uint64_t n_prior, uint32_t n_slices, void *stream);
int ldx_king_from_counts_dev(size_t m, const uint32_t *N, const uint32_t *HH, const uint32_t *IBS0, const uint32_t *HETa,
                             const uint32_t *HETb, float *kin, float *ibs, void *stream);
int ldx_sample_cells_dev(const uint32_t *counts, uint32_t n_ind, size_t ld, float *kin, float *ibs, size_t ld_out, void *stream);

/* ---- genotype products: the genotype matrix times a narrow dense matrix, both ways, from the bit planes ----------------------
 * This project's own definition, NOT validated against PLINK 2, GCTA or FastPCA.
 *
 * Individuals, called genotypes and kept SNPs are those of "sample relatedness" above.  g_ia in {0, 1, 2} is the ALT dosage of
 * individual a at SNP i (0 when missing), c_ia in {0, 1} says whether a is called at i; a SNP that is not kept is missing for
 * everybody.  The operator is A = [G | C]; all arithmetic is on integers:
 *     forward   y[a][c]  = sum_i ( g_ia w[i][c] + c_ia wc[i][c] )                          int64 [n_ind][k]
 *     reverse   z[i][c]  = sum_a g_ia u[a][c]      zc[i][c] = sum_a c_ia u[a][c]           int64 [n_snps][k] each
 * w, wc, u: int32 fixed-point values with |.| <= 2^30 (rows ld_w / ld_u apart), k in 1 .. LDX_GENO_MAX_COLS; wc may be NULL = 0.
 * The two are adjoint: sum u y == sum (w z + wc zc) exactly.  The sums do not depend on order or slicing: bit-reproducible.
 *
 * ldx_geno_matmul_dev: store and tables are what ldx_sample_planes_dev wrote for the same n_snps; row i of w belongs to SNP
 * snp_begin + i of that store.  accumulate = 0: the call first defines every word y[a][c < k]; accumulate = 1: it adds to what is
 * there (the stores of a long panel, chunks of a fileset).  Work: (slab of 128 individuals) x (32 columns) x (K slice of SNPs) on
 * the int8 matrix instruction: the genotype is the A operand, each weight four balanced base-256 digits in [-128, 127] (four
 * int8 columns), the int32 accumulators of the digits are recombined as sum_l 2^(8 l) acc_l in int64 at the end of the slice
 * and added to y with 64-bit integer atomics.  An accumulator takes at most 3 x 128 per SNP (g w and c wc), so slice SNPs <=
 * LDX_GENO_MAX_SLICE_SNPS.  n_slices = 0 lets the library choose; a value of the caller's is used as given (capped at the
 * K-blocks of 256 SNPs) and refused with LDX_E_ARG when a slice would pass the bound.  `tables` is part of the contract for a
 * shortcut on slabs without missing calls; the present kernel takes the general path everywhere and does not read it.
 *
 * ldx_geno_rmatmul_dev: alt, ref, keep as for ldx_sample_planes_dev.  Work: (slab of 128 SNPs) x (32 columns), K = all
 * individuals (2 x 128 x LDX_MAX_HAPS / 2 < 2^31), plain stores: every word z[i][c < k], zc[i][c < k] of every SNP is written
 * (0 for a SNP that is not kept), no memset by the caller.
 *
 * Argument rules, checked before any HIP call: a null pointer, an odd n_hap, k outside 1 .. LDX_GENO_MAX_COLS, a leading
 * dimension below k, n_ind or n_snps = 0, more than LDX_KING_MAX_STORE_SNPS SNPs in a store, an n_slices past the slice bound =
 * LDX_E_ARG; n_hap > LDX_MAX_HAPS (n_ind > LDX_MAX_HAPS / 2) or a bit plane of 4 GiB or more = LDX_E_UNSUPPORTED. */
#define LDX_GENO_MAX_COLS 64u
#define LDX_GENO_MAX_SLICE_SNPS 4194304u    /* 2^22: 3 x 128 x (slice SNPs) < 2^31 */
int ldx_geno_matmul_dev(const void *store, const uint32_t *tables, uint32_t n_ind, uint32_t n_snps, const int32_t *w,
                        const int32_t *wc, size_t ld_w, uint32_t k, int64_t *y, size_t ld_y, int accumulate, uint32_t n_slices,
                        void *stream);
int ldx_geno_rmatmul_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                         const int32_t *u, size_t ld_u, uint32_t k, int64_t *z, int64_t *zc, size_t ld_z, void *stream);

/* ---- weighted sample products: the genotype matrix against itself with a weight per SNP; the genetic relationship matrix ------
 * This project's own definition, written after Yang et al. 2011 (GCTA --make-grm, PLINK 2 --make-rel); NOT validated against
 * either program.
 *
 * Individuals, called genotypes, kept SNPs and the transposed store are those of "sample relatedness"; g_ia in {0, 1, 2} (0 when
 * the call is missing) and c_ia in {0, 1} those of "genotype products".  With three int32 weights per SNP of the store, |.| <=
 * LDX_WPROD_MAX_WEIGHT = 2^28, laid out int32 [n_snps][3] = {q2, q1, q0}, row i belonging to SNP snp_begin + i of the store:
 *     S[a][b] = sum_i ( q2_i g_ia g_ib + q1_i (g_ia c_ib + c_ia g_ib) + q0_i c_ia c_ib )          int64 [n_ind][ld], the full square
 * The sum is exact and symmetric and does not depend on SNP order, slicing or chunking: bit-reproducible.  A term is at most
 * (4 + 2 + 2 + 1) 2^28 < 2^32 in size, so across the 2^27 SNPs of the largest store every partial sum stays below 9 x 2^55 < 2^59;
 * sums of several stores stay exact while their SNPs together do not pass 2^31 (9 x 2^28 x 2^31 < 2^63).
 *
 * ldx_sample_wprod_dev: store and tables are what ldx_sample_planes_dev wrote for the same n_snps (tables is part of the contract
 * for a shortcut on tiles without missing calls; the present kernel takes the general path everywhere and does not read it).
 * accumulate = 0: the call first defines every word S[a][b < n_ind]; accumulate = 1: it adds to what is there (the stores of a long
 * panel, chromosomes, .bed chunks).  workspace: ldx_sample_wprod_workspace_bytes(n_snps) bytes, 16-byte aligned, written by the
 * call (the weights' digit table: 24 bytes per SNP); no initialisation.
 * PRECONDITION: every weight lies in -2^28 .. 2^28.  The entry cannot check device memory before its launch; the Python layer
 * does (ops.sample_wprod, one device reduction).  A weight outside the range gives wrong sums, never a fault.
 * Work: (lower tile of 128 x 128 individuals) x (K slice) on v_mfma_i32_32x32x32_i8.  With u_ib = q2_i g_ib + q1_i c_ib and
 * v_ib = q1_i g_ib + q0_i c_ib the sum is sum_i (g_ia u_ib + c_ia v_ib); u and v take three values per SNP among the called
 * (g = 0, 1, 2), each |.| <= 3 x 2^28 < 2^30: four balanced base-256 digits in [-128, 127] (x + 0x80808080 has them, plus 128, in
 * its bytes).  The row operand is g resp. c as int8, the column operand digit l of u resp. v, selected from a per-SNP table by
 * byte masks made of the column individual's bit planes; 8 MFMAs per 32 x 32 x 32, 1024 per 128 x 128 x 256 block, into four int32
 * accumulators per cell, recombined as sum_l 256^l acc_l in int64 at the end of the slice and added to S with 64-bit integer
 * atomics; the mirror-image tile is written from the same integers.  No floating-point atomics anywhere.
 * An accumulator takes at most |g d| + |c d'| <= 2 x 128 + 128 = 384 per SNP, so slice SNPs <= LDX_WPROD_MAX_SLICE_SNPS:
 * 384 x 2^22 = 3 x 2^29 < 2^31.  n_slices = 0 lets the library choose (about four rounds of workgroups, no slice under
 * LDX_WPROD_MIN_SLICE_SNPS); a value of the caller's is used as given (capped at the K-blocks of 256 SNPs) and refused with
 * LDX_E_ARG when a slice would pass the bound.
 * Argument rules, checked before any HIP call: a null pointer, n_ind or n_snps = 0, ld < n_ind, more than LDX_KING_MAX_STORE_SNPS
 * SNPs, a workspace that is too small or not aligned, an n_slices past the slice bound = LDX_E_ARG; n_ind > LDX_MAX_HAPS / 2 =
 * LDX_E_UNSUPPORTED.
 *
 * The genetic relationship matrix (ops.grm_weights, ops.ld_grm): per SNP, from the counts {n called, het, hom} of
 * ldx_geno_snp_counts_dev, s = het + 2 hom.  A SNP is LIVE when it is kept, 0 < s < 2n, and -- with a bound maf_min --
 * (double)min(s, 2n - s) / (double)(2n) >= maf_min.  For a live SNP, every operation in fp64 rounded once, in this order:
 *     p = (double)s / (double)(2n)      w = 1.0 / ((2.0 p) (1.0 - p))
 *     x2 = w      x1 = -((2.0 p) w)      x0 = ((4.0 p) p) w
 * All 3 n_live values are quantised as ONE column by the genotype products' rule with 28 scale bits: e = the smallest integer
 * with max |x| 2^-e <= 1 (0 when no SNP is live), q = rint(x 2^(28 - e)), round-half-even; a SNP that is not live gets (0, 0, 0).
 * Then S 2^(e - 28) = sum over the live SNPs called in both of w^ (g_a - 2 p^)(g_b - 2 p^) with the quantised coefficients, and
 * with N[a][b] the live SNPs called in both (ldx_sample_counts_dev over keep = live) the cell is GCTA's default,
 *     grm[a][b] = (float)( ((double)S[a][b] 2^(e - 28)) / (double)N[a][b] );      -0.0f where N[a][b] == 0
 * (the conversion of S rounds once, to nearest-even, the scaling is exact, the division rounds once: numpy reproduces the cell bit
 * for bit, ops.grm_cell_host).  A missing call DROPS OUT of the pair's sum and of its N, as in GCTA: this is the one place where
 * the library does NOT set a missing genotype to the SNP's mean (the association scans and sample_pca do).  S and N add over
 * chromosomes and chunks of a fileset -- each with the weights of its own SNPs but ONE exponent e: ops.ld_grm quantises a
 * chunk with the exponent it is given -- before the division.
 * Against the GRM of the unquantised rational weights: a coefficient is off by at most 2^(e - 29), the three multiply at most
 * 4, 4 and 1, so |S 2^(e - 28) - exact| <= 9 n_live 2^(e - 29), before the division by N.
 * ldx_grm_cells_dev: grm float32 [n_ind][ld_out] from S int64 [n_ind][ld_s] and N uint32 [n_ind][ld_n]; |exp| <= LDX_GRM_MAX_EXP. */
#define LDX_WPROD_SCALE_BITS 28
#define LDX_WPROD_MAX_WEIGHT 268435456      /* 2^28 */
#define LDX_WPROD_MIN_SLICE_SNPS 16384u     /* the automatic choice makes no shorter slice: its atomics stay small beside its MFMAs */
#define LDX_WPROD_MAX_SLICE_SNPS 4194304u   /* 2^22: (2 x 128 + 128) x (slice SNPs) < 2^31 */
#define LDX_GRM_MAX_EXP 900
size_t ldx_sample_wprod_workspace_bytes(uint32_t n_snps);
int ldx_sample_wprod_dev(const void *store, const uint32_t *tables, uint32_t n_ind, uint32_t n_snps, const int32_t *q, int64_t *S,
                         size_t ld, int accumulate, uint32_t n_slices, void *workspace, size_t workspace_bytes, void *stream);
int ldx_grm_cells_dev(const int64_t *S, size_t ld_s, const uint32_t *N, size_t ld_n, uint32_t n_ind, int exp, float *grm,
                      size_t ld_out, void *stream);

/* ---- association scan: per SNP the least-squares fit of quantitative phenotypes on the genotype, an intercept and covariates --
 * This project's own definition (what PLINK 2 --glm reports for a quantitative trait: BETA, SE, T_STAT, P), NOT validated
 * against PLINK 2.  It differs from PLINK wherever a call is missing: a missing genotype is set to the SNP's MEAN over its
 * called individuals (as regenie, BOLT-LMM and fastGWA do), PLINK refits each SNP over its called individuals.
 *
 * Individuals, called genotypes and kept SNPs are those of "genotype products" above (a half-missing genotype is missing); the
 * scan sees all N = n_ind individuals of the panel (a subset is taken first, with ldx_panel_select_dev).
 * Design (the host's part, numpy fp64: ops.glm_design): D = [1 | X] with n_cov columns, thin QR D = Q R (refused when
 * |R_aa| <= 2^-20 max |R| on R's diagonal, when df = N - n_cov - 1 < 1, or on a non-finite value), Y~ = Y - Q (Q^T Y); a column
 * of Y~ whose largest |entry| is <= 2^-40 times the largest |entry| of its phenotype AS GIVEN (not centred) is set to 0: a
 * phenotype in the span of D leaves only the rounding of the projection, which the quantiser would scale to 30 bits (so does a
 * spread below about 1e-12 of a large offset: centre such a phenotype first); U = [Q | Y~],
 * k = n_cov + n_pheno <= LDX_GENO_MAX_COLS columns, is quantised as ONE matrix by the weights' rule (q int32, exponents e:
 * u^ = q 2^(e - 30)).  From here on everything is a function of integers: yy_j = (double)(sum_a q_aj^2) 2^(2 (e_j - 30)), the
 * integer sum exact and rounded once; the quantised Q^ is TREATED as orthonormal -- part of the definition.
 * Per SNP, from counts {n called, het, hom} and the rows z, zc of the reverse product of q: s = het + 2 hom, e2 = het + 4 hom,
 *     mu = (double)s / (double)n            gg = (double)(n e2 - s^2) / (double)n         (the numerator an exact int64)
 *     h_a = ((double)z_a - mu (double)zc_a) 2^(e_a - 30),  a < n_cov       d = gg - (((h_0^2 + h_1^2) + h_2^2) + ...)
 * per cell (SNP, phenotype j), column c = n_cov + j:  b = ((double)z_c - mu (double)zc_c) 2^(e_c - 30),
 *     beta = b / d     s2 = (yy_j - (b b) / d) / df     se = sqrt(s2 / d)     t = beta / se
 *     p = 2 P(T_df <= -|t|) = I_x(df / 2, 1 / 2),  x = df / (df + t^2)      neglog10_p = -log10 p, evaluated from ln p
 * every operation in fp64 rounded once, in this order: beta, se, t and the flags are reproduced bit for bit by numpy
 * (ops.glm_linear_host).  The tail is a continued fraction (modified Lentz) with the front factor in log space, so neglog10_p is
 * finite where p underflows to 0; for x >= (a + 1) / (a + b + 2) the complement 1 - I_{1-x}(1 / 2, df / 2) is taken, 1 - x formed
 * as t^2 / (df + t^2); ln B(df / 2, 1 / 2) is one difference of lgamma values per call.  |ln p| is within 2^-30 max(1, |ln p|) of
 * the exact value.  t = 0 gives p = 1, neglog10_p = 0 exactly.
 * flags, uint8 per cell, the first that applies; 0 and 5 are finite results, every other flag is NaN in all five outputs:
 *     0 OK      1 SNP not kept, or n = 0      2 genotype constant among the called (n e2 = s^2)      3 d max_vif < gg
 *     4 yy_j = 0 (the phenotype is constant after the covariates)
 *     5 s2 <= 0, a perfect fit: beta as computed, se = 0, t = +-inf (beta's sign), p = 0, neglog10_p = +inf
 *     6 the tail's continued fraction passed 512 steps
 *
 * ldx_geno_snp_counts_dev: counts[i] = {called, het, hom ALT, 0} over the individuals of SNP i, from the panel's tiled planes
 * with the reverse product's own genotype words, so that they agree with z, zc by construction.  Work: a workgroup per slab of
 * 128 SNPs, popcounts, the two halves of a row meet in LDS; plain 16-byte stores: every word of every row is written (0 for a SNP
 * that is not kept).  counts must be 16-byte aligned; the other argument rules are ldx_geno_rmatmul_dev's.
 * ldx_glm_linear_dev: z, zc int64 [n_snps][ld_z] (columns 0 .. n_cov - 1 of Q, then the phenotypes), counts as above, exps int64
 * [n_cov + n_pheno], yy double [n_pheno]; beta, se, t, p, neglog10_p double [n_snps][ld_out] and flags uint8 [n_snps][ld_out]: the
 * words [i][j < n_pheno] are written, the padding is not touched.  Work: a workgroup per 128 SNPs; mu, gg, h, d and flags 1 - 3
 * once per SNP (a wave per SNP, lane a on column a), then a thread per cell.  A null pointer, n_snps, n_cov or n_pheno = 0, n_cov +
 * n_pheno > LDX_GENO_MAX_COLS, a leading dimension below its width, n_ind <= n_cov + 1, or a max_vif that is not > 1 = LDX_E_ARG,
 * checked before any HIP call. */
int ldx_geno_snp_counts_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                            uint32_t *counts, void *stream);
int ldx_glm_linear_dev(const int64_t *z, const int64_t *zc, size_t ld_z, const uint32_t *counts, uint32_t n_snps, uint32_t n_ind,
                       uint32_t n_cov, uint32_t n_pheno, const int64_t *exps, const double *yy, double max_vif, double *beta,
                       double *se, double *t, double *p, double *neglog10_p, uint8_t *flags, size_t ld_out, void *stream);

/* ---- logistic association scan: per SNP the maximum-likelihood logistic fit of 0/1 phenotypes on the genotype, an intercept and
 * covariates ----
 * This project's own definition (what PLINK 2 --glm reports for a case/control trait without its Firth fallback: log odds ratio,
 * SE, Z, P), NOT validated against PLINK 2.
 *
 * Individuals, called genotypes, kept SNPs and mean imputation are those of "association scan": the scan sees all N = n_ind
 * individuals of the panel (a subset is taken first); the genotype column of SNP i is x_a = g_ia - mu_i for a called individual
 * and 0 for a missing one, mu_i = s / n over the called.
 * For a phenotype y in {0,1}^N and the design D = [1 | X], X with n_cov <= LDX_LOGIT_MAX_COV columns (intercept + 13 covariates +
 * genotype = 15 parameters, one slot of a 16-wide tile left free):
 *     theta^ = (gamma^, beta^) maximises l(theta) = sum_a [ y_a eta_a - log(1 + e^eta_a) ],  eta = D gamma + x beta
 *     beta = beta^, the log odds ratio per ALT allele
 *     se = sqrt([I(theta^)^-1]_bb),  I(theta) = sum_a w_a v_a v_a^T,  v_a = (d_a, x_a),  w_a = mu_a (1 - mu_a),
 *          the information evaluated AT the reported theta^, not one step before it
 *     z = beta / se          p = erfc(|z| / sqrt 2)
 *     neglog10_p = -ln p / ln 10 with ln p formed in log space (ln erfcx(t) - t^2, t = |z| / sqrt 2, from t = 5 on): finite where
 *          p underflows to 0; z = 0 gives p = 1, neglog10_p = 0 exactly.  |ln p| is within 2^-30 max(1, |ln p|) of the exact value.
 * beta^ and se do not depend on the parametrisation of the span of D: they are functions of the codes, X and y.  The iteration
 * path is not part of the definition.
 * Design (the host's part, numpy fp64: ops.logit_design): thin QR of D with the refusals of "association scan"; B = sqrt(N) Q,
 * stored column-major [n_cov + 1][N]; per phenotype the null fit gamma_0 on B by Newton from 0.  A phenotype with no case, no
 * control, or a null fit that does not converge has a NaN row in theta0: every cell of it carries flag 4.
 * Iteration (the device and its numpy mirror, ops.ld_glm_logistic_host): undamped Newton from (gamma_0, 0); an evaluation forms
 * I and U = sum_a v_a (y_a - mu_a) at the current point and solves I delta = U by Cholesky; when the Newton decrement
 * lambda^2 = U^T I^-1 U <= 2^-60 that step is applied and I evaluated once more at the new point for se; at most
 * LDX_LOGIT_MAX_ITER evaluations.  mu and 1 - mu are formed from e^-|eta| without cancellation.
 * flags, uint8 per cell, the first that applies; every flag other than 0 is NaN in all five outputs:
 *     0 OK      1 SNP not kept, or n = 0      2 genotype constant among the called
 *     3 collinear with the design: d max_vif < xx,  xx = sum_a x_a^2 (from the integer counts, as gg of "association scan"),
 *       d = xx - sum_c (sum_a Q_ac x_a)^2;  max_vif > 1
 *     4 phenotype unusable (a NaN in its row of theta0)
 *     5 no finite maximiser found: the cap was reached, or I lost positive definiteness (a pivot that is not > 0, or not finite).
 *       This covers complete and quasi-complete separation.  PLINK would fall back to Firth regression here; this scan does not.
 * n_iter, uint8 per cell: the information evaluations made (0 for the flags 1 - 4).
 * Reproducibility: no floating-point atomics; the individuals are walked in a fixed order (K-groups of 4, the last one padded with
 * zeros).  A cell's bits depend on that cell's SNP, y and design alone -- not on the other SNPs or phenotypes of the call, on keep,
 * or on the launch.  numpy does not reproduce beta^ bit for bit (the device's exp and the MFMA's internal order are its own);
 * accuracy is stated against an exact oracle: |beta - beta_exact| <= 2^-40 se_exact, |se / se_exact - 1| <= 2^-40.
 *
 * ldx_glm_logistic_dev: alt, ref, keep as ldx_geno_snp_counts_dev, counts its result for the same keep; design double
 * [n_cov + 1][ld_design] (B above), y uint8 [n_pheno][ld_design], theta0 double [n_pheno][n_cov + 1]; beta, se, z, p, neglog10_p
 * double [n_snps][ld_out] and flags, n_iter uint8 [n_snps][ld_out]: the words [i][j < n_pheno] are written with plain stores, the
 * padding is not touched.  Work: one wave per cell, four cells per workgroup; per evaluation a pass over the individuals, 64 at
 * a time -- a lane per individual for eta, mu, w, r, then I and U on v_mfma_f64_16x16x4_f64 (U in the 16th column) -- and a
 * 15 x 15 Cholesky solve in the wave's registers.  A null pointer, an odd n_hap, n_snps or n_pheno = 0, n_pheno > 65535,
 * n_cov > LDX_LOGIT_MAX_COV, a leading dimension below its width, n_ind <= n_cov + 2, or a max_vif that is not > 1 = LDX_E_ARG,
 * checked before any HIP call. */
#define LDX_LOGIT_MAX_COV 13u
#define LDX_LOGIT_MAX_ITER 30u
int ldx_glm_logistic_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                         const uint32_t *counts, const double *design, size_t ld_design, uint32_t n_cov, const uint8_t *y,
                         const double *theta0, uint32_t n_pheno, double max_vif, double *beta, double *se, double *z, double *p,
                         double *neglog10_p, uint8_t *flags, uint8_t *n_iter, size_t ld_out, void *stream);

/* ---- Firth logistic association scan: the penalised-likelihood fit of the same model, as a fallback for the cells the
 * maximum-likelihood scan flags 5, or for every cell ----
 * This project's own definition (the estimate PLINK 2 --glm firth-fallback / firth and logistf aim at), NOT validated against
 * PLINK 2 or logistf.
 *
 * The individuals, called genotypes, keep, mean imputation, design B = sqrt(N) Q, theta0 and the flags 1 - 4 are those of
 * "logistic association scan"; so are v_a, w_a, mu_a and I(theta).  The estimate is
 *     theta^ maximises  l*(theta) = l(theta) + 1/2 ln det I(theta)                                   (Firth 1993)
 *     modified score  U*(theta) = sum_a v_a [ y_a - mu_a + h_a (1/2 - mu_a) ],   h_a = w_a v_a^T I(theta)^-1 v_a
 *     beta = theta^_b,  se = sqrt([I(theta^)^-1]_bb)  (the UNPENALISED information at theta^),  z, p, neglog10_p as in the ML scan
 * theta^ is finite for every full-rank cell (Kosmidis & Firth 2021), separated ones included.  For the saturated 2 x 2 table
 * without covariates, a, b cases and c, d controls at genotype high, low, it is the Haldane-Anscombe estimate:
 *     beta = ln[(a + 1/2)(d + 1/2) / ((b + 1/2)(c + 1/2))]
 *     se^2 = 1 / (n_h mu_h (1 - mu_h)) + 1 / (n_l mu_l (1 - mu_l)),  mu_h = (a + 1/2) / (a + c + 1),  mu_l = (b + 1/2) / (b + d + 1),
 *            n_h = a + c,  n_l = b + d
 * beta^ and se do not depend on the parametrisation of the span of D (ln det I changes by a constant).  The iteration path is not
 * part of the definition.
 * Iteration (the device and its numpy mirror, ops.ld_glm_logistic_host(firth=)): Fisher scoring theta <- theta + I(theta)^-1 U*(theta)
 * from (theta0_j, 0) -- the start of the ML scan, whether the cell is reached by the fallback or not.  An evaluation forms I, its
 * Cholesky factor L and M = L^-1, then h_a = w_a |M v_a|^2 and U* in a second pass over the individuals, and solves I delta = U*;
 * when lambda*^2 = U*^T I^-1 U* <= 2^-88 that step is applied and I evaluated once more at the new point for se; at most
 * LDX_FIRTH_MAX_ITER information evaluations.  Scoring with I (not with the Hessian of l*) converges linearly: the stop constant
 * is chosen so that the steps not taken sum to less than 2^-40 se.  Safeguard: an evaluation whose lambda*^2
 * is not below that of the point before gives its point up for the one half as far along the step before, and the step length
 * stays halved for the rest of the fit (a variant with a single carrier has a hat value near 1 and the plain step overshoots
 * about twofold: without the safeguard such cells end in a 2-cycle).  A cell that never triggers it is not touched by it.
 * flags: 0 - 4 as in the ML scan; 5 = the cap was reached, or a pivot was lost (not > 0, or not finite).  n_iter: the information
 * evaluations of the Firth fit.  Accuracy, against an exact oracle of this definition: |beta - beta_exact| <= 2^-40 se_exact,
 * |se / se_exact - 1| <= 2^-40; the tail as in the ML scan.
 * Out of scope: a phenotype whose NULL maximum-likelihood fit fails keeps flag 4 (no null Firth fit is made);
 * profile-likelihood p-values (logistf's) are not computed, the test is Wald; pairwise-complete missing data is refused upstream.
 * Reproducibility: as the ML scan -- no floating-point atomics, every sum in a fixed order; a cell's bits depend on its SNP, y and
 * design alone, not on mode, the other cells, keep or the launch.
 *
 * ldx_glm_firth_dev: the arguments of ldx_glm_logistic_dev, then mode and firth uint8 [n_snps][ld_out].
 *     mode 0  fits every cell and derives the flags 1 - 4 itself by the ML scan's rules; firth = 1 where a fit was made (the flag
 *             is 0 or 5), 0 under the flags 1 - 4.
 *     mode 1  flags is input and output: a cell whose flag is not 5 on entry gets firth = 0 and nothing else of it is touched; a
 *             cell with flag 5 is refitted: the five outputs, flags (0 or 5), n_iter and firth = 1 are written.  Stream-ordered
 *             after the ML launch that wrote flags; nothing is read back and nothing is compacted on the host.
 * Work: one wave per cell, four cells per workgroup, no barrier; per evaluation pass A of the ML scan, the Cholesky and the
 * triangular inverse in the wave's registers, and pass B: T = M V on v_mfma_f64_16x16x4_f64, 16 individuals x 4 K-groups of
 * parameters x 4 column blocks = 16 instructions per 64 individuals, as many as pass A.  mode > 1, a null firth and every refusal
 * of ldx_glm_logistic_dev = LDX_E_ARG, checked before any HIP call. */
#define LDX_FIRTH_MAX_ITER 200u
int ldx_glm_firth_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                      const uint32_t *counts, const double *design, size_t ld_design, uint32_t n_cov, const uint8_t *y,
                      const double *theta0, uint32_t n_pheno, double max_vif, double *beta, double *se, double *z, double *p,
                      double *neglog10_p, uint8_t *flags, uint8_t *n_iter, size_t ld_out, uint32_t mode, uint8_t *firth,
                      void *stream);

/* ---- genotype QC and table tests: per-group genotype counts, exact HWE and Fisher tests, the chi-square tests of --model -----
 * This project's own definition (what PLINK --hardy, --missing, --het, --test-missing, --assoc fisher and --model report), NOT
 * validated against PLINK: no PLINK binary was available to compare with.
 *
 * Individuals, called genotypes (a half-missing genotype is missing) and keep are those of "genotype products" above.
 *
 * ldx_geno_group_counts_dev: member uint32 [n_ind]; bit g of member[a] set = individual a belongs to group g, g < n_groups <=
 * LDX_QC_MAX_GROUPS (higher bits are ignored).  Groups may overlap, be empty, or hold everybody.  counts uint32
 * [n_snps][n_groups][4] = {called, het, hom ALT, 0} over the group's individuals.  Every word is written with plain stores (no
 * memset by the caller), each 16-byte row as one group; a SNP that is not kept gets zeros.  The panel's two planes are read ONCE
 * for all groups: a workgroup per slab of 128 SNPs; the groups' bit words (16 individuals per 32-bit word on the even slots) are
 * made from member in LDS; the genotype words are the reverse product's own, so a group that holds every individual reproduces
 * ldx_geno_snp_counts_dev bit for bit; per word and group three AND + popcount.  Pad haplotypes count as not called.
 * A null pointer (keep may be NULL), an odd or zero n_hap, n_snps = 0, n_groups outside 1 .. LDX_QC_MAX_GROUPS or counts not
 * 16-byte aligned = LDX_E_ARG; n_hap > LDX_MAX_HAPS or a bit plane of 4 GiB or more = LDX_E_UNSUPPORTED; checked before any HIP call.
 *
 * The exact tests work on m tuples in contiguous device arrays (uint32), one thread per tuple; a tuple's bits depend on the
 * tuple alone; no floating-point atomics.  Outputs p, neglog10_p (double [m]) and flags (uint8 [m]).
 * THE TWO-SIDED TAIL RULE, shared by both: with the distribution's terms P(k), p = the sum of the terms no more probable than
 * the observed one, where term k is included iff P(k) / P(obs) <= 1 + 2^-30.  Exact ties occur (n = 6 with 4 ALT alleles:
 * P(2 het) = P(4 het)) and are the observed term's equals: they are included.  The device forms every term relative to the
 * observed one by the term ratio, from the observed term outwards; at most LDX_QC_MAX_N steps of three roundings each keep the
 * relative error below 2^-35 (2^-39 for n <= 5120), so the rule is decided correctly wherever no exact ratio lies in
 * [1 + 2^-31, 1 + 2^-29] -- a condition on the tuple that the test oracle asserts for every tuple it uses.
 * midp = 1 gives p - P(obs) / 2 (Lancaster: only the observed term is halved; PLINK also halves the ties).
 * Scaled sums: a term and the total are carried as v 2^(256 e), v in [2^-256, 2^256), the tail (terms <= 1 + 2^-30 of the
 * observed one, which is 1) in a plain double; ln p = ln(tail) - ln(total), neglog10_p = -ln p / ln 10: finite where p
 * underflows to 0 (all-heterozygous n = 2560: p about 1e-769).  When every term is in the tail p = 1 and neglog10_p = 0 exactly
 * (midp: p = 1 - P(obs) / 2).  Terms past the mode that fall below 2^-1280 of the observed one are dropped.  |ln p| is within
 * 2^-30 max(1, |ln p|) of the exact value.
 *
 * ldx_hwe_exact_dev: the exact test of Hardy-Weinberg proportions (Wigginton, Cutler, Abecasis 2005) on (n called, het, hom
 * ALT): given n and n_A = het + 2 hom ALT alleles, the heterozygote count k has the parity of n_A and runs to min(n_A, 2n - n_A);
 * P(k) ~ 2^k n! / (((n_A - k) / 2)! k! ((2n - n_A - k) / 2)!), P(k + 2) / P(k) = 4 n_AA n_BB / ((k + 2)(k + 1)).
 *     flags, the first that applies: 3 not a genotype table (het + hom > n) or n > LDX_QC_MAX_N: NaN      1 n = 0: NaN
 *                                    2 monomorphic: p = 1, neglog10_p = 0 exactly (midp or not)           0 OK
 * ldx_fisher_exact_dev: Fisher's exact test on the 2 x 2 table [[a, b], [c, d]]: the first cell x of the tables with these
 * margins, P(x + 1) / P(x) = (r1 - x)(c1 - x) / ((x + 1)(r2 - c1 + x + 1)), r1 = a + b, r2 = c + d, c1 = a + c.
 *     flags: 3 a + b + c + d > 2 LDX_QC_MAX_N: NaN      1 empty table: NaN      2 a zero row or column margin: p = 1, neglog10_p = 0      0 OK
 * A tuple outside the rules cannot be refused by these entries, which do not read device memory before the launch: it carries
 * flag 3 and NaN, and the host layer (ops.ld_hwe_from_counts, ops.ld_fisher_from_counts), which holds the integers, refuses it
 * as LDX_E_ARG before the call.
 *
 * ldx_model_tests_dev: the five tests of plink --model on (case n, het, hom; control n, het, hom), in this order: allelic,
 * Cochran-Armitage trend, genotypic, dominant, recessive.  chisq, p, neglog10_p double [m][5], flags uint8 [m][5], odds double [m].
 * R cases, S controls, N = R + S <= LDX_MAX_HAPS / 2; r0 r1 r2 / s0 s1 s2 the genotype counts, n_g = r_g + s_g.  Every integer is
 * exact in int64; the fp64 operations, each rounded once, are exactly these (ops.model_tests_host repeats chisq and odds bit
 * for bit):
 *     2 x 2 table [[a, b], [c, d]] with total T:  chisq = ((double)T (double)((ad - bc)^2)) / (double)((a + b)(c + d)(a + c)(b + d))
 *     allelic    T = 2N on allele counts a = r1 + 2 r2, b = 2R - a, c = s1 + 2 s2, d = 2S - c;  odds = (double)(ad) / (double)(bc)
 *     trend      U = N (r1 + 2 r2) - R (n1 + 2 n2),  D = N (n1 + 4 n2) - (n1 + 2 n2)^2,  chisq = ((double)N (double)(U^2)) / (double)(R S D)
 *     genotypic  chisq = sum over the cells in the order r0 r1 r2 s0 s1 s2, added one after the other from 0, of
 *                (double)((O N - row col)^2) / (double)(N row col);  2 df
 *     dominant   T = N on individuals: a = r1 + r2, b = r0, c = s1 + s2, d = s0          recessive  a = r2, b = r0 + r1, c = s2, d = s0 + s1
 * Dominant and recessive are with respect to ALT (code 1), NOT to the minor allele.
 * Tails: 1 df: the two-sided normal tail of sqrt(chisq), the function of "logistic association scan"; 2 df: ln p = -chisq / 2
 * exactly, p = exp(-chisq / 2).  |ln p| is within 2^-30 max(1, |ln p|) of the exact value.
 *     flags per test, the first that applies; every flag but 0 is NaN in chisq, p, neglog10_p (odds is NaN unless the allelic flag is 0):
 *     4 not two genotype tables (het + hom > n) or N > LDX_MAX_HAPS / 2 (refused by the host layer, as above)
 *     1 no called case or no called control      2 a zero margin: the statistic is undefined
 *     3 genotypic only: a cell below min_cell (PLINK's --cell, default 5)      0 OK
 * A null pointer, m = 0 or m > 2^38, a midp other than 0 or 1 = LDX_E_ARG, checked before any HIP call. */
#define LDX_QC_MAX_GROUPS 32u
#define LDX_QC_MAX_N 65536u                 /* individuals of an exact-test tuple (a Fisher table: 2 LDX_QC_MAX_N alleles) */
int ldx_geno_group_counts_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                              const uint32_t *member, uint32_t n_groups, uint32_t *counts, void *stream);
int ldx_hwe_exact_dev(size_t m, const uint32_t *n, const uint32_t *het, const uint32_t *hom, int midp, double *p,
                      double *neglog10_p, uint8_t *flags, void *stream);
int ldx_fisher_exact_dev(size_t m, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, int midp,
                         double *p, double *neglog10_p, uint8_t *flags, void *stream);
int ldx_model_tests_dev(size_t m, const uint32_t *case_n, const uint32_t *case_het, const uint32_t *case_hom,
                        const uint32_t *ctrl_n, const uint32_t *ctrl_het, const uint32_t *ctrl_hom, uint32_t min_cell,
                        double *chisq, double *p, double *neglog10_p, double *odds, uint8_t *flags, void *stream);

/* ---- epistasis scan: 3 x 3 x 2 genotype tables of SNP pairs in cases and controls, allelic and BOOST interaction tests -------
 * This project's own definition (what PLINK --fast-epistasis and --fast-epistasis boost report), NOT validated against PLINK: no
 * PLINK binary was available to compare with.
 *
 * Individuals, g in {0, 1, 2} and "called" are those of "pairwise-complete EM": a half-missing or second-ALT genotype is missing.
 * The two groups, cases and controls, are given as two PANELS over the same SNPs (ops.py makes them with PackedPanel.select), each
 * with its own even n_hap <= LDX_MAX_HAPS; an individual in neither panel is left out.
 *
 * THE TABLE of row i of SNP set I, row j of SNP set J and group c: n^c_ab, a, b in {0, 1, 2}, the individuals of group c called at
 * both SNPs with g_i = a and g_j = b.  18 exact integers per pair in the order case n00 n01 n02 n10 ... n22, then control (index
 * 9 c + 3 a + b with c = 0 for the cases).  The kernel forms, per group, the nine products of the three per-individual operands
 * dosage g, het t and called q of each side (GG TT GT TG GQ QG TQ QT QQ) on the FP4 matrix pipe, every product and every sum exact, and
 *     n11 = TT    n21 = (GT - TT) / 2    n12 = (TG - TT) / 2    n22 = (GG - n11 - 2 n12 - 2 n21) / 4
 *     row margins r1 = TQ, r2 = (GQ - TQ) / 2, column margins c1 = QT, c2 = (QG - QT) / 2, the rest by subtraction.
 *
 * THE TESTS.  Each is a function of the 18 integers alone, in fp64 with every operation rounded once (-ffp-contract=off), in the
 * order written here, and symmetric under swapping the two SNPs.  flags is the OR of the bits below.
 * per group the 2 x 2 allele table  a = S, b = 2A - S, c = 2B - S, d = 4N - 2A - 2B + S  with N = sum n, A = sum a n_ab,
 * B = sum b n_ab, S = sum ab n_ab (exact integers), L = ln((a d) / (b c)), V = (1/a + 1/d) + (1/b + 1/c).
 *     dir = L_case - L_ctrl, the direction of the interaction, in both tests.
 *     bit 2: a zero among the eight allele cells: dir is NaN (and so is the allelic chi-square).  No continuity correction.
 * LDX_EPI_ALLELIC (the default of --fast-epistasis):  Z = dir / sqrt(V_case + V_ctrl), chisq = Z Z, 1 df.
 * LDX_EPI_BOOST: the likelihood-ratio test of the saturated model against the log-linear model without the three-way term on the
 * 3 x 3 x 2 table (BOOST's exact statistic, Wan et al. 2010), 4 df.  The table is fitted in the one of its two orientations (as
 * given, or with the SNPs swapped: n^c_ab -> n^c_ba) whose 18 integers come first in lexicographic order; the statistic is thus a
 * function of the unordered pair.  mu starts at 1 in all 18 cells.  A cycle of iterative proportional fitting scales, in this
 * order, the margins SNP i x SNP j (s = mu^0_ab + mu^1_ab), SNP i x group (s = (mu^c_a0 + mu^c_a1) + mu^c_a2) and SNP j x group
 * (s = (mu^c_0b + mu^c_1b) + mu^c_2b): f = observed margin / s, or 0 where s = 0, and every cell of the margin is multiplied by f.
 * The iteration stops after the first cycle in which no cell moved by more than 2^-40 N_total (|mu after - mu before the cycle|),
 * or after LDX_EPI_MAX_CYCLES cycles.
 *     G2 = 2 sum over the cells with n > 0, in index order from 0, of n ln(n / mu);  chisq = G2 where G2 > 0, else 0.
 *     bit 1: a group has no jointly called individual: NaN, no fit.
 *     bit 4: the cycle cap was reached; the statistic is reported as it stands.
 *     bit 8: one of the 21 two-way margins is 0: the cell is reported, the df are nominally 4, p is conservative.
 * LDX_EPI_MAX_CYCLES is the smallest cap that no table without bit 8 among the test oracle's tuples (tests/ld_epistasis_exact.py)
 * reaches: the slowest of them stops in its 55th cycle (a table of 44 individuals with six empty cells; the tables of 100 and
 * more individuals stop within 24).  A table WITH bit 8 can crawl towards a boundary at the rate 1 / cycles: it is cut off here.
 * Tails, from chisq alone: allelic ln p = the two-sided normal tail of sqrt(chisq), the function of "logistic association scan";
 * boost ln p = -G2 / 2 + log1p(G2 / 2), the closed form of 4 df, so that neglog10_p stays finite where p is 0.
 * Accuracy, against an exact oracle (rationals up to the logarithms, then 60 decimal digits; the IPF iterated until nothing moves
 * above 1e-45), for every cell without bits 1, 2 (allelic) and 4: |chisq - exact| <= BOUND max(exact, 1), with BOUND =
 * LDX_EPI_REL_BOUND_ALLELIC = 2^-46 and LDX_EPI_REL_BOUND_BOOST = 4.17e-12 (2^-37.8).  numpy repeats mu and the cycle count bit
 * for bit (ops.epi_boost_host); the statistic itself goes through the device's own log.  Each bound is 8 x the worst error of the
 * numpy mirror on the oracle's tuples (1.78e-15 and 5.22e-13, tests/test_epistasis_host.py measures them).  The boost bound is
 * looser than the logistic scan's 2^-40 for a stated reason: the stop rule leaves mu within about 2^-40 N of the fit, and G2 is a
 * sum of terms n ln(n / mu) of both signs, each up to N ln 2 in size, that cancels down to a statistic of order 1 -- the residue
 * of the fit and the rounding of the terms do not shrink with it (the worst tuple has G2 = 1.17 at N = 3290).  Below 1 the
 * bound is absolute for the same reason.
 *
 * CELLS are float32 chi-squares.  A NaN cell is never a hit.  A cell depends on its 18 integers only: not on the tile, the path
 * (shortcut or nine-set loop), the other SNPs of the call, the phase or the order of the individuals; swapping the sides gives
 * the transpose bit for bit.
 *
 * ldx_epi_side: one SNP set as its two group panels: the tiled planes (ldx_plane_bytes of the group's n_hap) and the group's
 * per-SNP table cnt uint32 [n_snps][4] = {called, het, hom ALT, 0} (ldx_geno_snp_counts_dev of the group panel), 16-byte aligned.
 * A 128 x 128 tile none of whose 256 SNPs has an uncalled individual of a group (called = n_hap / 2) forms four of the nine sets
 * for that group and reads the margins from cnt; the integers are the same either way.
 * ldx_epi_counts_dev: counts[(s n_i + i) ld + j], s = 0 .. 17, uint32: what the loops produced, before any float.
 * ldx_epi_rect_dev: dense float32 chisq [n_i][ld]; dir (float32) and flags (uint8) in the same layout where not null.
 * ldx_epi_hits_dev: one ldx_hit {query = i, oppos = j, r_square = chisq, d_prime = dir} for every pair whose cell is >= bound: ONE
 * float32 compare, bound > 0.  Slots, batches, *n_hits and overflow are ldx_ld_rect_hits_dev's; ldx_area_finish_ex_dev finishes.
 * With n_tot, n_sig and best (all three or none; the caller zeroes them, [n_i] each) it also fills the per-SNP summary of the rows
 * of I: n_tot[x] the valid (non-NaN) tests of row x, n_sig[x] those with chisq >= bound_sig (> 0), both uint32 integer atomics,
 * and best[x] a uint64 atomicMax of (float bits of chisq) << 32 | (0xFFFFFFFF - partner): the largest chi-square and, on ties, the
 * smallest partner index, whatever the order of arrival; best[x] is 0 where n_tot[x] is.  The summary does not depend on hit_cap.
 * self = 1 (side_j must be side_i's panels): only the tiles tj <= ti are walked and only the pairs i > j tested, once each; the
 * summary credits both SNPs, each with the other as its partner.
 * ldx_epi_from_counts_dev: the epilogue alone on m tuples of 18 uint32 (tuples[18 k + s]): chisq (double), chisq32 (the cell), dir,
 * ln_p (double [m]), flags (uint8 [m]), mu (double [m][18], the fitted table in the tuple's orientation; NaN unless boost without
 * bit 1) and cycles (uint32 [m]); every output may be null.  A tuple with a group total above LDX_MAX_HAPS / 2 is no table of this
 * library: this entry does not read device memory before the launch, so the tuple carries flag 16 and NaN, and the host layer
 * (ops.ld_epistasis_from_counts), which holds the integers, refuses it as LDX_E_ARG before the call.
 * Work: a workgroup of 256 threads per tile, one per CU; four passes per tile, each the K loop over the cases' planes, then over
 * the controls', with the epilogue staged through LDS; plain vector stores; no floating-point atomics.
 * A null pointer (the optional outputs excepted), a test other than the two, n_i, n_j or a group's n_hap 0, an odd n_hap, ld below
 * n_j, a cnt that is not 16-byte aligned, bound or bound_sig not > 0, self without identical sides, m = 0 = LDX_E_ARG; a group's
 * n_hap > LDX_MAX_HAPS, a bit plane of 4 GiB or more, 2^31 or more tiles or workgroups = LDX_E_UNSUPPORTED; all checked before
 * any HIP call. */
#define LDX_EPI_ALLELIC 0
#define LDX_EPI_BOOST 1
#define LDX_EPI_MAX_CYCLES 55u
#define LDX_EPI_REL_BOUND_ALLELIC 0x1p-46
#define LDX_EPI_REL_BOUND_BOOST 4.17e-12
typedef struct ldx_epi_side {
    const void *alt_case, *ref_case;
    const uint32_t *cnt_case;
    const void *alt_ctrl, *ref_ctrl;
    const uint32_t *cnt_ctrl;
    uint32_t n_snps;
} ldx_epi_side;
int ldx_epi_counts_dev(const ldx_epi_side *side_i, const ldx_epi_side *side_j, uint32_t n_hap_case, uint32_t n_hap_ctrl,
                       uint32_t *counts, size_t ld, void *stream);
int ldx_epi_rect_dev(const ldx_epi_side *side_i, const ldx_epi_side *side_j, uint32_t n_hap_case, uint32_t n_hap_ctrl, int test,
                     float *chisq, float *dir, uint8_t *flags, size_t ld, void *stream);
int ldx_epi_hits_dev(const ldx_epi_side *side_i, const ldx_epi_side *side_j, uint32_t n_hap_case, uint32_t n_hap_ctrl, int test,
                     int self, float bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits, float bound_sig, uint32_t *n_tot,
                     uint32_t *n_sig, uint64_t *best, void *stream);
int ldx_epi_from_counts_dev(size_t m, int test, const uint32_t *tuples, double *chisq, float *chisq32, double *dir, double *ln_p,
                            uint8_t *flags, double *mu, uint32_t *cycles, void *stream);

/* ---- permutation tests: max(T) label permutation for the allelic and the trend test of a case/control scan -------------------
 * This project's own definition (what PLINK --assoc mperm and --model mperm report as EMP1 and EMP2), NOT validated against
 * PLINK: no PLINK binary was available to compare with.
 *
 * INDIVIDUALS.  The scan runs over the n individuals with a phenotype, in panel order, index k (ops.py takes them with
 * PackedPanel.select, as the epistasis scan does); n_case of them are cases.  g in {0, 1, 2}, "called" and half-missing
 * genotypes are those of "genotype products" above (geno_words).
 *
 * PERMUTATION p is a global 0-based index; a call covers [first, first + n_perm).  key(p, k) = the synthetic panels' key(seed,
 * i = p, h = k) below (the mix64 finaliser).  Individual k is a case in permutation p iff fewer than n_case individuals k' have
 * (key(p, k'), k') < (key(p, k), k) lexicographically.  So every permutation has exactly n_case cases, and a permutation depends
 * on (seed, p, n, n_case) alone: not on n_perm, first or the chunking of a run.
 *
 * THE LABEL PLANE: a tiled bit plane of ldx_plane_bytes(n_perm, 2 n) with the permutations as rows; the bit of haplotype slot 2k
 * is set iff k is a case, the odd slots are zero -- what ldx_pack_codes_dev makes as the alt plane of codes 1 on the even slot of
 * a case and 0 elsewhere, so a caller's own label matrix is packed by the existing code.  Every row must hold n_case cases.
 *
 * Per SNP over the n individuals: N called, n1 heterozygous, n2 homozygous ALT (cnt: ldx_geno_snp_counts_dev's table of the
 * panel), G = n1 + 2 n2, Q2 = n1 + 4 n2.  Per cell (SNP i, permutation p), with L_pk the label:
 *     R = sum_k called_k L_pk     a = sum_k g_k L_pk     S = N - R
 * THE STATISTIC.  Every integer is exact in int64; the fp64 operations are exactly these, each rounded once:
 *     LDX_PERM_ALLELIC  b = 2R - a, c = G - a, d = 2S - c, det = ad - bc, den = (a + b)(c + d)((a + c)(b + d))
 *                       chisq = ((double)(2N) (double)(det^2)) / (double)den
 *     LDX_PERM_TREND    U = N a - R G, den = R S (N Q2 - G^2)
 *                       chisq = ((double)N (double)(U^2)) / (double)den
 * Both are, bit for bit, ldx_model_tests_dev's chisq of tests 0 and 1 on any genotype table with these margins.  det^2, U^2 and
 * den are at most N^4 < 2^53 for N <= LDX_MAX_HAPS / 2: exact doubles.  A cell with den = 0 is INVALID (for a usable SNP: R = 0 or
 * R = N): it is neither counted nor enters a maximum.
 *
 * SNP FLAGS, from the observed labels (the host layer, ops.ld_mperm, forms them with ldx_perm_from_counts_dev on the group counts
 * of ldx_geno_group_counts_dev): 0 OK; 1 no called case or no called control; 2 den = 0; 3 dropped by keep.  A flagged SNP has NaN
 * stat and n_ge = 0 and takes part in no maximum.
 * RESULTS: stat[i] the observed chisq; n_ge[i] = #{p : cell (i, p) is valid and chisq >= stat[i]} (uint32); max[p] = the largest
 * valid chisq over the flag-0 SNPs, +0.0 if there is none; EMP1 = (n_ge + 1) / (R + 1), EMP2 = (#{p : max[p] >= stat[i]} + 1) /
 * (R + 1), each ONE fp64 division.
 *
 * ldx_perm_labels_dev: writes the label plane of permutations first .. first + n_perm - 1 of n = n_hap / 2 individuals, one
 *   workgroup per permutation (a radix select on the composite (key, k) in LDS); plain stores, every byte of the plane written.
 * ldx_perm_scan_dev: stat double [n_snps], the observed statistic of each SNP, NaN for a SNP that takes no part (flagged or not
 *   kept).  Adds to n_ge[i] (uint32) the permutations p of this call whose cell (i, p) is valid with chisq >= stat[i], and raises
 *   max[p] (uint64: the bits of a non-negative double, p local to the call) to the largest valid chisq over the SNPs of this call
 *   that take part.  The caller zeroes both; passing the same buffers again accumulates -- max over further SNP chunks or
 *   chromosomes (same labels), n_ge over further permutation chunks (same SNPs).  All compares are fp64 >= on the values above, so
 *   exact ties count.  Integer atomics only: the result does not depend on the order of arrival, the tile or the path.
 *   128 x 128 tiles of SNPs x permutations on the FP4 matrix pipe, a = (g / 2).(2 L) and R = (called / 2).(2 L); a tile none of
 *   whose SNPs has an uncalled individual (cnt called = n) forms a alone, with R = n_case.
 * ldx_perm_counts_dev: counts[(s n_snps + i) ld + p], s = 0 for a, 1 for R, uint32: what the loops produced, before any float.
 * ldx_perm_from_counts_dev: the scan's epilogue alone on m tuples (n[k] called, het[k], hom[k], r[k], a[k]): chisq double [m], flags
 *   uint8 [m], the first that applies: 4 no table has these margins (het + hom > n, r > n, a > 2r, a > G, G - a > 2(n - r)) or n >
 *   LDX_MAX_HAPS / 2      1 r = 0 or r = n: no called case or no called control      2 den = 0      0 OK; chisq is NaN unless 0.
 *   The entry does not read device memory before the launch, so a tuple that is no table carries flag 4 and NaN, and the host
 *   layer (ops.ld_mperm_from_counts), which holds the integers, refuses it as LDX_E_ARG before the call.
 * A null pointer, a test other than the two, n_snps, n_perm or m = 0, n_case outside 1 .. n - 1, an odd or zero n_hap, a cnt that is
 * not 16-byte aligned, ld < n_perm = LDX_E_ARG; n_hap > LDX_MAX_HAPS, a bit plane (the panel's or the labels') of 4 GiB or more,
 * 2^31 or more tiles = LDX_E_UNSUPPORTED; all checked before any HIP call. */
#define LDX_PERM_ALLELIC 0
#define LDX_PERM_TREND 1
int ldx_perm_labels_dev(uint64_t seed, uint64_t first, uint32_t n_perm, uint32_t n_hap, uint32_t n_case, void *labels, void *stream);
int ldx_perm_scan_dev(const void *alt, const void *ref, const uint32_t *cnt, uint32_t n_snps, uint32_t n_hap, const void *labels,
                      uint32_t n_perm, uint32_t n_case, int test, const double *stat, uint32_t *n_ge, uint64_t *max, void *stream);
int ldx_perm_counts_dev(const void *alt, const void *ref, const uint32_t *cnt, uint32_t n_snps, uint32_t n_hap, const void *labels,
                        uint32_t n_perm, uint32_t n_case, uint32_t *counts, size_t ld, void *stream);
int ldx_perm_from_counts_dev(size_t m, int test, const uint32_t *n, const uint32_t *het, const uint32_t *hom, const uint32_t *r,
                             const uint32_t *a, double *chisq, uint8_t *flags, void *stream);

/* ---- synthetic panels: deterministic, identical on host and device ------ */
/* codes int8 [n_snps][ld_codes] receive global SNPs [snp_offset, snp_offset + n_snps) (a rank's
 * shard).  thresholds: per-SNP ALT probability * 2^64 (computed on the host, see
 * ld_tools_amd/synth.py), covering whole LD blocks: thresholds[k] belongs to global SNP
 * (snp_offset / block_len) * block_len + k, up to the end of the block holding the last SNP.
 * rho_thr: within-block copy probability * 2^64.  miss_thr: probability * 2^64 of code 2. */
int ldx_synth_codes_dev(int8_t *codes, uint32_t n_snps, uint32_t n_hap, size_t ld_codes,
                        uint64_t seed, const uint64_t *thresholds, uint64_t rho_thr,
                        uint32_t block_len, uint64_t miss_thr, uint32_t snp_offset, void *stream);
/* The same with SNPs that are not "ordinary" (what a sub-panel of the ALL-panel variants holds: ld_area.py:215-225 takes
 * every rs variant of the window, monomorphic in the sub-panel or not): mono_thr = probability * 2^64 that a SNP is
 * monomorphic (every code 0; one in eight of them every code 1), miss_rows_thr = probability * 2^64 that a SNP carries the
 * miss_thr codes at all (2^64 - 1: every SNP, as ldx_synth_codes_dev). */
int ldx_synth_codes_ex_dev(int8_t *codes, uint32_t n_snps, uint32_t n_hap, size_t ld_codes,
                           uint64_t seed, const uint64_t *thresholds, uint64_t rho_thr,
                           uint32_t block_len, uint64_t miss_thr, uint32_t snp_offset,
                           uint64_t mono_thr, uint64_t miss_rows_thr, void *stream);

/* ---- host-pointer conveniences (same kernels; allocate, copy, synchronise) ------------- */
/* calc_ld for ONE pair of code vectors of lengths h1, h2 (zip semantics of calc_ld.py:30-31:
 * n = min(h1, h2) for the haplotype count, allele counts over the full vectors; any lengths >= 1).
 * counts[6] = {n, n11, a1, r1, a2, r2}; raw = unrounded; rounded = round(x, 4) as doubles, exact for any
 * magnitude; freq4[2] = round4(fa1), round4(fa2).  One H2D copy, ONE kernel (counts straight from the codes,
 * epilogue, rounding) and one 80-byte D2H copy per call, through device scratch cached per host thread. */
int ldx_calc_ld_host(const int8_t *g1, uint32_t h1, const int8_t *g2, uint32_t h2,
                     uint32_t counts[6], ldx_ld64 *raw, ldx_ld64 *rounded, double freq4[2],
                     uint8_t *flags);

/* ---- instrumentation ------------------------------------------------------------------- */
/* Peak-rate probe for the v_and_b32 + v_bcnt_u32_b32 pair (the inner loop's two instructions):
 * runs `iters` rounds of 64 AND + 64 BCNT per lane on `blocks` x `threads` threads (threads a multiple
 * of 64, <= 1024), no memory traffic, and writes a checksum to sink[blocks*threads]. */
int ldx_probe_andpop_dev(uint32_t *sink, uint32_t blocks, uint32_t threads, uint32_t iters, void *stream);

/* Peak-rate probe for the matrix pipe: `iters` rounds of 8 back-to-back int8 MFMAs per wave on independent
 * accumulators, operands in registers.  variant 0 = v_mfma_i32_32x32x32_i8 (32768 MACs each),
 * 1 = v_mfma_i32_16x16x64_i8 (16384 MACs each).  threads <= 256. */
int ldx_probe_mfma_dev(uint32_t *sink, uint32_t blocks, uint32_t threads, uint32_t iters, int variant,
                       void *stream);

/* Tests / tuning: force the number of passes a matrix-kernel launch hands out as two half-height tickets
 * (n_short >= 0), or restore the launch heuristic (n_short < 0).  Results do not depend on it. */
int ldx_debug_force_short_passes(int n_short);
/* Tuning builds (-DLDX_TUNING) count events of the fp32 epilogue tier: out[0] = units it handled, [1] = lane-steps parked
 * for the fp64 tier, [2] = units redone because the queue overflowed, [3] = mirror evaluations behind the fp64 tier.
 * Product builds leave the counters at zero.  Synchronises the device. */
int ldx_debug_counters(uint64_t out[8], int reset);

#ifdef __cplusplus
}
#endif
#endif /* LDX_H */

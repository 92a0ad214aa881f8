// The pairwise-complete tile: what pwc_kernel (ldx_pwc.hip, the rectangle) and pwband_kernel (ldx_pwband.hip, the
// band) share -- the cell functions, the workgroup's LDS, and tile_body: one 256 x 128 tile from the hole test to the last
// cell, with both K loops (the hole-free shortcut and the general 4 / 8-pass loop with two-operand LDS images).  What a kernel
// does with a cell is its own: tile_body hands every cell's integers to an epilogue functor.
//   * counting: v_mfma_f32_32x32x64_f8f6f4 with FP4 operands (ldx_fp4.h), every product an exact small integer, every fp32
//     accumulator an exact count < 2^24.  Both planes enter: called = alt | ref.
//       haplotype form, 4 sets:  c = a4(alt_x) . b4(alt_y)       a = a4(alt_x) . b4(called_y)
//                                b = a4(called_x) . b4(alt_y)    n = a4(called_x) . b4(called_y)
//       dosage form, 6 sets, on per-individual operands (ldx_fp4.h, "Pairwise-complete dosage LD"): q = ind_called, w = alt
//       masked by both slots of q, hom = the even bits of w & (w >> 1);  G = expand32_a4_dosage(w), Q = even_a4(q),
//       M = even_a4(hom), O = odd_a4(q) on the I side;  U = expand32_b4_dosage(w), V = expand32_b4_called_hom(q, hom) on J:
//                                S = G . U     B = Q . U     A = G . V     N = Q . V     HA = M . V     HB = O . V
//   * tile: rect_kernel's.  A workgroup (4 waves, two workgroups per CU, hence <= 256 registers per wave) owns 256 rows of I x
//     one 128-row slab of J; a wave 64 x 128 = 2 x 4 accumulator tiles of 32 x 32: 128 accumulator registers.  J sits on the
//     accumulator's column side: a half-wave holds 32 consecutive cells of one output row.
//   * shortcut: a workgroup whose I rows and J slab hold no SNP with acnt + rcnt != n_hap (read from the tables, workgroup-
//     uniform) runs rect_kernel's K loop -- ONE set, c, or S as the dosage rectangle counts it, in all eight tiles -- and takes
//     the other integers from the per-SNP tables.  The dosage form's homozygotes come from the caller's per-panel table
//     (kHomTable: ldx_dosage_stats_dev's hom, which on a row without holes is HA) or are counted in the prologue.
//   * general loop: the eight tiles' worth of registers hold ALL sets of a part of the wave's cells -- 4 sets x 2 tiles, or 6
//     sets x 1 tile -- and the wave covers its 64 x 128 cells in 4 (8) passes over K, each followed by its cells' epilogue.  A
//     pass expands the J slab again: per cell the general loop costs what a 64 (32) x 128 workgroup tile would, and the tiles
//     without holes pay nothing for it.
//   * both paths end in the same functions of the integers, pw_var_* / pw_rs / r32_cell, so a cell cannot depend on its tile;
//     the shortcut only evaluates pw_rs once per SNP instead of once per cell.
//   * K loop: a K-block is 256 haplotypes; per K-block the workgroup expands the J slab's bits ONCE into an LDS image [2 operands]
//     [4 steps][2 halves][128 rows][16 B], double-buffered (2 x 32 KiB), one block_sync per K-block; a lane loads the 16 bytes
//     of its own I rows from each plane and expands them in registers.  Plain HIP: the compiler tracks every load.
// The epilogue functor (by reference; its state lives in registers once tile_body is inlined):
//     static constexpr bool kCells   the cell's 1 / sqrt of the two variances are wanted (false: the integers alone)
//     static constexpr bool kReduce  row_done() and pass_done() are called
//     cell(i, j, t, k, rs_x, rs_y)   one cell, called by the whole wave: SNP i of I, SNP j of J (either may lie beyond its panel),
//                                    t the cell's column tile among those of the pass (a constant once unrolled), its integers
//                                    k[] in the order of ldx_ld_rect_pw_counts_dev.  A lane meets the cells of one row side by side
//     row_done(i)                    after a lane's cells of row i: one per column tile of the pass
//     pass_done<kT>(j0)              after the last cell of a pass over kT column tiles (the shortcut: the tile's only pass,
//                                    kT = 4); the lane's column of tile t is j0 + 32 t
#pragma once

#include "ldx_fp4.h"

namespace ldx {
namespace pwc {

constexpr uint32_t kWaves = 4, kThreads = kWaves * 64u;
constexpr uint32_t kWaveRows = 64;                    // I rows per wave: two 32-row accumulator tiles
constexpr uint32_t kTileRows = kWaves * kWaveRows;    // I rows per workgroup: 256
constexpr uint32_t kAcc = 8;                          // accumulator tiles of a wave: 2 x 4
constexpr uint32_t kOpVecs = 4u * 2u * kSlab;         // 16-byte vectors of one operand's image: [4 steps][2 halves][128 rows]
constexpr uint32_t kImageVecs = 2u * kOpVecs;         // one buffer: two operands
constexpr uint32_t kBlockVecs = 2u * kSlab;           // 16-byte vectors of one K-block of a slab in the plane (two chunks)

// the sets, numbered in the order of ldx_ld_rect_pw_counts_dev, and the general loop's passes
template <bool kDosage>
struct Geo {
    static constexpr uint32_t kSets = kDosage ? 6u : 4u;           // n a b c  /  N A B HA HB S
    static constexpr uint32_t kLast = kSets - 1u;                  // c / S: the shortcut's one set
    static constexpr uint32_t kG = kAcc / kSets;                   // tiles of a pass, side by side along J: 2 / 1
    static constexpr uint32_t kPasses = kAcc / kG;                 // 4 / 8
};

struct Side {
    const uint4 *alt, *ref;   // tiled bit planes (ldx_plane_bytes)
    const uint32_t *acnt;     // [n] ALT counts
    const uint32_t *rcnt;     // [n] REF counts
    uint32_t n;               // SNPs
    const uint32_t *hom;      // [n] homozygotes of a row without holes (kHomTable), else unused
};

// the workgroup's LDS: 73 232 bytes
struct Smem {
    uint4 image[2][kImageVecs];                // the J slab's expanded K-block, two operands, double-buffered: 2 x 32 KiB
    double c_a[kSlab], c_rs[kSlab];            // the shortcut's per-SNP tables: {a, rs} of the slab's 128 columns
    double r_a[kTileRows], r_rs[kTileRows];    // ... and of the workgroup's 256 rows
    uint32_t c_hom[kSlab], r_hom[kTileRows];   // ... and the homozygotes (dosage form)
    uint32_t wflag[kWaves];
};

// ---- the cell: functions of the pair's integers alone (include/ldx.h), every product exact in fp64 ---------------------------
__device__ __forceinline__ double pw_var_hap(double n, double a) { return a * (n - a); }
__device__ __forceinline__ double pw_var_dosage(double N, double A, double HA) { return N * (A + 2.0 * HA) - A * A; }
__device__ __forceinline__ double pw_rs(double v) { return v > 0.0 ? 1.0 / __builtin_sqrt(v) : 0.0; }

__device__ __forceinline__ v16f mfma4(const v4i &a, const v4i &b, const v16f &c)
{
    const v8i a8 = {a.x, a.y, a.z, a.w, 0, 0, 0, 0};
    const v8i b8 = {b.x, b.y, b.z, b.w, 0, 0, 0, 0};
    // cbsz = blgp = 4: FP4 operands (4 registers each); scale operands 0 = the unscaled instruction
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 0, 0, 0);
}

// One tile: I block ti (rows 256 ti ..) x J slab tj, nblocks K-blocks of 256 haplotypes; tid = threadIdx.x.  Called by the whole workgroup; the
// first barrier inside publishes what the caller wrote to LDS of its own before the call, and a caller that runs tile after
// tile needs a barrier between two calls (the tables and the image are reused).
template <bool kDosage, bool kHomTable, typename Epi>
__device__ __forceinline__ void tile_body(Smem &sm, const Side &si, const Side &sj, uint32_t nblocks, uint32_t n_hap, uint32_t ti,
                                          uint32_t tj, uint32_t tid, Epi &epi)
{
    using G = Geo<kDosage>;
    constexpr uint32_t kSets = G::kSets, kLast = G::kLast, kG = G::kG;
    const uint32_t lane = tid & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t nchunks = 2u * nblocks;
    const double n_obs = kDosage ? (double)(n_hap / 2u) : (double)n_hap;

    // ---- which path: does a SNP of this tile hold a hole?  Thread t owns row t of the I block and, t < 128, column t of the slab.
    const uint32_t x_r = ti * kTileRows + tid, x_c = tj * kSlab + tid;
    const bool valid_r = x_r < si.n, valid_c = tid < kSlab && x_c < sj.n;
    uint32_t a_r = 0, a_c = 0;
    bool hole = false;
    if (valid_r) {
        a_r = si.acnt[x_r];
        hole = a_r + si.rcnt[x_r] != n_hap;
    }
    if (valid_c) {
        a_c = sj.acnt[x_c];
        hole = hole || a_c + sj.rcnt[x_c] != n_hap;
    }
    const bool wave_hole = __any(hole);
    if (lane == 0) sm.wflag[wave] = wave_hole ? 1u : 0u;
    if constexpr (kDosage && kHomTable) {   // (read by hole-free tiles only: there the table's count is HA)
        sm.r_hom[tid] = valid_r ? si.hom[x_r] : 0u;
        if (tid < kSlab) sm.c_hom[tid] = valid_c ? sj.hom[x_c] : 0u;
    } else {
        sm.r_hom[tid] = 0u;
        if (tid < kSlab) sm.c_hom[tid] = 0u;
    }
    block_sync();
    const bool general = __builtin_amdgcn_readfirstlane(sm.wflag[0] | sm.wflag[1] | sm.wflag[2] | sm.wflag[3]) != 0u;

    if (!general) {   // the shortcut's tables (published by the barrier in front of the K loop)
        if constexpr (kDosage && !kHomTable) {
            // the homozygotes of the tile's 128 + 256 SNPs: all threads share the 16-byte vectors, consecutive threads take
            // consecutive rows of one chunk (the slab's 128, then the I block's), several trips' loads in flight together
            constexpr uint32_t kList = kSlab + kTileRows;
            const uint32_t total = kList * nchunks;
#pragma unroll 4
            for (uint32_t idx = tid; idx < total; idx += kThreads) {
                const uint32_t ch = idx / kList, rr = idx - ch * kList;
                const uint32_t x = ti * kTileRows + (rr - kSlab);   // (an I row)
                uint4 w = {0u, 0u, 0u, 0u};
                if (rr < kSlab) w = sj.alt[(tj * nchunks + ch) * kSlab + rr];   // (pad rows of the slab are zero bits)
                else if (x < si.n) w = si.alt[((x / kSlab) * nchunks + ch) * kSlab + (x & (kSlab - 1u))];
                uint32_t c = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t ww = word_of(w, q);
                    c += __builtin_popcount(ww & (ww >> 1) & 0x55555555u);
                }
                if (c) atomicAdd(rr < kSlab ? &sm.c_hom[rr] : &sm.r_hom[rr - kSlab], c);
            }
            block_sync();
        }
        const double v_r = !valid_r ? 0.0 : (kDosage ? pw_var_dosage(n_obs, (double)a_r, (double)sm.r_hom[tid]) : pw_var_hap(n_obs, (double)a_r));
        sm.r_a[tid] = (double)a_r, sm.r_rs[tid] = pw_rs(v_r);
        if (tid < kSlab) {
            const double v_c = !valid_c ? 0.0 : (kDosage ? pw_var_dosage(n_obs, (double)a_c, (double)sm.c_hom[tid]) : pw_var_hap(n_obs, (double)a_c));
            sm.c_a[tid] = (double)a_c, sm.c_rs[tid] = pw_rs(v_c);
        }
    }

    // this wave's 64 rows lie in ONE slab of I (64 divides 128).  The last I block may reach past the padded plane (an odd
    // number of slabs): such a wave reads the last slab instead -- its rows are >= n_i, nothing of it is stored.
    const uint32_t row0 = ti * kTileRows + wave * kWaveRows;
    const uint32_t slabs_i = n_slabs(si.n);
    const uint32_t slab_i = row0 / kSlab < slabs_i ? row0 / kSlab : slabs_i - 1u;
    // lane's A source: row (row0 % 128) + l32 (+ 32 for the second tile), chunk 2 blk + half; planes are < 4 GiB: 32-bit indices
    const uint32_t a_off = (slab_i * nchunks + half) * kSlab + (row0 & (kSlab - 1u)) + l32;
    // thread's share of the J image: row tid % 128, chunk 2 blk + tid / 128
    const uint32_t b_row = tid & (kSlab - 1u), b_half = tid >> 7;
    const uint32_t b_off = (tj * nchunks + b_half) * kSlab + b_row;
    const uint32_t b_dst = b_half * kSlab + b_row;   // + step * 256
    auto load = [&](const uint4 *plane, uint32_t off, uint32_t blk) { return plane[off + (size_t)blk * kBlockVecs]; };

    v16f acc[kAcc];
    auto clear = [&]() {
#pragma unroll
        for (uint32_t t = 0; t < kAcc; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;
    };
    // accumulator element e of a tile is row (e & 3) + 8 (e >> 2) + 4 half of its 32, column l32
    auto tile_row = [&](int e) { return (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * half; };

    if (!general) {
        // ---- the shortcut: rect_kernel's K loop, one set in the wave's 2 x 4 tiles (acc[4 m + tt]).  One K-block per trip: the
        // next block's loads first, then the 4 x 8 MFMAs of this one out of `acur` and image[blk & 1], then the next block's J
        // bits become image[(blk + 1) & 1] -- last read in block blk - 1, which every wave left through the barrier at its end
        // -- and the barrier publishes it.  (Beyond the last block the loads repeat it: discarded.)
        auto expand_b = [&](uint4 *buf, const uint4 &bits) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t w = word_of(bits, q);
                *reinterpret_cast<v4i *>(buf + b_dst + (uint32_t)q * kBlockVecs) = kDosage ? expand32_b4_dosage(w) : expand32_b4(w);
            }
        };
        clear();
        uint4 acur[2], anxt[2];
        acur[0] = load(si.alt, a_off, 0u), acur[1] = load(si.alt, a_off + 32u, 0u);
        expand_b(sm.image[0], load(sj.alt, b_off, 0u));
        block_sync();   // (also publishes the tables)
        auto read_bf = [&](v4i (&bf)[4], const uint4 *rd, int w) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
                bf[tt] = *reinterpret_cast<const v4i *>(rd + ((uint32_t)w * 2u + half) * kSlab + 32u * tt + l32);
        };
        for (uint32_t blk = 0; blk < nblocks; ++blk) {
            const uint32_t nb = blk + 1u < nblocks ? blk + 1u : blk;
            const uint4 bits = load(sj.alt, b_off, nb);
            anxt[0] = load(si.alt, a_off, nb), anxt[1] = load(si.alt, a_off + 32u, nb);
            const uint4 *const rd = sm.image[blk & 1u];
            v4i bf[2][4], af[2][2];
            read_bf(bf[0], rd, 0);
#pragma unroll
            for (int m = 0; m < 2; ++m) af[0][m] = expand32_a4(acur[m].x);
            // the scheduling barriers keep the order as written (rect_kernel): the global loads at the top of the block, and
            // step w + 1's fragment reads and A expansion in front of step w's eight MFMAs
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
                    for (int tt = 0; tt < 4; ++tt) acc[4 * m + tt] = mfma4(af[w & 1][m], bf[w & 1][tt], acc[4 * m + tt]);
                __builtin_amdgcn_sched_barrier(0);
            }
            expand_b(sm.image[(blk + 1u) & 1u], bits);
            block_sync();
            acur[0] = anxt[0];
            acur[1] = anxt[1];
        }
        // the epilogue: n from the launch, a / b (and the homozygotes) and rs from the tables, c / S from the accumulators
        const uint32_t j0 = tj * kSlab + l32;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const uint32_t ri = wave * kWaveRows + 32u * m + tile_row(e);
                const double ra = sm.r_a[ri], rrs = sm.r_rs[ri];   // two addresses per wave: broadcast
                [[maybe_unused]] const double rh = (double)sm.r_hom[ri];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const uint32_t cj = 32u * tt + l32;
                    double k[kSets];
                    k[0] = n_obs, k[1] = ra, k[2] = sm.c_a[cj], k[kLast] = (double)acc[4 * m + tt][e];
                    if constexpr (kDosage) k[3] = rh, k[4] = (double)sm.c_hom[cj];
                    epi.cell(ti * kTileRows + ri, j0 + 32u * tt, tt, k, rrs, sm.c_rs[cj]);
                }
                if constexpr (Epi::kReduce) epi.row_done(ti * kTileRows + ri);
            }
        }
        if constexpr (Epi::kReduce) epi.template pass_done<4>(tj * kSlab + l32);
    } else {
        // ---- the general loop: pass ps holds every set of the kG tiles (m0, t0 ..) of the wave, acc[kG s + g]; the same block
        // structure, both planes, both operands of the image; then the epilogue of those cells
        auto expand_b = [&](uint4 *buf, const uint4 &alt, const uint4 &ref) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t wa = word_of(alt, q), wr = word_of(ref, q);
                v4i *const dst = reinterpret_cast<v4i *>(buf + b_dst + (uint32_t)q * kBlockVecs);
                if constexpr (kDosage) {
                    const uint32_t qc = ind_called(wa, wr), w = wa & (qc | (qc << 1));
                    dst[0] = expand32_b4_dosage(w);
                    dst[kOpVecs] = expand32_b4_called_hom(qc, w & (w >> 1));
                } else {
                    dst[0] = expand32_b4(wa);
                    dst[kOpVecs] = expand32_b4(wa | wr);
                }
            }
        };
        for (uint32_t ps = 0; ps < G::kPasses; ++ps) {
            const uint32_t m0 = ps / (4u / kG), t0 = (ps % (4u / kG)) * kG;
            const uint32_t a_at = a_off + 32u * m0;
            clear();
            uint4 a_alt = load(si.alt, a_at, 0u), a_ref = load(si.ref, a_at, 0u);
            // (image[0] is free: every wave left the last pass's reads through the barrier at the end of its last block)
            expand_b(sm.image[0], load(sj.alt, b_off, 0u), load(sj.ref, b_off, 0u));
            block_sync();
            for (uint32_t blk = 0; blk < nblocks; ++blk) {
                const uint32_t nb = blk + 1u < nblocks ? blk + 1u : blk;
                const uint4 b_alt = load(sj.alt, b_off, nb), b_ref = load(sj.ref, b_off, nb);
                const uint4 n_alt = load(si.alt, a_at, nb), n_ref = load(si.ref, a_at, nb);
                __builtin_amdgcn_sched_barrier(0);   // the global loads stay at the top of the block
                const uint4 *const rd = sm.image[blk & 1u];
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const uint32_t wa = word_of(a_alt, w), wr = word_of(a_ref, w);
                    v4i f0[kG], f1[kG];
#pragma unroll
                    for (uint32_t g = 0; g < kG; ++g) {
                        const uint4 *const at = rd + ((uint32_t)w * 2u + half) * kSlab + 32u * (t0 + g) + l32;
                        f0[g] = *reinterpret_cast<const v4i *>(at);
                        f1[g] = *reinterpret_cast<const v4i *>(at + kOpVecs);
                    }
                    if constexpr (kDosage) {
                        const uint32_t qc = ind_called(wa, wr), ww = wa & (qc | (qc << 1));
                        const v4i xg = expand32_a4_dosage(ww), xq = even_a4(qc), xm = even_a4(ww & (ww >> 1)), xo = odd_a4(qc);
#pragma unroll
                        for (uint32_t g = 0; g < kG; ++g) {
                            acc[kG * 5 + g] = mfma4(xg, f0[g], acc[kG * 5 + g]);   // S
                            acc[kG * 2 + g] = mfma4(xq, f0[g], acc[kG * 2 + g]);   // B
                            acc[kG * 1 + g] = mfma4(xg, f1[g], acc[kG * 1 + g]);   // A
                            acc[kG * 0 + g] = mfma4(xq, f1[g], acc[kG * 0 + g]);   // N
                            acc[kG * 3 + g] = mfma4(xm, f1[g], acc[kG * 3 + g]);   // HA
                            acc[kG * 4 + g] = mfma4(xo, f1[g], acc[kG * 4 + g]);   // HB
                        }
                    } else {
                        const v4i xa = expand32_a4(wa), xc = expand32_a4(wa | wr);
#pragma unroll
                        for (uint32_t g = 0; g < kG; ++g) {
                            acc[kG * 3 + g] = mfma4(xa, f0[g], acc[kG * 3 + g]);   // c
                            acc[kG * 2 + g] = mfma4(xc, f0[g], acc[kG * 2 + g]);   // b
                            acc[kG * 1 + g] = mfma4(xa, f1[g], acc[kG * 1 + g]);   // a
                            acc[kG * 0 + g] = mfma4(xc, f1[g], acc[kG * 0 + g]);   // n
                        }
                    }
                }
                expand_b(sm.image[(blk + 1u) & 1u], b_alt, b_ref);
                block_sync();
                a_alt = n_alt;
                a_ref = n_ref;
            }
            // the epilogue of this pass's cells: every integer from the accumulators, pw_rs per cell
            const uint32_t j0 = tj * kSlab + 32u * t0 + l32;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t i = ti * kTileRows + wave * kWaveRows + 32u * m0 + tile_row(e);
#pragma unroll
                for (uint32_t g = 0; g < kG; ++g) {
                    double k[kSets], rs_x = 0.0, rs_y = 0.0;
#pragma unroll
                    for (uint32_t s = 0; s < kSets; ++s) k[s] = (double)acc[kG * s + g][e];
                    if constexpr (Epi::kCells) {
                        if constexpr (kDosage) {
                            rs_x = pw_rs(pw_var_dosage(k[0], k[1], k[3]));
                            rs_y = pw_rs(pw_var_dosage(k[0], k[2], k[4]));
                        } else {
                            rs_x = pw_rs(pw_var_hap(k[0], k[1]));
                            rs_y = pw_rs(pw_var_hap(k[0], k[2]));
                        }
                    }
                    epi.cell(i, j0 + 32u * g, (int)g, k, rs_x, rs_y);
                }
                if constexpr (Epi::kReduce) epi.row_done(i);
            }
            if constexpr (Epi::kReduce) epi.template pass_done<kG>(j0);
        }
    }
}

}  // namespace pwc
}  // namespace ldx

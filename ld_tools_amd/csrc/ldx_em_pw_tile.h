// The tile of the EM kernels (em_rect_kernel of ldx_em.hip, emband_kernel of ldx_emband.hip): the
// five integers N A B S H of every cell of I slab ti x J slab tj, handed one cell per lane to the caller's emit functor -- the
// way tile_body of ldx_pwc_tile.h serves pwc_kernel and pwband_kernel.  ldx_em.hip's header describes the operands, the two K
// loops and the staging; here is only what a caller needs:
//   * tile_body<kPairwise> is called by the whole workgroup (256 threads, 2 x 2 waves of 64 x 64 cells).
//     kPairwise: the hole test on the tile's 128 rows and 128 columns (acnt + rcnt != n_hap) picks, workgroup-uniformly, the
//     two-set shortcut (N = n_hap / 2, A and B from acnt) or the four-pass five-set general loop.
//     !kPairwise: always the shortcut -- the plain form's cells; ref and rcnt are not read, and a null acnt (a caller that
//     wants S and H alone) gives A = B = 0.
//   * its first barrier publishes what the caller wrote to LDS of its own before the call; between two calls of one workgroup
//     the caller puts a block_sync() (tables, images and staged words are rewritten).
//   * emit(i, j, N, A, B, S, H) is called by EVERY lane of a wave at once (a hit appender may ballot), with 128 ti <= i <
//     128 (ti + 1) and 128 tj <= j < 128 (tj + 1); rows and columns beyond the panels come by with zero integers (the shortcut
//     skips the rows beyond the panel), so the functor tests its own bounds before it reads the integers.
#pragma once

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
static_assert(kImage == em::kImage && 2u * kImage <= em::kLdsBytes && kStage <= em::kLdsBytes, "the general loop lives in the two-set loop's LDS");

struct Side {
    const uint4 *alt, *ref;   // tiled bit planes (ldx_plane_bytes)
    const uint32_t *acnt;     // [n] ALT counts (null: the plain counts form)
    const uint32_t *rcnt;     // [n] REF counts
    uint32_t n;               // SNPs
};

// the tile's LDS: 65 KiB and 16 bytes
struct Smem {
    __attribute__((aligned(16))) unsigned char lds[em::kLdsBytes];   // K loops: two image buffers; epilogues: staged counts
    uint32_t cstat[kSlab];    // acnt of the slab's 128 columns
    uint32_t rstat[kSlab];    // acnt of the workgroup's 128 rows
    uint32_t wflag[em::kWaves];
};

__device__ __forceinline__ v16f mfma2(const v2i &a, const v2i &b, const v16f &c)
{
    const v8i a8 = {a.x, 0, a.y, 0, 0, 0, 0, 0};
    const v8i b8 = {b.x, 0, b.y, 0, 0, 0, 0, 0};
    // cbsz = blgp = 4: FP4 operands (4 registers each); scale operands 0 = the unscaled instruction
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 0, 0, 0);
}

template <bool kPairwise, typename Emit>
__device__ __forceinline__ void tile_body(Smem &sm, const Side &si, const Side &sj, uint32_t nblocks, uint32_t n_hap, uint32_t ti,
                                          uint32_t tj, uint32_t tid, Emit &emit)
{
    unsigned char *const lds = sm.lds;
    const uint32_t lane = tid & 63u, l32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wr = wave >> 1, wc = wave & 1u;   // the wave's 64 rows / 64 columns inside the 128 x 128 tile
    const uint32_t nchunks = 2u * nblocks;

    // ---- which path: does a SNP of this tile hold a hole?  Thread t < 128 owns column t of the slab, thread 128 + t row t.
    bool general = false;
    {
        const bool is_col = tid < kSlab;
        const uint32_t *const acnt = is_col ? sj.acnt : si.acnt;
        const uint32_t x = (is_col ? tj : ti) * kSlab + (tid & (kSlab - 1u));
        const bool live = x < (is_col ? sj.n : si.n);
        const uint32_t a = live && acnt ? acnt[x] : 0u;   // (a null table reads as zeros)
        (is_col ? sm.cstat : sm.rstat)[tid & (kSlab - 1u)] = a;
        if constexpr (kPairwise) {
            const uint32_t *const rcnt = is_col ? sj.rcnt : si.rcnt;
            const bool hole = live && a + rcnt[x] != n_hap;
            const bool wave_hole = __any(hole);
            if (lane == 0) sm.wflag[wave] = wave_hole ? 1u : 0u;
            block_sync();
            general = __builtin_amdgcn_readfirstlane(sm.wflag[0] | sm.wflag[1] | sm.wflag[2] | sm.wflag[3]) != 0u;
        }
    }

    if (!general) {
        // ---- the shortcut: the two-set K loop and epilogue; N, A and B from the launch and the tables
        v16f acc_s[2][2], acc_h[2][2];
        em::count_two_sets(lds, si.alt, sj.alt, ti, tj, nblocks, tid, acc_s, acc_h);
        const uint32_t *const stage = em::stage_two_sets(lds, tid, acc_s, acc_h);
        const uint32_t j = tj * kSlab + wc * kWaveCols + lane;
        const uint32_t a_j = sm.cstat[wc * kWaveCols + lane];
        const uint32_t row0 = ti * kSlab + wr * kWaveRows;
        const uint32_t rows = row0 < si.n ? (si.n - row0 < kWaveRows ? si.n - row0 : kWaveRows) : 0u;   // wave-uniform
        for (uint32_t rr = 0; rr < rows; ++rr) {
            __builtin_assume(row0 + rr < si.n);   // (a functor's own row test folds: its column test leaves the loop)
            const uint32_t packed = stage[rr * kWaveCols + lane];
            const uint32_t a_i = sm.rstat[wr * kWaveRows + rr];   // one address per wave: broadcast
            emit(row0 + rr, j, n_hap / 2u, a_i, a_j, packed >> em::kPackShift, packed & ((1u << em::kPackShift) - 1u));
        }
        return;
    }
    if constexpr (kPairwise) {
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
            uint4 a_alt = load(si.alt, a_off, 0u), a_ref = load(si.ref, a_off, 0u);
            // (the first buffer is free: every wave left the last pass's epilogue through the barrier at its end)
            expand_b(lds, load(sj.alt, b_off, 0u), load(sj.ref, b_off, 0u));
            block_sync();
            for (uint32_t blk = 0; blk < nblocks; ++blk) {
                const uint32_t nb = blk + 1u < nblocks ? blk + 1u : blk;
                const uint4 b_alt = load(sj.alt, b_off, nb), b_ref = load(sj.ref, b_off, nb);
                const uint4 n_alt = load(si.alt, a_off, nb), n_ref = load(si.ref, a_off, nb);
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
                emit(i0 + 2u * rr, j, N, ab >> kShiftA, ab & ((1u << kShiftA) - 1u), sh >> em::kPackShift,
                     sh & ((1u << em::kPackShift) - 1u));
            }
            block_sync();   // the next pass's first image overwrites what was staged
        }
    }
}

}  // namespace em_pw
}  // namespace ldx

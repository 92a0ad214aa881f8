// Firth logistic association scans (include/ldx.h, "Firth logistic association scan"): per (SNP, phenotype) cell the
// logistic fit of a 0/1 phenotype that maximises Firth's penalised likelihood l + 1/2 ln det I, by Fisher scoring on the modified
// score from the null fit.  The launch shape, the LDS tile, the cell's flags, phase 1, pass A, the Cholesky, the two triangular
// solves and the result store are ldx_logit_fit.h's, shared with the maximum-likelihood scan; this file keeps firth_kernel's
// iteration.
//   * an evaluation is two passes over the individuals, 64 at a time:
//       pass A  the information (information_pass without the gradient), then the 15 x 15 Cholesky I = L L^T, lane i on row i,
//               and M = L^-1 row by row (row k goes through LDS to the lanes below it).  When the step before was the last,
//               se = 1 / L_PP ends the fit here.
//       pass B  phase 1 again (eta, mu, w, r and the tile V); T = M V on the same MFMA: A[i][k] = M[i][4q + k] for the four K-groups
//               q of parameters, B[k][j] = V[4q + k][16 blk + j] for the four column blocks of 16 individuals -- 16 MFMAs a step,
//               as pass A.  C/D: col = lane & 15 (the individual), row = (lane >> 4) + 4 reg (the parameter), so
//               |M v_a|^2 = the four registers squared and summed, then two shfl_xor steps across lane >> 4; the lane whose
//               lane >> 4 is the block keeps it: lane a holds the sum of individual a again.  h_a = w_a |M v_a|^2, the adjusted
//               residual r_a + h_a (1/2 - mu_a) multiplies the lane's own column of the tile into fifteen partial sums of U*.
//     U* is joined by the fixed butterfly; lambda*^2 = |L^-1 U*|^2 comes out of the forward solve.
//   * the update: theta + length x step; an evaluation whose lambda*^2 did not fall goes back to the point before and halves length.
#include "ldx_logit_fit.h"

namespace ldx {
namespace firth {

using namespace logit;

// waves per SIMD the register budget is cut for (DESIGN.md 3.18 has the measurements; tools/ld_firth_timing.py builds the others)
#ifndef LDX_FIRTH_MIN_WAVES
#define LDX_FIRTH_MIN_WAVES 2
#endif
constexpr uint32_t kMinWaves = LDX_FIRTH_MIN_WAVES;
constexpr double kStop = 0x1p-88;

__global__ void __launch_bounds__(kThreads, kMinWaves) firth_kernel(Args p)
{
    __shared__ double s_tile[kWaves][kTile];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t snp = blockIdx.x * kWaves + wave, j = blockIdx.y;
    if (snp >= p.n_snps) return;   // (wave-uniform; the kernel has no workgroup barrier)
    const size_t o = (size_t)snp * p.ld_out + j;
    if (p.mode == 1u && __builtin_amdgcn_readfirstlane((uint32_t)p.flags[o]) != 5u) {
        if (lane == 0u) p.firth[o] = 0;   // a cell the ML scan settled: nothing else of it is touched
        return;
    }
    double *const tile = s_tile[wave];
    Cell c;
    double th[kPar - 1u], bt = 0.0;
    uint32_t flag = cell_setup(p, snp, j, lane, tile, c, th);
    const uint32_t P = c.P;
    const bool fitted = flag == 0u;

    double beta = NAN, se = NAN;
    uint32_t iter = 0;
    if (flag == 0u) {
        const uint32_t ci = lane & 15u, ck = lane >> 4;
        bool last = false;
        double length = 1.0, before = INFINITY, from = 0.0, step = 0.0;
        flag = 5u;   // until an evaluation ends the fit
        while (iter < LDX_FIRTH_MAX_ITER) {
            ++iter;
            // ---- pass A: the information
            v4d acc0, acc1;
            information_pass<false>(p, c, th, bt, acc0, acc1);
            double row[kPar];
            rows_of_accumulator(c, acc0, acc1, row);
            if (!cholesky_rows(c, row)) break;   // flag 5
            if (last) {
                beta = bt, se = se_of_last(c, row);
                flag = 0u;
                break;
            }
            // ---- M = L^-1, lane i on row i: row k is final once the rows above it are; it goes to the tile (M[k][j] at 17 k + j),
            // and the lanes below add L[i][k] M[k][j] to their sums
            {
                double part[kPar - 1u];
#pragma unroll
                for (uint32_t m = 0; m < kPar - 1u; ++m) part[m] = 0.0;
#pragma unroll
                for (uint32_t k = 0; k < kPar; ++k) {
                    const double rk = 1.0 / row[k];   // of use in lane k alone, where row[k] is the pivot
                    if (lane == k) {
#pragma unroll
                        for (uint32_t m = 0; m < k; ++m) tile[k * 17u + m] = -(part[m] * rk);
                        tile[k * 17u + k] = rk;
                    }
                    wave_sync();
                    if (lane > k) {
#pragma unroll
                        for (uint32_t m = 0; m <= k && m < kPar - 1u; ++m) part[m] += row[k] * tile[k * 17u + m];
                    }
                }
            }
            // the A operands of pass B: A[i = ci][k = ck] of K-group q is M[ci][4 q + ck], zero above the diagonal and in row 15
            double ma[4];
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                const uint32_t m = 4u * q + ck;
                ma[q] = ci < kPar && m <= ci ? tile[ci * 17u + m] : 0.0;
            }
            wave_sync();
            // ---- pass B: the hat diagonal and the modified score
            double us[kPar];
#pragma unroll
            for (uint32_t m = 0; m < kPar; ++m) us[m] = 0.0;
            for (uint32_t s = 0; s < c.steps; ++s) {
                double mu, w, r;
                phase1(p, c, th, bt, s, mu, w, r);
                wave_sync();
                const uint32_t left = p.n_ind - s * 64u, blocks = left >= 64u ? 4u : (left + 15u) / 16u;
                double hs = 0.0;
                for (uint32_t blk = 0; blk < blocks; ++blk) {
                    v4d t = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (uint32_t q = 0; q < 4u; ++q) {
                        const uint32_t m = 4u * q + ck;
                        const double bv = m < kPar ? tile[m * kStride + 16u * blk + ci] : 0.0;
                        t = __builtin_amdgcn_mfma_f64_16x16x4f64(ma[q], bv, t, 0, 0, 0);
                    }
                    double ss = ((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + t[3] * t[3];
                    ss += __shfl_xor(ss, 16);
                    ss += __shfl_xor(ss, 32);
                    if (ck == blk) hs = ss;
                }
                const double adj = r + (w * hs) * (0.5 - mu);
#pragma unroll
                for (uint32_t m = 0; m < kPar; ++m) us[m] += tile[m * kStride + lane] * adj;   // the lane's own column
                wave_sync();
            }
            double u = 0.0;
#pragma unroll
            for (uint32_t m = 0; m < kPar; ++m) {
                const double t = wave_sum(us[m]);
                if (lane == m) u = t;
            }
            // lambda*^2 and the step
            double dec;
            const double zf = solve_forward(c, row, u, dec);
            const double delta = solve_backward(c, row, zf);
            if (!(dec == dec) || isinf(dec)) break;   // flag 5
            // the safeguard: a point whose lambda*^2 is not below that of the point before is given up for one half as far along
            // the same step, and the step length stays halved for the rest of the fit.  Lane k keeps parameter k of the point
            // before (from) and of its step (step); a length of 1 leaves the bits of the plain update.
            if (dec >= before) {
                length *= 0.5;
            } else {
                double own = 0.0;
#pragma unroll
                for (uint32_t k = 0; k < kPar - 1u; ++k)
                    if (lane == k) own = th[k];
                if (lane == P) own = bt;
                from = own, step = delta, before = dec;
                if (dec <= kStop) last = true;   // this step is the last: the information once more, at the new point
            }
            const double moved = from + length * step;
#pragma unroll
            for (uint32_t k = 0; k < kPar - 1u; ++k)
                if (k < P) th[k] = __shfl(moved, (int)k);
            bt = __shfl(moved, (int)P);
        }
    }
    if (lane == 0u) {
        store_cell(p, o, flag, beta, se, iter);
        p.firth[o] = fitted ? 1 : 0;
    }
}

}  // namespace firth
}  // namespace ldx

using namespace ldx;

extern "C" int ldx_glm_firth_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                                 const uint32_t *counts, const double *design, size_t ld_design, uint32_t n_cov, const uint8_t *y,
                                 const double *theta0, uint32_t n_pheno, double max_vif, double *beta, double *se, double *z,
                                 double *p, double *neglog10_p, uint8_t *flags, uint8_t *n_iter, size_t ld_out, uint32_t mode,
                                 uint8_t *firth, void *stream)
{
    logit::Args a;
    if (const int rc = logit::fill_args("ldx_glm_firth_dev", alt, ref, n_snps, n_hap, keep, counts, design, ld_design, n_cov, y,
                                        theta0, n_pheno, max_vif, beta, se, z, p, neglog10_p, flags, n_iter, ld_out, true, mode,
                                        firth, a))
        return rc;
    const dim3 grid((n_snps + logit::kWaves - 1u) / logit::kWaves, n_pheno);
    firth::firth_kernel<<<grid, logit::kThreads, 0, (hipStream_t)stream>>>(a);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

// Logistic association scans (include/ldx.h, "logistic association scan"): per (SNP, phenotype) cell the
// maximum-likelihood logistic fit of a 0/1 phenotype on the genotype, the intercept and the covariates, by Newton from the null fit.
// The launch shape, the LDS tile, the cell's flags (cell_setup), phase1, rows_of_accumulator, se_of_last, the result store and the
// entry's argument rules are ldx_logit_fit.h's, shared with the Firth scan.  This file keeps logit_kernel's iteration -- an evaluation
// is ONE pass with the gradient in the information's spare 16th column, then Newton's step, until the decrement |L^-1 U|^2 stops it
// and the information is evaluated once more for se -- and, spelled IN PLACE, the pass, the Cholesky and the two solves: through
// the header's information_pass, cholesky_rows and solve_* (the same operations, which firth_kernel uses) this kernel measured 0.5 -
// 1 % slower.  A change to one of those three steps is made in both places.
#include "ldx_logit_fit.h"

namespace ldx {
namespace logit {

// waves per SIMD the register budget is cut for.  Measured at 100 000 SNPs x 2504 individuals, 10 covariates, one phenotype
// (tools/ld_logistic_timing.py): 1 (no spill) 98.7 ms, 2 (then 72, now 80 bytes of scratch per lane, in the solve) 46.1 ms, 3 72.9 ms, 4 64.6 ms
constexpr uint32_t kMinWaves = 2;
constexpr double kDecrement = 0x1p-60;

__global__ void __launch_bounds__(kThreads, kMinWaves) logit_kernel(Args p)
{
    __shared__ double s_tile[kWaves][kTile];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t snp = blockIdx.x * kWaves + wave, j = blockIdx.y;
    if (snp >= p.n_snps) return;   // (wave-uniform; the kernel has no workgroup barrier)
    Cell c;
    double th[kPar - 1u], bt = 0.0;
    uint32_t flag = cell_setup(p, snp, j, lane, s_tile[wave], c, th);
    const uint32_t P = c.P;

    double beta = NAN, se = NAN;
    uint32_t iter = 0;
    if (flag == 0u) {
        bool last = false;
        flag = 5u;   // until a pass ends the fit
        while (iter < LDX_LOGIT_MAX_ITER) {
            ++iter;
            // the pass: information_pass<true> of the header, in place
            const uint32_t ci = lane & 15u, ck = lane >> 4;
            v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
            for (uint32_t s = 0; s < c.steps; ++s) {
                double mu, w, r;
                phase1(p, c, th, bt, s, mu, w, r);
                c.tile[kRowR * kStride + lane] = r;
                c.tile[kRowW * kStride + lane] = w;
                wave_sync();
                const uint32_t left = p.n_ind - s * 64u, groups = left >= 64u ? 16u : (left + 3u) / 4u;
                for (uint32_t t = 0; t < groups; ++t) {
                    const double v = c.tile[ci * kStride + 4u * t + ck];
                    const double wt = c.tile[kRowW * kStride + 4u * t + ck];
                    const double av = ci == 15u ? 0.0 : v, bv = ci == 15u ? v : wt * v;
                    if (t & 1u) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc1, 0, 0, 0);
                    else acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc0, 0, 0, 0);
                }
                wave_sync();
            }
            double row[kPar];
            const double u = rows_of_accumulator(c, acc0, acc1, row);
            // cholesky_rows, solve_forward and solve_backward of the header, in place
            double *const tile = c.tile;
            bool pd = true;
#pragma unroll
            for (uint32_t k = 0; k < kPar; ++k) {
                const double acc = __shfl(row[k], (int)k);
                if (!(acc > 0.0) || isinf(acc)) pd = false;
                const double dg = sqrt(acc);
                const double l = lane == k ? dg : row[k] / dg;
                row[k] = l;
                double *const col = tile + 16u * 17u + 16u * (k & 1u);
                if (lane < kPar) col[lane] = l;
                wave_sync();
#pragma unroll
                for (uint32_t m = k + 1u; m < kPar; ++m) row[m] -= l * col[m];
            }
            if (!pd) break;   // flag 5
            if (last) {
                beta = bt, se = se_of_last(c, row);
                flag = 0u;
                break;
            }
            if (lane < kPar) {
#pragma unroll
                for (uint32_t k = 0; k < kPar; ++k) tile[lane * 17u + k] = row[k];
            }
            double zc = 0.0, dec = 0.0, uu = u;
#pragma unroll
            for (uint32_t k = 0; k < kPar; ++k) {
                const double t = __shfl(uu / row[k], (int)k);
                if (lane == k) zc = t;
                uu -= row[k] * t;
                dec += t * t;
            }
            wave_sync();
            double diag = 1.0;
#pragma unroll
            for (uint32_t k = 0; k < kPar; ++k)
                if (lane == k) diag = row[k];
            for (int k = (int)kPar - 1; k >= 0; --k) {
                const double d = __shfl(zc / diag, k);
                if ((int)lane == k) zc = d;
                if ((int)lane < k) zc -= tile[(uint32_t)k * 17u + lane] * d;
            }
            wave_sync();
            const double delta = zc;
            if (!(dec == dec) || isinf(dec)) break;   // flag 5
#pragma unroll
            for (uint32_t k = 0; k < kPar - 1u; ++k)
                if (k < P) th[k] += __shfl(delta, (int)k);
            bt += __shfl(delta, (int)P);
            if (dec <= kDecrement) last = true;   // this step was the last: the information once more, at the new point
        }
    }
    if (lane == 0u) store_cell(p, (size_t)snp * p.ld_out + j, flag, beta, se, iter);
}

}  // namespace logit
}  // namespace ldx

using namespace ldx;

extern "C" int ldx_glm_logistic_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                                    const uint32_t *counts, const double *design, size_t ld_design, uint32_t n_cov,
                                    const uint8_t *y, const double *theta0, uint32_t n_pheno, double max_vif, double *beta,
                                    double *se, double *z, double *p, double *neglog10_p, uint8_t *flags, uint8_t *n_iter,
                                    size_t ld_out, void *stream)
{
    logit::Args a;
    if (const int rc = logit::fill_args("ldx_glm_logistic_dev", alt, ref, n_snps, n_hap, keep, counts, design, ld_design, n_cov, y,
                                        theta0, n_pheno, max_vif, beta, se, z, p, neglog10_p, flags, n_iter, ld_out, false, 0u, nullptr, a))
        return rc;
    const dim3 grid((n_snps + logit::kWaves - 1u) / logit::kWaves, n_pheno);
    logit::logit_kernel<<<grid, logit::kThreads, 0, (hipStream_t)stream>>>(a);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

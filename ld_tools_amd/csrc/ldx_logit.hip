// Logistic association scans (include/ldx.h, "logistic association scan"): per (SNP, phenotype) cell the
// maximum-likelihood logistic fit of a 0/1 phenotype on the genotype, the intercept and the covariates, by Newton from the null fit.
//   * logit_kernel: ONE WAVE PER CELL, four cells (consecutive SNPs, one phenotype) per workgroup.  The waves of a workgroup share
//     nothing but the LDS allocation -- no barrier, no atomics: a cell's bits depend on its SNP, its phenotype and the design alone.
//   * a pass over the individuals, 64 at a time (one 16-byte chunk of the SNP's row in the tiled planes = 64 individuals):
//       phase 1, a lane per individual: the lane loads its column of the design (coalesced), forms x, eta, mu, w, r and leaves the
//                row v = (d, x), r and w in the wave's LDS tile;
//       phase 2, sixteen K-groups of 4 individuals: I += sum_a v_a (w_a v_a)^T on v_mfma_f64_16x16x4_f64 -- A[i][k] = v_a[i],
//                B[k][j] = w_a v_a[j]; the spare 16th column carries the gradient: B[k][15] = r_a, A row 15 = 0.  Two accumulators
//                (even and odd K-groups) are joined once at the end of the pass.
//     C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg.
//   * the 15 x 15 system of a pass: the accumulator goes through LDS to one row per lane, unused parameters become identity rows,
//     and the wave runs a Cholesky factorisation, lane i on row i, the pivot column passed through LDS; two triangular solves.
// Individuals are walked in their order; the pad individuals of the last step are zeros in v, w and r, which add nothing.
#include <math.h>

#include "ldx_fp4.h"
#include "ldx_tail.h"   // normal_tail

namespace ldx {
namespace logit {

constexpr uint32_t kWaves = 4;                 // cells of a workgroup
constexpr uint32_t kThreads = 64u * kWaves;
// waves per SIMD the register budget is cut for.  Measured at 100 000 SNPs x 2504 individuals, 10 covariates, one phenotype
// (tools/ld_logistic_timing.py): 1 (no spill) 98.7 ms, 2 (72 bytes of scratch per lane, in the solve) 46.1 ms, 3 72.9 ms, 4 64.6 ms
constexpr uint32_t kMinWaves = 2;
constexpr uint32_t kPar = 15;                  // parameters of the tile: intercept + LDX_LOGIT_MAX_COV + genotype
constexpr uint32_t kRowR = 15, kRowW = 16;     // rows of the LDS tile that hold r and w
constexpr uint32_t kStride = 68;               // doubles per row of the tile: rows i and i + 1 start 8 banks apart
constexpr uint32_t kTile = 17u * kStride;      // doubles of a wave's tile
constexpr double kDecrement = 0x1p-60;

typedef double v4d __attribute__((ext_vector_type(4)));

struct Args {
    const uint32_t *alt, *ref;   // the panel's tiled planes, as words
    const uint8_t *keep;
    const uint32_t *counts;
    uint32_t n_snps, n_ind, hap_chunks;
    const double *design;        // [n_par - 1][ld_design]
    size_t ld_design;
    uint32_t n_dcol;             // n_cov + 1 columns of the design
    const uint8_t *y;
    const double *theta0;
    uint32_t n_pheno;
    double max_vif;
    double *beta, *se, *z, *p, *nlp;
    uint8_t *flags, *n_iter;
    size_t ld_out;
};

// the sum over the lanes in the order of a fixed butterfly: the same bits in every lane and in every launch
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// LDS traffic of ONE wave is executed in order; this keeps the compiler from moving a read of the tile above the writes of other
// lanes of the wave that it cannot see as a dependence
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(kThreads, kMinWaves) logit_kernel(Args p)
{
    __shared__ double s_tile[kWaves][kTile];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t snp = blockIdx.x * kWaves + wave, j = blockIdx.y;
    if (snp >= p.n_snps) return;   // (wave-uniform; the kernel has no workgroup barrier)
    double *const tile = s_tile[wave];
    const uint32_t P = p.n_dcol;   // columns of the design = index of the genotype among the parameters
    const uint32_t steps = (p.n_ind + 63u) / 64u;
    const size_t row_words = (((size_t)(snp / kSlab) * p.hap_chunks) * kSlab + (snp & (kSlab - 1u))) * 4u + (lane >> 4);
    const uint32_t bit = 2u * (lane & 15u);

    // this lane's genotype of step s: x = g - mu for a called individual, 0 otherwise
    const long long n = p.counts[4u * (size_t)snp], het = p.counts[4u * (size_t)snp + 1u], hom = p.counts[4u * (size_t)snp + 2u];
    const long long s1 = het + 2 * hom, e2 = het + 4 * hom, num = n * e2 - s1 * s1;
    const bool kept = p.keep == nullptr || p.keep[snp] != 0;
    uint32_t flag = (!kept || n == 0) ? 1u : (num == 0 ? 2u : 0u);
    const double mu_g = flag == 0u ? (double)s1 / (double)n : 0.0;
    auto geno_x = [&](uint32_t s) -> double {
        const size_t at = row_words + (size_t)s * kSlab * 4u;
        const GenoWords g = geno_words(p.alt[at], p.ref[at]);
        const uint32_t q = (g.q >> bit) & 1u, hz = (g.z >> bit) & 1u, ht = (g.t >> bit) & 1u;
        return q && s * 64u + lane < p.n_ind ? (double)(ht + 2u * hz) - mu_g : 0.0;
    };

    // flag 3: d = xx - sum_c (sum_a Q_ac x_a)^2 with Q = B / sqrt N, xx from the integers as in the linear scan
    if (flag == 0u) {
        double dot[kPar - 1u];
#pragma unroll
        for (uint32_t c = 0; c < kPar - 1u; ++c) dot[c] = 0.0;
        for (uint32_t s = 0; s < steps; ++s) {
            const uint32_t a = s * 64u + lane;
            const double x = geno_x(s);
            if (a < p.n_ind) {
#pragma unroll
                for (uint32_t c = 0; c < kPar - 1u; ++c)
                    if (c < P) dot[c] += p.design[c * p.ld_design + a] * x;
            }
        }
        const double xx = (double)num / (double)n;
        double sum = 0.0;
#pragma unroll
        for (uint32_t c = 0; c < kPar - 1u; ++c)
            if (c < P) {
                const double h = wave_sum(dot[c]);
                sum += (h * h) / (double)p.n_ind;
            }
        const double d = xx - sum;
        if (d * p.max_vif < xx) flag = 3u;
    }
    double th[kPar - 1u] = {}, bt = 0.0;
    if (flag == 0u) {
#pragma unroll
        for (uint32_t c = 0; c < kPar - 1u; ++c) {
            th[c] = c < P ? p.theta0[(size_t)j * P + c] : 0.0;
            if (th[c] != th[c]) flag = 4u;
        }
    }

    double beta = NAN, se = NAN;
    uint32_t iter = 0;
    if (flag == 0u) {
        const uint8_t *const yj = p.y + (size_t)j * p.ld_design;
        const uint32_t ci = lane & 15u, ck = lane >> 4;
        bool last = false;
        flag = 5u;   // until a pass ends the fit
        while (iter < LDX_LOGIT_MAX_ITER) {
            ++iter;
            v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
            for (uint32_t s = 0; s < steps; ++s) {
                // phase 1: a lane per individual
                const uint32_t a = s * 64u + lane;
                const bool live = a < p.n_ind;
                const double x = geno_x(s);
                double eta = 0.0;
#pragma unroll
                for (uint32_t c = 0; c < kPar - 1u; ++c) {
                    double b = 0.0;
                    if (c < P) {
                        b = live ? p.design[c * p.ld_design + a] : 0.0;
                        eta += th[c] * b;
                    }
                    tile[c * kStride + lane] = b;
                }
                eta += bt * x;
                // rows P + 1 .. 14 hold zeros (the loop above wrote them, this line the last), row P the genotype
                tile[(kPar - 1u) * kStride + lane] = 0.0;
                tile[P * kStride + lane] = x;
                const double e = exp(-fabs(eta)), den = 1.0 + e;
                const double hi = 1.0 / den, lo = e / den;          // the larger and the smaller of mu and 1 - mu
                const double mu = eta >= 0.0 ? hi : lo, om = eta >= 0.0 ? lo : hi;
                const bool yes = live && yj[a] != 0;
                tile[kRowR * kStride + lane] = live ? (yes ? om : -mu) : 0.0;
                tile[kRowW * kStride + lane] = live ? hi * lo : 0.0;
                wave_sync();
                // phase 2: the K-groups of this step that hold an individual
                const uint32_t left = p.n_ind - s * 64u, groups = left >= 64u ? 16u : (left + 3u) / 4u;
                for (uint32_t t = 0; t < groups; ++t) {
                    const double v = tile[ci * kStride + 4u * t + ck];
                    const double w = tile[kRowW * kStride + 4u * t + ck];
                    const double av = ci == 15u ? 0.0 : v, bv = ci == 15u ? v : w * v;
                    if (t & 1u) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc1, 0, 0, 0);
                    else acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc0, 0, 0, 0);
                }
                wave_sync();
            }
            // the accumulator to one row per lane: C[row = ck + 4 reg][col = ci]
#pragma unroll
            for (uint32_t r = 0; r < 4u; ++r) tile[(ck + 4u * r) * 17u + ci] = acc0[r] + acc1[r];
            wave_sync();
            double row[kPar], u;
            {
                const uint32_t ri = lane < 15u ? lane : 0u;
#pragma unroll
                for (uint32_t c = 0; c < kPar; ++c) row[c] = tile[ri * 17u + c];
                u = tile[ri * 17u + 15u];
                if (lane > P) {   // a parameter the cell does not have: an identity row, no gradient
#pragma unroll
                    for (uint32_t c = 0; c < kPar; ++c) row[c] = c == lane ? 1.0 : 0.0;
                    u = 0.0;
                }
            }
            wave_sync();
            // Cholesky, lane i on row i: after column c, row[c] holds L[i][c] in the lanes i >= c
            bool pd = true;
#pragma unroll
            for (uint32_t c = 0; c < kPar; ++c) {
                const double acc = __shfl(row[c], (int)c);
                if (!(acc > 0.0) || isinf(acc)) pd = false;
                const double dg = sqrt(acc);
                const double l = lane == c ? dg : row[c] / dg;
                row[c] = l;
                // the column goes to the other lanes through the tile (two buffers in turn: one wave_sync per column)
                double *const col = tile + 16u * 17u + 16u * (c & 1u);
                if (lane < kPar) col[lane] = l;
                wave_sync();
#pragma unroll
                for (uint32_t k = c + 1u; k < kPar; ++k) row[k] -= l * col[k];
            }
            if (!pd) break;   // flag 5
            if (last) {
                // the genotype is the last parameter that is coupled: [I^-1]_PP = 1 / L_PP^2
                double dgl = 0.0;
#pragma unroll
                for (uint32_t c = 0; c < kPar; ++c)
                    if (lane == c) dgl = row[c];
                beta = bt, se = 1.0 / __shfl(dgl, (int)P);
                flag = 0u;
                break;
            }
            // L to the tile, a row per lane: the backward solve reads its columns
            if (lane < kPar) {
#pragma unroll
                for (uint32_t c = 0; c < kPar; ++c) tile[lane * 17u + c] = row[c];
            }
            // forward: L zf = U, zf[c] left in lane c; the decrement |zf|^2 in the order c = 0, 1, ...
            double zc = 0.0, dec = 0.0;
#pragma unroll
            for (uint32_t c = 0; c < kPar; ++c) {
                const double t = __shfl(u / row[c], (int)c);
                if (lane == c) zc = t;
                u -= row[c] * t;
                dec += t * t;
            }
            wave_sync();
            // backward: L^T delta = zf, delta[c] left in lane c; lane i < c reads L[c][i]
            double diag = 1.0;
#pragma unroll
            for (uint32_t c = 0; c < kPar; ++c)
                if (lane == c) diag = row[c];
            for (int c = (int)kPar - 1; c >= 0; --c) {
                const double d = __shfl(zc / diag, c);
                if ((int)lane == c) zc = d;
                if ((int)lane < c) zc -= tile[(uint32_t)c * 17u + lane] * d;
            }
            wave_sync();
            if (!(dec == dec) || isinf(dec)) break;   // flag 5
#pragma unroll
            for (uint32_t c = 0; c < kPar - 1u; ++c)
                if (c < P) th[c] += __shfl(zc, (int)c);
            bt += __shfl(zc, (int)P);
            if (dec <= kDecrement) last = true;   // this step was the last: the information once more, at the new point
        }
    }
    if (lane == 0u) {
        double zs = NAN, pv = NAN, nlp = NAN;
        if (flag == 0u && !(se == se && beta == beta && !isinf(se) && !isinf(beta))) flag = 5u;
        if (flag == 0u) {
            zs = beta / se;
            normal_tail(zs, pv, nlp);
        } else {
            beta = se = NAN;
        }
        const size_t o = (size_t)snp * p.ld_out + j;
        p.beta[o] = beta, p.se[o] = se, p.z[o] = zs, p.p[o] = pv, p.nlp[o] = nlp;
        p.flags[o] = (uint8_t)flag, p.n_iter[o] = (uint8_t)iter;
    }
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
    const char *const who = "ldx_glm_logistic_dev";
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, ref); LDX_ARG_PTR(who, counts); LDX_ARG_PTR(who, design); LDX_ARG_PTR(who, y);
    LDX_ARG_PTR(who, theta0); LDX_ARG_PTR(who, beta); LDX_ARG_PTR(who, se); LDX_ARG_PTR(who, z); LDX_ARG_PTR(who, p);
    LDX_ARG_PTR(who, neglog10_p); LDX_ARG_PTR(who, flags); LDX_ARG_PTR(who, n_iter);
    LDX_ARG_REQUIRE(n_hap != 0u && n_hap % 2u == 0u, "%s: n_hap %u must be even and non-zero (haplotypes 2a and 2a + 1 are individual a)",
                    who, n_hap);
    if (n_hap > LDX_MAX_HAPS) {
        set_error("%s: n_hap %u > LDX_MAX_HAPS", who, n_hap);
        return LDX_E_UNSUPPORTED;
    }
    LDX_ARG_REQUIRE(n_snps != 0u && n_pheno != 0u, "%s: n_snps %u and n_pheno %u must be non-zero", who, n_snps, n_pheno);
    LDX_ARG_REQUIRE(n_pheno <= 65535u, "%s: n_pheno %u > 65535 in one call", who, n_pheno);
    LDX_ARG_REQUIRE(n_cov <= LDX_LOGIT_MAX_COV, "%s: n_cov %u > LDX_LOGIT_MAX_COV = %u", who, n_cov, LDX_LOGIT_MAX_COV);
    const uint32_t n_ind = n_hap / 2u;
    LDX_ARG_REQUIRE(ld_design >= n_ind, "%s: ld_design %zu < n_ind %u", who, ld_design, n_ind);
    LDX_ARG_REQUIRE(ld_out >= n_pheno, "%s: ld_out %zu < n_pheno %u", who, ld_out, n_pheno);
    LDX_ARG_REQUIRE(n_ind > n_cov + 2u, "%s: n_ind %u leaves no degree of freedom beside the intercept, %u covariates and the genotype",
                    who, n_ind, n_cov);
    LDX_ARG_REQUIRE(max_vif > 1.0, "%s: max_vif must be > 1", who);
    if (const int rc = plane_check(who, nullptr, n_snps, n_hap)) return rc;
    logit::Args a{};
    a.alt = (const uint32_t *)alt, a.ref = (const uint32_t *)ref, a.keep = keep, a.counts = counts;
    a.n_snps = n_snps, a.n_ind = n_ind, a.hap_chunks = n_chunks(n_hap);
    a.design = design, a.ld_design = ld_design, a.n_dcol = n_cov + 1u;
    a.y = y, a.theta0 = theta0, a.n_pheno = n_pheno, a.max_vif = max_vif;
    a.beta = beta, a.se = se, a.z = z, a.p = p, a.nlp = neglog10_p, a.flags = flags, a.n_iter = n_iter, a.ld_out = ld_out;
    const dim3 grid((n_snps + logit::kWaves - 1u) / logit::kWaves, n_pheno);
    logit::logit_kernel<<<grid, logit::kThreads, 0, (hipStream_t)stream>>>(a);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

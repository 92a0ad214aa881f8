// Linear association scans (include/ldx.h, "association scan"): per SNP the least-squares fit of each phenotype
// on the genotype, the intercept and the covariates, from the integers of the reverse genotype product.
//   * snp_counts_kernel: the called, heterozygous and homozygous-ALT individuals per SNP, straight from the panel's tiled planes.
//     A workgroup owns a slab of 128 SNPs; thread (row, half) walks the chunks half, half + 2, ... of its row -- 16-byte loads that
//     consecutive rows coalesce -- makes the genotype words with geno_words (the reverse product's own) and counts their bits; the
//     two halves meet in LDS and half 0 stores the row as one 16-byte group.
//   * glm_linear_kernel: a workgroup owns 128 SNPs.  Phase 1, once per SNP: a wave takes a SNP, lane a the covariate column a
//     (consecutive lanes on consecutive int64 columns), and leaves mu, d and the SNP's flag in LDS; the sum of the h_a^2 runs over
//     the lanes in order.  Phase 2, once per cell: thread c of the workgroup takes cell (c / p, c % p) -- again consecutive lanes
//     on consecutive columns -- computes beta, se, t and the t tail, and stores the six outputs.  The tail's continued fraction
//     ends at a different step in every lane.
// beta, se, t and the flags are fp64 + - x / sqrt on exactly converted integers in the order written here (-ffp-contract=off):
// ops.glm_linear_host repeats them bit for bit.
#include <math.h>

#include "ldx_fp4.h"

namespace ldx {
namespace glm {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kRows = 128;        // SNPs of a statistics workgroup
constexpr int kMaxSteps = 512;         // passes of the continued fraction (two terms each) before flag 6
constexpr double kEps = 0x1p-50;       // |del - 1| at which the fraction has converged
constexpr double kTiny = 1e-300;
constexpr double kLn10 = 2.302585092994046;

__global__ void __launch_bounds__(kThreads) snp_counts_kernel(const uint4 *alt, const uint4 *ref, const uint8_t *keep,
                                                              uint32_t n_snps, uint32_t hap_chunks, uint4 *counts)
{
    __shared__ uint32_t part[3][kSlab];
    const uint32_t row = threadIdx.x & (kSlab - 1u), half = threadIdx.x >> 7;
    const uint32_t s = blockIdx.x * kSlab + row;
    const bool kept = s < n_snps && (keep == nullptr || keep[s] != 0);
    uint32_t n = 0, het = 0, hom = 0;
    if (kept) {
        // whole chunks are counted: the pad haplotypes of the last ones are zero bits in both planes, so not called (the reverse
        // product does not need that: it bounds its weights by n_ind)
        for (uint32_t c = half; c < hap_chunks; c += 2u) {
            const size_t o = ((size_t)blockIdx.x * hap_chunks + c) * kSlab + row;
            const uint4 va = alt[o], vr = ref[o];
#pragma unroll
            for (int wd = 0; wd < 4; ++wd) {
                const GenoWords g = geno_words(word_of(va, wd), word_of(vr, wd));
                n += __popc(g.q), het += __popc(g.t), hom += __popc(g.z);
            }
        }
    }
    if (half == 1u) part[0][row] = n, part[1][row] = het, part[2][row] = hom;
    block_sync();
    if (half == 0u && s < n_snps) counts[s] = uint4{n + part[0][row], het + part[1][row], hom + part[2][row], 0u};
}

struct LinArgs {
    const long long *z, *zc;
    size_t ld_z;
    const uint32_t *counts;
    uint32_t n_snps, n_cov, n_pheno;
    const long long *exps;
    const double *yy;
    double df, max_vif, ln_beta;   // ln_beta = ln B(df / 2, 1 / 2), the same for every cell
    double *beta, *se, *t, *p, *nlp;
    uint8_t *flags;
    size_t ld_out;
};

// the continued fraction of the incomplete beta function I_x(a, b) by the modified Lentz method, for x < (a + 1) / (a + b + 2);
// false when kMaxSteps passes do not bring it to kEps
__device__ __forceinline__ bool beta_cf(double a, double b, double x, double &h)
{
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < kTiny) d = kTiny;
    d = 1.0 / d;
    h = d;
    for (int m = 1; m <= kMaxSteps; ++m) {
        const double dm = (double)m, m2 = 2.0 * dm;
        double aa = dm * (b - dm) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < kTiny) d = kTiny;
        c = 1.0 + aa / c;
        if (fabs(c) < kTiny) c = kTiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < kTiny) d = kTiny;
        c = 1.0 + aa / c;
        if (fabs(c) < kTiny) c = kTiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= kEps) return true;
    }
    return false;
}

// p = 2 P(T_df <= -|t|) = I_x(df / 2, 1 / 2), x = df / (df + t^2), and -log10 p from ln p: the front factor stays in log space,
// so a p below the fp64 range still has its -log10.  Small |t| takes the complement 1 - I_{1-x}(1 / 2, df / 2), 1 - x formed as
// t^2 / (df + t^2).  false: the iteration cap.
__device__ __forceinline__ bool t_tail(double t, double df, double ln_beta, double &pv, double &nlp)
{
    const double t2 = t * t, a = 0.5 * df, b = 0.5;
    if (t2 == 0.0) {
        pv = 1.0, nlp = 0.0;
        return true;
    }
    if (isinf(t2)) {
        pv = 0.0, nlp = INFINITY;
        return true;
    }
    const double den = df + t2, x = df / den, omx = t2 / den;
    const double front = a * -log1p(t2 / df) + b * log(omx) - ln_beta;   // ln of x^a (1 - x)^b / B(a, b)
    double h, lnp;
    if (x < (a + 1.0) / (a + b + 2.0)) {
        if (!beta_cf(a, b, x, h)) return false;
        lnp = front - log(a) + log(h);
        pv = exp(lnp);
    } else {
        if (!beta_cf(b, a, omx, h)) return false;
        const double comp = exp(front - log(b)) * h;
        pv = 1.0 - comp;
        lnp = log1p(-comp);
    }
    nlp = -lnp / kLn10;
    return true;
}

__global__ void __launch_bounds__(kThreads) glm_linear_kernel(LinArgs p)
{
    __shared__ double s_mu[kRows], s_d[kRows];
    __shared__ uint32_t s_flag[kRows];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t row0 = blockIdx.x * kRows;
    const uint32_t rows = p.n_snps - row0 < kRows ? p.n_snps - row0 : kRows;

    // phase 1: the per-SNP part, a wave per SNP, lane a on covariate column a
    const double scale = lane < p.n_cov ? ldexp(1.0, (int)(p.exps[lane] - 30)) : 0.0;
    for (uint32_t r = wave; r < rows; r += kThreads / 64u) {
        const size_t i = (size_t)row0 + r;
        const long long n = p.counts[4u * i], het = p.counts[4u * i + 1u], hom = p.counts[4u * i + 2u];
        const long long s = het + 2 * hom, e2 = het + 4 * hom, num = n * e2 - s * s;
        uint32_t flag = n == 0 ? 1u : (num == 0 ? 2u : 0u);
        double mu = 0.0, d = 0.0;
        if (flag == 0u) {   // (wave-uniform)
            const double nd = (double)n;
            mu = (double)s / nd;
            const double gg = (double)num / nd;
            double hh = 0.0;
            if (lane < p.n_cov) {
                const double h = ((double)p.z[i * p.ld_z + lane] - mu * (double)p.zc[i * p.ld_z + lane]) * scale;
                hh = h * h;
            }
            double sum = 0.0;
            for (uint32_t a = 0; a < p.n_cov; ++a) sum += __shfl(hh, (int)a);   // in the order a = 0, 1, ...
            d = gg - sum;
            if (d * p.max_vif < gg) flag = 3u;
        }
        if (lane == 0u) s_mu[r] = mu, s_d[r] = d, s_flag[r] = flag;
    }
    block_sync();

    // phase 2: the cells
    const uint32_t cells = rows * p.n_pheno;
    for (uint32_t cell = threadIdx.x; cell < cells; cell += kThreads) {
        const uint32_t r = cell / p.n_pheno, j = cell - r * p.n_pheno;
        const size_t i = (size_t)row0 + r;
        uint32_t flag = s_flag[r];
        double beta = NAN, se = NAN, t = NAN, pv = NAN, nlp = NAN;
        if (flag == 0u) {
            const double yy = p.yy[j];
            if (yy == 0.0) {
                flag = 4u;
            } else {
                const double mu = s_mu[r], d = s_d[r];
                const size_t at = i * p.ld_z + p.n_cov + j;
                const double b = ((double)p.z[at] - mu * (double)p.zc[at]) * ldexp(1.0, (int)(p.exps[p.n_cov + j] - 30));
                beta = b / d;
                const double s2 = (yy - (b * b) / d) / p.df;
                if (s2 <= 0.0) {
                    flag = 5u, se = 0.0, t = copysign(INFINITY, beta), pv = 0.0, nlp = INFINITY;
                } else {
                    se = sqrt(s2 / d);
                    t = beta / se;
                    if (!t_tail(t, p.df, p.ln_beta, pv, nlp)) flag = 6u, beta = se = t = pv = nlp = NAN;
                }
            }
        }
        const size_t o = i * p.ld_out + j;
        p.beta[o] = beta, p.se[o] = se, p.t[o] = t, p.p[o] = pv, p.nlp[o] = nlp;
        p.flags[o] = (uint8_t)flag;
    }
}

}  // namespace glm
}  // namespace ldx

using namespace ldx;

extern "C" int ldx_geno_snp_counts_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                                       uint32_t *counts, void *stream)
{
    const char *const who = "ldx_geno_snp_counts_dev";
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, ref); LDX_ARG_PTR(who, counts);
    LDX_ARG_REQUIRE(((uintptr_t)counts & 15u) == 0u, "%s: counts must be 16-byte aligned (a row is stored as one group)", who);
    LDX_ARG_REQUIRE(n_hap != 0u && n_hap % 2u == 0u, "%s: n_hap %u must be even and non-zero (haplotypes 2a and 2a + 1 are individual a)",
                    who, n_hap);
    if (n_hap > LDX_MAX_HAPS) {
        set_error("%s: n_hap %u > LDX_MAX_HAPS", who, n_hap);
        return LDX_E_UNSUPPORTED;
    }
    LDX_ARG_REQUIRE(n_snps != 0u, "%s: n_snps is 0", who);
    if (const int rc = plane_check(who, nullptr, n_snps, n_hap)) return rc;
    glm::snp_counts_kernel<<<n_slabs(n_snps), glm::kThreads, 0, (hipStream_t)stream>>>(
        (const uint4 *)alt, (const uint4 *)ref, keep, n_snps, n_chunks(n_hap), (uint4 *)counts);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_glm_linear_dev(const int64_t *z, const int64_t *zc, size_t ld_z, const uint32_t *counts, uint32_t n_snps,
                                  uint32_t n_ind, uint32_t n_cov, uint32_t n_pheno, const int64_t *exps, const double *yy,
                                  double max_vif, double *beta, double *se, double *t, double *p, double *neglog10_p,
                                  uint8_t *flags, size_t ld_out, void *stream)
{
    const char *const who = "ldx_glm_linear_dev";
    LDX_ARG_PTR(who, z); LDX_ARG_PTR(who, zc); LDX_ARG_PTR(who, counts); LDX_ARG_PTR(who, exps); LDX_ARG_PTR(who, yy);
    LDX_ARG_PTR(who, beta); LDX_ARG_PTR(who, se); LDX_ARG_PTR(who, t); LDX_ARG_PTR(who, p); LDX_ARG_PTR(who, neglog10_p);
    LDX_ARG_PTR(who, flags);
    LDX_ARG_REQUIRE(n_snps != 0u, "%s: n_snps is 0", who);
    LDX_ARG_REQUIRE(n_cov != 0u && n_pheno != 0u, "%s: n_cov %u and n_pheno %u must be non-zero (the intercept is a covariate)", who,
                    n_cov, n_pheno);
    LDX_ARG_REQUIRE((uint64_t)n_cov + n_pheno <= LDX_GENO_MAX_COLS, "%s: n_cov %u + n_pheno %u > LDX_GENO_MAX_COLS = %u", who, n_cov,
                    n_pheno, LDX_GENO_MAX_COLS);
    LDX_ARG_REQUIRE(ld_z >= (size_t)n_cov + n_pheno, "%s: ld_z %zu < n_cov + n_pheno %u", who, ld_z, n_cov + n_pheno);
    LDX_ARG_REQUIRE(ld_out >= n_pheno, "%s: ld_out %zu < n_pheno %u", who, ld_out, n_pheno);
    LDX_ARG_REQUIRE(n_ind > n_cov + 1u, "%s: n_ind %u leaves no degree of freedom beside %u covariates and the genotype", who, n_ind,
                    n_cov);
    LDX_ARG_REQUIRE(max_vif > 1.0, "%s: max_vif must be > 1", who);
    glm::LinArgs a{};
    a.z = (const long long *)z, a.zc = (const long long *)zc, a.ld_z = ld_z, a.counts = counts;
    a.n_snps = n_snps, a.n_cov = n_cov, a.n_pheno = n_pheno;
    a.exps = (const long long *)exps, a.yy = yy;
    a.df = (double)(n_ind - n_cov - 1u), a.max_vif = max_vif;
    int sign = 0;   // lgamma_r: std::lgamma would write the process-wide signgam
    a.ln_beta = lgamma_r(0.5 * a.df, &sign) + lgamma_r(0.5, &sign) - lgamma_r(0.5 * a.df + 0.5, &sign);
    a.beta = beta, a.se = se, a.t = t, a.p = p, a.nlp = neglog10_p, a.flags = flags, a.ld_out = ld_out;
    glm::glm_linear_kernel<<<(n_snps + glm::kRows - 1u) / glm::kRows, glm::kThreads, 0, (hipStream_t)stream>>>(a);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

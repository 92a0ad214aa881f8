// The cell fit that the two logistic scans share (logit_kernel of ldx_logit.hip, firth_kernel of ldx_firth.hip; include/ldx.h,
// "logistic association scan" and "Firth logistic association scan"): the launch shape and the LDS tile, the
// flags 1 to 4 of a cell, phase 1 of a step, the information pass on v_mfma_f64_16x16x4_f64, the 15 x 15 Cholesky with its two
// triangular solves, se and the result store, and the argument rules of the two C entries -- written once, so that the two kernels
// cannot drift apart in what the project requires them to agree on bit for bit.  Each kernel keeps its own iteration.
//   * ONE WAVE PER CELL, four cells (consecutive SNPs, one phenotype) per workgroup.  The waves of a workgroup share nothing but
//     the LDS allocation -- no barrier, no atomics: a cell's bits depend on its SNP, its phenotype and the design alone.
//   * a pass over the individuals, 64 at a time (one 16-byte chunk of the SNP's row in the tiled planes = 64 individuals):
//       phase 1, a lane per individual: the lane loads its column of the design (coalesced), forms x, eta, mu, w, r and leaves the
//                row v = (d, x) in the wave's LDS tile;
//       phase 2, sixteen K-groups of 4 individuals: I += sum_a v_a (w_a v_a)^T on v_mfma_f64_16x16x4_f64 -- A[i][k] = v_a[i],
//                B[k][j] = w_a v_a[j]; the spare 16th column carries the gradient where the kernel asks for it: B[k][15] = r_a,
//                A row 15 = 0.  Two accumulators (even and odd K-groups) are joined once at the end of the pass.
//     C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg.
//   * the 15 x 15 system of a pass: the accumulator goes through LDS to one row per lane, unused parameters become identity rows,
//     and the wave runs a Cholesky factorisation, lane i on row i, the pivot column passed through LDS; two triangular solves.
// Individuals are walked in their order; the pad individuals of the last step are zeros in v, w and r, which add nothing.
// Every sum keeps its order and its grouping (-ffp-contract=off): a change here changes the bits of both scans alike.
#pragma once

#include <math.h>

#include "ldx_fp4.h"
#include "ldx_tail.h"   // normal_tail

namespace ldx {
namespace logit {

constexpr uint32_t kWaves = 4;                 // cells of a workgroup
constexpr uint32_t kThreads = 64u * kWaves;
constexpr uint32_t kPar = 15;                  // parameters of the tile: intercept + LDX_LOGIT_MAX_COV + genotype
constexpr uint32_t kRowR = 15, kRowW = 16;     // rows of the LDS tile that hold r (gradient passes alone) and w
constexpr uint32_t kStride = 68;               // doubles per row of the tile: rows i and i + 1 start 8 banks apart
constexpr uint32_t kTile = 17u * kStride;      // doubles of a wave's tile

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
    uint32_t mode;               // Firth alone: 0 every cell; 1 the cells whose flag is 5 on entry
    uint8_t *firth;              // Firth alone
};

// what a wave holds of its cell: set by cell_setup, read by the passes.  The point -- th, the design's coefficients, and bt, the
// genotype's -- stays a local of the kernel, whose iteration moves it.
struct Cell {
    double *tile;                // the wave's LDS tile
    const uint8_t *yj;           // the phenotype's row of y
    size_t row_words;            // this lane's word of the SNP's row in the planes, at step 0
    uint32_t lane, P, steps;     // P: columns of the design = index of the genotype among the parameters
    double mu_g;                 // mean of the called genotypes
    uint32_t bit;                // of this lane's individual in a genotype word
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

// this lane's genotype of step s: x = g - mu for a called individual, 0 otherwise
__device__ __forceinline__ double geno_x(const Args &p, const Cell &c, uint32_t s)
{
    const size_t at = c.row_words + (size_t)s * kSlab * 4u;
    const GenoWords g = geno_words(p.alt[at], p.ref[at]);
    const uint32_t q = (g.q >> c.bit) & 1u, hz = (g.z >> c.bit) & 1u, ht = (g.t >> c.bit) & 1u;
    return q && s * 64u + c.lane < p.n_ind ? (double)(ht + 2u * hz) - c.mu_g : 0.0;
}

// The cell of (snp, j) and its flag: 1 not kept or never called, 2 monomorphic, 3 collinear with the design, 4 a phenotype without
// a null fit, else 0 with th = theta0 (the kernel starts bt at 0).
__device__ __forceinline__ uint32_t cell_setup(const Args &p, uint32_t snp, uint32_t j, uint32_t lane, double *tile, Cell &c,
                                               double (&th)[kPar - 1u])
{
    c.tile = tile, c.yj = p.y + (size_t)j * p.ld_design, c.lane = lane, c.P = p.n_dcol, c.steps = (p.n_ind + 63u) / 64u;
    c.row_words = (((size_t)(snp / kSlab) * p.hap_chunks) * kSlab + (snp & (kSlab - 1u))) * 4u + (lane >> 4);
    c.bit = 2u * (lane & 15u);
    const uint32_t P = c.P;
    const long long n = p.counts[4u * (size_t)snp], het = p.counts[4u * (size_t)snp + 1u], hom = p.counts[4u * (size_t)snp + 2u];
    const long long s1 = het + 2 * hom, e2 = het + 4 * hom, num = n * e2 - s1 * s1;
    const bool kept = p.keep == nullptr || p.keep[snp] != 0;
    uint32_t flag = (!kept || n == 0) ? 1u : (num == 0 ? 2u : 0u);
    c.mu_g = flag == 0u ? (double)s1 / (double)n : 0.0;

    // flag 3: d = xx - sum_c (sum_a Q_ac x_a)^2 with Q = B / sqrt N, xx from the integers as in the linear scan
    if (flag == 0u) {
        double dot[kPar - 1u];
#pragma unroll
        for (uint32_t k = 0; k < kPar - 1u; ++k) dot[k] = 0.0;
        for (uint32_t s = 0; s < c.steps; ++s) {
            const uint32_t a = s * 64u + lane;
            const double x = geno_x(p, c, s);
            if (a < p.n_ind) {
#pragma unroll
                for (uint32_t k = 0; k < kPar - 1u; ++k)
                    if (k < P) dot[k] += p.design[k * p.ld_design + a] * x;
            }
        }
        const double xx = (double)num / (double)n;
        double sum = 0.0;
#pragma unroll
        for (uint32_t k = 0; k < kPar - 1u; ++k)
            if (k < P) {
                const double h = wave_sum(dot[k]);
                sum += (h * h) / (double)p.n_ind;
            }
        const double d = xx - sum;
        if (d * p.max_vif < xx) flag = 3u;
    }
#pragma unroll
    for (uint32_t k = 0; k < kPar - 1u; ++k) th[k] = 0.0;
    if (flag == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < kPar - 1u; ++k) {
            th[k] = k < P ? p.theta0[(size_t)j * P + k] : 0.0;
            if (th[k] != th[k]) flag = 4u;
        }
    }
    return flag;
}

// phase 1 of step s, a lane per individual: the tile's rows 0 .. 14 (V: rows P + 1 .. 14 zeros, row P the genotype) and this
// individual's mu, w and r = y - mu (zeros for a pad individual)
__device__ __forceinline__ void phase1(const Args &p, const Cell &c, const double (&th)[kPar - 1u], double bt, uint32_t s, double &mu,
                                       double &w, double &r)
{
    const uint32_t lane = c.lane, P = c.P, a = s * 64u + lane;
    const bool live = a < p.n_ind;
    const double x = geno_x(p, c, s);
    double eta = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < kPar - 1u; ++k) {
        double b = 0.0;
        if (k < P) {
            b = live ? p.design[k * p.ld_design + a] : 0.0;
            eta += th[k] * b;
        }
        c.tile[k * kStride + lane] = b;
    }
    eta += bt * x;
    // rows P + 1 .. 14 hold zeros (the loop above wrote them, this line the last), row P the genotype
    c.tile[(kPar - 1u) * kStride + lane] = 0.0;
    c.tile[P * kStride + lane] = x;
    const double e = exp(-fabs(eta)), den = 1.0 + e;
    const double hi = 1.0 / den, lo = e / den;          // the larger and the smaller of mu and 1 - mu
    mu = eta >= 0.0 ? hi : lo;
    const double om = eta >= 0.0 ? lo : hi;
    const bool yes = live && c.yj[a] != 0;
    r = live ? (yes ? om : -mu) : 0.0;
    w = live ? hi * lo : 0.0;
}

// One pass over the individuals at the point (th, bt): the information in the two accumulators (even and odd K-groups), and with
// kGradient the gradient in their 16th column -- r goes to the tile's row 15 and B[k][15] = r_a; without, that column is zero.
template <bool kGradient>
__device__ __forceinline__ void information_pass(const Args &p, const Cell &c, const double (&th)[kPar - 1u], double bt, v4d &acc0,
                                                 v4d &acc1)
{
    const uint32_t lane = c.lane, ci = lane & 15u, ck = lane >> 4;
    acc0 = acc1 = v4d{0.0, 0.0, 0.0, 0.0};
    for (uint32_t s = 0; s < c.steps; ++s) {
        double mu, w, r;
        phase1(p, c, th, bt, s, mu, w, r);
        if (kGradient) c.tile[kRowR * kStride + lane] = r;
        c.tile[kRowW * kStride + lane] = w;
        wave_sync();
        // phase 2: the K-groups of this step that hold an individual
        const uint32_t left = p.n_ind - s * 64u, groups = left >= 64u ? 16u : (left + 3u) / 4u;
        for (uint32_t t = 0; t < groups; ++t) {
            const double v = c.tile[ci * kStride + 4u * t + ck];
            const double wt = c.tile[kRowW * kStride + 4u * t + ck];
            const double av = ci == 15u ? 0.0 : v, bv = ci == 15u ? (kGradient ? v : 0.0) : wt * v;
            if (t & 1u) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc1, 0, 0, 0);
            else acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc0, 0, 0, 0);
        }
        wave_sync();
    }
}

// the accumulators to one row per lane, C[row = ck + 4 reg][col = ci]: row[] is the information's row of this lane's parameter, an
// identity row for a parameter the cell does not have; returns the 16th column's entry of that row (the gradient; 0 for such a
// parameter)
__device__ __forceinline__ double rows_of_accumulator(const Cell &c, const v4d &acc0, const v4d &acc1, double (&row)[kPar])
{
    const uint32_t lane = c.lane, ci = lane & 15u, ck = lane >> 4;
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) c.tile[(ck + 4u * r) * 17u + ci] = acc0[r] + acc1[r];
    wave_sync();
    const uint32_t ri = lane < 15u ? lane : 0u;
#pragma unroll
    for (uint32_t k = 0; k < kPar; ++k) row[k] = c.tile[ri * 17u + k];
    double u = c.tile[ri * 17u + 15u];
    if (lane > c.P) {
#pragma unroll
        for (uint32_t k = 0; k < kPar; ++k) row[k] = k == lane ? 1.0 : 0.0;
        u = 0.0;
    }
    wave_sync();
    return u;
}

// Cholesky, lane i on row i: after column k, row[k] holds L[i][k] in the lanes i >= k; false where a pivot is not in (0, inf)
__device__ __forceinline__ bool cholesky_rows(const Cell &c, double (&row)[kPar])
{
    bool pd = true;
#pragma unroll
    for (uint32_t k = 0; k < kPar; ++k) {
        const double acc = __shfl(row[k], (int)k);
        if (!(acc > 0.0) || isinf(acc)) pd = false;
        const double dg = sqrt(acc);
        const double l = c.lane == k ? dg : row[k] / dg;
        row[k] = l;
        // the column goes to the other lanes through the tile (two buffers in turn: one wave_sync per column)
        double *const col = c.tile + 16u * 17u + 16u * (k & 1u);
        if (c.lane < kPar) col[c.lane] = l;
        wave_sync();
#pragma unroll
        for (uint32_t m = k + 1u; m < kPar; ++m) row[m] -= l * col[m];
    }
    return pd;
}

// se of the genotype from the factor at the last point: it is the last parameter that is coupled, so [I^-1]_PP = 1 / L_PP^2
__device__ __forceinline__ double se_of_last(const Cell &c, const double (&row)[kPar])
{
    double dgl = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < kPar; ++k)
        if (c.lane == k) dgl = row[k];
    return 1.0 / __shfl(dgl, (int)c.P);
}

// forward: L zf = u (lane k holds u[k]), zf[k] returned in lane k; dec = |zf|^2 in the order k = 0, 1, ...  L goes to the tile, a
// row per lane, for the backward solve to read its columns.
__device__ __forceinline__ double solve_forward(const Cell &c, const double (&row)[kPar], double u, double &dec)
{
    if (c.lane < kPar) {
#pragma unroll
        for (uint32_t k = 0; k < kPar; ++k) c.tile[c.lane * 17u + k] = row[k];
    }
    double zc = 0.0;
    dec = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < kPar; ++k) {
        const double t = __shfl(u / row[k], (int)k);
        if (c.lane == k) zc = t;
        u -= row[k] * t;
        dec += t * t;
    }
    wave_sync();
    return zc;
}

// backward: L^T delta = zf, delta[k] returned in lane k; lane i < k reads L[k][i] from the tile
__device__ __forceinline__ double solve_backward(const Cell &c, const double (&row)[kPar], double zc)
{
    double diag = 1.0;
#pragma unroll
    for (uint32_t k = 0; k < kPar; ++k)
        if (c.lane == k) diag = row[k];
    for (int k = (int)kPar - 1; k >= 0; --k) {
        const double d = __shfl(zc / diag, k);
        if ((int)c.lane == k) zc = d;
        if ((int)c.lane < k) zc -= c.tile[(uint32_t)k * 17u + c.lane] * d;
    }
    wave_sync();
    return zc;
}

// the seven output words of cell o, by one lane: a fit that is not finite is flag 5, every flag other than 0 is NaN
__device__ __forceinline__ void store_cell(const Args &p, size_t o, uint32_t flag, double beta, double se, uint32_t iter)
{
    double zs = NAN, pv = NAN, nlp = NAN;
    if (flag == 0u && !(se == se && beta == beta && !isinf(se) && !isinf(beta))) flag = 5u;
    if (flag == 0u) {
        zs = beta / se;
        normal_tail(zs, pv, nlp);
    } else {
        beta = se = NAN;
    }
    p.beta[o] = beta, p.se[o] = se, p.z[o] = zs, p.p[o] = pv, p.nlp[o] = nlp;
    p.flags[o] = (uint8_t)flag, p.n_iter[o] = (uint8_t)iter;
}

// The argument rules of the two C entries in their order, under the caller's name, and the kernel's arguments from them; everything
// returns before any HIP call.  The Firth entry (is_firth) has its own two rules behind the pointers; the ML entry leaves mode 0 and
// firth null.
inline int fill_args(const char *who, const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                     const uint32_t *counts, const double *design, size_t ld_design, uint32_t n_cov, const uint8_t *y,
                     const double *theta0, uint32_t n_pheno, double max_vif, double *beta, double *se, double *z, double *p,
                     double *neglog10_p, uint8_t *flags, uint8_t *n_iter, size_t ld_out, bool is_firth, uint32_t mode, uint8_t *firth,
                     Args &a)
{
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, ref); LDX_ARG_PTR(who, counts); LDX_ARG_PTR(who, design); LDX_ARG_PTR(who, y);
    LDX_ARG_PTR(who, theta0); LDX_ARG_PTR(who, beta); LDX_ARG_PTR(who, se); LDX_ARG_PTR(who, z); LDX_ARG_PTR(who, p);
    LDX_ARG_PTR(who, neglog10_p); LDX_ARG_PTR(who, flags); LDX_ARG_PTR(who, n_iter);
    if (is_firth) {
        LDX_ARG_PTR(who, firth);
        LDX_ARG_REQUIRE(mode <= 1u, "%s: mode %u is neither 0 (every cell) nor 1 (the cells flagged 5)", who, mode);
    }
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
    a = Args{};
    a.alt = (const uint32_t *)alt, a.ref = (const uint32_t *)ref, a.keep = keep, a.counts = counts;
    a.n_snps = n_snps, a.n_ind = n_ind, a.hap_chunks = n_chunks(n_hap);
    a.design = design, a.ld_design = ld_design, a.n_dcol = n_cov + 1u;
    a.y = y, a.theta0 = theta0, a.n_pheno = n_pheno, a.max_vif = max_vif;
    a.beta = beta, a.se = se, a.z = z, a.p = p, a.nlp = neglog10_p, a.flags = flags, a.n_iter = n_iter, a.ld_out = ld_out;
    a.mode = mode, a.firth = firth;
    return LDX_OK;
}

}  // namespace logit
}  // namespace ldx

// Genotype QC and table tests (include/ldx.h, "genotype QC and table tests").
//   * group_counts_kernel<NG>: the called, heterozygous and homozygous-ALT individuals of every SNP within each of up to NG groups
//     of individuals, in ONE pass over the panel's tiled planes.  A workgroup owns a slab of 128 SNPs, as snp_counts_kernel of
//     ldx_glm.hip does, and thread (row, half) walks the chunks half, half + 2, ... of its row.
//       prologue: the groups' bit words -- 16 individuals per 32-bit word on the even slots, the layout of GenoWords::q/t/z --
//                 are made from `member` in LDS: a wave takes a chunk of 64 individuals, lane = individual, one ballot per group
//                 hands the chunk's 64 membership bits to lane g, which spreads them over the chunk's four words.
//       loop:     geno_words of the row's word (the reverse product's own), then per group three AND + popcount against the
//                 group's word, an LDS broadcast read (all lanes of a wave are on the same chunk).
//       epilogue: the halves meet in LDS (the bit words' space, reused), and the slab's rows leave as consecutive 16-byte groups.
//     NG in {1, 2, 4, 8, 16, 32} is the smallest that holds n_groups: the 3 NG counters live in registers.
//   * hwe_kernel / fisher_kernel: one thread per tuple.  Both sum a unimodal distribution by its term ratio from the OBSERVED
//     term outwards (exact_tail<Ratio>: the tail rule is written once), terms and the total carried as v 2^(256 e) so that
//     neither a ratio of 10^1541 nor its inverse leaves the range.
//   * model_kernel: one thread per tuple, the five chi-square tests of `plink --model`; integers exact in int64, then fp64
//     operations rounded once each in the order written in include/ldx.h (-ffp-contract=off): ops.model_tests_host repeats
//     chisq and odds bit for bit.
#include <math.h>

#include "ldx_fp4.h"
#include "ldx_tail.h"   // normal_tail

namespace ldx {
namespace qc {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kPartStride = kSlab + 1u;   // words between two counters of the meeting buffer: g and g + 1 on adjacent banks
constexpr uint32_t kMaxWords = LDX_MAX_HAPS / 32u;   // 32-bit words of a row: 320

template <uint32_t NG>
__global__ void __launch_bounds__(kThreads) group_counts_kernel(const uint4 *alt, const uint4 *ref, const uint8_t *keep,
                                                                const uint32_t *member, uint32_t n_snps, uint32_t n_ind,
                                                                uint32_t hap_chunks, uint32_t n_groups, uint4 *counts)
{
    // the groups' words [word][NG] during the loop, the halves' counters [3 NG][kPartStride] after it
    constexpr uint32_t kWords = NG * (3u * kPartStride > kMaxWords ? 3u * kPartStride : kMaxWords);
    __shared__ __attribute__((aligned(16))) uint32_t s_buf[kWords];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t row = threadIdx.x & (kSlab - 1u), half = threadIdx.x >> 7;
    const uint32_t s = blockIdx.x * kSlab + row;

    for (uint32_t c = wave; c < hap_chunks; c += kThreads / 64u) {
        const uint32_t a = c * 64u + lane;
        const uint32_t mem = a < n_ind ? member[a] : 0u;   // pad individuals belong to no group
        unsigned long long mine = 0ull;
#pragma unroll
        for (uint32_t g = 0; g < NG; ++g) {
            const unsigned long long b = __ballot((mem >> g) & 1u);
            if (lane == g) mine = b;
        }
        if (lane < NG) {
#pragma unroll
            for (uint32_t wd = 0; wd < 4u; ++wd)
                s_buf[(c * 4u + wd) * NG + lane] = spread16((uint32_t)(mine >> (16u * wd)) & 0xFFFFu);
        }
    }
    block_sync();

    const bool kept = s < n_snps && (keep == nullptr || keep[s] != 0);
    uint32_t n[NG], het[NG], hom[NG];
#pragma unroll
    for (uint32_t g = 0; g < NG; ++g) n[g] = het[g] = hom[g] = 0u;
    if (kept) {
        // whole chunks are walked: the pad haplotypes of the last ones are zero bits in both planes, so not called
        for (uint32_t c = half; c < hap_chunks; c += 2u) {
            const size_t o = ((size_t)blockIdx.x * hap_chunks + c) * kSlab + row;
            const uint4 va = alt[o], vr = ref[o];
#pragma unroll
            for (int wd = 0; wd < 4; ++wd) {
                const GenoWords w = geno_words(word_of(va, wd), word_of(vr, wd));
                const uint32_t *const m = s_buf + (c * 4u + (uint32_t)wd) * NG;
#pragma unroll
                for (uint32_t g = 0; g < NG; ++g) {
                    const uint32_t mg = m[g];
                    n[g] += __popc(w.q & mg), het[g] += __popc(w.t & mg), hom[g] += __popc(w.z & mg);
                }
            }
        }
    }
    block_sync();   // every wave is done with the groups' words
    if (half == 1u) {
#pragma unroll
        for (uint32_t g = 0; g < NG; ++g) {
            s_buf[(0u * NG + g) * kPartStride + row] = n[g];
            s_buf[(1u * NG + g) * kPartStride + row] = het[g];
            s_buf[(2u * NG + g) * kPartStride + row] = hom[g];
        }
    }
    block_sync();
    if (half == 0u) {
#pragma unroll
        for (uint32_t g = 0; g < NG; ++g) {
            s_buf[(0u * NG + g) * kPartStride + row] += n[g];
            s_buf[(1u * NG + g) * kPartStride + row] += het[g];
            s_buf[(2u * NG + g) * kPartStride + row] += hom[g];
        }
    }
    block_sync();
    // the slab's rows [row][group] are consecutive 16-byte groups of the output
    const uint32_t row0 = blockIdx.x * kSlab;
    const uint32_t rows = n_snps - row0 < kSlab ? n_snps - row0 : kSlab;
    uint4 *const out = counts + (size_t)row0 * n_groups;
    for (uint32_t k = threadIdx.x; k < rows * n_groups; k += kThreads) {
        const uint32_t r = k / n_groups, g = k - r * n_groups;
        out[k] = uint4{s_buf[(0u * NG + g) * kPartStride + r], s_buf[(1u * NG + g) * kPartStride + r],
                       s_buf[(2u * NG + g) * kPartStride + r], 0u};
    }
}

// ---- exact tests ---------------------------------------------------------------------------------------------------------------
constexpr double kLn2x256 = 256.0 * 0.6931471805599453;
constexpr double kTie = 1.0 + 0x1p-30;   // a term is "no more probable than the observed one" up to this ratio
constexpr double kUp = 0x1p256, kDown = 0x1p-256;

// The two-sided tail of a distribution on the terms 0 .. L - 1 given by its ratios: rt(i, num, den) sets P(i + 1) / P(i) =
// num / den (both exact, non-zero) for i < L - 1.  Every term is carried relative to the observed one, io, as v 2^(256 e) with
// v in [2^-256, 2^256): the terms no more probable than it (ratio <= 1 + 2^-30) are at most about 1 and add up in a plain
// double, the total in the scaled form.  ln p = ln(tail) - ln(total); midp takes half of the observed term (which is 1) off
// the tail.  When every term is in the tail p is 1 and ln p is 0 exactly (with midp: the total stands in for the tail).
template <class Ratio>
__device__ __forceinline__ void exact_tail(const Ratio &rt, uint32_t L, uint32_t io, bool midp, double &pv, double &nlp)
{
    double S = 1.0, tail = 1.0;
    int eS = 0;
    uint32_t inc = 1u;   // terms in the tail
    auto take = [&](double v, int e) {
        if (e == eS) S += v;
        else if (e > eS) S = ldexp(S, -256 * (e - eS)) + v, eS = e;
        else S += ldexp(v, -256 * (eS - e));
        if (e < 0) {
            tail += ldexp(v, 256 * e), ++inc;
        } else if (e == 0) {
            if (v <= kTie) tail += v, ++inc;
        } else if (e == 1) {
            const double x = v * kUp;   // v < 2^256: no overflow
            if (x <= kTie) tail += x, ++inc;
        }
    };
    for (int dir = 0; dir < 2; ++dir) {
        double v = 1.0;
        int e = 0;
        const uint32_t steps = dir == 0 ? L - 1u - io : io;
        for (uint32_t k = 0; k < steps; ++k) {
            double num, den;
            if (dir == 0) rt(io + k, num, den);
            else rt(io - 1u - k, den, num);
            v = (v * num) / den;
            if (v >= kUp) v *= kDown, ++e;
            else if (v < kDown) v *= kUp, --e;
            // past the mode and below 2^-1280 of the observed term: what is left adds nothing to either sum, and is in the tail
            if (e < -4 && num < den) {
                inc += steps - k;
                break;
            }
            take(v, e);
        }
    }
    const bool all = inc == L;   // then no term passed 1 + 2^-30: eS is 0
    double t = all ? S : tail;
    if (midp) t -= 0.5;
    double lnp = log(t) - (log(S) + (double)eS * kLn2x256);
    pv = ldexp(t / S, -256 * eS);
    if (all && !midp) pv = 1.0, lnp = 0.0;
    if (pv > 1.0) pv = 1.0;
    if (lnp > 0.0) lnp = 0.0;
    nlp = lnp == 0.0 ? 0.0 : -lnp / kTailLn10;
}

// heterozygote counts k = k0, k0 + 2, ... of n individuals with nA ALT and nB REF alleles: P(k + 2) / P(k) = 4 hA hB / ((k + 2)(k + 1))
struct HweRatio {
    uint32_t nA, nB, k0;
    __device__ __forceinline__ void operator()(uint32_t i, double &num, double &den) const
    {
        const uint32_t k = k0 + 2u * i;
        num = 4.0 * (double)((nA - k) >> 1) * (double)((nB - k) >> 1);
        den = (double)(k + 2u) * (double)(k + 1u);
    }
};

// first cells x = lo, lo + 1, ... of the 2 x 2 tables with row margins r1, r2 and first column margin c1:
// P(x + 1) / P(x) = (r1 - x)(c1 - x) / ((x + 1)(r2 - c1 + x + 1))
struct FisherRatio {
    uint32_t r1, r2, c1, lo;
    __device__ __forceinline__ void operator()(uint32_t i, double &num, double &den) const
    {
        const uint32_t x = lo + i;
        num = (double)(r1 - x) * (double)(c1 - x);
        den = (double)(x + 1u) * (double)(r2 + x + 1u - c1);
    }
};

__global__ void __launch_bounds__(kThreads) hwe_kernel(size_t m, const uint32_t *n_, const uint32_t *het_, const uint32_t *hom_,
                                                       int midp, double *p, double *nlp, uint8_t *flags)
{
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= m) return;
    const uint32_t n = n_[k], het = het_[k], hom = hom_[k];
    double pv = NAN, lp = NAN;
    uint32_t flag = 0u;
    if (n > LDX_QC_MAX_N || het > n || hom > n - het) {
        flag = 3u;
    } else if (n == 0u) {
        flag = 1u;
    } else {
        const uint32_t nA = het + 2u * hom, nB = 2u * n - nA;
        if (nA == 0u || nB == 0u) {
            flag = 2u, pv = 1.0, lp = 0.0;
        } else {
            const uint32_t k0 = nA & 1u, kmax = nA < nB ? nA : nB;
            exact_tail(HweRatio{nA, nB, k0}, (kmax - k0) / 2u + 1u, (het - k0) / 2u, midp != 0, pv, lp);
        }
    }
    p[k] = pv, nlp[k] = lp, flags[k] = (uint8_t)flag;
}

__global__ void __launch_bounds__(kThreads) fisher_kernel(size_t m, const uint32_t *a_, const uint32_t *b_, const uint32_t *c_,
                                                          const uint32_t *d_, int midp, double *p, double *nlp, uint8_t *flags)
{
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= m) return;
    const uint32_t a = a_[k], b = b_[k], c = c_[k], d = d_[k];
    const uint64_t total = (uint64_t)a + b + c + d;
    double pv = NAN, lp = NAN;
    uint32_t flag = 0u;
    if (total > 2u * LDX_QC_MAX_N) {
        flag = 3u;
    } else if (total == 0u) {
        flag = 1u;
    } else {
        const uint32_t r1 = a + b, r2 = c + d, c1 = a + c, c2 = b + d;
        if (r1 == 0u || r2 == 0u || c1 == 0u || c2 == 0u) {
            flag = 2u, pv = 1.0, lp = 0.0;
        } else {
            const uint32_t lo = c1 > r2 ? c1 - r2 : 0u, hi = r1 < c1 ? r1 : c1;
            exact_tail(FisherRatio{r1, r2, c1, lo}, hi - lo + 1u, a - lo, midp != 0, pv, lp);
        }
    }
    p[k] = pv, nlp[k] = lp, flags[k] = (uint8_t)flag;
}

// ---- the five chi-square tests of --model --------------------------------------------------------------------------------------
struct ModelArgs {
    size_t m;
    const uint32_t *cn, *chet, *chom, *un, *uhet, *uhom;
    uint32_t min_cell;
    double *chisq, *p, *nlp, *odds;
    uint8_t *flags;
};

// chi-square of the 2 x 2 table [[a, b], [c, d]] with total T: T (ad - bc)^2 / ((a + b)(c + d)(a + c)(b + d)); false on a zero margin
__device__ __forceinline__ bool chisq_2x2(long long T, long long a, long long b, long long c, long long d, double &x2)
{
    const long long den = (a + b) * (c + d) * ((a + c) * (b + d));
    if (den == 0) return false;
    const long long det = a * d - b * c;
    x2 = ((double)T * (double)(det * det)) / (double)den;
    return true;
}

__device__ __forceinline__ void tail_1df(double x2, double &pv, double &lp) { normal_tail(sqrt(x2), pv, lp); }

__global__ void __launch_bounds__(kThreads) model_kernel(ModelArgs q)
{
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= q.m) return;
    const long long R = q.cn[k], r1 = q.chet[k], r2 = q.chom[k], S = q.un[k], s1 = q.uhet[k], s2 = q.uhom[k];
    double x2[5], pv[5], lp[5], odds = NAN;
    uint32_t flag[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) x2[t] = pv[t] = lp[t] = NAN, flag[t] = 0u;
    if (R + S > (long long)(LDX_MAX_HAPS / 2u) || r1 + r2 > R || s1 + s2 > S) {
#pragma unroll
        for (int t = 0; t < 5; ++t) flag[t] = 4u;
    } else if (R == 0 || S == 0) {
#pragma unroll
        for (int t = 0; t < 5; ++t) flag[t] = 1u;
    } else {
        const long long N = R + S, r0 = R - r1 - r2, s0 = S - s1 - s2;
        const long long n0 = r0 + s0, n1 = r1 + s1, n2 = r2 + s2;
        // allelic: ALT and REF alleles of the cases and of the controls
        const long long a = r1 + 2 * r2, b = 2 * R - a, c = s1 + 2 * s2, d = 2 * S - c;
        if (chisq_2x2(2 * N, a, b, c, d, x2[0])) {
            tail_1df(x2[0], pv[0], lp[0]);
            odds = (double)(a * d) / (double)(b * c);
        } else {
            flag[0] = 2u;
        }
        // trend
        {
            const long long U = N * (r1 + 2 * r2) - R * (n1 + 2 * n2);
            const long long D = N * (n1 + 4 * n2) - (n1 + 2 * n2) * (n1 + 2 * n2);
            const long long den = R * S * D;
            if (den == 0) {
                flag[1] = 2u;
            } else {
                x2[1] = ((double)N * (double)(U * U)) / (double)den;
                tail_1df(x2[1], pv[1], lp[1]);
            }
        }
        // genotypic: the 2 x 3 table, the cells in the order case 0, 1, 2, control 0, 1, 2
        {
            const long long row[2] = {R, S}, col[3] = {n0, n1, n2}, O[6] = {r0, r1, r2, s0, s1, s2};
            bool small = false;
#pragma unroll
            for (int i = 0; i < 6; ++i) small = small || O[i] < (long long)q.min_cell;
            if (n0 == 0 || n1 == 0 || n2 == 0) {
                flag[2] = 2u;
            } else if (small) {
                flag[2] = 3u;
            } else {
                double sum = 0.0;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const long long rc = row[i / 3] * col[i % 3], dev = O[i] * N - rc;
                    sum += (double)(dev * dev) / (double)(N * rc);
                }
                x2[2] = sum;
                lp[2] = (0.5 * sum) / kTailLn10;   // ln p = -chisq / 2 exactly
                pv[2] = exp(-0.5 * sum);
            }
        }
        // dominant and recessive, with respect to ALT
        if (chisq_2x2(N, r1 + r2, r0, s1 + s2, s0, x2[3])) tail_1df(x2[3], pv[3], lp[3]);
        else flag[3] = 2u;
        if (chisq_2x2(N, r2, r0 + r1, s2, s0 + s1, x2[4])) tail_1df(x2[4], pv[4], lp[4]);
        else flag[4] = 2u;
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        q.chisq[5u * k + t] = x2[t], q.p[5u * k + t] = pv[t], q.nlp[5u * k + t] = lp[t];
        q.flags[5u * k + t] = (uint8_t)flag[t];
    }
    q.odds[k] = odds;
}

static uint32_t tuple_grid(size_t m) { return (uint32_t)((m + kThreads - 1u) / kThreads); }

}  // namespace qc
}  // namespace ldx

using namespace ldx;

extern "C" int ldx_geno_group_counts_dev(const void *alt, const void *ref, uint32_t n_snps, uint32_t n_hap, const uint8_t *keep,
                                         const uint32_t *member, uint32_t n_groups, uint32_t *counts, void *stream)
{
    const char *const who = "ldx_geno_group_counts_dev";
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, ref); LDX_ARG_PTR(who, member); LDX_ARG_PTR(who, counts);
    LDX_ARG_REQUIRE(((uintptr_t)counts & 15u) == 0u, "%s: counts must be 16-byte aligned (a row is stored as one group)", who);
    LDX_ARG_REQUIRE(n_hap != 0u && n_hap % 2u == 0u, "%s: n_hap %u must be even and non-zero (haplotypes 2a and 2a + 1 are individual a)",
                    who, n_hap);
    if (n_hap > LDX_MAX_HAPS) {
        set_error("%s: n_hap %u > LDX_MAX_HAPS", who, n_hap);
        return LDX_E_UNSUPPORTED;
    }
    LDX_ARG_REQUIRE(n_snps != 0u, "%s: n_snps is 0", who);
    LDX_ARG_REQUIRE(n_groups >= 1u && n_groups <= LDX_QC_MAX_GROUPS, "%s: n_groups %u outside 1 .. LDX_QC_MAX_GROUPS = %u", who,
                    n_groups, LDX_QC_MAX_GROUPS);
    if (const int rc = plane_check(who, nullptr, n_snps, n_hap)) return rc;
    const uint32_t grid = n_slabs(n_snps), chunks = n_chunks(n_hap), n_ind = n_hap / 2u;
    const hipStream_t st = (hipStream_t)stream;
#define LDX_QC_LAUNCH(NG)                                                                                                    \
    qc::group_counts_kernel<NG><<<grid, qc::kThreads, 0, st>>>((const uint4 *)alt, (const uint4 *)ref, keep, member, n_snps, \
                                                               n_ind, chunks, n_groups, (uint4 *)counts)
    if (n_groups == 1u) LDX_QC_LAUNCH(1u);
    else if (n_groups == 2u) LDX_QC_LAUNCH(2u);
    else if (n_groups <= 4u) LDX_QC_LAUNCH(4u);
    else if (n_groups <= 8u) LDX_QC_LAUNCH(8u);
    else if (n_groups <= 16u) LDX_QC_LAUNCH(16u);
    else LDX_QC_LAUNCH(32u);
#undef LDX_QC_LAUNCH
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_hwe_exact_dev(size_t m, const uint32_t *n, const uint32_t *het, const uint32_t *hom, int midp, double *p,
                                 double *neglog10_p, uint8_t *flags, void *stream)
{
    const char *const who = "ldx_hwe_exact_dev";
    LDX_ARG_PTR(who, n); LDX_ARG_PTR(who, het); LDX_ARG_PTR(who, hom); LDX_ARG_PTR(who, p); LDX_ARG_PTR(who, neglog10_p);
    LDX_ARG_PTR(who, flags);
    LDX_ARG_REQUIRE(m != 0u && m <= (size_t)1 << 38, "%s: m %zu must lie in 1 .. 2^38", who, m);
    LDX_ARG_REQUIRE(midp == 0 || midp == 1, "%s: midp must be 0 or 1", who);
    qc::hwe_kernel<<<qc::tuple_grid(m), qc::kThreads, 0, (hipStream_t)stream>>>(m, n, het, hom, midp, p, neglog10_p, flags);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_fisher_exact_dev(size_t m, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, int midp,
                                    double *p, double *neglog10_p, uint8_t *flags, void *stream)
{
    const char *const who = "ldx_fisher_exact_dev";
    LDX_ARG_PTR(who, a); LDX_ARG_PTR(who, b); LDX_ARG_PTR(who, c); LDX_ARG_PTR(who, d); LDX_ARG_PTR(who, p);
    LDX_ARG_PTR(who, neglog10_p); LDX_ARG_PTR(who, flags);
    LDX_ARG_REQUIRE(m != 0u && m <= (size_t)1 << 38, "%s: m %zu must lie in 1 .. 2^38", who, m);
    LDX_ARG_REQUIRE(midp == 0 || midp == 1, "%s: midp must be 0 or 1", who);
    qc::fisher_kernel<<<qc::tuple_grid(m), qc::kThreads, 0, (hipStream_t)stream>>>(m, a, b, c, d, midp, p, neglog10_p, flags);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_model_tests_dev(size_t m, const uint32_t *case_n, const uint32_t *case_het, const uint32_t *case_hom,
                                   const uint32_t *ctrl_n, const uint32_t *ctrl_het, const uint32_t *ctrl_hom, uint32_t min_cell,
                                   double *chisq, double *p, double *neglog10_p, double *odds, uint8_t *flags, void *stream)
{
    const char *const who = "ldx_model_tests_dev";
    LDX_ARG_PTR(who, case_n); LDX_ARG_PTR(who, case_het); LDX_ARG_PTR(who, case_hom); LDX_ARG_PTR(who, ctrl_n);
    LDX_ARG_PTR(who, ctrl_het); LDX_ARG_PTR(who, ctrl_hom); LDX_ARG_PTR(who, chisq); LDX_ARG_PTR(who, p);
    LDX_ARG_PTR(who, neglog10_p); LDX_ARG_PTR(who, odds); LDX_ARG_PTR(who, flags);
    LDX_ARG_REQUIRE(m != 0u && m <= (size_t)1 << 38, "%s: m %zu must lie in 1 .. 2^38", who, m);
    qc::ModelArgs q{m, case_n, case_het, case_hom, ctrl_n, ctrl_het, ctrl_hom, min_cell, chisq, p, neglog10_p, odds, flags};
    qc::model_kernel<<<qc::tuple_grid(m), qc::kThreads, 0, (hipStream_t)stream>>>(q);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

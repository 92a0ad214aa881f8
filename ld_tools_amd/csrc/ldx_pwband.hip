// Pairwise-complete LD on the band (include/ldx.h, "pairwise-complete bands"): the in-window pairs i > j of ONE
// panel with the cell of ldx_ld_rect_pw_dev -- r over the haplotypes (dosage form: the individuals) called at both SNPs --
// stored in the band layout (ldx_ld_pw_band_dev), summed into LD scores (ldx_ld_pw_score_dev) or filtered into neighbour
// records (ldx_ld_pw_neighbors_dev); and the per-SNP diagonal of such a band (ldx_pw_snp_stats_dev).
//   * cell: tile_body (ldx_pwc_tile.h), the tile of pwc_kernel with both of its K loops, panel x panel.  A cell is a function
//     of the pair's integers alone, so it is the rectangle's cell at (i, j) bit for bit, whichever tile computes it.  The
//     hole-free dosage tiles read their homozygotes from the caller's table (ldx_dosage_stats_dev's hom).
//   * window: low[i] = the first j with (double)pos_i - (double)pos_j <= window, searched per SNP into the workspace
//     (band_layout_kernel's comparison).  Positions are non-decreasing, so the band kernel's per-cell predicate -- j < i and
//     pos_i - pos_j <= window -- IS low[i] <= j < i: a cell needs one table word of its row, not two positions.
//   * walk: only the lower band.  I block ti (rows [256 ti, r1), r1 = min(256 (ti + 1), n)) meets the slabs low[256 ti] / 128 ..
//     (r1 - 1) / 128: low is non-decreasing, so these cover every in-window j < i of the block.  The plan kernel writes the
//     exclusive prefix of those counts, and their total, into the workspace; tile t is (ti, tj) with prefix[ti] <= t <
//     prefix[ti + 1] (a binary search) and tj = first slab + t - prefix[ti].  The grid is fixed -- two workgroups per CU -- and a
//     workgroup strides over the tile numbers: no host read of the total.  Consecutive tile numbers, which run side by side,
//     share the 256 rows of one I block and walk its slabs; the next I block starts at most two slabs later, so the slabs are
//     shared between neighbouring blocks through the L2 as well.  Plan, tile loop, row tables, predicates, launch and argument
//     rules are ldx_band_plan.h's, shared with emband_kernel.
//   * epilogues: Store writes values[offsets[i] + j - lo[i]] under ldx_ld_band_dev's guard; Nbr appends both orientations of a
//     pair in one HitAppender call; Score adds the cell's term to its row's and its column's sum as the cells go by, in doubles
//     (integers <= 2^32, at most 256 of them: exact): a row's sum is complete when the lane has met the row's column tiles and
//     is reduced over the 32 lanes of the half-wave, a column's when the pass ends and is reduced over the two half-waves; then
//     ONE 64-bit integer atomic per row / column and wave.  A launch adds to ONE word of every SNP (Args::word); the
//     annotation words take further launches.
#include "ldx_band_plan.h"
#include "ldx_pwc_tile.h"

namespace ldx {
namespace pwband {

using namespace pwc;

enum Op : int { kStore = 0, kScore = 1, kNbr = 2 };
static_assert(kThreads == bandplan::kBandThreads, "the walk's workgroup");

struct Args {
    Side s;                    // the panel: both sides of every tile
    uint32_t nblocks;          // K-blocks of 256 haplotypes
    uint32_t n_hap;
    bandplan::Plan plan;
    const uint32_t *lo;        // store: the caller's layout
    const uint64_t *offsets;
    float *values;
    uint64_t n_cells;
    const uint8_t *annot;      // score: category masks or null
    uint32_t st;               // words per SNP: 1 + n_annot
    uint32_t word;             // the word this launch adds to: 0 = every pair, 1 + k = the other SNP carries category k
    unsigned long long *sums;
    float bound;               // neighbours: kept iff r *f32 r >= bound
    ldx_hit *hits;
    uint64_t hit_cap;
    unsigned long long *n_hits;
};

// the band's own per-tile tables, beside tile_body's: 4 480 bytes
struct BandLds : bandplan::RowTables<kTileRows> {
    uint8_t r_sel[kTileRows], c_sel[kSlab];   // score: does the row's / the column's mask select this launch's word
};

template <int kOp, bool kDosage>
struct BandEpi {
    static constexpr bool kCells = true, kReduce = kOp == kScore;
    static constexpr uint32_t kSets = Geo<kDosage>::kSets, kLast = Geo<kDosage>::kLast;
    const Args &p;
    const BandLds &bl;
    HitAppender hit;
    uint32_t ti = 0, tj = 0;                      // the tile
    double rs = 0.0, cs[4] = {0.0, 0.0, 0.0, 0.0};   // score: the lane's share of its row's sum and of its (up to) four columns' sums

    __device__ __forceinline__ void cell(uint32_t i, uint32_t j, int t, const double (&k)[kSets], double rs_x, double rs_y)
    {
        const uint32_t li = i - ti * kTileRows;
        const float c = r32_cell(k[kLast], k[0], k[1], rs_x, k[2], rs_y).r;
        const bool inside = bandplan::inside(bl, li, i, j);
        if constexpr (kOp == kStore) {
            uint64_t idx;
            if (bandplan::store_at(bl, li, j, inside, p.n_cells, idx)) p.values[idx] = c;
        } else if constexpr (kOp == kNbr) {
            const float s2 = c * c;   // ONE float32 multiply; -0.0f (degenerate) and +0.0f give 0 < bound
            hit.append_both(inside && s2 >= p.bound, i, j, c, s2);
        } else {
            // score_term as a double: an integer <= 2^32, so the sums of a tile's <= 256 terms are exact.  This launch's word
            // takes the term into row i if column j's mask selects the word, and into column j if row i's mask does
            const float s2 = c * c;
            const double x = inside ? __builtin_rint((double)s2 * 0x1p32) : 0.0;
            rs += bl.c_sel[j - tj * kSlab] ? x : 0.0;
            cs[t] += bl.r_sel[li] ? x : 0.0;
        }
    }

    // the row's sum over the 32 lanes of its half-wave, then ONE 64-bit integer atomic (rs != 0: a cell inside, so i < n)
    __device__ __forceinline__ void row_done(uint32_t i)
    {
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) rs += __shfl_xor(rs, o);
        if ((threadIdx.x & 31u) == 0u && rs != 0.0) atomicAdd(p.sums + (size_t)i * p.st + p.word, (unsigned long long)rs);
        rs = 0.0;
        // (the columns' sums are made HERE, row by row: the atomic's branch ends a block, and the compiler would sink the four
        // chains of additions into the pass's last block -- and keep every cell's term in a register until then)
#pragma unroll
        for (int t = 0; t < 4; ++t) asm volatile("" : "+v"(cs[t]));
    }
    // the columns' sums over the two half-waves (the lane's 16 rows of every row tile are in), one atomic each
    template <uint32_t kT>
    __device__ __forceinline__ void pass_done(uint32_t j0)
    {
#pragma unroll
        for (uint32_t t = 0; t < kT; ++t) {
            const double both = cs[t] + __shfl_xor(cs[t], 32);
            if ((threadIdx.x & 32u) == 0u && both != 0.0)
                atomicAdd(p.sums + (size_t)(j0 + 32u * t) * p.st + p.word, (unsigned long long)both);
            cs[t] = 0.0;
        }
    }
};

template <int kOp, bool kDosage>
__global__ void __launch_bounds__(kThreads, 2) pwband_kernel(Args p)
{
    __shared__ Smem sm;
    __shared__ BandLds bl;
    const uint32_t n = p.s.n;
    BandEpi<kOp, kDosage> epi{p, bl, HitAppender{p.hits, p.hit_cap, p.n_hits, threadIdx.x & 63u}};
    bandplan::walk<kTileRows>(p.plan, n, [&](uint32_t ti, uint32_t tj, uint32_t tid) {
        bandplan::fill_rows<kOp == kStore>(bl, p.plan, p.lo, p.offsets, n, ti, tid);
        if constexpr (kOp == kScore) {   // bit c of (mask << 1) | 1 selects word c
            const uint32_t x_r = ti * kTileRows + tid, x_c = tj * kSlab + tid;
            bl.r_sel[tid] = (uint8_t)(((((p.annot && x_r < n) ? (uint32_t)p.annot[x_r] << 1 : 0u) | 1u) >> p.word) & 1u);
            if (tid < kSlab) bl.c_sel[tid] = (uint8_t)(((((p.annot && x_c < n) ? (uint32_t)p.annot[x_c] << 1 : 0u) | 1u) >> p.word) & 1u);
        }
        epi.ti = ti, epi.tj = tj;
        tile_body<kDosage, true>(sm, p.s, p.s, p.nblocks, p.n_hap, ti, tj, tid, epi);   // (its first barrier publishes the tables)
    });
    if constexpr (kOp == kNbr) epi.hit.close();   // what is left of the wave's last batch
}

// diag / live of one SNP over its OWN called set: one wavefront per row.  Haplotype form: a r > 0, from the tables.  Dosage
// form: the individuals with both codes called -- N of them, A = the sum of their dosages, HA homozygous ALT -- from both
// planes (called_sums, ldx_band_plan.h); live iff N (A + 2 HA) - A^2 > 0.
__global__ void __launch_bounds__(256) snp_stats_kernel(const uint32_t *__restrict__ alt, const uint32_t *__restrict__ ref,
                                                        const uint32_t *__restrict__ acnt, const uint32_t *__restrict__ rcnt,
                                                        uint32_t n_snps, uint32_t nchunks, bool dosage, float *__restrict__ diag,
                                                        uint8_t *__restrict__ live)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= n_snps) return;   // wave-uniform
    bool lv;
    if (!dosage) {
        lv = acnt[row] != 0u && rcnt[row] != 0u;
    } else {
        const bandplan::CalledSums c = bandplan::called_sums<true>(alt, ref, row, nchunks, lane);
        lv = (uint64_t)c.N * (c.A + 2u * (uint64_t)c.HA) > (uint64_t)c.A * c.A;   // (Cauchy-Schwarz: never below)
    }
    if (lane != 0u) return;
    diag[row] = lv ? 1.0f : -0.0f;
    if (live) live[row] = lv ? 1u : 0u;
}

// every SNP's own term WRITES its words: the call needs no memset of `sums` (score_init_kernel's rule, ldx_mfma.hip)
__global__ void score_init_kernel(const float *__restrict__ diag, const uint8_t *__restrict__ annot, uint32_t st, uint32_t n_snps,
                                  uint64_t *__restrict__ sums)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_snps) return;
    const uint64_t t = score_term(diag[i]);
    const uint32_t m = annot ? ((uint32_t)annot[i] << 1) | 1u : 1u;   // bit c selects word c
    for (uint32_t c = 0; c < st; ++c) sums[(size_t)i * st + c] = ((m >> c) & 1u) ? t : 0u;
}

// low, the plan, then the band (bandplan::launch); the tile bound is I blocks x slabs
template <int kOp>
static int launch(Args &p, bool dosage, const int64_t *positions, int64_t window, void *workspace, hipStream_t s)
{
    const uint32_t n = p.s.n;
    const uint64_t tiles = (uint64_t)((n + kTileRows - 1u) / kTileRows) * n_slabs(n);
    auto go = [&](const bandplan::Plan &plan, uint32_t grid) {
        p.plan = plan;
        // (Score: one pass over the band per word -- the sums of one word are what fits the registers beside the accumulators --
        // so K annotation categories cost 1 + K passes)
        for (uint32_t word = 0; word < (kOp == kScore ? p.st : 1u); ++word) {
            p.word = word;
            if (dosage) pwband_kernel<kOp, true><<<grid, kThreads, 0, s>>>(p);
            else pwband_kernel<kOp, false><<<grid, kThreads, 0, s>>>(p);
            LDX_HIP(hipGetLastError());
        }
        return (int)LDX_OK;
    };
    return bandplan::launch<kTileRows>(positions, n, window, workspace, s, tiles, go);
}

}  // namespace pwband
}  // namespace ldx

using namespace ldx;

// the panel's pointers and shape rules, in rect_args_ok's order; everything returns before any HIP call
#define LDX_PWB_PANEL(who)                                                                     \
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, ref); LDX_ARG_PTR(who, acnt); LDX_ARG_PTR(who, rcnt); \
    LDX_ARG_REQUIRE(hom != nullptr || !dosage, "%s: hom is a null pointer (the dosage form reads ldx_dosage_stats_dev's table)", who)

// only the dosage form pairs haplotypes
static const char *odd_reason(bool dosage)
{
    return dosage ? "dosage pairs haplotypes 2k and 2k + 1 into individuals" : nullptr;
}

static pwband::Args make_args(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, const uint32_t *hom,
                              uint32_t n_snps, uint32_t n_hap)
{
    pwband::Args p{};
    p.s = pwc::Side{(const uint4 *)alt, (const uint4 *)ref, acnt, rcnt, n_snps, hom};
    p.nblocks = n_chunks(n_hap) / 2u;
    p.n_hap = n_hap;
    p.st = 1u;
    return p;
}

extern "C" size_t ldx_ld_pw_band_workspace_bytes(uint32_t n_snps) { return bandplan::workspace_bytes<pwc::kTileRows>(n_snps); }

extern "C" int ldx_pw_snp_stats_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, uint32_t n_snps,
                                    uint32_t n_hap, int dosage, float *diag, uint8_t *live, void *stream)
{
    const char *const who = "ldx_pw_snp_stats_dev";
    LDX_ARG_PTR(who, alt); LDX_ARG_PTR(who, ref); LDX_ARG_PTR(who, acnt); LDX_ARG_PTR(who, rcnt);
    LDX_ARG_PTR(who, diag);
    if (const int rc = bandplan::shape_ok(who, n_snps, n_hap, odd_reason(dosage != 0))) return rc;
    pwband::snp_stats_kernel<<<(n_snps + 3u) / 4u, 256, 0, (hipStream_t)stream>>>(
        (const uint32_t *)alt, (const uint32_t *)ref, acnt, rcnt, n_snps, n_chunks(n_hap), dosage != 0, diag, live);
    LDX_HIP(hipGetLastError());
    return LDX_OK;
}

extern "C" int ldx_ld_pw_band_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, const uint32_t *hom,
                                  uint32_t n_snps, uint32_t n_hap, int dosage, const int64_t *positions, int64_t window,
                                  const uint32_t *lo, const uint64_t *offsets, float *values, uint64_t n_cells, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    const char *const who = "ldx_ld_pw_band_dev";
    LDX_PWB_PANEL(who);
    LDX_ARG_PTR(who, lo);
    LDX_ARG_PTR(who, offsets);
    LDX_ARG_REQUIRE(values != nullptr || n_cells == 0u, "%s: values is a null pointer but n_cells is %llu", who,
                    (unsigned long long)n_cells);
    if (const int rc = bandplan::band_args_ok<pwc::kTileRows>(who, n_snps, n_hap, odd_reason(dosage != 0), positions, window,
                                                              workspace, workspace_bytes))
        return rc;
    if (n_cells == 0u) return LDX_OK;   // no pair in any window: nothing to write
    pwband::Args p = make_args(alt, ref, acnt, rcnt, hom, n_snps, n_hap);
    p.lo = lo, p.offsets = offsets, p.values = values, p.n_cells = n_cells;
    return pwband::launch<pwband::kStore>(p, dosage != 0, positions, window, workspace, (hipStream_t)stream);
}

extern "C" int ldx_ld_pw_score_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt, const uint32_t *hom,
                                   uint32_t n_snps, uint32_t n_hap, int dosage, const int64_t *positions, int64_t window,
                                   const uint8_t *annot, uint32_t n_annot, const float *diag, uint64_t *sums, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    const char *const who = "ldx_ld_pw_score_dev";
    LDX_PWB_PANEL(who);
    LDX_ARG_PTR(who, diag);
    LDX_ARG_PTR(who, sums);
    LDX_ARG_REQUIRE(n_annot <= 8u, "%s: n_annot %u > 8", who, n_annot);
    LDX_ARG_REQUIRE(annot != nullptr || n_annot == 0u, "%s: annot is a null pointer but n_annot is %u", who, n_annot);
    if (const int rc = bandplan::band_args_ok<pwc::kTileRows>(who, n_snps, n_hap, odd_reason(dosage != 0), positions, window,
                                                              workspace, workspace_bytes))
        return rc;
    pwband::Args p = make_args(alt, ref, acnt, rcnt, hom, n_snps, n_hap);
    p.annot = n_annot ? annot : nullptr, p.st = 1u + n_annot, p.sums = (unsigned long long *)sums;
    pwband::score_init_kernel<<<(n_snps + 255u) / 256u, 256, 0, (hipStream_t)stream>>>(diag, p.annot, p.st, n_snps, sums);
    LDX_HIP(hipGetLastError());
    return pwband::launch<pwband::kScore>(p, dosage != 0, positions, window, workspace, (hipStream_t)stream);
}

extern "C" int ldx_ld_pw_neighbors_dev(const void *alt, const void *ref, const uint32_t *acnt, const uint32_t *rcnt,
                                       const uint32_t *hom, uint32_t n_snps, uint32_t n_hap, int dosage, const int64_t *positions,
                                       int64_t window, float r2_bound, ldx_hit *hits, uint64_t hit_cap, uint64_t *n_hits,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    const char *const who = "ldx_ld_pw_neighbors_dev";
    LDX_PWB_PANEL(who);
    if (const int rc = hit_args_ok(who, r2_bound, hits, hit_cap, n_hits)) return rc;
    if (const int rc = bandplan::band_args_ok<pwc::kTileRows>(who, n_snps, n_hap, odd_reason(dosage != 0), positions, window,
                                                              workspace, workspace_bytes))
        return rc;
    pwband::Args p = make_args(alt, ref, acnt, rcnt, hom, n_snps, n_hap);
    p.bound = r2_bound, p.hits = hits, p.hit_cap = hit_cap, p.n_hits = (unsigned long long *)n_hits;
    LDX_HIP(hipMemsetAsync(n_hits, 0, sizeof(uint64_t), (hipStream_t)stream));   // the slot counter starts at 0
    return pwband::launch<pwband::kNbr>(p, dosage != 0, positions, window, workspace, (hipStream_t)stream);
}

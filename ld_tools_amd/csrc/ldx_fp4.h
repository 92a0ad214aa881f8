// What the FP4 counting kernels share (triangle_mfma_kernel of ldx_mfma.hip, rect_kernel of ldx_rect.hip, em_rect_kernel of
// ldx_em.hip, pwc_kernel of ldx_pwc.hip and pwband_kernel of ldx_pwband.hip through ldx_pwc_tile.h): the operand encoding -- the exactness argument of the whole library, written once -- and the rectangle walk.
#pragma once

#include "ldx_common.h"

namespace ldx {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// ---- FP4 (E2M1) operands for v_mfma_f32_32x32x64_f8f6f4: twice the int8 rate (64 haplotypes per 32 cycles) -----------
// A nibble with ONE bit at position p in {0, 1, 2} reads 0.5 / 1 / 2 (position 3 is the sign: -0), so a haplotype bit
// becomes the nibble of its own 4-bit group with NO data movement -- one AND per eight haplotypes -- as long as the
// other operand carries the bit at position 2 - p: every co-occurrence multiplies to 1 and the fp32 accumulators hold
// n11 exactly (< 2^24).  The K order inside an instruction is free (both operands use the same one): register v of an
// operand holds haplotypes {v, v + 4, ..., v + 28} of the 32-bit word for v < 2, and {2, 6, ...} / {3, 7, ...} of the
// word shifted down by two for v = 2, 3.  5 VALU per 32 haplotypes on the A side, 6 on the B side (the int8 forms of
// ldx_mfma.hip: 14 and 24).  tools/probes/fp4rate.hip checks the exactness and the rate on the device.
__device__ __forceinline__ v4i expand32_a4(uint32_t w)
{
    const uint32_t t = w >> 2;
    return v4i{(int)(w & 0x11111111u), (int)(w & 0x22222222u), (int)(t & 0x11111111u), (int)(t & 0x22222222u)};   // 0.5, 1, 0.5, 1
}
__device__ __forceinline__ v4i expand32_b4(uint32_t w)
{
    const uint32_t t = w >> 2;
    return v4i{(int)((w << 2) & 0x44444444u), (int)(w & 0x22222222u), (int)((w) & 0x44444444u), (int)(t & 0x22222222u)};   // 2, 1, 2, 1
}

// Genotype dosage ("Dosage LD"): the A operand stays the haplotype bit (0.5 / 1 / 0.5 / 1), the B operand
// carries, at the place of haplotype h, the ALT dosage g in {0, 1, 2} of the INDIVIDUAL of h -- haplotypes 2k and 2k + 1, two
// adjacent bits of one word -- times the factor that makes the product g: 2 g against A's 0.5 (E2M1 0100 = 2, 0110 = 4), g
// against A's 1 (0010 = 1, 0100 = 2).  With s = w >> 1 the even bits of o = w | s, n = w & s, x = w ^ s say g >= 1, g == 2,
// g == 1; every mask below picks a bit that comes from an even position, so o, n and x need no mask of their own.  The
// accumulators then hold S = sum over individuals of g_i g_j exactly (every product <= 2, S <= 2 n_hap < 2^24).  18 VALU per
// 32 haplotypes where expand32_b4 takes 6; MFMA count, A side and LDS image are the haplotype kernel's.
__device__ __forceinline__ v4i expand32_b4_dosage(uint32_t w)
{
    const uint32_t s = w >> 1, o = w | s, n = w & s, x = w ^ s;
    return v4i{(int)(((o << 2) & 0x44444444u) | ((n << 1) & 0x22222222u)),    // individual 2q:     2 g
               (int)(((x << 1) & 0x22222222u) | ((n << 2) & 0x44444444u)),    //                      g
               (int)((o & 0x44444444u) | ((n >> 1) & 0x22222222u)),           // individual 2q + 1: 2 g
               (int)(((x >> 1) & 0x22222222u) | (n & 0x44444444u))};          //                      g
}

// Pairwise-complete dosage LD (ldx_pwc.hip; DESIGN.md, "Pairwise-complete LD"): counts over the individuals CALLED at both SNPs
// need per-INDIVIDUAL operands.  An individual's bit -- called q, heterozygous t, homozygous ALT n -- lives on its EVEN
// haplotype slot, which is registers 0 and 2 of an operand (slots 4k and 4k + 2 of the word); registers 1 and 3, the odd
// slots, are then free and carry a second per-individual bit that only meets a partner parked on the odd slots too.
//   A side (0.5 / 1):  expand32_a4_dosage  g / 2 on the even slot (het 0001 = 0.5, hom 0010 = 1);
//                      even_a4(z)          0.5 where z has the individual's bit (the EM tile's het_a4, as four registers);
//                      odd_a4(z)           1 on the ODD slot of the individual (0010), nothing on the even one.
//   B side (2 / 4 / 1): expand32_b4_dosage  2 g on the even slot (and g on the odd one, which the three A operands above
//                                          multiply by 0);
//                      expand32_b4_called_hom(q, n)  2 on the even slot where q (0100), 1 on the odd slot where n (0010).
// Every product is g_x g_y, g, or 1 -- an integer <= 4 -- and every sum at most 4 N <= 20 480 < 2^24: exact in any order.  The
// words that enter are made by ind_called and by masking ALT with both slots of it, so that a half-missing genotype is missing.
__device__ __forceinline__ uint32_t ind_called(uint32_t alt, uint32_t ref)
{
    const uint32_t c = alt | ref;
    return c & (c >> 1) & 0x55555555u;
}
// The genotype words of one 32-bit word of a panel row (16 individuals, each on the even slot of its two haplotypes): q called,
// z homozygous ALT, t heterozygous.  The reverse genotype product (ldx_geno.hip) and the per-SNP genotype counts (ldx_glm.hip)
// both take their words from here, so the counts agree with the products by construction.
struct GenoWords {
    uint32_t q, z, t;
};
__device__ __forceinline__ GenoWords geno_words(uint32_t wa, uint32_t wr)
{
    const uint32_t q = ind_called(wa, wr);
    const uint32_t a = wa & (q | (q << 1));   // a half-missing genotype is missing
    return GenoWords{q, a & (a >> 1) & 0x55555555u, (a ^ (a >> 1)) & q};
}
// 16 bits to the even slots of a word: the bits of 16 individuals in the layout of GenoWords::q/t/z
__device__ __forceinline__ uint32_t spread16(uint32_t x)
{
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    return (x | (x << 1)) & 0x55555555u;
}
__device__ __forceinline__ v4i even_a4(uint32_t z)
{
    return v4i{(int)(z & 0x11111111u), 0, (int)((z >> 2) & 0x11111111u), 0};   // 0.5, -, 0.5, -
}
__device__ __forceinline__ v4i odd_a4(uint32_t z)
{
    return v4i{0, (int)((z << 1) & 0x22222222u), 0, (int)((z >> 1) & 0x22222222u)};   // -, 1, -, 1
}
__device__ __forceinline__ v4i expand32_a4_dosage(uint32_t w)
{
    const uint32_t s = w >> 1, n = w & s, x = w ^ s;   // every mask picks a bit that comes from an even position
    return v4i{(int)((x & 0x11111111u) | ((n << 1) & 0x22222222u)), 0,           // individual 2q:     g / 2
               (int)(((x >> 2) & 0x11111111u) | ((n >> 1) & 0x22222222u)), 0};   // individual 2q + 1: g / 2
}
__device__ __forceinline__ v4i expand32_b4_called_hom(uint32_t q, uint32_t n)
{
    return v4i{(int)((q << 2) & 0x44444444u), (int)((n << 1) & 0x22222222u),     // individual 2q:     2 q, n
               (int)(q & 0x44444444u), (int)((n >> 1) & 0x22222222u)};           // individual 2q + 1: 2 q, n
}

// word w of the 16 bytes (128 haplotypes) a lane holds of one row and chunk
__device__ __forceinline__ uint32_t word_of(const uint4 &v, int w)
{
    return w == 0 ? v.x : (w == 1 ? v.y : (w == 2 ? v.z : v.w));
}

// The rectangle walk: workgroup b -> (I block ti, J slab tj) of Ti x Tj.  Bands of kBandTiles I blocks; inside a band the J
// slab is the slow index, so that consecutive workgroups (which the dispatcher deals round-robin to the XCDs) share one J slab
// and each XCD keeps returning to the same two I blocks of the band while the J slabs stream past.  kBandTiles is the
// kernel's: 4096 rows' worth of its I blocks ("Rectangular LD", has the reasoning and the budget).
template <uint32_t kBandTiles>
__device__ __forceinline__ void tile_of(uint32_t b, uint32_t Ti, uint32_t Tj, uint32_t &ti, uint32_t &tj)
{
    const uint32_t per_band = kBandTiles * Tj;
    const uint32_t band = b / per_band, rem = b - band * per_band;
    const uint32_t left = Ti - band * kBandTiles, gi = left < kBandTiles ? left : kBandTiles;
    tj = rem / gi;
    ti = band * kBandTiles + (rem - tj * gi);
}

}  // namespace ldx

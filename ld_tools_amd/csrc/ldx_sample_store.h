// The layout of the transposed (individual-major) store that ldx_sample_planes_dev writes (include/ldx.h, "sample relatedness"):
// shared by its writer and the counting kernel (ldx_king.hip) and by the forward genotype product (ldx_geno.hip).
#pragma once

#include "ldx_common.h"

namespace ldx {
namespace king {

__host__ __device__ inline uint32_t pad_ind(uint32_t n_ind) { return n_slabs(n_ind) * kSlab; }
__host__ __device__ inline uint32_t snp_chunks(uint32_t n_snps) { return (uint32_t)(((uint64_t)n_snps + 255u) / 256u * 2u); }
__host__ __device__ inline size_t plane_vecs(uint32_t n_ind, uint32_t n_snps)
{
    return (size_t)n_slabs(n_ind) * snp_chunks(n_snps) * kSlab;
}

}  // namespace king
}  // namespace ldx

// tile_kernel_defs.h -- what the tile kernels of chol_kernels.hip and sinv_kernels.hip share: the vector and address-space
// types of their global accesses and the staging constants of the small-batch product (k_tile_gemm_nt_small, k_sinv_gemm).
// Device translation units only.
#pragma once
#include "ba_kernels.h"

namespace apex {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int NB = kNB;

typedef double __attribute__((address_space(1)))* GlobalF64;
typedef const double __attribute__((address_space(1)))* GlobalCF64;
typedef double f64x2_t __attribute__((ext_vector_type(2)));
typedef const f64x2_t __attribute__((address_space(1)))* GlobalCF64x2;

constexpr int KS = 48;            // K chunk of the small-batch kernel
constexpr int PS = KS + 2;        // LDS pitch: 50 doubles = 100 dwords, rows shift by 36 banks -> conflict-free b64 reads

}  // namespace apex

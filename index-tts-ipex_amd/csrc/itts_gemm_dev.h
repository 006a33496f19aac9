// Device helpers shared by the shift-GEMM kernels (gemm_simple / gemm_mfma / gemm_glds / gemm_p8): the reflect-padding row
// index, the LDS-DMA wrapper and the XCD-aware workgroup order.
#pragma once
#include "itts_common.h"

namespace itts {

// torch 'reflect' padding (no edge repeat); valid for |overhang| < T
__device__ __forceinline__ int reflect_idx(int t, int T) {
  if (t < 0) t = -t;
  if (t >= T) t = 2 * (T - 1) - t;
  return t;
}

// 16 bytes per lane global -> LDS (global_load_lds_dwordx4): no VGPR staging, the LDS address is wave-uniform base + lane * 16
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// XCD-aware, bijective remap of a 1-D grid: workgroup `orig` of `nwg` runs on XCD orig & 7, so consecutive LOGICAL ids (= the
// column tiles of one row tile) are handed to workgroups of one XCD and their A rows hit that L2
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = orig & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
}

}  // namespace itts

// The pieces of the bf16 decode GEMV that more than one kernel is built from, ONE definition: gemv_bf16_kernel and
// gemv_wave_kernel (decode_gemv.hip) and the projection part of qkv_attn_fused_kernel (decode_fused.hip), whose published
// q / k / v must equal what gemv_bf16_kernel stores (tests/test_gpu_fullsize.py::test_fused_qkv_attention_launch_equals_two_launches_bf16).
// Moving text between this header and a kernel must not change the kernel by one instruction.
#pragma once
#include "itts_decode.h"
#include "itts_wave_dev.h"
#include "decode_pinned.h"

namespace itts {

// phase stamps of the decode GEMVs (tools/ubench_gemv2.hip); nothing in a product build
#ifdef ITTS_GEMV_STAMPS
#define GEMV_STAMP(i)                                                                   \
  {                                                                                     \
    unsigned long long t_;                                                              \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
    if (threadIdx.x == 0 && g.stamp) g.stamp[(size_t)blockIdx.x * 8 + (i)] = t_;        \
  }
#else
#define GEMV_STAMP(i)
#endif

// ---- pieces shared by gemv_bf16_kernel, fused_gemv_part (qkv_attn_fused_kernel) and, gemv_reduce apart, gemv_wave_kernel ----
// one 16-byte weight fragment (8 bf16) times 8 activations held as bf16 pairs (XQ: u32x4 or uint32_t[4]): 4 x v_dot2c
template <typename XQ>
__device__ __forceinline__ float gemv_dot8(const u32x4& w, const XQ& xq, float acc) {
#pragma unroll
  for (int e = 0; e < 4; ++e) acc = half_dot2(w[e], xq[e], acc);
  return acc;
}
// wave reduction of every (row, batch) sum, then one lane per output: lane l < RPW * NB keeps (row l / NB, batch l % NB)
template <int RPW, int NB>
__device__ __forceinline__ float gemv_reduce(const float (&acc)[RPW][NB], int lane) {
  float mine = 0.f;
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float t = wave_sum_rl(acc[r][b]);
      mine = lane == r * NB + b ? t : mine;
    }
  return mine;
}
// the output value: fp8 row scale (1 for bf16 weights), bias, activation
__device__ __forceinline__ float gemv_out(const GemvArgs& g, float mine, float spre, float bpre) {
  const float v = mine * spre + (g.bias ? bpre : 0.f);
  return g.act == ACT_GELU_NEW ? gelu_new_rn(v) : act_apply(g.act, v);
}

// 8 bf16 weights of row n at column k, read exactly once per step: non-temporal (gemv_bf16_kernel, fused_gemv_part)
__device__ __forceinline__ u32x4 gemv_load_w(const bf16_t* __restrict__ W, int n, int K, int k) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(W + (size_t)n * K + k));
}

}  // namespace itts

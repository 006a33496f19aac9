// The per-key arithmetic of the single-query cache attention, ONE definition for the three kernels that must agree bit for bit:
// decode_attn2_kernel (decode_attn.hip) and the attention part of qkv_attn_fused_kernel (decode_fused.hip), the launch path, and phase P2 of
// decode_engine_kernel (decode_engine.hip) - tests/test_gpu_engine_persistent.py and tests/test_gpu_fullsize.py compare them.
// Every kernel keeps its own skeleton (shared memory, the order of its loads, how it obtains this step's q / k / v, its waits
// and stamps, where the result goes) and calls these through a one-line lambda of its own: that is the form in which the three
// kernels stay instruction-identical to their hand-written text (the window softmax and the merges are
// still written out per kernel, section 7 says why).
//
// Thread <-> key mapping: LPK lanes share one key row (VEC dims each).  KV is the register fragment of one row (CacheVec<> or
// V8<>: get(i)).
#pragma once
#include "itts_wave_dev.h"

namespace itts {

// the register fragment of one K/V cache row as LPK lanes hold it (VEC dims each): decode_attn2_kernel (decode_attn.hip) and the
// attention part of qkv_attn_fused_kernel (decode_fused.hip)
template <typename TC> struct CacheVec;
template <> struct CacheVec<bf16_t> {
  static constexpr int VEC = 8, LPK = 8;
  uint4 raw;
#ifdef ITTS_KV_PLAIN_LOADS
  __device__ __forceinline__ void load(const bf16_t* p) { raw = *reinterpret_cast<const uint4*>(p); }
#else
  // the cache is read once per step and never again before it has left every cache: nontemporal (streaming) loads
  __device__ __forceinline__ void load(const bf16_t* p) {
    const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    raw = make_uint4(t[0], t[1], t[2], t[3]);
  }
#endif
  __device__ __forceinline__ float get(int i) const {
    const uint32_t w = (&raw.x)[i >> 1];
    return (i & 1) ? half_hi(w) : half_lo(w);
  }
};
// the opt-in e4m3 cache (decode_attn2_kernel only): the thread <-> key mapping of the 16-bit cache - 8 lanes per key row, 8 dims
// each, one nontemporal 8-byte load per lane - so SLOTS, the blind rows, the register window, the stream step and the DPP
// summation order are the 16-bit form's, and the kernel computes, operation for operation, what the 16-bit form computes on a
// cache holding the same values (tests/test_gpu_decode_attn_fp8.py)
template <> struct CacheVec<fp8_t> {
  static constexpr int VEC = 8, LPK = 8;
  u32x2 raw;
  __device__ __forceinline__ void load(const fp8_t* p) { raw = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p)); }
  __device__ __forceinline__ float get(int i) const { return fp8_get(raw[i >> 2], i & 3); }
};
template <> struct CacheVec<float> {
  static constexpr int VEC = 4, LPK = 16;
  float4 raw;
  __device__ __forceinline__ void load(const float* p) { raw = *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ float get(int i) const { return (&raw.x)[i]; }
};

// score of one key row for this slot (the LPK lanes of the key hold VEC dims each; DPP sums them: quad swaps, half-row mirror, row
// mirror - no LDS crossbar trips)
template <int LPK, int VEC, typename KV>
__device__ __forceinline__ float attn_score(const float (&qr)[VEC], const KV& kk) {
  float sc = 0.f;
#pragma unroll
  for (int i = 0; i < VEC; ++i) sc = fmaf(qr[i], kk.get(i), sc);
  sc = dpp_add<0xB1>(sc);
  sc = dpp_add<0x4E>(sc);
  sc = dpp_add<0x141>(sc);
  if (LPK == 16) sc = dpp_add<0x140>(sc);
  return sc;
}

// online update for a row beyond the window (ok: inside the sequence and not the appended row)
template <int LPK, int VEC, typename KV>
__device__ __forceinline__ void attn_consume(float& m, float& l, float (&acc)[VEC], const float (&qr)[VEC], const KV& kk, const KV& vv,
                                             bool ok) {
  float sc = attn_score<LPK>(qr, kk);
  sc = ok ? sc : -INFINITY;  // also discards whatever an out-of-range row produced
  const float mn = fmaxf(m, sc);
  const float corr = mn > -INFINITY ? __expf(m - mn) : 1.f;
  const float p = ok ? __expf(sc - mn) : 0.f;
  l = fmaf(l, corr, p);  // contraction pinned: same operation in every build of this loop (decode_pinned.h)
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = fmaf(p, ok ? vv.get(i) : 0.f, acc[i] * corr);
  m = mn;
}

}  // namespace itts

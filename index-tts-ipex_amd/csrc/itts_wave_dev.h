// Wave-level device helpers shared by kernels that must produce the same bits as each other: the launch path's decode GEMVs
// and attention (decode_gemv.hip, decode_attn.hip, decode_fused.hip) and the persistent decode engine (decode_engine.hip) reduce with the same tree, the same slot
// butterflies (wave_bfly_max / wave_bfly_sum: decode_attn2_kernel, qkv_attn_fused_kernel, the engine's attention phase) and pack
// with the same rounding because both include this file; the single-beam sampler (decode_sampler.hip) and the beam kernels (beam.hip)
// share the top-k primitives (order_key, hist_add_wave).
#pragma once
#include "itts_common.h"

namespace itts {

// 8 weights (or 8 halves of one K/V cache row) of a lane, read exactly once per step: non-temporal 16-byte loads
// (MI355X_MICROARCH "nt-weights")
template <typename TW> struct V8;
template <> struct V8<bf16_t> {
  u32x4 raw;
  __device__ __forceinline__ void load(const bf16_t* p) { raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }
  __device__ __forceinline__ float get(int i) const {
    const uint32_t w = raw[i >> 1];
    return (i & 1) ? half_hi(w) : half_lo(w);
  }
};
template <> struct V8<float> {
  f32x4 a, b;
  __device__ __forceinline__ void load(const float* p) {
    a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    b = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + 4));
  }
  __device__ __forceinline__ float get(int i) const { return i < 4 ? a[i] : b[i - 4]; }
};

template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// full-wave sum, result uniform in every lane: DPP inside the 16-lane rows (quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror), then one v_readlane per row - no ds_bpermute (an LDS-crossbar round trip with an lgkmcnt
// wait) on the dependent chain
__device__ __forceinline__ float wave_sum_rl(float v) {
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x141>(v);
  v = dpp_add<0x140>(v);
  const int iv = __float_as_int(v);
  const float a = __int_as_float(__builtin_amdgcn_readlane(iv, 0)), b = __int_as_float(__builtin_amdgcn_readlane(iv, 16));
  const float c = __int_as_float(__builtin_amdgcn_readlane(iv, 32)), d = __int_as_float(__builtin_amdgcn_readlane(iv, 48));
  return (a + b) + (c + d);
}
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
  half2_t v = {(bf16_t)a, (bf16_t)b};
  return __builtin_bit_cast(uint32_t, v);
}

// butterfly step of a reduction over the lanes lane ^ o, o = 8, 16, 32, without the LDS crossbar: lane ^ 8 is a DPP rotate
// inside the 16-lane row; lane ^ 16 and lane ^ 32 are v_permlane16_swap / v_permlane32_swap (CDNA4), which hand every lane BOTH
// partners' values (tools/probe_permlane.hip prints the lane maps) - a sum or max of the two results is the butterfly step
__device__ __forceinline__ float wave_bfly_max(float x, int o) {
  if (o == 8) return fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xf, 0xf, true)));
  const u32x2 r = o == 16 ? __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false)
                          : __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float wave_bfly_sum(float x, int o) {
  if (o == 8) return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xf, 0xf, true));
  const u32x2 r = o == 16 ? __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false)
                          : __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// order-preserving key of a score: larger float <=> larger unsigned
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// value of lane l (wave-uniform l) in every lane: v_readlane_b32, no LDS crossbar round trip
__device__ __forceinline__ float lane_val(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// histogram increment aggregated over the wave: the digits of log-probabilities crowd into a handful of bins (the top
// byte is sign + high exponent bits), and 64 lanes adding to one LDS word serialise; here each distinct digit of the
// wave costs one atomic.  Every lane of the wave must call it (act = does this lane contribute).
__device__ __forceinline__ void hist_add_wave(unsigned* hist, unsigned digit, bool act, int lane) {
  unsigned long long m = __ballot(act);
  while (m) {  // wave-uniform
    const int leader = __ffsll((long long)m) - 1;
    const unsigned dl = (unsigned)__shfl((int)digit, leader, 64);
    const unsigned long long same = __ballot(act && digit == dl);
    if (lane == leader) atomicAdd(&hist[dl], (unsigned)__popcll(same));
    m &= ~same;
  }
}

}  // namespace itts

// ---------------------------------------------------------------------------------------------
// decode_attn_group_kv8: the grouped cache attention of a beam decode step (decode_attn_group.hip) on the e4m3 K/V
// cache (opt-in on top of both switches: itts_gpt_set_group_attn_kv_fp8 / ITTS_GROUP_ATTN_KV_FP8).  A cache row is
// 64 bytes, not 128, so the mapping of lanes to bytes, the unit and the V transpose are this kernel's own.
//
// Kept from 5o: grid (H, B / nb), 4 waves per (head, item), the item's nb queries as the 16 columns of an MFMA tile, units dealt to
// the waves (unit t to wave t & 3), one online-softmax state per wave, one merge through LDS at the end, no workgroup barrier in
// the key loop, need(j) read in passes until a ballot finds every set empty, query q admits key (j, r) iff anc[q][j] == r and
// kv_start[q] <= j < pos_q, masked to -inf before the maximum, the cache row at pos never admitted.
// Unit: 64 positions = 4 KiB of K + 4 KiB of V, the bytes a unit of the 16-bit kernel has in flight; the four-wave deal is 256.
// K: lane (fr, fg) loads ONE 16-byte piece per 16-key quarter hh: dims 16 fg .. + 15 of key 16 hh + fr (a wave-load covers 16 whole
// rows, 1 KiB contiguous on the trunk).  The contraction of S^T = K Q^T runs over a permutation of the dims: k-step c takes bytes
// 8 c .. + 7 of the lane's load and qhi[c] / qlo[c] hold q dims 16 fg + 8 c .. + 7 - no second load, no shuffle.
// V: lane (kg = lane >> 2, dg = lane & 3) loads dims 16 dg .. + 15 of keys 4 kg .. + 3, transposes the four 4 x 4 byte blocks with
// v_perm_b32 and writes a wave-private LDS tile [dim][key] in BYTES, one dword of four keys per dim; lane (fr = dim, fg) reads keys
// 4 fg .. + 3 of both halves of a 32-key k-step back as two dwords.  With k-slot (fg, e) = key 16 (e / 4) + 4 fg + e % 4 the lane's
// probabilities are already the B operand of O^T = V^T P^T, twice per unit.
// LDS tile: 64 rows of 16 dwords, NO padding; dword column c of row d lies at c ^ (d & 14) ^ ((d >> 2) & 8), and a lane writes
// its four dims of a block in the order b ^ dg (the v_perm selectors are per lane, so that costs nothing).  A pure row stride
// cannot serve both sides: the writes need an odd stride in dwords, the reads need the sixteen row starts 4 banks apart.
// Checked by enumeration for 64 banks x 4 bytes over the wave and for 32 banks over each half wave: every dword write and every
// dword read touches 64 (32) distinct banks.
// Decoding: e4m3 is exact in bf16 and in binary16.  gfx950's one-step packed converts with a scale of 1 where the compiler has
// them, else v_cvt_pk_f32_fp8 and the upper halves (bf16) / a packed convert (binary16).  The MFMAs stay half_mfma16 on 16-bit
// operands; q * scale and P enter as hi + lo with fp32 accumulation (an fp8 MFMA would round q).
// This step's k / v: rounded with fp8_pack4 (the bytes decode_attn2_kernel<fp8_t> and kv_scatter_kernel write), appended to each
// beam's own row at pos as 16-byte vector stores and taken into wave 0's state from registers: fp32 FMAs over the decoded
// rounded k, weight exp(0), the accumulator initialised with the decoded rounded v.
// kc / vc must be 16-byte aligned (every row is 64 bytes).
// ---------------------------------------------------------------------------------------------
#include "itts_decode.h"
#include "itts_wave_dev.h"

#if defined(__has_builtin)
#if !defined(ITTS_HALF_F16) && __has_builtin(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8)
#define ITTS_KV8_ONE_STEP 1
#elif defined(ITTS_HALF_F16) && __has_builtin(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8)
#define ITTS_KV8_ONE_STEP 1
#endif
#endif

namespace itts {
namespace {

constexpr int G8_U = 64;  // positions per unit

// LDS written by some lanes of a wave and read by others: the hardware runs a wave's LDS operations in order, the compiler must
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ u32x4 ld16(const uint8_t* p) { return *reinterpret_cast<const u32x4*>(p); }

// x[0 .. 7] = hi + lo in the 16-bit type, as two MFMA operands
__device__ __forceinline__ void split_hi_lo(const float* x, half8_bits& hi, half8_bits& lo) {
  u32x4 h, l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bf16_t a = (bf16_t)x[2 * i], b = (bf16_t)x[2 * i + 1];
    h[i] = pack_bf16((float)a, (float)b);
    l[i] = pack_bf16(x[2 * i] - (float)a, x[2 * i + 1] - (float)b);
  }
  hi = __builtin_bit_cast(half8_bits, h);
  lo = __builtin_bit_cast(half8_bits, l);
}

// four e4m3 bytes -> four values of the 16-bit type in byte order, exact in both builds
__device__ __forceinline__ u32x2 dec4(uint32_t w) {
  u32x2 r;
#ifdef ITTS_KV8_ONE_STEP
#ifdef ITTS_HALF_F16
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.f, false));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.f, true));
#else
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.f, false));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.f, true));
#endif
#else
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
#ifdef ITTS_HALF_F16
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(lo[0], lo[1]));  // exact: nothing to round
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(hi[0], hi[1]));
#else
  r[0] = __builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u);  // the upper halves
  r[1] = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
#endif
#endif
  return r;
}
__device__ __forceinline__ half8_bits dec8(uint32_t w0, uint32_t w1) {
  const u32x2 a = dec4(w0), b = dec4(w1);
  return __builtin_bit_cast(half8_bits, u32x4{a[0], a[1], b[0], b[1]});
}

// dword index of (dim d, key column c = key / 4) in a wave's transposed V tile
__device__ __forceinline__ int vt_idx(int d, int c) { return d * 16 + (c ^ (d & 14) ^ ((d >> 2) & 8)); }

template <bool TILED>
__global__ __launch_bounds__(256) void decode_attn_group_kv8_kernel(bf16_t* __restrict__ ctx, const float* __restrict__ qkv,
                                                                    uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                                    const int* __restrict__ len, const int* __restrict__ kv_start,
                                                                    const int* __restrict__ prefix, const uint8_t* __restrict__ anc,
                                                                    int nb, int H, int Smax, float scale, int ctx_bt) {
  constexpr int DH = 64, NW = 4, U = G8_U;
  __shared__ __attribute__((aligned(16))) uint32_t s_vt[NW][DH * 16];  // per wave: V of the current unit, [dim][key] in bytes
  __shared__ __attribute__((aligned(4))) uint8_t s_anc[NW][16][U];     // per wave: clamped ancestry of the unit being issued
  __shared__ __attribute__((aligned(4))) uint8_t s_row[NW][U];         // per wave: physical row of each position in this pass
  __shared__ float s_m[NW][16], s_l[NW][16];
  __shared__ float s_o[NW][16][DH + 1];
  const int h = blockIdx.x, b0 = blockIdx.y * nb, B = gridDim.y * nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int D = H * DH;
  // ---- the lane's query (fr) and the item's range of positions ----
  const bool qok = fr < nb;
  const int qrow = b0 + (qok ? fr : 0);
  const int mylen = len[qrow], myks = kv_start[qrow];
  const int pos = prefix[0] + mylen;
  const unsigned parmask = (unsigned)__ballot(qok && fg == 0 && (mylen & 1)) & 0xFFFFu;  // bit q: live ancestry half of beam q
  int posmax = qok ? pos : 0, ksmin = qok ? myks : 0x7FFFFFFF;
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    posmax = max(posmax, __shfl_xor(posmax, o, 64));
    ksmin = min(ksmin, __shfl_xor(ksmin, o, 64));
  }
  // ---- q * scale as hi + lo operands (dims 16 fg .. + 15); this step's k / v (wave 0): rounded, appended, taken into the state ----
  const float* qp = qkv + (size_t)qrow * 3 * D + h * DH;
  half8_bits qhi[2], qlo[2];
  float m = -INFINITY, l = 0.f;
  f32x4 acc[4];
#pragma unroll
  for (int d0 = 0; d0 < 4; ++d0) acc[d0] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    float qs[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(qp + 16 * fg + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) qs[4 * i + e] = qok ? v[e] * scale : 0.f;
    }
    split_hi_lo(qs, qhi[0], qlo[0]);
    split_hi_lo(qs + 8, qhi[1], qlo[1]);
    if (wave == 0) {
      float dot = 0.f;
      u32x4 kw, vw;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 kf = *reinterpret_cast<const f32x4*>(qp + D + 16 * fg + 4 * i);
        const f32x4 vf = *reinterpret_cast<const f32x4*>(qp + 2 * D + 16 * fg + 4 * i);
        kw[i] = fp8_pack4(kf[0], kf[1], kf[2], kf[3]);
        vw[i] = fp8_pack4(vf[0], vf[1], vf[2], vf[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) dot = fmaf(qs[4 * i + e], fp8_get(kw[i], e), dot);
      }
      if (qok) {  // the beam's own physical row, whatever the ancestry says
        const size_t o = (((size_t)qrow * H + h) * Smax + pos) * DH + 16 * fg;
        *reinterpret_cast<u32x4*>(kc + o) = kw;
        *reinterpret_cast<u32x4*>(vc + o) = vw;
      }
      dot = wave_bfly_sum(dot, 16);
      dot = wave_bfly_sum(dot, 32);
      if (qok) {
        m = dot;
        l = fg == 0 ? 1.f : 0.f;  // l is summed over fg at the end
#pragma unroll
        for (int d0 = 0; d0 < 4; ++d0) {  // the accumulator's dims of this lane: 16 * d0 + 4 * fg + r
          const f32x4 vf = *reinterpret_cast<const f32x4*>(qp + 2 * D + 16 * d0 + 4 * fg);
          const uint32_t w = fp8_pack4(vf[0], vf[1], vf[2], vf[3]);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[d0][r] = fp8_get(w, r);
        }
      }
    }
  }
  // ---- the key loop ----
  const int ntl = (posmax + U - 1) / U;  // units [0, ntl) hold the positions < posmax
  int t = ksmin / U;
  t += (wave - t) & 3;                    // the first unit of this wave that holds a position >= ksmin
  const int kg = lane >> 2, dg = lane & 3;  // V duty: keys 4 * kg .. + 3, dims 16 * dg .. + 15
  // the lane writes dim 4 w + (b ^ dg) of block w as its b-th store: the selectors of the two v_perm stages, per lane
  const uint32_t selA = (dg & 2) ? 0x07030602u : 0x05010400u, selB = (dg & 2) ? 0x05010400u : 0x07030602u;
  const uint32_t selC = (dg & 1) ? 0x07060302u : 0x05040100u, selD = (dg & 1) ? 0x05040100u : 0x07060302u;
  unsigned rem = 0;            // rows of position `lane` of the unit not yet read
  uint32_t araw[4] = {0, 0, 0, 0};  // raw ancestry bytes of the next unit to prepare: beam q in byte q & 3 of word q >> 2
  auto load_anc = [&](int tt) {
    const int j = min(tt * U + lane, Smax - 1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      araw[g] = 0;
      if (4 * g < nb) {  // wave-uniform; inside, every load is issued (beams >= nb re-read the last beam's byte, which prep ignores)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int q = min(4 * g + i, nb - 1);
          araw[g] |= (uint32_t)anc[((size_t)((parmask >> q) & 1u) * B + b0 + q) * Smax + j] << (8 * i);
        }
      }
    }
  };
  auto prep = [&](int tt) {  // araw -> s_anc, rem
    wave_lds_sync();
    unsigned part = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (q < nb) {  // wave-uniform
        const int c = min((int)((araw[q >> 2] >> (8 * (q & 3))) & 255u), nb - 1);  // entries at >= pos may be 255
        s_anc[wave][q][lane] = (uint8_t)c;
        part |= 1u << c;
      }
    }
    const int j = tt * U + lane;
    rem = (j >= ksmin && j < posmax) ? part : 0u;
  };
  auto issue = [&](int tt, u32x4 (&kk)[4], u32x4 (&vv)[4], uint32_t& adm) {
    wave_lds_sync();
    s_row[wave][lane] = rem ? (uint8_t)__builtin_ctz(rem) : (uint8_t)255;
    rem &= rem - 1;
    wave_lds_sync();
#pragma unroll
    for (int hh = 0; hh < 4; ++hh) {  // K in operand layout: key 16 * hh + fr, dims 16 * fg .. + 15
      const int j = min(tt * U + 16 * hh + fr, Smax - 1);
      int r = s_row[wave][16 * hh + fr];
      r = r == 255 ? 0 : r;
      kk[hh] = ld16(kc + (((size_t)(b0 + r) * H + h) * Smax + j) * DH + 16 * fg);
    }
    const uint32_t rv = *reinterpret_cast<const uint32_t*>(&s_row[wave][4 * kg]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = min(tt * U + 4 * kg + i, Smax - 1);
      int r = (rv >> (8 * i)) & 255u;
      r = r == 255 ? 0 : r;
      vv[i] = ld16(vc + (((size_t)(b0 + r) * H + h) * Smax + j) * DH + 16 * dg);
    }
    adm = 0;
#pragma unroll
    for (int hh = 0; hh < 4; ++hh) {
      const uint32_t aw = *reinterpret_cast<const uint32_t*>(&s_anc[wave][fr][16 * hh + 4 * fg]);
      const uint32_t rw = *reinterpret_cast<const uint32_t*>(&s_row[wave][16 * hh + 4 * fg]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = tt * U + 16 * hh + 4 * fg + r;
        const bool ok = qok && ((aw >> (8 * r)) & 255u) == ((rw >> (8 * r)) & 255u) && j >= myks && j < pos;
        adm |= (ok ? 1u : 0u) << (4 * hh + r);
      }
    }
  };
  auto compute = [&](const u32x4 (&kk)[4], const u32x4 (&vv)[4], uint32_t adm) {
    wave_lds_sync();
#pragma unroll
    for (int w = 0; w < 4; ++w) {  // V, transposed: the 4 x 4 byte block of dims 16 * dg + 4 * w .. + 3, keys 4 * kg .. + 3
      const uint32_t x0 = __builtin_amdgcn_perm(vv[1][w], vv[0][w], selA), x1 = __builtin_amdgcn_perm(vv[1][w], vv[0][w], selB);
      const uint32_t y0 = __builtin_amdgcn_perm(vv[3][w], vv[2][w], selA), y1 = __builtin_amdgcn_perm(vv[3][w], vv[2][w], selB);
      const uint32_t o[4] = {__builtin_amdgcn_perm(y0, x0, selC), __builtin_amdgcn_perm(y0, x0, selD),
                             __builtin_amdgcn_perm(y1, x1, selC), __builtin_amdgcn_perm(y1, x1, selD)};
#pragma unroll
      for (int b = 0; b < 4; ++b) s_vt[wave][vt_idx(16 * dg + 4 * w + (b ^ dg), kg)] = o[b];
    }
    f32x4 s[4];
#pragma unroll
    for (int hh = 0; hh < 4; ++hh) {
      s[hh] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const half8_bits kf = dec8(kk[hh][2 * c], kk[hh][2 * c + 1]);
        s[hh] = half_mfma16(kf, qhi[c], s[hh]);
        s[hh] = half_mfma16(kf, qlo[c], s[hh]);
      }
    }
    float sc[16], tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      sc[e] = ((adm >> e) & 1u) ? s[e >> 2][e & 3] : -INFINITY;  // masked before the maximum
      tmax = fmaxf(tmax, sc[e]);
    }
    tmax = wave_bfly_max(tmax, 16);
    tmax = wave_bfly_max(tmax, 32);
    const float mn = fmaxf(m, tmax);
    float p[16];
    if (mn > -INFINITY) {
      const float alpha = __expf(m - mn);  // exp(-inf) = 0 for a fresh state
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        p[e] = __expf(sc[e] - mn);
        ps += p[e];
      }
      l = fmaf(l, alpha, ps);
#pragma unroll
      for (int d0 = 0; d0 < 4; ++d0) acc[d0] *= alpha;
      m = mn;
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) p[e] = 0.f;
    }
    wave_lds_sync();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {  // keys 32 * ks .. + 31: k-slot (fg, e) = key 32 * ks + 16 * (e / 4) + 4 * fg + e % 4
      half8_bits phi, plo;
      split_hi_lo(p + 8 * ks, phi, plo);
#pragma unroll
      for (int d0 = 0; d0 < 4; ++d0) {
        const int d = 16 * d0 + fr;
        const half8_bits vf = dec8(s_vt[wave][vt_idx(d, 8 * ks + fg)], s_vt[wave][vt_idx(d, 8 * ks + 4 + fg)]);
        acc[d0] = half_mfma16(vf, phi, acc[d0]);
        acc[d0] = half_mfma16(vf, plo, acc[d0]);
      }
    }
  };
  u32x4 kn[4], vn[4];
  uint32_t admn = 0;
  bool have = t < ntl;
  if (have) {
    load_anc(t);
    prep(t);
    if (t + 4 < ntl) load_anc(t + 4);
    issue(t, kn, vn, admn);
  }
  while (have) {
    u32x4 kcur[4], vcur[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kcur[i] = kn[i];
      vcur[i] = vn[i];
    }
    const uint32_t admc = admn;
    if (__ballot(rem != 0) == 0) {  // every position's rows are read: on to this wave's next unit
      t += 4;
      have = t < ntl;
      if (have) {
        prep(t);
        if (t + 4 < ntl) load_anc(t + 4);
      }
    }
    if (have) issue(t, kn, vn, admn);
    compute(kcur, vcur, admc);
  }
  // ---- merge the four waves ----
  l = wave_bfly_sum(l, 16);
  l = wave_bfly_sum(l, 32);
  if (fg == 0) {
    s_m[wave][fr] = m;
    s_l[wave][fr] = l;
  }
#pragma unroll
  for (int d0 = 0; d0 < 4; ++d0)
#pragma unroll
    for (int r = 0; r < 4; ++r) s_o[wave][fr][16 * d0 + 4 * fg + r] = acc[d0][r];
  __syncthreads();
  for (int idx = tid; idx < nb * DH; idx += 256) {
    const int q = idx >> 6, d = idx & 63;
    float MM = s_m[0][q];
#pragma unroll
    for (int w = 1; w < NW; ++w) MM = fmaxf(MM, s_m[w][q]);
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float e = s_m[w][q] > -INFINITY ? __expf(s_m[w][q] - MM) : 0.f;
      o = fmaf(e, s_o[w][q][d], o);
      L = fmaf(e, s_l[w][q], L);
    }
    const int b = b0 + q;  // wave 0 always holds the appended key: L >= exp(m0 - MM) > 0
    stf(ctx + (TILED ? tile_off(b, h * DH + d, ctx_bt) : (size_t)b * D + h * DH + d), o / L);
  }
}

}  // namespace

int decode_attn_group_kv8(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start,
                          const int* prefix_dev, int B, int H, int dh, int Smax, int tc, hipStream_t s, int ctx_tiled,
                          const uint8_t* anc, int nb) {
  ITTS_REQUIRE(dh == 64, "decode_attn_group_kv8: head dim must be 64");
  ITTS_REQUIRE(nb >= 2 && nb <= 16, "decode_attn_group_kv8: needs 2 <= nb <= 16 beams per item");
  ITTS_REQUIRE(B % nb == 0, "decode_attn_group_kv8: B must be a multiple of nb");
  ITTS_REQUIRE(anc, "decode_attn_group_kv8: the beam ancestry is missing");
  ITTS_REQUIRE(tc == FP8, "decode_attn_group_kv8: the cache must be the fp8 (e4m3) type (a 16-bit cache has decode_attn_group)");
  ITTS_REQUIRE(to == BF16, "decode_attn_group_kv8: ctx must be the 16-bit type");
  ITTS_REQUIRE(((uintptr_t)kc | (uintptr_t)vc) % 16 == 0, "decode_attn_group_kv8: the caches must be 16-byte aligned");
  const float scale = 1.f / sqrtf((float)dh);
  const dim3 grid(H, B / nb);
  const int bt = ctx_tiled ? (B + 15) / 16 : 0;
  if (ctx_tiled)
    hipLaunchKernelGGL(decode_attn_group_kv8_kernel<true>, grid, dim3(256), 0, s, (bf16_t*)ctx, qkv, (uint8_t*)kc, (uint8_t*)vc, len,
                       kv_start, prefix_dev, anc, nb, H, Smax, scale, bt);
  else
    hipLaunchKernelGGL(decode_attn_group_kv8_kernel<false>, grid, dim3(256), 0, s, (bf16_t*)ctx, qkv, (uint8_t*)kc, (uint8_t*)vc, len,
                       kv_start, prefix_dev, anc, nb, H, Smax, scale, bt);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace itts

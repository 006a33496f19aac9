// ---------------------------------------------------------------------------------------------
// decode_attn_group_split: the grouped cache attention of a beam decode step (decode_attn_group.hip) with the keys
// of one (head, item) dealt to NS workgroups (opt-in on top of group_attn: itts_gpt_set_group_attn_split / ITTS_GROUP_ATTN_SPLIT;
// DESIGN.md 5q).  The unsplit kernel's grid is (H, items): at 3 to 6 sentences and H = 20 that is 60 to 120 workgroups on 256 CUs,
// each walking its whole history.  Here the grid is (H, items, NS), 2 <= NS <= 8, and a second, small kernel merges the NS partials.
// decode_attn_group.hip is byte for byte what it was; the key loop below is its text.
//
// Work split: the host does not know S (the step is replayed from a captured graph, len lives on the device), so every workgroup
// derives its chunk from the item's ksmin / posmax, which it reduces anyway: t_first = ksmin >> 5, ntl = ceil(posmax / 32),
// n = max(ntl - t_first, 0), per = ceil(n / NS) rounded up to a multiple of 4 (each of the four waves of a split gets the same
// share), split z owns tiles [t_first + z * per, min(t_first + (z + 1) * per, ntl)).  Inside the chunk tile t goes to wave t & 3,
// and everything of 5o holds: the passes over need(j), the admission mask, K in operand layout, the per-wave transposed V tile,
// hi + lo operands, one unit of look-ahead, masking to -inf before the maximum, no workgroup barrier in the key loop.
// This step's k / v: only split 0 appends the rounded rows (the same 16-byte stores) and only its wave 0 takes the appended key
// into its state from registers; the other splits neither read the cache row at pos nor write the cache.
// Epilogue: the four waves merge through LDS with max-rescaling, but nothing is normalised: per query q < nb the workgroup writes
// the fp32 accumulator to part_o[z][b][h][0 .. 63] and (m, l) to part_ml[z][b][h][0 .. 1] with plain vector stores.  A split that
// admitted no key for a row (an empty chunk, a chunk outside the row's [kv_start, pos)) writes exactly (-inf, 0) and zeros, and
// every (z, b, h) slot of a launch is written: the merge never reads stale data.
// decode_attn_group_merge_kernel<TILED>: 16 lanes per (row, head), four dims each; the NS partials in the fixed order z = 0 ..
// NS - 1: MM = max m, e_z = m_z > -inf ? exp(m_z - MM) : 0, o = sum e_z o_z, L = sum e_z l_z, ctx = o / L in the 16-bit type
// (row-major or tile_off).  Split 0 always holds the appended key: L > 0.  No atomics, no tickets, no polling.
// ---------------------------------------------------------------------------------------------
#include "itts_decode.h"
#include "itts_wave_dev.h"

namespace itts {
namespace {

constexpr int GA_VS = 36;  // halves per [dim] row of the transposed V tile: 32 keys + 4 (rows stay 8-byte aligned)

// LDS written by some lanes of a wave and read by others: the hardware runs a wave's LDS operations in order, the compiler must
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ u32x4 ld16(const bf16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

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

// grid (H, items, NS).  part_o [NS][B][H][64], part_ml [NS][B][H][2] (m, l), fp32
__global__ __launch_bounds__(256) void decode_attn_group_split_kernel(float* __restrict__ part_o, float* __restrict__ part_ml,
                                                                      const float* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                                      bf16_t* __restrict__ vc, const int* __restrict__ len,
                                                                      const int* __restrict__ kv_start, const int* __restrict__ prefix,
                                                                      const uint8_t* __restrict__ anc, int nb, int H, int Smax,
                                                                      float scale) {
  constexpr int DH = 64, NW = 4;
  __shared__ __attribute__((aligned(16))) bf16_t s_vt[NW][DH * GA_VS];  // per wave: V of the current unit, [dim][key]
  __shared__ __attribute__((aligned(4))) uint8_t s_anc[NW][16][32];     // per wave: clamped ancestry of the tile being issued
  __shared__ __attribute__((aligned(4))) uint8_t s_row[NW][32];         // per wave: physical row of each position in this pass
  __shared__ float s_m[NW][16], s_l[NW][16];
  __shared__ float s_o[NW][16][DH + 1];
  const int h = blockIdx.x, b0 = blockIdx.y * nb, B = gridDim.y * nb, z = blockIdx.z, NS = gridDim.z;
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
  // ---- q * scale as hi + lo operands; this step's k / v (wave 0 of split 0): rounded, appended, taken into the state ----
  const float* qp = qkv + (size_t)qrow * 3 * D + h * DH;
  half8_bits qhi[2], qlo[2];
  float m = -INFINITY, l = 0.f;
  f32x4 acc[4];
#pragma unroll
  for (int d0 = 0; d0 < 4; ++d0) acc[d0] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    float qs[16];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(qp + 32 * c + 8 * fg + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) qs[8 * c + 4 * i + e] = qok ? v[e] * scale : 0.f;
      }
    split_hi_lo(qs, qhi[0], qlo[0]);
    split_hi_lo(qs + 8, qhi[1], qlo[1]);
    if (wave == 0 && z == 0) {
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        u32x4 kw, vw;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const f32x4 kf = *reinterpret_cast<const f32x4*>(qp + D + 32 * c + 8 * fg + 4 * i);
          const f32x4 vf = *reinterpret_cast<const f32x4*>(qp + 2 * D + 32 * c + 8 * fg + 4 * i);
#pragma unroll
          for (int e = 0; e < 4; ++e) dot = fmaf(qs[8 * c + 4 * i + e], (float)(bf16_t)kf[e], dot);
          kw[2 * i] = pack_bf16(kf[0], kf[1]);
          kw[2 * i + 1] = pack_bf16(kf[2], kf[3]);
          vw[2 * i] = pack_bf16(vf[0], vf[1]);
          vw[2 * i + 1] = pack_bf16(vf[2], vf[3]);
        }
        if (qok) {  // the beam's own physical row, whatever the ancestry says
          const size_t o = (((size_t)qrow * H + h) * Smax + pos) * DH + 32 * c + 8 * fg;
          *reinterpret_cast<u32x4*>(kc + o) = kw;
          *reinterpret_cast<u32x4*>(vc + o) = vw;
        }
      }
      dot = wave_bfly_sum(dot, 16);
      dot = wave_bfly_sum(dot, 32);
      if (qok) {
        m = dot;
        l = fg == 0 ? 1.f : 0.f;  // l is summed over fg at the end
#pragma unroll
        for (int d0 = 0; d0 < 4; ++d0) {  // the accumulator's dims of this lane: 16 * d0 + 4 * fg + r
          const f32x4 vf = *reinterpret_cast<const f32x4*>(qp + 2 * D + 16 * d0 + 4 * fg);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[d0][r] = (float)(bf16_t)vf[r];
        }
      }
    }
  }
  // ---- this split's chunk of the item's tiles, and the key loop over it ----
  const int ntl = (posmax + 31) >> 5;  // tiles [0, ntl) hold the positions < posmax
  const int t_first = ksmin >> 5;      // the first tile that holds a position >= ksmin
  const int per = ((max(ntl - t_first, 0) + NS - 1) / NS + 3) & ~3;
  const int t_end = min(t_first + (z + 1) * per, ntl);  // tiles [t_first + z * per, t_end) are this split's
  int t = t_first + z * per;
  t += (wave - t) & 3;                 // the first tile of this wave in the chunk
  const int jj = lane & 31, hq = lane >> 5;  // ancestry duty: position jj of the tile, beams hq, hq + 2, ..
  const int kg = lane >> 3, dg = lane & 7;   // V duty: keys 4 * kg .. + 3, dims 8 * dg .. + 7
  unsigned rem = 0;                          // rows of position jj not yet read
  uint32_t a0 = 0, a1 = 0;                   // raw ancestry bytes of the next tile to prepare
  auto load_anc = [&](int tt) {
    const int j = min(tt * 32 + jj, Smax - 1);
    a0 = a1 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      // every load is issued (beams >= nb re-read the last beam's byte, which prep ignores): a load under a lane-dependent
      // branch would wait for its result before the next one is requested
      const int q = min(hq + 2 * i, nb - 1);
      const uint32_t v = anc[((size_t)((parmask >> q) & 1u) * B + b0 + q) * Smax + j];
      if (i < 4) a0 |= v << (8 * i);
      else a1 |= v << (8 * (i - 4));
    }
  };
  auto prep = [&](int tt) {  // a0 / a1 -> s_anc, rem
    wave_lds_sync();
    unsigned part = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q = hq + 2 * i;
      if (q < nb) {
        const int c = min((int)(((i < 4 ? a0 : a1) >> (8 * (i & 3))) & 255u), nb - 1);  // entries at >= pos may be 255
        s_anc[wave][q][jj] = (uint8_t)c;
        part |= 1u << c;
      }
    }
    part |= (unsigned)__shfl_xor((int)part, 32, 64);
    const int j = tt * 32 + jj;
    rem = (j >= ksmin && j < posmax) ? part : 0u;
  };
  auto issue = [&](int tt, u32x4 (&kk)[4], u32x4 (&vv)[4], uint32_t& adm) {
    wave_lds_sync();
    if (lane < 32) s_row[wave][lane] = rem ? (uint8_t)__builtin_ctz(rem) : (uint8_t)255;
    rem &= rem - 1;
    wave_lds_sync();
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {  // K in operand layout: key 16 * hh + fr, dims 32 * c + 8 * fg
      const int j = min(tt * 32 + 16 * hh + fr, Smax - 1);
      int r = s_row[wave][16 * hh + fr];
      r = r == 255 ? 0 : r;
      const bf16_t* p = kc + (((size_t)(b0 + r) * H + h) * Smax + j) * DH + 8 * fg;
      kk[2 * hh] = ld16(p);
      kk[2 * hh + 1] = ld16(p + 32);
    }
    const uint32_t rv = *reinterpret_cast<const uint32_t*>(&s_row[wave][4 * kg]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = min(tt * 32 + 4 * kg + i, Smax - 1);
      int r = (rv >> (8 * i)) & 255u;
      r = r == 255 ? 0 : r;
      vv[i] = ld16(vc + (((size_t)(b0 + r) * H + h) * Smax + j) * DH + 8 * dg);
    }
    adm = 0;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const uint32_t aw = *reinterpret_cast<const uint32_t*>(&s_anc[wave][fr][16 * hh + 4 * fg]);
      const uint32_t rw = *reinterpret_cast<const uint32_t*>(&s_row[wave][16 * hh + 4 * fg]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = tt * 32 + 16 * hh + 4 * fg + r;
        const bool ok = qok && ((aw >> (8 * r)) & 255u) == ((rw >> (8 * r)) & 255u) && j >= myks && j < pos;
        adm |= (ok ? 1u : 0u) << (4 * hh + r);
      }
    }
  };
  auto compute = [&](const u32x4 (&kk)[4], const u32x4 (&vv)[4], uint32_t adm) {
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // V, transposed: dim 8 * dg + i of keys 4 * kg .. + 3
      const int w = i >> 1;
      u32x2 x;
      if (i & 1) {
        x[0] = (vv[0][w] >> 16) | (vv[1][w] & 0xFFFF0000u);
        x[1] = (vv[2][w] >> 16) | (vv[3][w] & 0xFFFF0000u);
      } else {
        x[0] = (vv[0][w] & 0xFFFFu) | (vv[1][w] << 16);
        x[1] = (vv[2][w] & 0xFFFFu) | (vv[3][w] << 16);
      }
      *reinterpret_cast<u32x2*>(&s_vt[wave][(8 * dg + i) * GA_VS + 4 * kg]) = x;
    }
    f32x4 s[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      s[hh] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const half8_bits kf = __builtin_bit_cast(half8_bits, kk[2 * hh + c]);
        s[hh] = half_mfma16(kf, qhi[c], s[hh]);
        s[hh] = half_mfma16(kf, qlo[c], s[hh]);
      }
    }
    float sc[8], tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sc[e] = ((adm >> e) & 1u) ? s[e >> 2][e & 3] : -INFINITY;  // masked before the maximum
      tmax = fmaxf(tmax, sc[e]);
    }
    tmax = wave_bfly_max(tmax, 16);
    tmax = wave_bfly_max(tmax, 32);
    const float mn = fmaxf(m, tmax);
    float p[8];
    if (mn > -INFINITY) {
      const float alpha = __expf(m - mn);  // exp(-inf) = 0 for a fresh state
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        p[e] = __expf(sc[e] - mn);
        ps += p[e];
      }
      l = fmaf(l, alpha, ps);
#pragma unroll
      for (int d0 = 0; d0 < 4; ++d0) acc[d0] *= alpha;
      m = mn;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) p[e] = 0.f;
    }
    half8_bits phi, plo;
    split_hi_lo(p, phi, plo);
    wave_lds_sync();
#pragma unroll
    for (int d0 = 0; d0 < 4; ++d0) {
      const bf16_t* vr = &s_vt[wave][(16 * d0 + fr) * GA_VS + 4 * fg];
      const u32x2 v0 = *reinterpret_cast<const u32x2*>(vr), v1 = *reinterpret_cast<const u32x2*>(vr + 16);
      const half8_bits vf = __builtin_bit_cast(half8_bits, u32x4{v0[0], v0[1], v1[0], v1[1]});
      acc[d0] = half_mfma16(vf, phi, acc[d0]);
      acc[d0] = half_mfma16(vf, plo, acc[d0]);
    }
  };
  u32x4 kn[4], vn[4];
  uint32_t admn = 0;
  bool have = t < t_end;
  if (have) {
    load_anc(t);
    prep(t);
    if (t + 4 < t_end) load_anc(t + 4);
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
    if (__ballot(rem != 0) == 0) {  // every position's rows are read: on to this wave's next tile
      t += 4;
      have = t < t_end;
      if (have) {
        prep(t);
        if (t + 4 < t_end) load_anc(t + 4);
      }
    }
    if (have) issue(t, kn, vn, admn);
    compute(kcur, vcur, admc);
  }
  // ---- merge the four waves; the partial stays un-normalised ----
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
  if (tid < nb * 16) {  // query q, dims 4 * d4 .. + 3
    const int q = tid >> 4, d4 = tid & 15;
    float MM = s_m[0][q];
#pragma unroll
    for (int w = 1; w < NW; ++w) MM = fmaxf(MM, s_m[w][q]);
    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {  // a wave (a split) that admitted no key: m = -inf, weight 0 -> (-inf, 0) and zeros
      const float e = s_m[w][q] > -INFINITY ? __expf(s_m[w][q] - MM) : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = fmaf(e, s_o[w][q][4 * d4 + r], o[r]);
      L = fmaf(e, s_l[w][q], L);
    }
    const size_t slot = ((size_t)z * B + b0 + q) * H + h;
    *reinterpret_cast<f32x4*>(part_o + slot * DH + 4 * d4) = o;
    if (d4 == 0) *reinterpret_cast<float2*>(part_ml + slot * 2) = float2{MM, L};
  }
}

// 256 threads = 16 (row, head) pairs of 16 lanes, lane dl owns dims 4 * dl .. + 3.  BH = B * H pairs
template <bool TILED>
__global__ __launch_bounds__(256) void decode_attn_group_merge_kernel(bf16_t* __restrict__ ctx, const float* __restrict__ part_o,
                                                                      const float* __restrict__ part_ml, int BH, int H, int NS,
                                                                      int ctx_bt) {
  const int pair = blockIdx.x * 16 + (threadIdx.x >> 4), dl = threadIdx.x & 15;
  if (pair >= BH) return;
  float MM = -INFINITY;
  for (int z = 0; z < NS; ++z) MM = fmaxf(MM, part_ml[((size_t)z * BH + pair) * 2]);
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  float L = 0.f;
  for (int z = 0; z < NS; ++z) {
    const size_t slot = (size_t)z * BH + pair;
    const float2 ml = *reinterpret_cast<const float2*>(part_ml + slot * 2);
    const f32x4 oz = *reinterpret_cast<const f32x4*>(part_o + slot * 64 + 4 * dl);
    const float e = ml.x > -INFINITY ? __expf(ml.x - MM) : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = fmaf(e, oz[r], o[r]);
    L = fmaf(e, ml.y, L);
  }
  const int b = pair / H, col = (pair - b * H) * 64 + 4 * dl;  // split 0 always holds the appended key: L > 0
  u32x2 w;
  w[0] = pack_bf16(o[0] / L, o[1] / L);
  w[1] = pack_bf16(o[2] / L, o[3] / L);
  // four neighbouring dims are neighbours in both layouts (tile_off keeps k % 8 together)
  *reinterpret_cast<u32x2*>(ctx + (TILED ? tile_off(b, col, ctx_bt) : (size_t)b * H * 64 + col)) = w;
}

}  // namespace

int decode_attn_group_split(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start,
                            const int* prefix_dev, int B, int H, int dh, int Smax, int tc, hipStream_t s, int ctx_tiled,
                            const uint8_t* anc, int nb, int nsplit, float* part_o, float* part_ml) {
  ITTS_REQUIRE(dh == 64, "decode_attn_group_split: head dim must be 64");
  ITTS_REQUIRE(nb >= 2 && nb <= 16, "decode_attn_group_split: needs 2 <= nb <= 16 beams per item");
  ITTS_REQUIRE(B % nb == 0, "decode_attn_group_split: B must be a multiple of nb");
  ITTS_REQUIRE(anc, "decode_attn_group_split: the beam ancestry is missing");
  ITTS_REQUIRE(tc == BF16, "decode_attn_group_split: the cache must be the 16-bit type (no fp32, no fp8 cache)");
  ITTS_REQUIRE(!ctx_tiled || to == BF16, "decode_attn_group_split: tiled ctx is the 16-bit type only");
  ITTS_REQUIRE(to == BF16, "decode_attn_group_split: ctx must be the 16-bit type");
  ITTS_REQUIRE(nsplit >= 2 && nsplit <= GROUP_SPLIT_MAX, "decode_attn_group_split: needs 2 <= nsplit <= 8 splits");
  ITTS_REQUIRE(part_o && part_ml, "decode_attn_group_split: the partial workspaces are missing");
  const float scale = 1.f / sqrtf((float)dh);
  const int bt = ctx_tiled ? (B + 15) / 16 : 0, BH = B * H;
  hipLaunchKernelGGL(decode_attn_group_split_kernel, dim3(H, B / nb, nsplit), dim3(256), 0, s, part_o, part_ml, qkv, (bf16_t*)kc,
                     (bf16_t*)vc, len, kv_start, prefix_dev, anc, nb, H, Smax, scale);
  ITTS_HIP_CHECK(hipGetLastError());
  if (ctx_tiled)
    hipLaunchKernelGGL(decode_attn_group_merge_kernel<true>, dim3((BH + 15) / 16), dim3(256), 0, s, (bf16_t*)ctx, part_o, part_ml, BH,
                       H, nsplit, bt);
  else
    hipLaunchKernelGGL(decode_attn_group_merge_kernel<false>, dim3((BH + 15) / 16), dim3(256), 0, s, (bf16_t*)ctx, part_o, part_ml, BH,
                       H, nsplit, bt);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// NS for H * items workgroups of the unsplit kernel (1: do not split).  Measured (profiles/group_attn_split.txt): the rule wants the
// largest NS of a band that is not slower than the unsplit kernel at S = 200, 500 AND 900 on the trunk, and the host cannot see S.
// At 60 to 240 workgroups every NS loses at S = 200 (1.15 to 1.9 of the time: the second launch and the partials cost more than
// the short history gives back), so no band has such an NS: the switch at 1 keeps the unsplit kernel, 2 .. 8 force the split
int group_split_rule(int H, int items) {
  (void)H;
  (void)items;
  return 1;
}

}  // namespace itts

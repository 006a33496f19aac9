// ---------------------------------------------------------------------------------------------
// decode_attn_group: cache attention of one decode step under beams with the beam GROUP as the unit of work (opt-in:
// itts_gpt_set_group_attn / ITTS_GROUP_ATTN).  decode_attn2_kernel<.., ANC> runs one workgroup per (beam row, head)
// and every workgroup gathers its whole history through the row's ancestry, although the nb beams of an item share every
// position up to their common ancestor: each shared K / V row is fetched nb times.  Here one workgroup of 4 waves serves a
// (head, item): every needed (position, physical row) is fetched once and scored for all nb queries on the matrix cores.
//
// Work split: the item's nb queries are the 16 columns of an MFMA tile (columns >= nb are zero and never stored).  Keys are
// dealt to the four waves in tiles of 32 positions (tile t to wave t & 3); a wave keeps its own online-softmax state for all
// queries and the waves merge once at the end through LDS.  No workgroup barrier inside the key loop.
// Which rows: need(j) = the set of physical rows that hold position j for some beam (a bit mask built from the nb ancestry
// bytes of the position).  A tile is read in passes: pass p takes, for every position, the p-th row of its set (positions with
// fewer rows are masked), until every set is empty - one pass on the trunk, whichever rows the positions alternate between, up
// to nb passes behind the common ancestor.  Query q admits key (j, r) iff anc[q][j] == r and kv_start[q] <= j < pos_q.
// Data: K goes global -> registers in operand layout (lane (fr, fg): key fr, dims 32 * ks + 8 * fg), S^T = K Q^T; a lane then
// owns query fr and keys 4 * fg + r of both 16-key halves, and with k-slot (fg, e) = key 16 * (e / 4) + 4 * fg + e % 4 its eight
// probabilities ARE the B operand of O^T = V^T P^T.  V is staged per wave in a private LDS tile, transposed on the way in
// ([dim][key], 8-byte writes of four keys), and read back as two 8-byte reads per lane and dim tile.  The unit (tile, pass)
// behind the current one is requested before the current one is computed; the ancestry bytes one tile ahead of that.
// Precision: q * scale and P each enter the MFMA as hi + lo of the 16-bit type (two MFMAs each), accumulation is fp32.
// This step's k / v: rounded to the cache type, appended to each beam's OWN row at pos (the bits decode_attn2_kernel writes) and
// taken into wave 0's state from registers (fp32 score, weight exp(0) at the start); the cache row at pos is never admitted.
// Rows outside [kv_start, pos) may hold anything finite: they are masked before the maximum and get weight exp(-inf) = 0.
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

template <bool TILED>
__global__ __launch_bounds__(256) void decode_attn_group_kernel(bf16_t* __restrict__ ctx, const float* __restrict__ qkv,
                                                                bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                                const int* __restrict__ len, const int* __restrict__ kv_start,
                                                                const int* __restrict__ prefix, const uint8_t* __restrict__ anc,
                                                                int nb, int H, int Smax, float scale, int ctx_bt) {
  constexpr int DH = 64, NW = 4;
  __shared__ __attribute__((aligned(16))) bf16_t s_vt[NW][DH * GA_VS];  // per wave: V of the current unit, [dim][key]
  __shared__ __attribute__((aligned(4))) uint8_t s_anc[NW][16][32];     // per wave: clamped ancestry of the tile being issued
  __shared__ __attribute__((aligned(4))) uint8_t s_row[NW][32];         // per wave: physical row of each position in this pass
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
  // ---- q * scale as hi + lo operands; this step's k / v (wave 0): rounded, appended, taken into the state ----
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
    if (wave == 0) {
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
  // ---- the key loop ----
  const int ntl = (posmax + 31) >> 5;  // tiles [0, ntl) hold the positions < posmax
  int t = ksmin >> 5;
  t += (wave - t) & 3;                 // the first tile of this wave that holds a position >= ksmin
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
    if (__ballot(rem != 0) == 0) {  // every position's rows are read: on to this wave's next tile
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

int decode_attn_group(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start,
                      const int* prefix_dev, int B, int H, int dh, int Smax, int tc, hipStream_t s, int ctx_tiled,
                      const uint8_t* anc, int nb) {
  ITTS_REQUIRE(dh == 64, "decode_attn_group: head dim must be 64");
  ITTS_REQUIRE(nb >= 2 && nb <= 16, "decode_attn_group: needs 2 <= nb <= 16 beams per item");
  ITTS_REQUIRE(B % nb == 0, "decode_attn_group: B must be a multiple of nb");
  ITTS_REQUIRE(anc, "decode_attn_group: the beam ancestry is missing");
  ITTS_REQUIRE(tc == BF16, "decode_attn_group: the cache must be the 16-bit type (no fp32, no fp8 cache)");
  ITTS_REQUIRE(!ctx_tiled || to == BF16, "decode_attn_group: tiled ctx is the 16-bit type only");
  ITTS_REQUIRE(to == BF16, "decode_attn_group: ctx must be the 16-bit type");
  const float scale = 1.f / sqrtf((float)dh);
  const dim3 grid(H, B / nb);
  const int bt = ctx_tiled ? (B + 15) / 16 : 0;
  if (ctx_tiled)
    hipLaunchKernelGGL(decode_attn_group_kernel<true>, grid, dim3(256), 0, s, (bf16_t*)ctx, qkv, (bf16_t*)kc, (bf16_t*)vc, len,
                       kv_start, prefix_dev, anc, nb, H, Smax, scale, bt);
  else
    hipLaunchKernelGGL(decode_attn_group_kernel<false>, grid, dim3(256), 0, s, (bf16_t*)ctx, qkv, (bf16_t*)kc, (bf16_t*)vc, len,
                       kv_start, prefix_dev, anc, nb, H, Smax, scale, bt);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace itts

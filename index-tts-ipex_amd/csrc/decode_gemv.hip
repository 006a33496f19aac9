// Decode GEMVs of the launch path, second generation (the per-token loop is launch/latency bound at B <= 8:
// SURVEY.md 8d, MI355X_MICROARCH "launches-baseline"), so each kernel here is built to
//   * touch every weight byte exactly once with 16-byte lane loads that are ALL issued before the first use
//     (deep memory-level parallelism, no LDS round trip for streamed weights - cdna_hip_programming "GEMV" row),
//   * keep the tiny activation vectors in LDS (fused LayerNorm / ln_f+final_norm / split-KV combine prologues),
//   * spread over >= 256 workgroups so every CU pulls on HBM.
// The other kernels of the launch path's decode step: decode_attn.hip (cache attention), decode_fused.hip (projection and
// attention in one launch), decode_sampler.hip (samplers, step embedding).
#include <cstdlib>

#include "itts_decode.h"
#include "itts_gemv_dev.h"
#include "itts_wave_dev.h"
#include "decode_pinned.h"

namespace itts {
namespace {

// ---------------------------------------------------------------------------------------------
// gemv2: Y[b, n] (+)= act( prologue(X)[b, :] . W[n, :] + bias[n] )
//   prologue: 0 plain, 1 LayerNorm, 2 LayerNorm o LayerNorm (ln_f then final_norm)
// block = 4 waves; wave w owns RPW rows; each lane holds RPW x NCH 16-byte weight fragments in registers.
// Single-latency structure: the weight fragments, the activation rows, gamma and beta are all requested
// before anything is consumed; LayerNorm statistics are one shifted-moment pass (pivot = x[0]) reduced
// with ONE barrier; the normalised rows go to LDS for the dot-product phase.
// ---------------------------------------------------------------------------------------------
template <int NB>
struct RowStats {
  float mean[NB], rstd[NB];
};

// sum[b], sq[b] (shifted moments of this thread's elements) -> per-row mean / rstd, one barrier
template <int NB>
__device__ __forceinline__ RowStats<NB> reduce_stats(const float (&sum)[NB], const float (&sq)[NB],
                                                     const float (&pivot)[NB], int K, float eps,
                                                     float (*red)[2 * NB], int lane, int wave) {
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const float s = wave_sum(sum[b]), q = wave_sum(sq[b]);
    if (lane == 0) {
      red[wave][2 * b] = s;
      red[wave][2 * b + 1] = q;
    }
  }
  __syncthreads();
  RowStats<NB> st;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const float s = red[0][2 * b] + red[1][2 * b] + red[2][2 * b] + red[3][2 * b];
    const float q = red[0][2 * b + 1] + red[1][2 * b + 1] + red[2][2 * b + 1] + red[3][2 * b + 1];
    const float md = s / K;
    st.mean[b] = pivot[b] + md;
    st.rstd[b] = rsqrtf(fmaxf(q / K - md * md, 0.f) + eps);
  }
  return st;
}

template <typename TW, int NB, int RPW, int NCH>
__global__ __launch_bounds__(256) void gemv2_kernel(GemvArgs g) {
  constexpr int XCH = (NB * NCH + 1) / 2;  // float4 chunks of X per thread (NB*K <= NB*512*NCH floats)
  extern __shared__ __attribute__((aligned(16))) float sx[];  // [NB][K]
  __shared__ float red[2][4][2 * NB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = g.K, B = g.B, BK = B * K;
  const TW* __restrict__ W = (const TW*)g.W;
  const int n0 = (blockIdx.x * 4 + wave) * RPW;
  // 1. request everything: weight fragments, activation rows, LayerNorm parameters, pivots
  V8<TW> w[RPW][NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int k = c * 512 + lane * 8;
    if (k < K) {
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const int n = min(n0 + r, g.N - 1);
        w[r][c].load(W + (size_t)n * K + k);
      }
    }
  }
  float4 x[XCH], gm[XCH], bt[XCH], gm2[XCH], bt2[XCH];
  const bool ln = g.prologue >= 1, ln2 = g.prologue == 2;
#pragma unroll
  for (int j = 0; j < XCH; ++j) {
    const int i = tid * 4 + j * 1024;
    if (i < BK) {
      x[j] = *reinterpret_cast<const float4*>(g.X + i);
      const int col = i % K;
      gm[j] = gm2[j] = make_float4(1.f, 1.f, 1.f, 1.f);
      bt[j] = bt2[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ln && g.ln_gamma) {  // null = plain normalisation (affine folded into W by the packer)
        gm[j] = *reinterpret_cast<const float4*>(g.ln_gamma + col);
        bt[j] = *reinterpret_cast<const float4*>(g.ln_beta + col);
      }
      if (ln2 && g.ln2_gamma) {
        gm2[j] = *reinterpret_cast<const float4*>(g.ln2_gamma + col);
        bt2[j] = *reinterpret_cast<const float4*>(g.ln2_beta + col);
      }
    }
  }
  float pivot[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) pivot[b] = (ln && b < B) ? g.X[(size_t)b * K] : 0.f;
  // 2. LayerNorm(s) in registers, result to LDS
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0 ? !ln : !ln2) break;
    float sum[NB], sq[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) sum[b] = sq[b] = 0.f;
    if (pass == 1) {
#pragma unroll
      for (int b = 0; b < NB; ++b) pivot[b] = 0.f;  // LayerNorm output: mean ~ beta, well conditioned
    }
#pragma unroll
    for (int j = 0; j < XCH; ++j) {
      const int i = tid * 4 + j * 1024;
      if (i < BK) {
        const int b = i / K;
        const float v[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
#pragma unroll
        for (int bb = 0; bb < NB; ++bb)
          if (bb == b) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float d = v[e] - pivot[bb];
              sum[bb] += d;
              sq[bb] = fmaf(d, d, sq[bb]);
            }
          }
      }
    }
    const RowStats<NB> st = reduce_stats<NB>(sum, sq, pivot, K, g.ln_eps, red[pass], lane, wave);
#pragma unroll
    for (int j = 0; j < XCH; ++j) {
      const int i = tid * 4 + j * 1024;
      if (i < BK) {
        const int b = i / K;
        float m = 0.f, r = 1.f;
#pragma unroll
        for (int bb = 0; bb < NB; ++bb)
          if (bb == b) {
            m = st.mean[bb];
            r = st.rstd[bb];
          }
        const float4 G = pass ? gm2[j] : gm[j], Bt = pass ? bt2[j] : bt[j];
        x[j].x = (x[j].x - m) * r * G.x + Bt.x;
        x[j].y = (x[j].y - m) * r * G.y + Bt.y;
        x[j].z = (x[j].z - m) * r * G.z + Bt.z;
        x[j].w = (x[j].w - m) * r * G.w + Bt.w;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < XCH; ++j) {
    const int i = tid * 4 + j * 1024;
    if (i < BK) *reinterpret_cast<float4*>(sx + i) = x[j];
  }
  __syncthreads();
  if (n0 >= g.N) return;
  // 3. dot products
  float acc[RPW][NB];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int k = c * 512 + lane * 8;
    if (k < K) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b >= B) break;
        const float4 x0 = *reinterpret_cast<const float4*>(sx + b * K + k);
        const float4 x1 = *reinterpret_cast<const float4*>(sx + b * K + k + 4);
        const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[r][b] = fmaf(xv[i], w[r][c].get(i), acc[r][b]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = wave_sum(acc[r][b]);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int n = n0 + r;
      if (n >= g.N) continue;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b >= B) break;
        float v = acc[r][b] + (g.bias ? g.bias[n] : 0.f);
        v = act_apply(g.act, v);
        float* y = g.Y + (size_t)b * g.ldy + n;
        *y = g.accumulate ? (*y + v) : v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// gemv_bf16: the throughput-path GEMV (bf16 weights).  Same contract as gemv2, built from the measured
// anatomy of these 3-10 us kernels (tools/ubench_gemv.hip; DESIGN.md "decode GEMV"):
//   * branch-free: every load has a clamped address and is unconditional, so hipcc's in-order vmcnt
//     bookkeeping is exact - the activations (requested FIRST) are consumed while the weight fragments
//     (requested second) are still streaming;
//   * LayerNorm statistics with DPP row reductions (4 DPP + 2 bpermute instead of 6 bpermute);
//   * activations are kept in LDS as bf16 pairs and multiplied with v_dot2c_f32_bf16: 4 VALU ops per
//     16-byte weight fragment instead of 8 cvt + 8 fma (the kernels are short enough to be issue-bound);
//   * the output can be written as bf16 (gelu(fc) feeding proj2) to halve the next kernel's LDS fill.
// ---------------------------------------------------------------------------------------------
// PRO: 0 plain, 1 LayerNorm without affine (gamma/beta are folded into W by the packer), 2 LayerNorm(affine) then
// LayerNorm without affine (ln_f, then final_norm folded into mel_head).  XBF: X is bf16 [B, K].  YBF: Y is bf16.
// (A wave-specialised variant - dedicated activation waves - was measured slower.)
// Every batch row uses the SAME thread <-> element mapping, so a row's result does not depend on its position in
// the batch (the padding/batch invariance the reference's tests/padding_test.py checks).
// W8: weights stored as OCP fp8 e4m3 bytes with one power-of-two scale per output row (BASELINE config 5): half the
// weight stream; two v_cvt_scalef32_pk_bf16_fp8 per 4 weights feed the same v_dot2c, the row scale multiplies the sum.

// WAVES per workgroup: 4, or 5 so that the per-layer projections (3840 / 1280 / 5120 rows) split into exactly 256
// workgroups - one per CU, every CU streaming the same share of the weights and loading x once.
template <int NB, int RPW, int NCH, int PRO, bool XBF, bool YBF, bool W8 = false, int WAVES = 4>
__global__ __launch_bounds__(WAVES * 64) void gemv_bf16_kernel(GemvArgs g) {
  constexpr int NTHR = WAVES * 64;
  GEMV_STAMP(0)
  constexpr int EPC = XBF ? 8 : 4;                                  // elements per 16-byte chunk
  constexpr int KCH = (NCH * 512 + NTHR * EPC - 1) / (NTHR * EPC);  // chunks per row per thread
  extern __shared__ __attribute__((aligned(16))) uint32_t sxb[];    // [NB][K/2] bf16 pairs
  __shared__ float red[2][WAVES][2 * NB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = g.K;
  const float invK = 1.f / (float)K;  // off the critical path: the LayerNorm chain multiplies instead of dividing
  const int n0 = (blockIdx.x * WAVES + wave) * RPW;
  // ---- 1. activations (+ LayerNorm parameters) first, weights second; all unconditional ----
  u32x4 xr[NB][KCH];  // XBF: 8 bf16; else 4 floats
  f32x4 pm[PRO == 3 ? NB : 1][KCH], pl[PRO == 3 ? NB : 1][KCH], po[PRO == 3 ? NB : 1][KCH][ATTN_NSPLIT][2];
  static_assert(PRO != 3 || (XBF && ATTN_NSPLIT == 4), "prologue 3 feeds bf16 pairs and reads 4 partials as one float4");
  f32x4 gm[PRO == 2 ? KCH : 1], bt[PRO == 2 ? KCH : 1];
  bool xok[KCH];
#pragma unroll
  for (int j = 0; j < KCH; ++j) {
    const int i = (tid + j * NTHR) * EPC;
    xok[j] = i < K;
    const int ic = xok[j] ? i : K - EPC;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const size_t ro = (size_t)min(b, g.B - 1) * K + ic;
      if constexpr (PRO == 3) {
        // x is the attention output, still in ATTN_NSPLIT partials: this thread's 8 dims of head ic / 64
        const size_t bh = (size_t)min(b, g.B - 1) * (K >> 6) + (ic >> 6);
        const float* ml = g.attn_ml + bh * 2 * ATTN_NSPLIT;
        pm[b][j] = *reinterpret_cast<const f32x4*>(ml);
        pl[b][j] = *reinterpret_cast<const f32x4*>(ml + ATTN_NSPLIT);
#pragma unroll
        for (int sp = 0; sp < ATTN_NSPLIT; ++sp) {
          const float* po_ = g.attn_o + (bh * ATTN_NSPLIT + sp) * 64 + (ic & 63);
          po[b][j][sp][0] = *reinterpret_cast<const f32x4*>(po_);
          po[b][j][sp][1] = *reinterpret_cast<const f32x4*>(po_ + 4);
        }
      } else if (XBF) {
        xr[b][j] = *reinterpret_cast<const u32x4*>((const bf16_t*)g.X + ro);
      } else {
        xr[b][j] = *reinterpret_cast<const u32x4*>(g.X + ro);
      }
    }
    if (PRO == 2) {
      gm[j] = *reinterpret_cast<const f32x4*>(g.ln_gamma + ic);
      bt[j] = *reinterpret_cast<const f32x4*>(g.ln_beta + ic);
    }
  }
  float pivot[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) pivot[b] = (PRO == 1 || PRO == 2) ? g.X[(size_t)min(b, g.B - 1) * K] : 0.f;
  const bf16_t* __restrict__ W = (const bf16_t*)g.W;
  const uint8_t* __restrict__ Wq = (const uint8_t*)g.W8;
  u32x4 w[W8 ? 1 : RPW][W8 ? 1 : NCH];
  u32x2 w8[W8 ? RPW : 1][W8 ? NCH : 1];  // 8 fp8 weights per lane and chunk
  const int klast = (NCH - 1) * 512 + lane * 8;
  const bool kok = klast < K;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int k = c == NCH - 1 ? (kok ? klast : K - 8) : c * 512 + lane * 8;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      if constexpr (W8)
        w8[r][c] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(Wq + (size_t)min(n0 + r, g.N - 1) * K + k));
      else
        w[r][c] = gemv_load_w(W, min(n0 + r, g.N - 1), K, k);
    }
  }
  // epilogue operands of the output this lane will finish, (row lane / NB, batch lane % NB): bias, fp8 row scale and the
  // residual-stream value it accumulates into are requested now (youngest loads, unconditional), so the epilogue has no
  // dependent memory latency of its own
  const int er = min(lane / NB, RPW - 1), eb = lane % NB;
  const int en = min(n0 + er, g.N - 1);
  const float* bp = g.bias ? g.bias : reinterpret_cast<const float*>(W8 ? g.W8 : g.W);  // any readable address when there is no bias
  const float bpre = bp[en];
  const float spre = W8 ? g.wscale[en] : 1.f;
  const float ypre = YBF ? 0.f : g.Y[(size_t)min(eb, g.B - 1) * g.ldy + en];
  // every request of this kernel is now in flight.  The fence keeps it that way: without it the machine scheduler sinks
  // most of the weight loads below the first wait on X (fewer live registers), i.e. two thirds of the weight stream
  // would be requested one memory latency late
  __builtin_amdgcn_sched_barrier(0);
  GEMV_STAMP(1)
#ifdef ITTS_GEMV_STAMPS
  { unsigned pr_ = xr[0][0][0]; asm volatile("" ::"v"(pr_)); }
  GEMV_STAMP(2)
#endif
  // ---- 2. LayerNorm(s) in registers (one barrier each), bf16 pairs to LDS ----
  if (!XBF) {
    float xv[NB][KCH][4];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int j = 0; j < KCH; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[b][j][e] = __uint_as_float(xr[b][j][e]);
#pragma unroll
    for (int pass = 0; pass < PRO; ++pass) {
      float s[NB], q[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        s[b] = q[b] = 0.f;
        const float pv = pass == 0 ? pivot[b] : 0.f;
#pragma unroll
        for (int j = 0; j < KCH; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float d = xok[j] ? xv[b][j][e] - pv : 0.f;
            s[b] += d;
            q[b] = fmaf(d, d, q[b]);
          }
        s[b] = wave_sum_rl(s[b]);
        q[b] = wave_sum_rl(q[b]);
      }
      if (lane == 0)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          red[pass][wave][2 * b] = s[b];
          red[pass][wave][2 * b + 1] = q[b];
        }
      __syncthreads();
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float S = 0.f, Q = 0.f;
#pragma unroll
        for (int ww = 0; ww < WAVES; ++ww) {
          S += red[pass][ww][2 * b];
          Q += red[pass][ww][2 * b + 1];
        }
        // contraction pinned (decode_pinned.h): the persistent engine repeats these operations bit for bit
        const float md = __fmul_rn(S, invK);
        const float mean = __fadd_rn(pass == 0 ? pivot[b] : 0.f, md);
        const float rstd = __builtin_amdgcn_rsqf(__fadd_rn(fmaxf(ln_var_rn(Q, invK, md), 0.f), g.ln_eps));
#pragma unroll
        for (int j = 0; j < KCH; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = (xv[b][j][e] - mean) * rstd;
            if (PRO == 2 && pass == 0) v = ln_affine_rn(v, gm[j][e], bt[j][e]);  // pinned: the persistent engine's head repeats it
            xv[b][j][e] = v;
          }
      }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int j = 0; j < KCH; ++j)
        if (xok[j]) {
          const int i = (tid + j * NTHR) * 4;
          uint2 p;
          p.x = pack_bf16(xv[b][j][0], xv[b][j][1]);
          p.y = pack_bf16(xv[b][j][2], xv[b][j][3]);
          *reinterpret_cast<uint2*>(sxb + (b * K + i) / 2) = p;
        }
  } else {
    if constexpr (PRO == 3) {
      // merge the split-attention partials: weights exp(max_p - max), one division per head
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < KCH; ++j) {
          const float M = fmaxf(fmaxf(pm[b][j][0], pm[b][j][1]), fmaxf(pm[b][j][2], pm[b][j][3]));
          float wgt[ATTN_NSPLIT], L = 0.f;
#pragma unroll
          for (int sp = 0; sp < ATTN_NSPLIT; ++sp) {
            wgt[sp] = pm[b][j][sp] > -INFINITY ? __expf(pm[b][j][sp] - M) : 0.f;
            L = fmaf(wgt[sp], pl[b][j][sp], L);
          }
          const float inv = 1.f / L;
          float xm[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float a = 0.f;
#pragma unroll
            for (int sp = 0; sp < ATTN_NSPLIT; ++sp) a = fmaf(wgt[sp], po[b][j][sp][e >> 2][e & 3], a);
            xm[e] = a * inv;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) xr[b][j][e] = pack_bf16(xm[2 * e], xm[2 * e + 1]);
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int j = 0; j < KCH; ++j)
        if (xok[j]) *reinterpret_cast<u32x4*>(sxb + (b * K + (tid + j * NTHR) * 8) / 2) = xr[b][j];
  }
  __syncthreads();
  GEMV_STAMP(3)
  // ---- 3. dot products: 4 x v_dot2c per weight fragment and batch row ----
  float acc[RPW][NB];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int k = c == NCH - 1 ? (kok ? klast : K - 8) : c * 512 + lane * 8;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      u32x4 xq = *reinterpret_cast<const u32x4*>(sxb + (b * K + k) / 2);
      if (c == NCH - 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) xq[e] = kok ? xq[e] : 0u;
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        if constexpr (W8) {
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2) {
            const uint32_t q = w8[r][c][h2];  // 4 fp8: bytes 0,1 -> pair 2*h2, bytes 2,3 -> pair 2*h2 + 1
            acc[r][b] = half_dot2(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q, 1.0f, false)), xq[2 * h2], acc[r][b]);
            acc[r][b] = half_dot2(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q, 1.0f, true)), xq[2 * h2 + 1], acc[r][b]);
          }
        } else {
          acc[r][b] = gemv_dot8(w[r][c], xq, acc[r][b]);
        }
      }
    }
  }
  // wave reduction, then one lane per output: lane l < RPW * NB stores (row l / NB, batch l % NB)
  const float mine = gemv_reduce(acc, lane);
  GEMV_STAMP(4)
  if (lane < RPW * NB && n0 + er < g.N && eb < g.B) {
    const float v = gemv_out(g, mine, spre, bpre);
    const size_t o = (size_t)eb * g.ldy + en;
    if (YBF)
      ((bf16_t*)g.Y)[o] = (bf16_t)v;
    else
      g.Y[o] = g.accumulate ? ypre + v : v;
  }
  GEMV_STAMP(5)
}

// ---------------------------------------------------------------------------------------------
// gemv_wave_kernel: the same projection, but every WAVE is autonomous.  A wave needs, for its RPW weight rows, exactly
// the activations x[c*512 + lane*8 .. +8] that multiply its lane's weight fragments - so each lane loads those itself
// (L2 hits: every wave of the grid reads the same 5-20 KB), LayerNorm statistics are two DPP wave reductions per row on
// registers, and the normalised bf16 pairs feed v_dot2c directly.  No LDS, no barrier, no inter-wave dependency: the
// phase timeline of the block-cooperative kernel above (tools/ubench_gemv2.hip) showed its LayerNorm + 2 barriers on the
// critical path for 1.4 us while the weight stream had already landed, and a serial lane-0 epilogue of 0.5 us.
// The epilogue is spread over lanes: lane l < RPW*NB finishes output (row l / NB, batch l % NB) with ONE store.
// ---------------------------------------------------------------------------------------------
template <int NB, int RPW, int NCH, int PRO, bool XBF, bool YBF, bool W8>
__global__ __launch_bounds__(256) void gemv_wave_kernel(GemvArgs g) {
  GEMV_STAMP(0)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = g.K;
  const int n0 = (blockIdx.x * 4 + wave) * RPW;
  int kc[NCH];
  bool kok[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int k = c * 512 + lane * 8;
    kok[c] = k < K;
    kc[c] = kok[c] ? k : K - 8;  // clamped, in bounds; masked below
  }
  // ---- 1. every request of the wave: activations first (LayerNorm starts on them), then weights, then the epilogue operands
  u32x4 xraw[NB][NCH][XBF ? 1 : 2];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const size_t ro = (size_t)min(b, g.B - 1) * K + kc[c];
      if constexpr (XBF) {
        xraw[b][c][0] = *reinterpret_cast<const u32x4*>((const bf16_t*)g.X + ro);
      } else {
        xraw[b][c][0] = *reinterpret_cast<const u32x4*>(g.X + ro);
        xraw[b][c][1] = *reinterpret_cast<const u32x4*>(g.X + ro + 4);
      }
    }
  f32x4 gm[PRO == 2 ? NCH : 1][2], bt[PRO == 2 ? NCH : 1][2];
  if constexpr (PRO == 2) {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        gm[c][hh] = *reinterpret_cast<const f32x4*>(g.ln_gamma + kc[c] + 4 * hh);
        bt[c][hh] = *reinterpret_cast<const f32x4*>(g.ln_beta + kc[c] + 4 * hh);
      }
  }
  const bf16_t* __restrict__ W = (const bf16_t*)g.W;
  const uint8_t* __restrict__ Wq = (const uint8_t*)g.W8;
  u32x4 w[W8 ? 1 : RPW][W8 ? 1 : NCH];
  u32x2 w8[W8 ? RPW : 1][W8 ? NCH : 1];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const size_t wo = (size_t)min(n0 + r, g.N - 1) * K + kc[c];
      if constexpr (W8)
        w8[r][c] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(Wq + wo));
      else
        w[r][c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(W + wo));
    }
  // epilogue operands of the output this lane will finish: (row lane / NB, batch lane % NB)
  const int er = min(lane / NB, RPW - 1), eb = lane % NB;
  const int en = min(n0 + er, g.N - 1);
  const float* bp = g.bias ? g.bias : reinterpret_cast<const float*>(W8 ? g.W8 : g.W);  // any readable address without a bias
  const float bpre = bp[en];
  const float spre = W8 ? g.wscale[en] : 1.f;
  const float ypre = YBF ? 0.f : g.Y[(size_t)min(eb, g.B - 1) * g.ldy + en];
  __builtin_amdgcn_sched_barrier(0);  // keep all of the above in flight before the first wait (see gemv_bf16_kernel)
  GEMV_STAMP(1)
  // ---- 2. LayerNorm(s) in registers: two wave reductions per row and pass, then bf16 pairs ----
  uint32_t xq[NB][NCH][4];
  if constexpr (!XBF) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float xv[NCH][8];
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[c][e] = __uint_as_float(xraw[b][c][e >> 2][e & 3]);
#pragma unroll
      for (int pass = 0; pass < PRO; ++pass) {
        // one pass: moments about a pivot (the row's first element for the raw residual stream, 0 for a LayerNorm output),
        // both sums go through the wave reduction together
        const float pv = pass == 0 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xv[0][0]), 0)) : 0.f;
        float sm = 0.f, sq = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float d = kok[c] ? xv[c][e] - pv : 0.f;
            sm += d;
            sq = fmaf(d, d, sq);
          }
        sm = wave_sum_rl(sm);
        sq = wave_sum_rl(sq);
        const float md = sm / K;
        const float mean = pv + md;
        const float rstd = rsqrtf(fmaxf(sq / K - md * md, 0.f) + g.ln_eps);
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float v = (xv[c][e] - mean) * rstd;
            if (PRO == 2 && pass == 0) v = v * gm[c][e >> 2][e & 3] + bt[c][e >> 2][e & 3];
            xv[c][e] = v;
          }
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) xq[b][c][e] = kok[c] ? pack_bf16(xv[c][2 * e], xv[c][2 * e + 1]) : 0u;
    }
  } else {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) xq[b][c][e] = kok[c] ? xraw[b][c][0][e] : 0u;
  }
  GEMV_STAMP(3)
  // ---- 3. dot products ----
  float acc[RPW][NB];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      if constexpr (W8) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          const uint32_t q = w8[r][c][h2];
          const uint32_t lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q, 1.0f, false));
          const uint32_t hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q, 1.0f, true));
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            acc[r][b] = half_dot2(lo, xq[b][c][2 * h2], acc[r][b]);
            acc[r][b] = half_dot2(hi, xq[b][c][2 * h2 + 1], acc[r][b]);
          }
        }
      } else {
#pragma unroll
        for (int b = 0; b < NB; ++b)
          acc[r][b] = gemv_dot8(w[r][c], xq[b][c], acc[r][b]);
      }
    }
  // ---- 4. wave reduction, then one lane per output ----
  float mine = 0.f;  // (written out here: gemv_reduce changes this kernel's code)
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float t = wave_sum_rl(acc[r][b]);
      mine = lane == r * NB + b ? t : mine;
    }
  GEMV_STAMP(4)
  if (lane < RPW * NB && n0 + er < g.N && eb < g.B) {
    const float v = gemv_out(g, mine, spre, bpre);
    const size_t o = (size_t)eb * g.ldy + en;
    if (YBF)
      ((bf16_t*)g.Y)[o] = (bf16_t)v;
    else
      g.Y[o] = g.accumulate ? ypre + v : v;
  }
  GEMV_STAMP(5)
}

template <typename TW, int NB, int RPW, int NCH>
int launch_gemv2(const GemvArgs& g, hipStream_t s) {
  const int rows_per_block = 4 * RPW;
  dim3 grid((g.N + rows_per_block - 1) / rows_per_block), blk(256);
  const size_t lds = (size_t)NB * g.K * 4;
  hipLaunchKernelGGL((gemv2_kernel<TW, NB, RPW, NCH>), grid, blk, lds, s, g);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

template <typename TW, int NB>
int dispatch_gemv2(const GemvArgs& g, hipStream_t s) {
  // rows per wave chosen so the grid stays >= ~300 workgroups
  const int nch = (g.K + 511) / 512;
  if (nch <= 1) return g.N >= 4096 ? launch_gemv2<TW, NB, 4, 1>(g, s) : launch_gemv2<TW, NB, 1, 1>(g, s);
  if (nch <= 3) return g.N >= 3072 ? launch_gemv2<TW, NB, 2, 3>(g, s) : launch_gemv2<TW, NB, 1, 3>(g, s);
  if (nch <= 10) return launch_gemv2<TW, NB, 1, 10>(g, s);
  set_error("gemv2: K too large");
  return E_INVALID;
}

}  // namespace

bool gemv2_supported(const GemvArgs& g) {
  const int nb = g.B <= 2 ? g.B : 4;
  return g.B >= 1 && g.B <= 4 && g.K % 8 == 0 && g.K <= 5120 && (size_t)nb * g.K * 4 <= 64 * 1024 && g.prologue <= 2;
}

int gemv2(const GemvArgs& g, int tw, hipStream_t s) {
  ITTS_REQUIRE(g.X && g.W && g.Y && g.N > 0, "gemv2: bad args");
  ITTS_REQUIRE(gemv2_supported(g), "gemv2: unsupported shape");
#define GO(TW)                                                  \
  if (g.B == 1) return dispatch_gemv2<TW, 1>(g, s);             \
  if (g.B == 2) return dispatch_gemv2<TW, 2>(g, s);             \
  return dispatch_gemv2<TW, 4>(g, s);
  if (tw == F32) {
    GO(float)
  }
  GO(bf16_t)
#undef GO
}

static bool g_gemv_w5 = false;  // ITTS_GEMV_W5=1: 5-wave workgroups, exactly 256 of them per projection
static int g_gemv_mode = 0;  // ITTS_GEMV_MODE: 0 / 2 block-cooperative kernel (default, measured fastest), 1 wave-autonomous kernel
                             // everywhere, 3 wave-autonomous only for the short bf16-x projection

// The one table of gemv_bf16: which calls it takes, and the rows per wave / 512-column chunks / waves per workgroup each one
// gets (the prologue and the two element types are template arguments as GemvArgs states them).  Pure host arithmetic:
// itts_gemv_which exports it, tests/test_gemv_selector.py pins it.
bool gemv_bf16_pick(const GemvArgs& g, bool w5, GemvPick* p) {
  const int nch = (g.K + 511) / 512;
  if (!(g.B >= 1 && g.B <= 4 && g.K % 8 == 0 && g.K >= 64 && nch <= 10)) return false;
  if (g.x_bf16 && g.prologue == 3) {  // the merged split-attention partials: whole heads, both partial buffers
    if (g.y_bf16 || g.K % 64 != 0 || !(nch <= 1 || nch == 3) || !g.attn_o || !g.attn_ml) return false;
  } else if (g.x_bf16) {
    if (g.prologue != 0 || g.y_bf16 || nch == 2) return false;
  } else if (g.prologue == 0 || nch > 3 || (g.prologue == 2 && g.y_bf16)) {
    // (fp32 x with prologue 3 passes, as it always has; the launcher has no instantiation for it and says so)
    return false;
  }
  // the shapes of the decode step; rows per wave from the tools/ubench_gemv.hip sweep
  p->nb = g.B;
  p->nch = nch <= 1 ? 1 : nch <= 3 ? 3 : nch <= 4 ? 4 : 10;
  // gemv_bf16_kernel masks only its last chunk: every earlier one must lie inside K (fp32 x at 2 chunks would run the 3-chunk
  // kernel, bf16 x at 5-9 chunks the 10-chunk one, reading the next row's weights and activations); those calls fall to gemv2
  if (g.K < (p->nch - 1) * 512) return false;
  p->rpw = nch <= 1 ? 1 : g.prologue == 2 ? 4 : 2;  // micro configs 1, the head 4, the per-layer projections 2
  p->waves = 4;
  if (w5 && g.B <= 2) {
    // one workgroup per CU: 5 waves x RPW rows x 256 workgroups = N (3840 -> RPW 3, 5120 -> RPW 4, 1280 -> RPW 1)
    int rpw = 0;
    if (p->nch == 3 && !g.x_bf16 && g.prologue == 1) rpw = g.y_bf16 ? (g.N == 5120 ? 4 : 0) : (g.N == 3840 ? 3 : 0);  // fc, qkv
    if ((p->nch == 3 || nch == 10) && g.x_bf16 && g.N == 1280) rpw = 1;                                              // proj, proj2
    if (rpw) {
      p->rpw = rpw;
      p->waves = 5;
    }
  }
  return true;
}

bool gemv_bf16_supported(const GemvArgs& g) {
  GemvPick p;
  return gemv_bf16_pick(g, false, &p);
}

template <int NB, int RPW, int NCH, int PRO, bool XBF, bool YBF, int WAVES = 4>
static int launch_gemv_bf16(const GemvArgs& g, hipStream_t s) {
  dim3 grid((g.N + WAVES * RPW - 1) / (WAVES * RPW)), blk(WAVES * 64);
  // measured (bench, 2 rows): all block-cooperative 0.602 ms per step, all wave-autonomous 0.615 ms - the per-wave copies
  // of x cost more address-pipeline time (16 clk per KiB wave-load per CU) than the LDS hand-over and its barriers
  const bool block = WAVES != 4 || PRO == 3 || g_gemv_mode == 2 || g_gemv_mode == 0 || (g_gemv_mode == 3 && !(XBF && NCH < 4));
  const size_t lds = (size_t)NB * g.K * 2;
  if (block) {
    if (g.W8)
      hipLaunchKernelGGL((gemv_bf16_kernel<NB, RPW, NCH, PRO, XBF, YBF, true, WAVES>), grid, blk, lds, s, g);
    else
      hipLaunchKernelGGL((gemv_bf16_kernel<NB, RPW, NCH, PRO, XBF, YBF, false, WAVES>), grid, blk, lds, s, g);
  } else {
    if (g.W8)
      hipLaunchKernelGGL((gemv_wave_kernel<NB, RPW, NCH, PRO, XBF, YBF, true>), grid, blk, 0, s, g);
    else
      hipLaunchKernelGGL((gemv_wave_kernel<NB, RPW, NCH, PRO, XBF, YBF, false>), grid, blk, 0, s, g);
  }
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// the instantiations that exist, one line each: (rows per wave, chunks, waves) of the pick x (prologue, x bf16, y bf16) of the call
template <int NB>
static int dispatch_gemv_bf16(const GemvArgs& g, const GemvPick& p, hipStream_t s) {
#define GEMV_CASE(RPW, NCH, WAVES, PRO, XBF, YBF)                                                                           \
  if (p.rpw == RPW && p.nch == NCH && p.waves == WAVES && g.prologue == PRO && (g.x_bf16 != 0) == XBF && (g.y_bf16 != 0) == YBF) \
    return launch_gemv_bf16<NB, RPW, NCH, PRO, XBF, YBF, WAVES>(g, s);
  GEMV_CASE(1, 1, 4, 1, false, true)  // micro configs
  GEMV_CASE(1, 1, 4, 1, false, false)
  GEMV_CASE(1, 1, 4, 2, false, false)
  GEMV_CASE(1, 1, 4, 0, true, false)
  GEMV_CASE(1, 1, 4, 3, true, false)
  GEMV_CASE(2, 3, 4, 1, false, true)   // fc
  GEMV_CASE(2, 3, 4, 1, false, false)  // qkv
  GEMV_CASE(4, 3, 4, 2, false, false)  // head
  GEMV_CASE(2, 3, 4, 0, true, false)   // proj
  GEMV_CASE(2, 3, 4, 3, true, false)   // proj fed by split attention
  GEMV_CASE(2, 4, 4, 0, true, false)
  GEMV_CASE(2, 10, 4, 0, true, false)  // proj2
  GEMV_CASE(4, 3, 5, 1, false, true)   // ITTS_GEMV_W5 (1-2 rows): fc
  GEMV_CASE(3, 3, 5, 1, false, false)  // qkv
  GEMV_CASE(1, 3, 5, 0, true, false)   // proj
  GEMV_CASE(1, 3, 5, 3, true, false)   // proj fed by split attention
  GEMV_CASE(1, 10, 5, 0, true, false)  // proj2
#undef GEMV_CASE
  set_error("gemv_bf16: no instantiation for this shape");
  return E_INVALID;
}

int gemv_bf16(const GemvArgs& g, hipStream_t s) {
  static const bool once = [] {
    const char* m = getenv("ITTS_GEMV_MODE");
    g_gemv_mode = m ? atoi(m) : 0;
    g_gemv_w5 = getenv("ITTS_GEMV_W5") != nullptr;
    return true;
  }();
  (void)once;
  ITTS_REQUIRE((g.X || g.prologue == 3) && (g.W || g.W8) && g.Y && g.N > 0, "gemv_bf16: bad args");
  ITTS_REQUIRE(!g.W8 || g.wscale, "gemv_bf16: fp8 weights need their row scales");
  GemvPick p;
  ITTS_REQUIRE(gemv_bf16_pick(g, g_gemv_w5, &p), "gemv_bf16: unsupported shape");
  ITTS_REQUIRE(!(g.accumulate && g.y_bf16), "gemv_bf16: accumulate needs an fp32 output");
  if (p.nb == 1) return dispatch_gemv_bf16<1>(g, p, s);
  if (p.nb == 2) return dispatch_gemv_bf16<2>(g, p, s);
  if (p.nb == 3) return dispatch_gemv_bf16<3>(g, p, s);  // one sentence x 3 beams, the reference's default generate() mode
  return dispatch_gemv_bf16<4>(g, p, s);
}

}  // namespace itts

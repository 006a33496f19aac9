// Causal self-attention for APPENDED rows (the incremental packed latent pass, Engine::gpt_layers_append; itts_attention_append).
// Sequence b brings n_new[b] new queries, positions pos0[b] .. pos0[b] + n_new[b] - 1, in rows q_off[b] .. of the chunk's q / o; its
// keys and values are rows 0 .. pos0[b] + n_new[b] - 1 of its block of a K/V history (first row kv_off[b]), the new rows' k / v
// already in place (kv_rows_append_kernel below).  Query at position i sees keys 0 .. i.
//
// Two kernels, the append forms of attn_varlen_simple_kernel and attn_varlen_mfma_kernel (attention_varlen.hip) - copies, as those are
// copies of the prefill kernels; the originals are untouched.  A delivered row has the bits the varlen kernel of the same family
// gives that row in a pass over the COMPLETE sequence, because everything that row's arithmetic sees is the same:
//   - the query tiles are aligned to the sequence's key 0 (multiples of 64 for mfma, of 16 for simple): tile index pos0 / tile + x;
//   - the 64-key tiles start at key 0, and a tile's key count min(len, q0 + tile) rounds up to the same number of 64-key tiles
//     whether len is the current end or the final one (both lie in (q0, q0 + tile], inside one 64-key tile);
//   - keys behind the row's own position are masked to -inf before the softmax in both passes and enter P as exact zeros, so what the
//     pass over the complete sequence reads there (later rows) and what this one reads there (the clamped last row / zeros) meet the
//     accumulators as 0 * finite = 0;
//   - the online-softmax update, the P rounding and the store are the original's, statement for statement.
// Rows of a tile in front of pos0 are computed from a clamped (mfma) or zero (simple) query and never stored.  No key row at or
// behind pos0 + n_new is read (clamped as the original clamps to len - 1): what the history holds there may be anything.
//
// The four arrays travel by value (AppendArgs: 4 x 129 ints), checked on the host (attention_append_refusal, append_check.cpp).  A
// sequence with n_new = 0, and a workgroup whose tile lies behind its sequence's end, returns on a scalar compare before its first
// barrier.  No inter-workgroup communication, no spin wait, no atomics.
#include <algorithm>
#include <string>

#include "itts_kernels.h"

namespace itts {
namespace {

// ---- vector ALU (fp32 math): any head dim <= 128 / value dim <= 64 ----
constexpr int QB = 16;   // queries per block (4 per wave)
constexpr int KT = 64;   // keys per tile (one per lane)
constexpr int MAXDQK = 128, MAXDV = 64;

template <typename T>
__global__ __launch_bounds__(256) void attn_append_simple_kernel(AppendArgs a) {
  __shared__ float Ks[KT][MAXDQK + 1];
  __shared__ float Vs[KT][MAXDV];
  __shared__ float Qs[QB][MAXDQK];
  __shared__ float Ps[QB][KT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int nn = a.n_new[b], p0 = a.pos0[b], len = p0 + nn;
  if (nn <= 0) return;  // (uniform: nothing of this workgroup has reached a barrier)
  const int q0 = (p0 / QB + (gridDim.x - 1 - blockIdx.x)) * QB;
  if (q0 >= len) return;  // (uniform, likewise)
  // position i of the sequence is row i - p0 of its chunk rows (i >= p0) and row i of its history block
  const T* __restrict__ q = (const T*)a.q + (size_t)a.q_off[b] * a.ldq;
  const T* __restrict__ k = (const T*)a.k + (size_t)a.kv_off[b] * a.ldk;
  const T* __restrict__ v = (const T*)a.v + (size_t)a.kv_off[b] * a.ldv;
  T* __restrict__ o = (T*)a.o + (size_t)a.q_off[b] * a.ldo;

  for (int i = tid; i < QB * a.dqk; i += 256) {
    const int r = i / a.dqk, d = i - r * a.dqk;
    const int qi = q0 + r;
    Qs[r][d] = qi >= p0 && qi < len ? ldf(q + (size_t)(qi - p0) * a.ldq + h * a.dqk + d) * a.scale : 0.f;
  }
  float m[4], l[4], acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
    acc[r] = 0.f;
  }
  const int kend = min(len, q0 + QB);
  for (int j0 = 0; j0 < kend; j0 += KT) {
    __syncthreads();
    for (int i = tid; i < KT * a.dqk; i += 256) {
      const int r = i / a.dqk, d = i - r * a.dqk;
      const int j = j0 + r;
      Ks[r][d] = j < len ? ldf(k + (size_t)j * a.ldk + h * a.dqk + d) : 0.f;
    }
    for (int i = tid; i < KT * a.dv; i += 256) {
      const int r = i / a.dv, d = i - r * a.dv;
      const int j = j0 + r;
      Vs[r][d] = j < len ? ldf(v + (size_t)j * a.ldv + h * a.dv + d) : 0.f;
    }
    __syncthreads();
    const int j = j0 + lane;
    float corr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wave * 4 + r;
      const int qi = q0 + row;
      float sc = 0.f;
      for (int d = 0; d < a.dqk; ++d) sc = fmaf(Qs[row][d], Ks[lane][d], sc);
      const bool ok = j < len && qi < len && j <= qi;
      sc = ok ? sc : -INFINITY;
      const float mn = fmaxf(m[r], wave_max(sc));
      float p = 0.f;
      corr[r] = 1.f;
      if (mn > -INFINITY) {
        p = ok ? __expf(sc - mn) : 0.f;
        corr[r] = m[r] > -INFINITY ? __expf(m[r] - mn) : 0.f;
      }
      l[r] = l[r] * corr[r] + wave_sum(p);
      m[r] = mn;
      Ps[row][lane] = p;
    }
    __syncthreads();
    if (lane < a.dv) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wave * 4 + r;
        float s = 0.f;
#pragma unroll 8
        for (int jj = 0; jj < KT; ++jj) s = fmaf(Ps[row][jj], Vs[jj][lane], s);
        acc[r] = acc[r] * corr[r] + s;
      }
    }
  }
  if (lane < a.dv) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = q0 + wave * 4 + r;
      if (qi >= p0 && qi < len) stf(o + (size_t)(qi - p0) * a.ldo + h * a.dv + lane, l[r] > 0.f ? acc[r] / l[r] : 0.f);
    }
  }
}

// ---- matrix cores: 16-bit type, head dim 64.  One workgroup = 4 waves = 64 queries (16 per wave) ----
constexpr int DH = 64, QT = 64, KROW = 72;  // LDS row stride in halves (144 B: conflict-free for ds_read_b128)

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x141>(v));
  v = fmaxf(v, dpp_mov<0x140>(v));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  return v;
}

__global__ __launch_bounds__(256) void attn_append_mfma_kernel(AppendArgs a) {
  constexpr int DQK = 64, KS = DQK / 32, KQROW = DQK + 8;  // k-steps of S = Q K^T; LDS row stride of the key tile
  __shared__ __attribute__((aligned(16))) bf16_t sK[KT][KQROW];     // [key][dim]
  __shared__ __attribute__((aligned(16))) bf16_t sVt[DH][KROW];     // [dim][key]
  __shared__ __attribute__((aligned(16))) bf16_t sP[4][16][KROW];   // per wave [query][key]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int nn = a.n_new[b], p0 = a.pos0[b], len = p0 + nn;
  if (nn <= 0) return;  // (uniform: nothing of this workgroup has reached a barrier)
  const int q0 = (p0 / QT + (gridDim.x - 1 - blockIdx.x)) * QT;
  if (q0 >= len) return;  // (uniform, likewise)
  const bf16_t* __restrict__ q = (const bf16_t*)a.q + (size_t)a.q_off[b] * a.ldq;
  const bf16_t* __restrict__ k = (const bf16_t*)a.k + (size_t)a.kv_off[b] * a.ldk;
  const bf16_t* __restrict__ v = (const bf16_t*)a.v + (size_t)a.kv_off[b] * a.ldv;
  bf16_t* __restrict__ o = (bf16_t*)a.o + (size_t)a.q_off[b] * a.ldo;
  const int fr = lane & 15, fg = lane >> 4;
  // Q fragments of this wave's 16 rows (A operand: row fr, dims 32*ks + 8*fg .. +8); positions in front of pos0 read the first new
  // row, positions behind the end the last one: every row of S depends on its own Q row alone, and those rows are never stored
  const int qrow = min(max(q0 + wave * 16 + fr, p0), len - 1) - p0;
  half8_bits qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    qf[ks] = *reinterpret_cast<const half8_bits*>(q + (size_t)qrow * a.ldq + h * DQK + ks * 32 + fg * 8);
  f32x4 oacc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) oacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m[4], l[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
  }
  const int kend = min(len, q0 + QT);
  // loader mapping: thread -> key row tid/4 (64 keys), 16 dims (tid&3)*16 .. +16 (two 16-byte loads)
  const int lk = tid >> 2, ld = (tid & 3) * 16, ldk4 = (tid & 3) * (DQK / 4);
  for (int j0 = 0; j0 < kend; j0 += KT) {
    const int jr = min(j0 + lk, len - 1);
    const bf16_t* kp = k + (size_t)jr * a.ldk + h * DQK + ldk4;
    const bf16_t* vp = v + (size_t)jr * a.ldv + h * DH + ld;
    u32x4 kq[DQK / 32];
#pragma unroll
    for (int i = 0; i < DQK / 32; ++i) kq[i] = *reinterpret_cast<const u32x4*>(kp + 8 * i);
    const u32x4 v0 = *reinterpret_cast<const u32x4*>(vp), v1 = *reinterpret_cast<const u32x4*>(vp + 8);
    __syncthreads();  // previous tile fully consumed
#pragma unroll
    for (int i = 0; i < DQK / 32; ++i) *reinterpret_cast<u32x4*>(&sK[lk][ldk4 + 8 * i]) = kq[i];
    {
      const unsigned short* e0 = reinterpret_cast<const unsigned short*>(&v0);
      const unsigned short* e1 = reinterpret_cast<const unsigned short*>(&v1);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        reinterpret_cast<unsigned short*>(&sVt[ld + i][0])[lk] = e0[i];
        reinterpret_cast<unsigned short*>(&sVt[ld + 8 + i][0])[lk] = e1[i];
      }
    }
    __syncthreads();
    // ---- S = Q K^T : 4 key tiles of 16 x 2 k-steps ----
    f32x4 s[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      s[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const half8_bits kf = *reinterpret_cast<const half8_bits*>(&sK[nt * 16 + fr][ks * 32 + fg * 8]);
        s[nt] = half_mfma16(qf[ks], kf, s[nt]);
      }
    }
    // ---- mask + online softmax (rows fg*4 + r, columns fr + 16 nt) ----
    float p[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = q0 + wave * 16 + fg * 4 + r;
      float mx = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int j = j0 + nt * 16 + fr;
        const bool ok = j < len && j <= qi;
        const float sc = ok ? s[nt][r] * a.scale : -INFINITY;
        p[nt][r] = sc;
        mx = fmaxf(mx, sc);
      }
      mx = row16_max(mx);
      const float mn = fmaxf(m[r], mx);
      const float corr = mn > -INFINITY ? __expf(m[r] - mn) : 1.f;
      float sum = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float e = p[nt][r] > -INFINITY ? __expf(p[nt][r] - mn) : 0.f;
        p[nt][r] = e;
        sum += e;
      }
      sum = row16_sum(sum);
      l[r] = l[r] * corr + sum;
      m[r] = mn;
#pragma unroll
      for (int t = 0; t < 4; ++t) oacc[t][r] *= corr;
    }
    // ---- P -> wave-private LDS tile [query][key] (16-bit), then as A operand ----
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) sP[wave][fg * 4 + r][nt * 16 + fr] = (bf16_t)p[nt][r];
    __builtin_amdgcn_wave_barrier();
    half8_bits pf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) pf[ks] = *reinterpret_cast<const half8_bits*>(&sP[wave][fr][ks * 32 + fg * 8]);
    // ---- O += P V : 4 dim tiles of 16 x 2 k-steps (keys) ----
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const half8_bits vf = *reinterpret_cast<const half8_bits*>(&sVt[t * 16 + fr][ks * 32 + fg * 8]);
        oacc[t] = half_mfma16(pf[ks], vf, oacc[t]);
      }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = q0 + wave * 16 + fg * 4 + r;
    if (qi < p0 || qi >= len) continue;
    const float inv = l[r] > 0.f ? 1.f / l[r] : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[(size_t)(qi - p0) * a.ldo + h * DH + t * 16 + fr] = (bf16_t)(oacc[t][r] * inv);
  }
}

// ---- the history write: one workgroup per (new row, sequence); U = the copy unit (16 bytes where everything is aligned) ----
template <typename U>
__global__ __launch_bounds__(128) void kv_rows_append_kernel(AppendArgs a, const U* __restrict__ ksrc, const U* __restrict__ vsrc, int lds,
                                                             int wk, int wv) {  // ld* and w* in units of U
  const int b = blockIdx.y, r = blockIdx.x;
  if (r >= a.n_new[b]) return;
  const size_t src = (size_t)(a.q_off[b] + r) * lds;
  const size_t dst = (size_t)a.kv_off[b] + a.pos0[b] + r;
  U* __restrict__ kd = (U*)a.k + dst * a.ldk;
  U* __restrict__ vd = (U*)a.v + dst * a.ldv;
  for (int i = threadIdx.x; i < wk; i += 128) kd[i] = ksrc[src + i];
  for (int i = threadIdx.x; i < wv; i += 128) vd[i] = vsrc[src + i];
}

// tiles of `tile` queries, aligned to key 0, that the longest append of the call touches (0: every n_new is 0)
int append_tiles(const AppendArgs& a, int tile) {
  int mx = 0;
  for (int b = 0; b < a.nseq; ++b)
    if (a.n_new[b] > 0) mx = std::max(mx, (a.pos0[b] + a.n_new[b] - 1) / tile - a.pos0[b] / tile + 1);
  return mx;
}

}  // namespace

int attention_append(const AppendArgs& a, int dt, int kernel, hipStream_t s) {
  const char* why = attention_append_refusal(a, dt, kernel);
  ITTS_REQUIRE(!why, (std::string("attention_append: ") + why).c_str());
  const int which = kernel ? kernel : attention_append_which(a, dt);
  const int tiles = append_tiles(a, which == 2 ? QT : QB);
  if (tiles == 0) return OK;  // nothing was appended
  if (which == 2) {
    hipLaunchKernelGGL(attn_append_mfma_kernel, dim3(tiles, a.H, a.nseq), dim3(256), 0, s, a);
  } else {
    const dim3 grid(tiles, a.H, a.nseq);
    if (dt == F32)
      hipLaunchKernelGGL(attn_append_simple_kernel<float>, grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL(attn_append_simple_kernel<bf16_t>, grid, dim3(256), 0, s, a);
  }
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

int kv_rows_append(const AppendArgs& a, const void* ksrc, const void* vsrc, int lds, int wk, int wv, int dt, hipStream_t s) {
  const char* why = kv_rows_append_refusal(a, ksrc, vsrc, lds, wk, wv, dt);
  ITTS_REQUIRE(!why, (std::string("kv_rows_append: ") + why).c_str());
  int rows = 0;
  for (int b = 0; b < a.nseq; ++b) rows = std::max(rows, a.n_new[b]);
  if (rows == 0) return OK;
  const int es = dt == F32 ? 4 : 2, per = 16 / es;
  AppendArgs u = a;
  const dim3 grid(rows, a.nseq);
  const bool vec = !(lds % per) && !(wk % per) && !(wv % per) && !(a.ldk % per) && !(a.ldv % per) &&
                   !(((uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)ksrc | (uintptr_t)vsrc) & 15);
  if (vec) {
    u.ldk = a.ldk / per, u.ldv = a.ldv / per;
    hipLaunchKernelGGL(kv_rows_append_kernel<u32x4>, grid, dim3(128), 0, s, u, (const u32x4*)ksrc, (const u32x4*)vsrc, lds / per, wk / per,
                       wv / per);
  } else if (dt == F32) {
    hipLaunchKernelGGL(kv_rows_append_kernel<uint32_t>, grid, dim3(128), 0, s, u, (const uint32_t*)ksrc, (const uint32_t*)vsrc, lds, wk, wv);
  } else {
    hipLaunchKernelGGL(kv_rows_append_kernel<uint16_t>, grid, dim3(128), 0, s, u, (const uint16_t*)ksrc, (const uint16_t*)vsrc, lds, wk, wv);
  }
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace itts

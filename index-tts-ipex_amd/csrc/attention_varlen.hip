// Causal self-attention over PACKED sequences (the packed latent pass, Engine::gpt_latent_packed; itts_attention_varlen).
// Sequence b owns token rows [off[b], off[b + 1]) of q, k, v and o; query i of a sequence sees keys 0 .. i of the same sequence
// and nothing else.  There are no pad rows: a workgroup is one (query tile, head, sequence) and tiles that sequence's keys from
// the sequence's OWN key 0, so what a sequence gets does not depend on its companions, their order, or where it lies.
//
// Two kernels, each the arithmetic of the existing kernel of its family run on that sequence alone (B = 1, Sq = Sk = len,
// causal, no kv_start): attn_varlen_simple_kernel = attn_simple_kernel (attention.hip), attn_varlen_mfma_kernel =
// attn_mfma_kernel<64> (attention_mfma.hip) - the same 64-key tiles from key 0, online-softmax update, P rounding and store,
// statement for statement (copies: the two existing files are untouched).  tests/test_gpu_attention_varlen.py holds the new
// kernels to the bits of the old ones.
//
// The offsets travel by value in the argument block (at most VARLEN_MAX_SEQ + 1 ints, as the moves of rows_move_kernel and
// the slots of kv_admit_kernel do): no upload, checked on the host.  Every row index is clamped to or tested against the
// sequence's own length, so no read or store leaves [off[b], off[b + 1]).  A workgroup whose first query lies behind its
// sequence's end returns on a scalar compare before its first barrier.  blockIdx.x is reversed (the tiles with the most keys
// start first); which workgroup computes a tile changes no bit of it.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "itts_kernels.h"

namespace itts {
namespace {

// ---- vector ALU (fp32 math): any head dim <= 128 / value dim <= 64 ----
constexpr int QB = 16;   // queries per block (4 per wave)
constexpr int KT = 64;   // keys per tile (one per lane)
constexpr int MAXDQK = 128, MAXDV = 64;

template <typename T>
__global__ __launch_bounds__(256) void attn_varlen_simple_kernel(VarlenArgs a) {
  __shared__ float Ks[KT][MAXDQK + 1];
  __shared__ float Vs[KT][MAXDV];
  __shared__ float Qs[QB][MAXDQK];
  __shared__ float Ps[QB][KT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y, q0 = (gridDim.x - 1 - blockIdx.x) * QB;
  const int base = a.off[b], len = a.off[b + 1] - base;
  if (q0 >= len) return;  // (uniform: nothing of this workgroup has reached a barrier)
  const T* __restrict__ q = (const T*)a.q + (size_t)base * a.ldq;
  const T* __restrict__ k = (const T*)a.k + (size_t)base * a.ldk;
  const T* __restrict__ v = (const T*)a.v + (size_t)base * a.ldv;
  T* __restrict__ o = (T*)a.o + (size_t)base * a.ldo;

  for (int i = tid; i < QB * a.dqk; i += 256) {
    const int r = i / a.dqk, d = i - r * a.dqk;
    const int qi = q0 + r;
    Qs[r][d] = qi < len ? ldf(q + (size_t)qi * a.ldq + h * a.dqk + d) * a.scale : 0.f;
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
      if (qi < len) stf(o + (size_t)qi * a.ldo + h * a.dv + lane, l[r] > 0.f ? acc[r] / l[r] : 0.f);
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

__global__ __launch_bounds__(256) void attn_varlen_mfma_kernel(VarlenArgs a) {
  constexpr int DQK = 64, KS = DQK / 32, KQROW = DQK + 8;  // k-steps of S = Q K^T; LDS row stride of the key tile
  __shared__ __attribute__((aligned(16))) bf16_t sK[KT][KQROW];     // [key][dim]
  __shared__ __attribute__((aligned(16))) bf16_t sVt[DH][KROW];     // [dim][key]
  __shared__ __attribute__((aligned(16))) bf16_t sP[4][16][KROW];   // per wave [query][key]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y, q0 = (gridDim.x - 1 - blockIdx.x) * QT;
  const int base = a.off[b], len = a.off[b + 1] - base;
  if (q0 >= len) return;  // (uniform: nothing of this workgroup has reached a barrier)
  const bf16_t* __restrict__ q = (const bf16_t*)a.q + (size_t)base * a.ldq;
  const bf16_t* __restrict__ k = (const bf16_t*)a.k + (size_t)base * a.ldk;
  const bf16_t* __restrict__ v = (const bf16_t*)a.v + (size_t)base * a.ldv;
  bf16_t* __restrict__ o = (bf16_t*)a.o + (size_t)base * a.ldo;
  const int fr = lane & 15, fg = lane >> 4;
  // Q fragments of this wave's 16 rows (A operand: row fr, dims 32*ks + 8*fg .. +8); rows behind the sequence's end read its
  // last row (a sequence shorter than 16 rows included) and are never stored
  const int qrow = min(q0 + wave * 16 + fr, len - 1);
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
    if (qi >= len) continue;
    const float inv = l[r] > 0.f ? 1.f / l[r] : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[(size_t)qi * a.ldo + h * DH + t * 16 + fr] = (bf16_t)(oacc[t][r] * inv);
  }
}

int varlen_maxlen(const VarlenArgs& a) {
  int mx = 0;
  for (int b = 0; b < a.nseq; ++b) mx = std::max(mx, a.off[b + 1] - a.off[b]);
  return mx;
}

bool varlen_simple_forced() {
  static const bool no_mfma = getenv("ITTS_ATTN_SIMPLE") != nullptr;  // the switch of attention(): one meaning for both dispatchers
  return no_mfma;
}

}  // namespace

// The structural rule of the matrix-core kernel: type, head dims, leading dims, alignment.  No length enters it (the kernel clamps
// its Q rows, so it takes every length >= 1): a short companion cannot move another sequence onto another kernel.
bool attention_varlen_mfma_supported(const VarlenArgs& a, int dt) {
  return dt == BF16 && a.dqk == 64 && a.dv == 64 && a.ldq % 8 == 0 && a.ldk % 8 == 0 && a.ldv % 8 == 0 &&
         !(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v) & 15);
}

const char* attention_varlen_refusal(const VarlenArgs& a, int dt, int kernel) {
  if (!a.q || !a.k || !a.v || !a.o) return "null pointer (q, k, v, o, seq_off_host)";
  if (a.nseq < 1 || a.nseq > VARLEN_MAX_SEQ) return "nseq outside 1 .. 128";
  if (a.off[0] != 0) return "seq_off_host[0] must be 0";
  for (int b = 0; b < a.nseq; ++b)
    if (a.off[b + 1] <= a.off[b]) return "seq_off_host must be strictly increasing (every sequence has at least one row)";
  if (a.H < 1 || a.H > 65535) return "H is a grid dimension (1 .. 65535)";
  if (dt != F32 && dt != BF16) return "dtype must be ITTS_F32 or ITTS_BF16 (the library's 16-bit type)";
  if (a.dqk < 1 || a.dqk > 128 || a.dv < 1 || a.dv > 64) return "head dims out of range (1 <= dqk <= 128, 1 <= dv <= 64)";
  if (a.ldq < a.H * a.dqk || a.ldk < a.H * a.dqk || a.ldv < a.H * a.dv || a.ldo < a.H * a.dv)
    return "bad leading dims (ldq, ldk >= H * dqk; ldv, ldo >= H * dv)";
  if (kernel < 0 || kernel > 2) return "unknown kernel (0 dispatcher, 1 attn_varlen_simple, 2 attn_varlen_mfma)";
  if (kernel == 2 && !attention_varlen_mfma_supported(a, dt))
    return "attn_varlen_mfma needs the 16-bit type, dqk 64, dv 64, ldq / ldk / ldv % 8 == 0 and 16-byte aligned q, k, v";
  return nullptr;
}

int attention_varlen_which(const VarlenArgs& a, int dt) {
  return !varlen_simple_forced() && attention_varlen_mfma_supported(a, dt) ? 2 : 1;
}

int attention_varlen(const VarlenArgs& a, int dt, int kernel, hipStream_t s) {
  const char* why = attention_varlen_refusal(a, dt, kernel);
  ITTS_REQUIRE(!why, (std::string("attention_varlen: ") + why).c_str());
  const int which = kernel ? kernel : attention_varlen_which(a, dt);
  const int maxlen = varlen_maxlen(a);
  if (which == 2) {
    hipLaunchKernelGGL(attn_varlen_mfma_kernel, dim3((maxlen + QT - 1) / QT, a.H, a.nseq), dim3(256), 0, s, a);
  } else {
    const dim3 grid((maxlen + QB - 1) / QB, a.H, a.nseq);
    if (dt == F32)
      hipLaunchKernelGGL(attn_varlen_simple_kernel<float>, grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL(attn_varlen_simple_kernel<bf16_t>, grid, dim3(256), 0, s, a);
  }
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace itts

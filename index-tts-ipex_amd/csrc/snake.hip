// Fused anti-aliased SnakeBeta ("Activation1d"): replicate-pad -> x2 polyphase up-FIR (12 taps) ->
// x + sin^2(x*e^a)/(e^b+1e-9) -> replicate-pad -> stride-2 12-tap down-FIR, in one pass.
//
// Replaces the reference's CUDA kernel anti_alias_activation_forward
// (indextts/BigVGAN/alias_free_activation/cuda/anti_alias_activation_cuda.cu:43-181) and matches the
// torch path it mirrors (alias_free_torch/act.py:24-29, resample.py:24-33, filter.py:86-95), which is
// the parity target (SURVEY.md 2.2 "K1 caveats").
//
// MI355X design: activations are channels-last [B,T,C], so a 64-lane wave walks 64 adjacent channels
// and every load/store of a time step is one contiguous row segment.  Each lane owns one channel and
// slides along a run of RUN time steps holding the 12-sample window of activated up-sampled values
// and the 6-sample input window in registers: per output it does 2 new up-FIR phases (12 FMA), 2
// SnakeBeta evaluations and the 12-tap down-FIR (no 2x intermediate ever reaches HBM).  fp32 math,
// I/O in fp32 or bf16.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "itts_kernels.h"
#include "itts_snake_dev.h"

namespace itts {
namespace {

constexpr int RUN = 32;
constexpr int RUNL = 36;  // LDS-tiled kernel: a multiple of 6, the rotation period of its unrolled inner loop

template <typename T>
struct SnakeCtx {
  const T* __restrict__ x;  // base of this (batch, channel): element t at x[t*C]
  int Tn, C;
  float ea, inv_b;
  float fu[12], fd[12];
  __device__ __forceinline__ float xin(int t) const {
    t = t < 0 ? 0 : (t >= Tn ? Tn - 1 : t);
    return ldf(x + (size_t)t * C);
  }
  __device__ __forceinline__ float snake(float u) const {
    const float sn = __sinf(u * ea);
    return u + inv_b * sn * sn;
  }
  __device__ __forceinline__ float snake_precise(float u) const {
    const float sn = sinf(u * ea);
    return u + inv_b * sn * sn;
  }
  // activated up-sampled sample m (clamped to [0, 2T-1]) straight from global memory
  __device__ __forceinline__ float v_at(int m) const {
    m = m < 0 ? 0 : (m > 2 * Tn - 1 ? 2 * Tn - 1 : m);
    const int q = m >> 1;
    float u = 0.f;
    if (m & 1) {
#pragma unroll
      for (int r = 0; r < 6; ++r) u = fmaf(fu[2 * r], xin(q + 3 - r), u);
    } else {
#pragma unroll
      for (int r = 0; r < 6; ++r) u = fmaf(fu[2 * r + 1], xin(q + 2 - r), u);
    }
    return snake_precise(2.f * u);
  }
};

// item b of a padded ragged batch: the rows of its signal, lens[b] * mul clamped to the buffer
__device__ __forceinline__ int valid_rows(const int* __restrict__ lens, int mul, int b, int Tb) {
  const long v = (long)lens[b] * mul;
  return v < 0 ? 0 : (v > Tb ? Tb : (int)v);
}

// sentence b of a pack: the rows of its capacity and of its signal (len[b] * mul clamped to the capacity)
__device__ __forceinline__ int seg_rows(const SegTable& seg, int mul, int b) { return (seg.off[b + 1] - seg.off[b]) * mul; }
__device__ __forceinline__ int seg_valid_rows(const SegTable& seg, int mul, int b, int Tb) {
  const long v = (long)seg.len[b] * mul;
  return v < 0 ? 0 : (v > Tb ? Tb : (int)v);
}

// snake_aa_kernel (register window, any C) and snake_aa_lds_kernel (LDS-tiled, C % 8 == 0), then their length-aware forms
// snake_aa_len_kernel / snake_aa_lds_len_kernel and their segment forms snake_aa_seg_kernel / snake_aa_lds_seg_kernel: the same
// text compiled a second and a third time
#define ITTS_SNAKE_LEN 0
#include "snake_kernels_text.h"
#undef ITTS_SNAKE_LEN
#define ITTS_SNAKE_LEN 1
#include "snake_kernels_text.h"
#undef ITTS_SNAKE_LEN
#define ITTS_SNAKE_LEN 2
#include "snake_kernels_text.h"
#undef ITTS_SNAKE_LEN

template <typename T, bool FAST>
static int launch_snake_lds(void* y, const void* x, const float* la, const float* lb, const float* up12, const float* dn12,
                            int B, int Tn, int C, hipStream_t s, const int* lens = nullptr, int mul = 1) {
  int CT = C;
  if (C > 64) {
    CT = 64;
    while (C % CT) CT -= 8;
  }
  const int runs = 256 / CT, TT = runs * RUNL;
  const int tiles_t = (Tn + TT - 1) / TT, slabs = C / CT;
  const size_t lds = ((size_t)(TT + 12) * CT + (size_t)TT * CT) * sizeof(T);
  if (lens)
    hipLaunchKernelGGL((snake_aa_lds_len_kernel<T, FAST>), dim3((unsigned)((long)B * tiles_t * slabs)), dim3(256), lds, s, (T*)y,
                       (const T*)x, la, lb, up12, dn12, Tn, C, CT, tiles_t, slabs, lens, mul);
  else
    hipLaunchKernelGGL((snake_aa_lds_kernel<T, FAST>), dim3((unsigned)((long)B * tiles_t * slabs)), dim3(256), lds, s, (T*)y,
                       (const T*)x, la, lb, up12, dn12, Tn, C, CT, tiles_t, slabs);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// the segment form: grid (tiles of the longest capacity x slabs, sentences)
template <typename T, bool FAST>
static int launch_snake_lds_seg(void* y, const void* x, const float* la, const float* lb, const float* up12, const float* dn12,
                                int Tmax, int C, hipStream_t s, const SegTable& seg, int mul) {
  int CT = C;
  if (C > 64) {
    CT = 64;
    while (C % CT) CT -= 8;
  }
  const int runs = 256 / CT, TT = runs * RUNL;
  const int tiles_t = (Tmax + TT - 1) / TT, slabs = C / CT;
  const size_t lds = ((size_t)(TT + 12) * CT + (size_t)TT * CT) * sizeof(T);
  hipLaunchKernelGGL((snake_aa_lds_seg_kernel<T, FAST>), dim3((unsigned)((long)tiles_t * slabs), seg.n), dim3(256), lds, s, (T*)y,
                     (const T*)x, la, lb, up12, dn12, Tmax, C, CT, tiles_t, slabs, seg, mul);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// ---- [B,C,T] layout (the reference's native-op contract): one (b,c) row per blockIdx.y/z, LDS-staged tile ----
constexpr int BCT_TILE = 1024;

template <typename T>
__global__ __launch_bounds__(256) void snake_aa_bct_kernel(T* __restrict__ y, const T* __restrict__ x,
                                                           const float* __restrict__ la, const float* __restrict__ lb,
                                                           const float* __restrict__ up12, const float* __restrict__ dn12,
                                                           int C, int Tn) {
  __shared__ float xs[BCT_TILE + 12];
  __shared__ float vs[2 * BCT_TILE + 12];
  const int c = blockIdx.y, b = blockIdx.z;
  const int t0 = blockIdx.x * BCT_TILE;
  const int nt = min(BCT_TILE, Tn - t0);
  const T* __restrict__ xr = x + ((size_t)b * C + c) * Tn;
  T* __restrict__ yr = y + ((size_t)b * C + c) * Tn;
  const float ea = expf(la[c]);
  const float inv_b = 1.f / (expf(lb[c]) + 1e-9f);
  float fu[12], fd[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    fu[i] = up12[i];
    fd[i] = dn12[i];
  }
  for (int i = threadIdx.x; i < nt + 12; i += 256) {
    int t = t0 - 6 + i;
    t = t < 0 ? 0 : (t >= Tn ? Tn - 1 : t);
    xs[i] = ldf(xr + t);
  }
  __syncthreads();
  const int mlast = 2 * Tn - 1;
  for (int i = threadIdx.x; i < 2 * nt + 10; i += 256) {
    int m = 2 * t0 - 5 + i;
    m = m < 0 ? 0 : (m > mlast ? mlast : m);
    const int q = m >> 1;
    const int base = q - (t0 - 6);  // xs index of x[q]
    float u = 0.f;
    if (m & 1) {
#pragma unroll
      for (int r = 0; r < 6; ++r) u = fmaf(fu[2 * r], xs[base + 3 - r], u);
    } else {
#pragma unroll
      for (int r = 0; r < 6; ++r) u = fmaf(fu[2 * r + 1], xs[base + 2 - r], u);
    }
    u *= 2.f;
    const float sn = sinf(u * ea);
    vs[i] = u + inv_b * sn * sn;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nt; i += 256) {
    float o = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) o = fmaf(fd[j], vs[2 * i + j], o);
    stf(yr + t0 + i, o);
  }
}

}  // namespace

int snake_aa_bct(void* y, const void* x, const float* log_alpha, const float* log_beta, const float* up12,
                 const float* down12, int B, int C, int T, int dt, hipStream_t s) {
  ITTS_REQUIRE(y && x && log_alpha && log_beta && up12 && down12, "snake_aa_bct: null pointer");
  ITTS_REQUIRE(B > 0 && T > 0 && C > 0 && C <= 65535 && B <= 65535, "snake_aa_bct: bad dims");
  dim3 grid((T + BCT_TILE - 1) / BCT_TILE, C, B);
  if (dt == F32)
    hipLaunchKernelGGL(snake_aa_bct_kernel<float>, grid, dim3(256), 0, s, (float*)y, (const float*)x, log_alpha, log_beta,
                       up12, down12, C, T);
  else if (dt == BF16)
    hipLaunchKernelGGL(snake_aa_bct_kernel<bf16_t>, grid, dim3(256), 0, s, (bf16_t*)y, (const bf16_t*)x, log_alpha,
                       log_beta, up12, down12, C, T);
  else if (dt == F16)  // the reference dispatches float / half / bf16 (type_shim.h:20-43); fp32 arithmetic inside, as its kernel
    hipLaunchKernelGGL(snake_aa_bct_kernel<f16_t>, grid, dim3(256), 0, s, (f16_t*)y, (const f16_t*)x, log_alpha,
                       log_beta, up12, down12, C, T);
  else {
    set_error("snake_aa_bct: unsupported dtype");
    return E_INVALID;
  }
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

int snake_aa(void* y, const void* x, const float* log_alpha, const float* log_beta, const float* up12,
             const float* down12, int B, int T, int C, int dt, hipStream_t s) {
  ITTS_REQUIRE(y && x && log_alpha && log_beta && up12 && down12, "snake_aa: null pointer");
  ITTS_REQUIRE(B > 0 && T > 0 && C > 0, "snake_aa: bad dims");
  static const bool no_lds = getenv("ITTS_SNAKE_REG") != nullptr;
  if (!no_lds && C % 8 == 0 && C >= 8 && (dt == F32 || dt == BF16) && !(((uintptr_t)x | (uintptr_t)y) & 15)) {
    if (dt == F32) return launch_snake_lds<float, false>(y, x, log_alpha, log_beta, up12, down12, B, T, C, s);
    return launch_snake_lds<bf16_t, true>(y, x, log_alpha, log_beta, up12, down12, B, T, C, s);
  }
  const int nchunk = (T + RUN - 1) / RUN;
  const long total = (long)B * nchunk * C;
  const int blocks = (int)((total + 255) / 256);
  if (dt == F32)
    hipLaunchKernelGGL(snake_aa_kernel<float>, dim3(blocks), dim3(256), 0, s, (float*)y, (const float*)x, log_alpha,
                       log_beta, up12, down12, B, T, C, nchunk);
  else if (dt == BF16)
    hipLaunchKernelGGL(snake_aa_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, (bf16_t*)y, (const bf16_t*)x, log_alpha,
                       log_beta, up12, down12, B, T, C, nchunk);
  else if (dt == F16)
    hipLaunchKernelGGL(snake_aa_kernel<f16_t>, dim3(blocks), dim3(256), 0, s, (f16_t*)y, (const f16_t*)x, log_alpha,
                       log_beta, up12, down12, B, T, C, nchunk);
  else {
    set_error("snake_aa: unsupported dtype");
    return E_INVALID;
  }
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// snake_aa on a padded ragged batch: item b is the signal of its first lens[b] * mul rows (clamped to [0, T]), the rows behind it
// are written as zeros.  The first lens[b] * mul rows have the bits of snake_aa on the item cut to that length.
int snake_aa_len(void* y, const void* x, const float* log_alpha, const float* log_beta, const float* up12, const float* down12,
                 int B, int T, int C, const int* lens, int mul, int dt, hipStream_t s) {
  ITTS_REQUIRE(y && x && log_alpha && log_beta && up12 && down12 && lens, "snake_aa_len: null pointer");
  ITTS_REQUIRE(B > 0 && T > 0 && C > 0 && mul >= 1, "snake_aa_len: bad dims");
  static const bool no_lds = getenv("ITTS_SNAKE_REG") != nullptr;
  if (!no_lds && C % 8 == 0 && C >= 8 && (dt == F32 || dt == BF16) && !(((uintptr_t)x | (uintptr_t)y) & 15)) {
    if (dt == F32) return launch_snake_lds<float, false>(y, x, log_alpha, log_beta, up12, down12, B, T, C, s, lens, mul);
    return launch_snake_lds<bf16_t, true>(y, x, log_alpha, log_beta, up12, down12, B, T, C, s, lens, mul);
  }
  const int nchunk = (T + RUN - 1) / RUN;
  const long total = (long)B * nchunk * C;
  const int blocks = (int)((total + 255) / 256);
  if (dt == F32)
    hipLaunchKernelGGL(snake_aa_len_kernel<float>, dim3(blocks), dim3(256), 0, s, (float*)y, (const float*)x, log_alpha, log_beta,
                       up12, down12, B, T, C, nchunk, lens, mul);
  else if (dt == BF16)
    hipLaunchKernelGGL(snake_aa_len_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, (bf16_t*)y, (const bf16_t*)x, log_alpha,
                       log_beta, up12, down12, B, T, C, nchunk, lens, mul);
  else if (dt == F16)
    hipLaunchKernelGGL(snake_aa_len_kernel<f16_t>, dim3(blocks), dim3(256), 0, s, (f16_t*)y, (const f16_t*)x, log_alpha,
                       log_beta, up12, down12, B, T, C, nchunk, lens, mul);
  else {
    set_error("snake_aa_len: unsupported dtype");
    return E_INVALID;
  }
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// why a segment table cannot be run (null = it can): pure host code, asked by every entry that takes one before any HIP call
const char* seg_table_refusal(const SegTable& seg, int mul, int gap) {
  if (seg.n < 1 || seg.n > SEG_MAX) return "n outside [1, 128]";
  if (mul < 1) return "mul < 1";
  if (gap < 0) return "gap < 0";
  if (seg.off[0] < 0) return "off[0] < 0";
  for (int b = 0; b < seg.n; ++b) {
    if (seg.len[b] < 1) return "a length < 1";
    if (seg.off[b + 1] <= seg.off[b]) return "offsets not increasing";
    if ((long)seg.off[b + 1] - seg.off[b] < (long)seg.len[b] + gap) return "gap too small: a capacity below len + gap";
  }
  if ((long)seg.off[seg.n] * mul > 0x7fffffffL) return "the pack has more than 2^31 - 1 rows";
  return nullptr;
}

int seg_table_fill(SegTable& seg, const int* off_host, const int* lens_host, int n) {
  ITTS_REQUIRE(off_host && lens_host && n >= 1 && n <= SEG_MAX, "segment table: null pointer or n outside [1, 128]");
  seg.n = n;
  for (int b = 0; b <= n; ++b) seg.off[b] = off_host[b];
  for (int b = 0; b < n; ++b) seg.len[b] = lens_host[b];
  return OK;
}

// snake_aa over packed sentences: sentence b is rows [off[b] * mul, off[b + 1] * mul) of x / y [off[n] * mul, C], its signal the first
// len[b] * mul of them (replicate clamp at ITS last row), the rest of its capacity is written as zeros.  The signal rows have the bits
// of snake_aa on the sentence cut out; rows outside [off[0] * mul, off[n] * mul) are not touched.
int snake_aa_seg(void* y, const void* x, const float* log_alpha, const float* log_beta, const float* up12, const float* down12,
                 int C, const SegTable& seg, int mul, int dt, hipStream_t s) {
  ITTS_REQUIRE(y && x && log_alpha && log_beta && up12 && down12, "snake_aa_seg: null pointer");
  const char* why = seg_table_refusal(seg, mul, 0);
  ITTS_REQUIRE(!why, (std::string("snake_aa_seg: ") + why).c_str());
  ITTS_REQUIRE(C > 0, "snake_aa_seg: bad dims");
  int cap = 0;
  for (int b = 0; b < seg.n; ++b) cap = std::max(cap, seg.off[b + 1] - seg.off[b]);
  const long Tmax = (long)cap * mul;
  static const bool no_lds = getenv("ITTS_SNAKE_REG") != nullptr;
  if (!no_lds && C % 8 == 0 && C >= 8 && (dt == F32 || dt == BF16) && !(((uintptr_t)x | (uintptr_t)y) & 15)) {
    if (dt == F32) return launch_snake_lds_seg<float, false>(y, x, log_alpha, log_beta, up12, down12, (int)Tmax, C, s, seg, mul);
    return launch_snake_lds_seg<bf16_t, true>(y, x, log_alpha, log_beta, up12, down12, (int)Tmax, C, s, seg, mul);
  }
  const int nchunk = (int)((Tmax + RUN - 1) / RUN);
  const dim3 grid((unsigned)(((long)nchunk * C + 255) / 256), seg.n);
  if (dt == F32)
    hipLaunchKernelGGL(snake_aa_seg_kernel<float>, grid, dim3(256), 0, s, (float*)y, (const float*)x, log_alpha, log_beta, up12,
                       down12, 1, (int)Tmax, C, nchunk, seg, mul);
  else if (dt == BF16)
    hipLaunchKernelGGL(snake_aa_seg_kernel<bf16_t>, grid, dim3(256), 0, s, (bf16_t*)y, (const bf16_t*)x, log_alpha, log_beta, up12,
                       down12, 1, (int)Tmax, C, nchunk, seg, mul);
  else if (dt == F16)
    hipLaunchKernelGGL(snake_aa_seg_kernel<f16_t>, grid, dim3(256), 0, s, (f16_t*)y, (const f16_t*)x, log_alpha, log_beta, up12,
                       down12, 1, (int)Tmax, C, nchunk, seg, mul);
  else {
    set_error("snake_aa_seg: unsupported dtype");
    return E_INVALID;
  }
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace itts

// Samplers and step embedding of the launch path's decode step: sampler2_kernel (greedy), sampler_sample_kernel (do_sample=True,
// 1 <= top_k <= 128), sampler_wide_kernel (do_sample=True over the whole vocabulary: top_k < 1 or > 128),
// each with the token commit and the next step's input embedding fused in (itts_sampler_dev.h), and decode_embed2_kernel, the
// embedding of a step whose token the host supplies.
// Shared with the beam kernels of beam.hip through itts_sampler_dev.h: the candidate sort and overflow re-gather, the
// whole-vocabulary sort and block scan, commit and next embedding.  The radix select, gather, top-p and draw are this file's own text.
#include "itts_decode.h"
#include "itts_sampler_dev.h"
#include "itts_wave_dev.h"

namespace itts {
namespace {

// Mixed batches (ROWS, sampler_rows_step): row b's entry of a.rows replaces the scalar settings in this block's own copy of the
// argument block; false = a kernel of another class owns the row.  The entry goes through readfirstlane: its values are the same
// for every thread of the block, so they stay in scalar registers like the kernel arguments they replace, and the early return on
// them is taken by whole blocks - no barrier is passed by part of a block.  !ROWS: nothing is read, the kernel is what it was.
template <bool ROWS, int CLS>
__device__ __forceinline__ bool sampler_take_row(SamplerArgs& a, int b) {
  if constexpr (ROWS) {
    const int* r = reinterpret_cast<const int*>(a.rows + b);
    const int mode = __builtin_amdgcn_readfirstlane(r[0]), top_k = __builtin_amdgcn_readfirstlane(r[1]);
    if (row_class(mode, top_k) != CLS) return false;
    a.top_k = top_k;
    a.top_p = __int_as_float(__builtin_amdgcn_readfirstlane(r[2]));
    a.temperature = __int_as_float(__builtin_amdgcn_readfirstlane(r[3]));
    a.penalty = __int_as_float(__builtin_amdgcn_readfirstlane(r[4]));
  }
  return true;
}

// ---------------------------------------------------------------------------------------------
// sampler2: repetition penalty + argmax + bookkeeping, one 1024-thread block per row; the per-row length
// counter is advanced by the row's own block (no cross-block step counter, no extra launch).  (Its vectorised argmax shares
// sampler_score / sampler_commit / sampler_next_embedding only.)
// ---------------------------------------------------------------------------------------------
template <bool ROWS>
__global__ __launch_bounds__(1024) void sampler2_kernel(SamplerArgs a) {
  if (!sampler_take_row<ROWS, ROWCLS_GREEDY>(a, blockIdx.x)) return;
  __shared__ float sv[16];
  __shared__ int si[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* __restrict__ lg = a.logits + (size_t)b * a.V;
  uint8_t* seen = a.seen + (size_t)b * a.V;
  const int k_pre = a.step[b], unf_pre = a.unfinished[b];  // requested with the logits: nothing to wait for after the argmax
  float best = -INFINITY;
  int bi = 0x7fffffff;
  auto take = [&](float v, int i) {
    if (v > best || (v == best && i < bi)) {
      best = v;
      bi = i;
    }
  };
  auto score = [&](float v, int i) { return sampler_score(a, seen, v, i); };
  // 8 consecutive logits per thread as two 16-byte loads (rows are dword aligned), the tail scalar
  const int nvec = a.V >> 3;
  for (int c = tid; c < nvec; c += 1024) {
    const float4 q0 = *reinterpret_cast<const float4*>(lg + c * 8), q1 = *reinterpret_cast<const float4*>(lg + c * 8 + 4);
    const float q[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) take(score(q[e], c * 8 + e), c * 8 + e);
  }
  for (int i = nvec * 8 + tid; i < a.V; i += 1024) take(score(lg[i], i), i);
  // wave argmax without the LDS crossbar: DPP inside the 16-lane rows, v_permlane16/32_swap across them
  auto merge = [&](float ov, int oi) {
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  };
#define SAMPLER_DPP(CTRL)                                                                                  \
  merge(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(best), CTRL, 0xf, 0xf, true)),       \
        __builtin_amdgcn_update_dpp(0, bi, CTRL, 0xf, 0xf, true))
  SAMPLER_DPP(0xB1);
  SAMPLER_DPP(0x4E);
  SAMPLER_DPP(0x141);
  SAMPLER_DPP(0x140);
#undef SAMPLER_DPP
  {
    const u32x2 v16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(best), __float_as_uint(best), false, false);
    const u32x2 i16 = __builtin_amdgcn_permlane16_swap((unsigned)bi, (unsigned)bi, false, false);
    best = __uint_as_float(v16[0]);
    bi = (int)i16[0];
    merge(__uint_as_float(v16[1]), (int)i16[1]);
    const u32x2 v32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(best), __float_as_uint(best), false, false);
    const u32x2 i32 = __builtin_amdgcn_permlane32_swap((unsigned)bi, (unsigned)bi, false, false);
    best = __uint_as_float(v32[0]);
    bi = (int)i32[0];
    merge(__uint_as_float(v32[1]), (int)i32[1]);
  }
  if (lane == 0) {
    sv[wave] = best;
    si[wave] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w)
      if (sv[w] > best || (sv[w] == best && si[w] < bi)) {
        best = sv[w];
        bi = si[w];
      }
    sampler_commit(a, b, bi, si, k_pre, unf_pre);
  }
  __syncthreads();
  sampler_next_embedding(a, b, si, tid);
}

// ---------------------------------------------------------------------------------------------
// sampler_sample: the do_sample=True path of HF 4.36.2 GenerationMixin.sample as infer.py:116-124 configures it
// (RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax ->
// multinomial), one 1024-thread block per row.  Scores live in LDS; the k-th largest score is found by a 4-pass
// radix select on order-preserving keys (no sort of the vocabulary), the <= 128 survivors are bitonic-sorted by one
// wave, top-p and the draw run serially over them in the order torch.cumsum uses.
// ---------------------------------------------------------------------------------------------
template <bool ROWS>
__global__ __launch_bounds__(1024) void sampler_sample_kernel(SamplerArgs a) {
  if (!sampler_take_row<ROWS, ROWCLS_NARROW>(a, blockIdx.x)) return;
  extern __shared__ float ssc[];  // [V] processed scores
  __shared__ unsigned hist[256];
  __shared__ int s_bin, s_k, s_cnt;
  __shared__ float cval[BEAM_MAX_CAND];
  __shared__ int cidx[BEAM_MAX_CAND];
  __shared__ int si[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const float* __restrict__ lg = a.logits + (size_t)b * a.V;
  const uint8_t* seen = a.seen + (size_t)b * a.V;
  const int k_pre = a.step[b], unf_pre = a.unfinished[b];
  for (int i = tid; i < a.V; i += 1024) {
    float v = sampler_score(a, seen, lg[i], i);
    if (a.temperature != 1.f) v = v / a.temperature;  // TemperatureLogitsWarper: scores / temperature
    ssc[i] = v;
  }
  // ---- radix select: key of the top_k-th largest score ----
  unsigned prefix = 0;
  int kk = min(a.top_k, a.V);
  for (int pass = 3; pass >= 0; --pass) {
    const int shift = pass * 8;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < a.V; i0 += 1024) {  // every lane takes part in every round (wave-aggregated atomics)
      const int i = i0 + tid;
      const unsigned key = i < a.V ? order_key(ssc[i]) : 0u;
      const bool act = i < a.V && (pass == 3 || (key >> (shift + 8)) == (prefix >> (shift + 8)));
      hist_add_wave(hist, (key >> shift) & 255u, act, lane);
    }
    __syncthreads();
    if (tid < 64) {
      const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
      const unsigned own = h0 + h1 + h2 + h3;
      unsigned x = own;  // inclusive suffix sum over lanes (higher lanes = larger keys)
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_down(x, off, 64);
        if (lane + off < 64) x += t;
      }
      const unsigned above = x - own;
      if (above < (unsigned)kk && (unsigned)kk <= x) {  // exactly one lane
        unsigned acc = above;
        int bin = 4 * lane + 3;
        const unsigned hb[4] = {h0, h1, h2, h3};
#pragma unroll
        for (int j = 3; j >= 0; --j) {
          if (acc + hb[j] >= (unsigned)kk) {
            bin = 4 * lane + j;
            break;
          }
          acc += hb[j];
        }
        s_bin = bin;
        s_k = kk - (int)acc;
      }
    }
    __syncthreads();
    prefix |= (unsigned)s_bin << shift;
    kk = s_k;
  }
  // ---- gather the survivors (score >= k-th largest; ties kept as HF's `scores < kth` mask keeps them, up to BEAM_MAX_CAND) ----
  if (tid == 0) s_cnt = 0;
  if (tid < BEAM_MAX_CAND) {
    cval[tid] = -INFINITY;
    cidx[tid] = 0x7fffffff;
  }
  __syncthreads();
  for (int i = tid; i < a.V; i += 1024) {
    const float v = ssc[i];
    // -inf scores never count: with fewer than top_k finite scores HF's `scores < kth` (kth = -inf) keeps exactly the finite ones
    if (order_key(v) >= prefix && v > -INFINITY) {
      const int pos = atomicAdd(&s_cnt, 1);
      if (pos < BEAM_MAX_CAND) {
        cval[pos] = v;
        cidx[pos] = i;
      }
    }
  }
  __syncthreads();
  if (s_cnt > BEAM_MAX_CAND) regather_cands_ordered(ssc, a.V, prefix, cval, cidx, &s_cnt, tid);  // block-uniform: ties with the k-th score
  if (tid < 64) sort_cands_wave<true>(cval, cidx, lane);  // one wave, no barrier: descending score, ascending index on ties
  __syncthreads();
  if (tid < 64) {
    // wave 0: the exponentials and quotients in parallel (lane r and r + 64 of the sorted candidates), the running sums
    // sequentially in the restatement's order, every lane carrying them (values broadcast lane by lane)
    const int n = min(s_cnt, BEAM_MAX_CAND);
    const float m = cval[0];
    const float e0 = lane < n ? expf(cval[lane] - m) : 0.f, e1 = lane + 64 < n ? expf(cval[lane + 64] - m) : 0.f;
    auto ev = [&](int r) { return r < 64 ? lane_val(e0, r) : lane_val(e1, r - 64); };
    float Z = 0.f;
    for (int r = 0; r < n; ++r) Z += ev(r);
    int R = n;
    if (a.top_p < 1.f) {
      // TopPLogitsWarper: ascending cumulative probability <= 1 - top_p is removed; the best token always stays
      const float t0 = e0 / Z, t1 = e1 / Z;
      float tail = 0.f;
      R = 1;
      for (int r = n - 1; r >= 1; --r) {
        tail += r < 64 ? lane_val(t0, r) : lane_val(t1, r - 64);
        if (!(tail <= 1.f - a.top_p)) {
          R = r + 1;
          break;
        }
      }
    }
    float total = 0.f;
    for (int r = 0; r < R; ++r) total += ev(r);
    const int k = k_pre;
    const float u = a.uniforms[(size_t)min(k, a.max_gen - 1) * a.B + b];
    const float target = u * total;
    int pick = R - 1;
    float c = 0.f;
    for (int r = 0; r < R; ++r) {
      c += ev(r);
      if (c >= target) {
        pick = r;
        break;
      }
    }
    if (lane == 0) sampler_commit(a, b, cidx[pick], si, k_pre, unf_pre);
  }
  __syncthreads();
  sampler_next_embedding(a, b, si, tid);
}

// ---------------------------------------------------------------------------------------------
// sampler_wide: the same HF 4.36.2 sample() step when the TopK warper is off (top_k < 1) or wider than the 128 candidates
// sampler_sample_kernel keeps (top_k > 128): thousands of tokens can survive, so the whole vocabulary is sorted.  One
// 1024-thread block per row, V <= 16384:
//   1. scores (sampler_score, / temperature) and ids into LDS, padded to NP = the power of two >= max(V, 1024)
//   2. block bitonic sort: descending score, lower id first on ties; -inf scores and the padding sort last and never count
//   3. TopK (top_k >= 1 only): the n ranks whose score is >= the score at rank min(top_k, V) - 1 stay (ties with it stay, as
//      HF's `scores < kth` mask keeps them); without TopK the n finite scores
//   4. TopP (top_p < 1): e_r = expf(s_r - s_0); rank r >= 1 goes iff tail_r = sum_{j >= r} e_j <= (1 - top_p) * tail_0
//   5. draw: the first of the R kept ranks whose inclusive prefix sum of e is >= u * (the sum over the R ranks), else R - 1
//   6. sampler_commit / sampler_next_embedding, as in the other samplers
// Sums: every thread owns a run of NP / 1024 (<= 16) consecutive ranks; tail_r and the prefix sums are block scans of the run
// sums (wave scan by shuffles, then the sums of the other waves in wave order) finished inside the run - no fp32 atomics, the
// same bits on every run and in every batch.  The longest chain of dependent fp32 additions behind any sum is 53: <= 15 for
// a run's own sum, 6 levels of the wave scan, <= 15 wave sums, 1 to join them with the wave's part, <= 16 along the run.
// ---------------------------------------------------------------------------------------------
constexpr int WIDE_MAX_V = 16384;  // NP * 6 bytes of LDS: 96 KiB

template <bool ROWS>
__global__ __launch_bounds__(1024) void sampler_wide_kernel(SamplerArgs a, int NP) {
  if (!sampler_take_row<ROWS, ROWCLS_WIDE>(a, blockIdx.x)) return;
  extern __shared__ unsigned char wsm[];
  float* keys = reinterpret_cast<float*>(wsm);                                     // [NP] scores, sorted in place
  unsigned short* idx = reinterpret_cast<unsigned short*>(wsm + (size_t)NP * 4);  // [NP] their token ids
  __shared__ float wsum_tail[16], wsum_pre[16];
  __shared__ float s_thr, s_total;
  __shared__ int s_n, s_R, s_pick;
  __shared__ int si[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = a.V;
  const float* __restrict__ lg = a.logits + (size_t)b * V;
  const uint8_t* seen = a.seen + (size_t)b * V;
  const int k_pre = a.step[b], unf_pre = a.unfinished[b];
  const float u = a.uniforms[(size_t)min(k_pre, a.max_gen - 1) * a.B + b];
  if (tid == 0) {
    s_n = 0;
    s_R = 1;  // the best token always stays
    s_pick = 0x7fffffff;
  }
  for (int i = tid; i < NP; i += 1024) {
    float v = -INFINITY;
    if (i < V) {
      v = sampler_score(a, seen, lg[i], i);
      if (a.temperature != 1.f) v = v / a.temperature;  // TemperatureLogitsWarper: scores / temperature
      v = v > -INFINITY ? v : -INFINITY;                 // (a NaN would leave the sort without an order)
    }
    keys[i] = v;
    idx[i] = (unsigned short)(i < V ? i : 0xFFFF);  // the padding sorts behind every -inf score
  }
  __syncthreads();
  wide_sort<true>(keys, idx, NP, tid);  // descending score, ascending id on ties
  // ---- TopK: the kept ranks are a prefix [0, n) of the sorted order ----
  const int per = NP >> 10, r0 = tid * per;  // this thread's run of ranks
  const float s0 = keys[0];
  const float kth = a.top_k >= 1 ? keys[min(a.top_k, V) - 1] : -INFINITY;
  float e[16];
  int nk = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    e[q] = 0.f;
    if (q < per) {
      const float v = keys[r0 + q];
      if (v >= kth && v > -INFINITY) {
        e[q] = expf(v - s0);
        ++nk;
      }
    }
  }
  if (nk) atomicAdd(&s_n, nk);
  __syncthreads();
  const int n = max(s_n, 1);  // (no finite score at all: rank 0, the lowest id, is drawn)
  // ---- TopP: tail_r by a block scan from the last rank down ----
  int R = n;
  if (a.top_p < 1.f) {  // block-uniform
    float mine = 0.f;
#pragma unroll
    for (int q = 15; q >= 0; --q)
      if (q < per) mine += e[q];
    const float base = wide_scan_excl<true>(mine, wsum_tail, lane, wave);
    if (tid == 0) {
      float c = base;
#pragma unroll
      for (int q = 15; q >= 0; --q)
        if (q < per) c += e[q];
      s_thr = (1.f - a.top_p) * c;  // c = tail_0 = Z
    }
    __syncthreads();
    const float thr = s_thr;
    float c = base;
    int rmax = 0;
#pragma unroll
    for (int q = 15; q >= 0; --q)
      if (q < per) {
        c += e[q];
        const int r = r0 + q;
        if (r >= 1 && r < n && !(c <= thr)) rmax = max(rmax, r + 1);
      }
    if (rmax) atomicMax(&s_R, rmax);
    __syncthreads();
    R = s_R;
  }
  // ---- draw: inverse CDF of u over the R kept ranks ----
  float mine = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q)
    if (q < per) {
      if (r0 + q >= R) e[q] = 0.f;
      mine += e[q];
    }
  const float base = wide_scan_excl<false>(mine, wsum_pre, lane, wave);
  {
    float c = base;
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (q < per) {
        c += e[q];
        if (r0 + q == R - 1) s_total = c;
      }
  }
  __syncthreads();
  const float target = u * s_total;
  {
    float c = base;
    int first = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (q < per) {
        c += e[q];
        if (r0 + q < R && c >= target) first = min(first, r0 + q);
      }
    if (first != 0x7fffffff) atomicMin(&s_pick, first);
  }
  __syncthreads();
  if (tid == 0) {
    const int pick = min(s_pick, R - 1);
    if (a.kept) a.kept[b] = R;
    sampler_commit(a, b, idx[pick], si, k_pre, unf_pre);
  }
  __syncthreads();
  sampler_next_embedding(a, b, si, tid);
}

template <typename TW>
__global__ void decode_embed2_kernel(float* __restrict__ h, const TW* __restrict__ emb, const TW* __restrict__ pos,
                                     const int* __restrict__ tok, const int* __restrict__ len, int D) {
  const int b = blockIdx.x;
  const int t = tok[b];
  const int p = len[b] + 1;  // positions 0, 2, 3, ... (model.py:153-155)
  for (int i = threadIdx.x; i < D; i += blockDim.x)
    h[(size_t)b * D + i] = ldf(emb + (size_t)t * D + i) + ldf(pos + (size_t)p * D + i);
}

}  // namespace

// sampler_wide_kernel's 96 KiB of dynamic LDS have to be allowed once on every device ordinal that launches it; gpt_prefill
// calls this outside the capture of the decode step
int sampler_wide_prepare() {
  static DynLdsLatch latch, latch_rows;  // both instantiations: the scalar form and the one of mixed batches
  ITTS_TRY(allow_dynamic_lds(latch, (const void*)sampler_wide_kernel<false>, WIDE_MAX_V * 6));
  return allow_dynamic_lds(latch_rows, (const void*)sampler_wide_kernel<true>, WIDE_MAX_V * 6);
}

int sampler2_step(const SamplerArgs& a, int B, hipStream_t s) {
  ITTS_REQUIRE(!a.rows, "sampler: a row table runs through sampler_rows_step");
  if (a.do_sample) {
    ITTS_REQUIRE(a.uniforms && a.temperature > 0.f && a.top_p > 0.f && a.B == B,
                 "sampler: sampling needs uniforms, temperature > 0, top_p > 0");
    if (a.top_k >= 1 && a.top_k <= BEAM_MAX_CAND) {
      ITTS_REQUIRE((size_t)a.V * 4 <= 60 * 1024, "sampler: vocabulary too large for the LDS-resident sampler");
      hipLaunchKernelGGL(sampler_sample_kernel<false>, dim3(B), dim3(1024), (size_t)a.V * 4, s, a);
    } else {  // TopK off or wider than the narrow kernel's candidates: the whole vocabulary
      ITTS_REQUIRE(a.V >= 1 && a.V <= WIDE_MAX_V, "sampler: top_k outside [1, 128] needs a vocabulary of at most 16384");
      ITTS_TRY(sampler_wide_prepare());
      int np = 1024;
      while (np < a.V) np <<= 1;
      hipLaunchKernelGGL(sampler_wide_kernel<false>, dim3(B), dim3(1024), (size_t)np * 6, s, a, np);
    }
    ITTS_HIP_CHECK(hipGetLastError());
    return OK;
  }
  hipLaunchKernelGGL(sampler2_kernel<false>, dim3(B), dim3(1024), 0, s, a);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// Mixed batch: every class present gets its kernel over the whole grid; row b's block does its work in the kernel of rows[b]'s
// class and returns at once in the others, so the commit and the next-step embedding of every row run exactly once.  The
// launches follow one another on the stream and touch disjoint rows.  `classes`: what the caller's host copy of the table holds
// (bit ROWCLS_*); the entries themselves were checked where the table was built (c_api.cpp, Engine::gpt_set_sampling_rows).
int sampler_rows_step(const SamplerArgs& a, int B, int classes, hipStream_t s) {
  ITTS_REQUIRE(a.rows && a.B == B && classes > 0 && classes < 8, "sampler: a mixed batch needs its row table and the classes present");
  const bool narrow = classes >> ROWCLS_NARROW & 1, wide = classes >> ROWCLS_WIDE & 1;
  ITTS_REQUIRE(!(narrow || wide) || a.uniforms, "sampler: sampled rows need uniforms");
  ITTS_REQUIRE(!narrow || (size_t)a.V * 4 <= 60 * 1024, "sampler: vocabulary too large for the LDS-resident sampler");
  ITTS_REQUIRE(!wide || (a.V >= 1 && a.V <= WIDE_MAX_V), "sampler: top_k outside [1, 128] needs a vocabulary of at most 16384");
  if (wide) ITTS_TRY(sampler_wide_prepare());
  if (classes >> ROWCLS_GREEDY & 1) hipLaunchKernelGGL(sampler2_kernel<true>, dim3(B), dim3(1024), 0, s, a);
  if (narrow) hipLaunchKernelGGL(sampler_sample_kernel<true>, dim3(B), dim3(1024), (size_t)a.V * 4, s, a);
  if (wide) {
    int np = 1024;
    while (np < a.V) np <<= 1;
    hipLaunchKernelGGL(sampler_wide_kernel<true>, dim3(B), dim3(1024), (size_t)np * 6, s, a, np);
  }
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// One row's token choice (row admission, Engine::gpt_admit_rows): the same kernels with a grid of one block on an argument block
// whose per-row pointers start at the slot, so block 0 is that row.  uniforms[k * a.B + 0] of the advanced base is
// uniforms[k * B + slot] of the batch.  a.rows set: the <true> instantiations, which read the slot's own entry.
int sampler_slot_step(const SamplerArgs& a0, int slot, int cls, hipStream_t s) {
  ITTS_REQUIRE(slot >= 0 && slot < a0.B && cls >= ROWCLS_GREEDY && cls <= ROWCLS_WIDE, "sampler: slot outside the batch, or no such class");
  SamplerArgs a = a0;
  a.logits += (size_t)slot * a.V;
  a.seen += (size_t)slot * a.V;
  a.ids += (size_t)slot * a.max_gen;
  a.cur_tok += slot;
  a.unfinished += slot;
  a.step += slot;
  if (a.h_next) a.h_next += (size_t)slot * a.D;
  if (a.forced) a.forced += (size_t)slot * a.max_gen;
  if (a.uniforms) a.uniforms += slot;
  if (a.kept) a.kept += slot;
  if (a.rows) a.rows += slot;
  const bool rows = a.rows != nullptr;
  if (cls == ROWCLS_GREEDY) {
    if (rows) hipLaunchKernelGGL(sampler2_kernel<true>, dim3(1), dim3(1024), 0, s, a);
    else hipLaunchKernelGGL(sampler2_kernel<false>, dim3(1), dim3(1024), 0, s, a);
  } else {
    ITTS_REQUIRE(a.uniforms, "sampler: a sampled row needs uniforms");
    if (cls == ROWCLS_NARROW) {
      ITTS_REQUIRE((size_t)a.V * 4 <= 60 * 1024, "sampler: vocabulary too large for the LDS-resident sampler");
      if (rows) hipLaunchKernelGGL(sampler_sample_kernel<true>, dim3(1), dim3(1024), (size_t)a.V * 4, s, a);
      else hipLaunchKernelGGL(sampler_sample_kernel<false>, dim3(1), dim3(1024), (size_t)a.V * 4, s, a);
    } else {
      ITTS_REQUIRE(a.V >= 1 && a.V <= WIDE_MAX_V, "sampler: top_k outside [1, 128] needs a vocabulary of at most 16384");
      ITTS_TRY(sampler_wide_prepare());
      int np = 1024;
      while (np < a.V) np <<= 1;
      if (rows) hipLaunchKernelGGL(sampler_wide_kernel<true>, dim3(1), dim3(1024), (size_t)np * 6, s, a, np);
      else hipLaunchKernelGGL(sampler_wide_kernel<false>, dim3(1), dim3(1024), (size_t)np * 6, s, a, np);
    }
  }
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

int decode_embed2(float* h, const void* emb, const void* pos, const int* tok, const int* len, int B, int D, int tw,
                  hipStream_t s) {
  if (tw == F32)
    hipLaunchKernelGGL(decode_embed2_kernel<float>, dim3(B), dim3(256), 0, s, h, (const float*)emb, (const float*)pos, tok, len, D);
  else
    hipLaunchKernelGGL(decode_embed2_kernel<bf16_t>, dim3(B), dim3(256), 0, s, h, (const bf16_t*)emb, (const bf16_t*)pos, tok, len, D);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace itts

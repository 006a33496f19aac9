// Device-side bookkeeping shared by the sampler kernels (decode_sampler.hip) and the persistent decode engine's in-launch greedy
// sampler (decode_engine.hip): HF greedy search / sample() commit of one token per row + the next step's input embedding.
// sampler_sample_kernel (decode_sampler.hip) and beam_cand_kernel (beam.hip) share sort_cands_wave: one order, one tie rule.
#pragma once
#include "itts_decode.h"
#include "itts_wave_dev.h"

namespace itts {

// repetition penalty (RepetitionPenaltyLogitsProcessor over the row's id history, kept as a byte map) + stop suppression
__device__ __forceinline__ float sampler_score(const SamplerArgs& a, const uint8_t* seen_row, float v, int i) {
  if (a.preprocessed) return v;
  if (a.penalty != 1.f && seen_row[i]) v = v < 0.f ? v * a.penalty : v / a.penalty;
  if (a.suppress_stop && i == a.stop) v = -INFINITY;
  return v;
}

// bookkeeping shared by the greedy and the sampling kernels (thread 0 of the row's block)
__device__ __forceinline__ void sampler_commit(const SamplerArgs& a, int b, int choice, int* si, int k, int unf) {
  si[1] = -1;
  if (k < a.max_gen) {  // graph replays past the end are no-ops
    if (a.forced) {
      const int f = a.forced[(size_t)b * a.max_gen + k];
      choice = f >= 0 ? f : choice;
    }
    int tok = unf ? choice : a.stop;
    tok = tok < 0 ? 0 : (tok >= a.V ? a.V - 1 : tok);  // never index seen[] / emb[] outside the vocabulary
    a.ids[(size_t)b * a.max_gen + k] = tok;
    a.cur_tok[b] = tok;
    a.seen[(size_t)b * a.V + tok] = 1;
    a.unfinished[b] = unf && tok != a.stop;
    a.step[b] = k + 1;
    si[0] = tok;
    // position of the token fed at the next step: 0, 2, 3, ... (model.py:153-155); a given `input_tokens` token k was part of
    // the reference's first forward, at position k + 1 (model.py:141-144)
    si[1] = k < a.input_n ? k + 1 : k + 2;
  }
}

// next step's input row h[b] = mel_emb[tok] + mel_pos[k + 2], fused here (one launch less per token)
__device__ __forceinline__ void sampler_next_embedding(const SamplerArgs& a, int b, const int* si, int tid) {
  if (a.h_next && si[1] > 0) {
    const int tok = si[0], p = min(si[1], a.pos_rows - 1);
    for (int i = tid; i < a.D; i += 1024) {
      float v;
      if (a.emb_bf16)
        v = (float)((const bf16_t*)a.emb)[(size_t)tok * a.D + i] + (float)((const bf16_t*)a.pos)[(size_t)p * a.D + i];
      else
        v = ((const float*)a.emb)[(size_t)tok * a.D + i] + ((const float*)a.pos)[(size_t)p * a.D + i];
      a.h_next[(size_t)b * a.D + i] = v;
    }
  }
}

// bitonic sort of BEAM_MAX_CAND (value, index) pairs in LDS by ONE wave (lanes 0..63 = the BEAM_MAX_CAND / 2 comparators of a stage): a
// wave's LDS operations execute in program order, so the 28 stages need no workgroup barrier (at 16 waves each barrier
// costs ~0.4 us and the block form spent 11 us per sort); the fence only pins the compiler's order.
// BY_SCORE: descending value, ascending index on ties; else ascending index.
template <bool BY_SCORE>
__device__ __forceinline__ void sort_cands_wave(float* cv, int* ci, int lane) {
  static_assert(BEAM_MAX_CAND == 128, "one comparator per lane");
  for (int kq = 2; kq <= BEAM_MAX_CAND; kq <<= 1)
    for (int j = kq >> 1; j > 0; j >>= 1) {
      const int lo = ((lane & ~(j - 1)) << 1) | (lane & (j - 1)), hi = lo | j;
      const bool up = (lo & kq) == 0;
      const float v0 = cv[lo], v1 = cv[hi];
      const int i0 = ci[lo], i1 = ci[hi];
      const bool second_first = BY_SCORE ? (v1 > v0 || (v1 == v0 && i1 < i0)) : (i1 < i0);
      if (second_first == up) {
        cv[lo] = v1;
        cv[hi] = v0;
        ci[lo] = i1;
        ci[hi] = i0;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

// More than BEAM_MAX_CAND scores reached the k-th largest (ties with it): the atomic gather of sampler_sample_kernel / beam_cand_kernel
// then kept whichever BEAM_MAX_CAND arrived first, and a strictly larger score could be lost.  Gather again in the order of the
// restatement (oracle/hf_beam.py warp_row: score descending, id ascending, [:128]): every score strictly above the k-th - fewer than
// top_k <= BEAM_MAX_CAND of them, in any order, the sort behind this puts them in place - then wave 0 walks the vocabulary upwards
// and appends the ties in ascending id until the arrays are full.  Every thread of the block calls it, behind the barrier that
// follows the gather; *cnt is BEAM_MAX_CAND afterwards.  kth_key: order_key of the k-th largest score (the radix select's prefix).
__device__ __forceinline__ void regather_cands_ordered(const float* sc, int V, unsigned kth_key, float* cv, int* ci, int* cnt, int tid) {
  __syncthreads();  // every thread has read the overflowing count
  if (tid == 0) *cnt = 0;
  __syncthreads();
  for (int i = tid; i < V; i += 1024) {
    const float v = sc[i];
    if (order_key(v) > kth_key) {
      const int p = atomicAdd(cnt, 1);
      if (p < BEAM_MAX_CAND) {  // (always: fewer than top_k scores lie above the k-th)
        cv[p] = v;
        ci[p] = i;
      }
    }
  }
  __syncthreads();
  if (tid < 64) {
    int n = *cnt;
    for (int i0 = 0; i0 < V && n < BEAM_MAX_CAND; i0 += 64) {  // wave-uniform
      const int i = i0 + tid;
      const bool tie = i < V && order_key(sc[i]) == kth_key;
      const unsigned long long m = __ballot(tie);
      const int p = n + __popcll(m & ((1ull << tid) - 1ull));
      if (tie && p < BEAM_MAX_CAND) {
        cv[p] = sc[i];
        ci[p] = i;
      }
      n += __popcll(m);
    }
    if (tid == 0) *cnt = BEAM_MAX_CAND;
  }
  __syncthreads();
}

// ---- shared by the whole-vocabulary samplers: sampler_wide_kernel (decode_sampler.hip), beam_wide_cand_kernel /
//      beam_wide_pick_kernel (beam.hip) - one sort order, one tie rule, one summation structure ----

// exclusive block scan of one value per thread in thread order (REV: from the last thread down); one barrier
template <bool REV>
__device__ __forceinline__ float wide_scan_excl(float mine, float* wsum, int lane, int wave) {
  float inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = REV ? __shfl_down(inc, o, 64) : __shfl_up(inc, o, 64);
    if (REV ? lane + o < 64 : lane >= o) inc += t;
  }
  float ex = REV ? __shfl_down(inc, 1, 64) : __shfl_up(inc, 1, 64);
  if (lane == (REV ? 63 : 0)) ex = 0.f;
  if (lane == (REV ? 0 : 63)) wsum[wave] = inc;
  __syncthreads();
  float wb = 0.f;
  if (REV) {
    for (int w = 15; w > wave; --w) wb += wsum[w];
  } else {
    for (int w = 0; w < wave; ++w) wb += wsum[w];
  }
  return wb + ex;
}

// block bitonic sort of NP (a power of two >= 1024) (score, u16 id) pairs in LDS by 1024 threads: descending score, ascending
// id on ties.  The caller has put a barrier behind its writes of keys / idx; the sort ends with one
__device__ __forceinline__ void wide_sort_desc(float* keys, unsigned short* idx, int NP, int tid) {
  auto compare_swap = [&](int t, int j, int kk) {
    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
    const bool up = (lo & kk) == 0;
    const float k0 = keys[lo], k1 = keys[hi];
    const unsigned short i0 = idx[lo], i1 = idx[hi];
    const bool behind = k0 < k1 || (k0 == k1 && i0 > i1);  // entry lo belongs behind entry hi
    if (behind == up) {
      keys[lo] = k1;
      keys[hi] = k0;
      idx[lo] = i1;
      idx[hi] = i0;
    }
  };
  for (int kk = 2; kk <= NP; kk <<= 1) {
    int j = kk >> 1;
    for (; j > 64; j >>= 1) {
      for (int t = tid; t < NP / 2; t += 1024) compare_swap(t, j, kk);
      __syncthreads();
    }
    // j <= 64: the 64 comparators of a wave stay inside 128 entries no other wave touches, and a wave's LDS operations
    // execute in program order (sort_cands_wave): these stages need no workgroup barrier
    for (int t = tid; t < NP / 2; t += 1024)
      for (int jj = j; jj > 0; jj >>= 1) {
        compare_swap(t, jj, kk);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      }
    __syncthreads();
  }
}

}  // namespace itts

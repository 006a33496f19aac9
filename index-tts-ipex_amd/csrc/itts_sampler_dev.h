// Device code shared by the token-choice kernels, one definition of each stage listed here:
//   - sampler_commit / sampler_next_embedding: HF greedy search / sample() commit of one token per row + the next step's input
//     embedding (the sampler kernels of decode_sampler.hip and the persistent decode engine's in-launch greedy sampler)
//   - block_max / block_sum: every kernel of beam.hip; row_logsumexp, beam_seen_bitmap, processed_score: beam_cand_kernel and
//     typical_filter_kernel (sampler_score: the form of the one-beam samplers on their byte map)
//   - sort_cands_wave, regather_cands_ordered: the two narrow kernels (1 <= top_k <= 128), sampler_sample_kernel and beam_cand_kernel
//   - wide_sort<DESC>: sampler_wide_kernel, beam_wide_cand_kernel (descending), typical_filter_kernel (ascending); wide_scan_excl:
//     sampler_wide_kernel, beam_wide_cand_kernel, beam_wide_pick_kernel
// Every helper works on the caller's __shared__ arrays: no kernel's LDS layout depends on this file.  Written out per kernel and
// kept in step by hand, because every shared form measured slower or took a register more (DESIGN.md section 4a,
// profiles/token_choice_refactor.txt): the radix select, the candidate gather and the narrow top-p of the two narrow kernels; the
// fill, top-k count and top-p cut of the two whole-vocabulary kernels; log-sum-exp, bitmap and score inside beam_wide_cand_kernel.
#pragma once
#include "itts_decode.h"
#include "itts_wave_dev.h"

namespace itts {

// repetition penalty (RepetitionPenaltyLogitsProcessor; seen = the token is in the row's id history) + stop suppression on one
// score.  Temperature stays with the callers (beam_cand_kernel applies it only under do_sample)
__device__ __forceinline__ float processed_score(float v, bool seen, float penalty, int suppress_stop, int stop, int i) {
  if (penalty != 1.f && seen) v = v < 0.f ? v * penalty : v / penalty;
  if (suppress_stop && i == stop) v = -INFINITY;
  return v;
}
// The same on the byte map of the one-beam samplers: a SECOND copy of the two lines above, to be kept in step with them by hand.
// It is not a call of processed_score because the persistent engine's in-launch greedy sampler inlines it, and passing a.penalty /
// a.suppress_stop / a.stop as values (also behind a guard, also with a lazily evaluated `seen`) regroups the scalar argument
// loads of all 33 decode_engine_kernel instantiations
__device__ __forceinline__ float sampler_score(const SamplerArgs& a, const uint8_t* seen_row, float v, int i) {
  if (a.preprocessed) return v;
  if (a.penalty != 1.f && seen_row[i]) v = v < 0.f ? v * a.penalty : v / a.penalty;
  if (a.suppress_stop && i == a.stop) v = -INFINITY;
  return v;
}

// block reductions of 1024 threads: xor butterfly inside every wave, then the 16 wave results in order (red[16])
__device__ __forceinline__ float block_max(float v, float* red, int tid) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < 16; ++i) r = fmaxf(r, red[i]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < 16; ++i) r += red[i];
  __syncthreads();
  return r;
}
// log-sum-exp of lg[0 .. V): <= 16 strided terms per thread, then block_max / block_sum
__device__ __forceinline__ float row_logsumexp(const float* __restrict__ lg, int V, float* red, int tid) {
  float mx = -INFINITY;
  for (int i = tid; i < V; i += 1024) mx = fmaxf(mx, lg[i]);
  mx = block_max(mx, red, tid);
  float se = 0.f;
  for (int i = tid; i < V; i += 1024) se += expf(lg[i] - mx);
  se = block_sum(se, red, tid);
  return mx + logf(se);
}

// ids a beam has seen as a bitmap over the vocabulary (seenw[512]: V <= 16384 bits): the fake prompt ids (all fake_id, then
// start_tok: model.py:644-653) + its history hist[0 .. k).  An id outside the vocabulary has no score to penalise and no bit
__device__ __forceinline__ void beam_seen_bitmap(unsigned* seenw, int V, int fake_id, int start_tok, const int* hist, int k, int tid) {
  for (int i = tid; i < (V + 31) / 32; i += 1024) seenw[i] = 0u;
  __syncthreads();
  if (tid == 0) {
    if ((unsigned)fake_id < (unsigned)V) atomicOr(&seenw[fake_id >> 5], 1u << (fake_id & 31));
    if ((unsigned)start_tok < (unsigned)V) atomicOr(&seenw[start_tok >> 5], 1u << (start_tok & 31));
  }
  for (int i = tid; i < k; i += 1024) {
    const int t = hist[i];
    if ((unsigned)t < (unsigned)V) atomicOr(&seenw[t >> 5], 1u << (t & 31));
  }
  __syncthreads();
}
__device__ __forceinline__ bool seen_bit(const unsigned* seenw, int i) { return ((seenw[i >> 5] >> (i & 31)) & 1u) != 0; }

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

// ---- the whole-vocabulary kernels: sampler_wide_kernel (decode_sampler.hip), beam_wide_cand_kernel / beam_wide_pick_kernel
//      (beam.hip) - one sort order, one tie rule, one summation structure ----

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

// block bitonic sort of NP (a power of two >= 1024) (key, u16 id) pairs in LDS by 1024 threads: descending (DESC) or ascending
// key, ascending id on ties.  The caller has put a barrier behind its writes of keys / idx; the sort ends with one
template <bool DESC>
__device__ __forceinline__ void wide_sort(float* keys, unsigned short* idx, int NP, int tid) {
  auto compare_swap = [&](int t, int j, int kk) {
    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
    const bool up = (lo & kk) == 0;
    const float k0 = keys[lo], k1 = keys[hi];
    const unsigned short i0 = idx[lo], i1 = idx[hi];
    const bool behind = (DESC ? k0 < k1 : k0 > k1) || (k0 == k1 && i0 > i1);  // entry lo belongs behind entry hi
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

// Row admission into a running batched decode (Engine::gpt_admit_rows, itts_kv_admit, itts_rows_admit): kv_admit_kernel writes the
// K/V of an admission prefill into chosen slots of the cache, rows_admit_kernel gives those slots the state of a fresh generation,
// and admit_plan is the host function that says which slots are free.  Under beams (itts_beam_admit) beam_admit_kernel adds the
// beam state of a fresh generation for the admitted batch items.
#include <algorithm>
#include <cstdint>

#include "itts_decode.h"

namespace itts {
namespace {

// The prefill's fused qkv rows [n][S][3 * H * dh] -> positions 0 .. S - 1 of rows slot[i] of the caches [Bcache][H][Smax][dh].
// One lane moves EPL consecutive elements of a (row, head, position) run of dh elements, for K and for V: 16 bytes in and out
// where the types agree, 16 (half) or 2 x 16 (fp32) bytes in and 8 bytes out for the e4m3 cache (fp8_pack4: the bytes of
// kv_scatter_kernel).  Lanes follow the DESTINATION order (row, head, position, chunk): the positions of one (row, head) are
// contiguous in the cache, so a wave stores one contiguous KiB (512 bytes of e4m3) and loads dh-element runs 3 * H * dh elements
// apart.  Every element is written once by one lane: no LDS, no atomics, no hand-off.
template <typename TQ, typename TC>
struct KvAdmitTraits {
  static constexpr int EPL = sizeof(TC) == 1 ? 8 : 16 / (int)sizeof(TC);
};

template <typename TQ, typename TC>
__device__ __forceinline__ void kv_admit_move(TC* __restrict__ dst, const TQ* __restrict__ src) {
  if constexpr (sizeof(TC) == sizeof(TQ)) {  // fp32 -> fp32, half -> half: the bits as they are
    *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
  } else if constexpr (sizeof(TQ) == 2) {  // half -> e4m3
    const u32x4 w = *reinterpret_cast<const u32x4*>(src);
    *reinterpret_cast<u32x2*>(dst) = u32x2{fp8_pack4(half_lo(w[0]), half_hi(w[0]), half_lo(w[1]), half_hi(w[1])),
                                           fp8_pack4(half_lo(w[2]), half_hi(w[2]), half_lo(w[3]), half_hi(w[3]))};
  } else {  // fp32 -> e4m3
    const f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 4);
    *reinterpret_cast<u32x2*>(dst) = u32x2{fp8_pack4(lo[0], lo[1], lo[2], lo[3]), fp8_pack4(hi[0], hi[1], hi[2], hi[3])};
  }
}

template <typename TQ, typename TC>
__global__ __launch_bounds__(256) void kv_admit_kernel(KvAdmitArgs a) {
  constexpr int EPL = KvAdmitTraits<TQ, TC>::EPL;
  const unsigned cpr = (unsigned)a.dh / EPL;  // chunks per run
  const unsigned long long total = (unsigned long long)a.n * a.H * a.S * cpr;
  unsigned long long t = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (t >= total) return;
  const unsigned c = (unsigned)(t % cpr);
  t /= cpr;
  const unsigned s = (unsigned)(t % (unsigned)a.S);
  t /= (unsigned)a.S;
  const unsigned h = (unsigned)(t % (unsigned)a.H), i = (unsigned)(t / (unsigned)a.H);
  const size_t D = (size_t)a.H * a.dh;
  const TQ* src = reinterpret_cast<const TQ*>(a.qkv) + ((size_t)i * a.S + s) * 3 * D + (size_t)h * a.dh + c * EPL;
  const size_t o = (((size_t)a.slot[i] * a.H + h) * a.Smax + s) * a.dh + c * EPL;
  kv_admit_move<TQ, TC>(reinterpret_cast<TC*>(a.kc) + o, src + D);
  kv_admit_move<TQ, TC>(reinterpret_cast<TC*>(a.vc) + o, src + 2 * D);
}

// The state of a fresh generation for the admitted slots: what init_decode_state_kernel writes per row (the repetition bitmap,
// unfinished = 1, cur_tok = start, len = 0), the slot's left padding, its ids row filled with stop, its forced row (-1, or row i
// of forced_src [n][max_gen]) and - uniforms_src [n][max_gen] given - column slot of uniforms [max_gen][B].  blockIdx.y is the
// admitted row; no other slot is touched.
__global__ __launch_bounds__(256) void rows_admit_kernel(RowsAdmitArgs a) {
  const int i = blockIdx.y, slot = a.slot[i];
  const int lim = a.V > a.max_gen ? a.V : a.max_gen;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < lim; j += gridDim.x * 256) {
    if (j < a.V) a.seen[(size_t)slot * a.V + j] = (j == a.fake_id || j == a.start_tok) ? 1 : 0;
    if (j < a.max_gen) {
      a.ids[(size_t)slot * a.max_gen + j] = a.stop;
      if (a.forced) a.forced[(size_t)slot * a.max_gen + j] = a.forced_src ? a.forced_src[(size_t)i * a.max_gen + j] : -1;
      if (a.uniforms && a.uniforms_src) a.uniforms[(size_t)j * a.B + slot] = a.uniforms_src[(size_t)i * a.max_gen + j];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.unfinished[slot] = 1;
    a.cur_tok[slot] = a.start_tok;
    a.len[slot] = 0;
    a.kv_start[slot] = a.kvs[i];
  }
}

// The beam state of a fresh generation for the admitted batch items: what beam_init_kernel writes per group - running scores 0
// (beam_search: -1e9 for the beams behind the first, so that step 0 expands beam 0 only), the identity cache ancestry in BOTH
// ping-pong halves (the half base is rows * Smax with rows = items * nb, as every reader computes it), an empty hypothesis store
// (hyp_order = -1 marks a slot free), not done - and, uniforms_src [n][max_gen][2 * nb] given, the item's column of the draws
// [max_gen][items][2 * nb].  hyp_tok, hyp_score, hyp_len and beam_ids are not reset: nothing reads a history beyond the group's own
// len, and a hypothesis slot is read only where hyp_order >= 0.  blockIdx.y is the admitted item; no other item is touched.  An
// ancestry row is Smax bytes with Smax a multiple of 16: one 16-byte store per lane.  Every element is written once by one lane:
// no LDS, no atomics, no hand-off.
__global__ __launch_bounds__(256) void beam_admit_kernel(BeamAdmitArgs a) {
  const int i = blockIdx.y, g = a.item[i];
  const int nb = a.nb, nd = 2 * nb, cpr = a.Smax / 16;  // 16-byte chunks per ancestry row
  const int n_anc = 2 * nb * cpr, n_u = (a.uniforms && a.uniforms_src) ? a.max_gen * nd : 0;
  const size_t half = (size_t)a.items * nb * a.Smax;
  const int lim = n_anc > n_u ? n_anc : n_u;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < lim; j += gridDim.x * 256) {
    if (j < n_anc) {
      const int h = j / (nb * cpr), r = j - h * nb * cpr, q = r / cpr, c = r - q * cpr;
      const unsigned w = (unsigned)q * 0x01010101u;
      *reinterpret_cast<u32x4*>(a.anc + h * half + ((size_t)g * nb + q) * a.Smax + (size_t)c * 16) = u32x4{w, w, w, w};
    }
    if (j < n_u) {
      const int k = j / nd, e = j - k * nd;
      a.uniforms[((size_t)k * a.items + g) * nd + e] = a.uniforms_src[((size_t)i * a.max_gen + k) * nd + e];
    }
  }
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < nb) a.beam_scores[g * nb + t] = (a.do_sample || t == 0) ? 0.f : -1e9f;
    if (t <= nb) a.hyp_order[g * (nb + 1) + t] = -1;
    if (t == 0) {
      a.hyp_n[g] = 0;
      a.hyp_worst[g] = 1e9f;
      a.hyp_counter[g] = 0;
      a.done[g] = 0;
    }
  }
}

}  // namespace

// everything kv_admit refuses, without a HIP call (itts_kv_admit checks before it touches the device)
int kv_admit_check(const void* kc, const void* vc, const void* qkv, int n, int S, int H, int dh, int Smax, int Bcache, int tq, int tc,
                   const int* slots) {
  ITTS_REQUIRE(kc && vc && qkv && slots, "kv_admit: null pointer");
  ITTS_REQUIRE(n >= 1 && n <= ROWS_MOVE_MAX, "kv_admit: 1 <= n <= 128 rows");
  ITTS_REQUIRE(S >= 1 && H >= 1 && dh >= 1 && Smax >= 1 && Bcache >= 1 && S <= Smax, "kv_admit: need S, H, dh, Smax, Bcache >= 1 and S <= Smax");
  ITTS_REQUIRE(Bcache <= 65536, "kv_admit: more than 65536 cache rows");
  ITTS_REQUIRE((tq == F32 && (tc == F32 || tc == FP8)) || (tq == BF16 && (tc == BF16 || tc == FP8)),
               "kv_admit: type pair (tq, tc) must be fp32 -> fp32, 16-bit -> 16-bit, or either -> fp8 (e4m3) cache");
  const int epl = tc == FP8 ? 8 : tc == F32 ? 4 : 8;
  ITTS_REQUIRE(dh % epl == 0, "kv_admit: dh must be a multiple of the elements a lane moves (4 for an fp32 cache, else 8)");
  ITTS_REQUIRE((uintptr_t)qkv % 16 == 0 && (uintptr_t)kc % (tc == FP8 ? 8 : 16) == 0 && (uintptr_t)vc % (tc == FP8 ? 8 : 16) == 0,
               "kv_admit: qkv must be 16-byte aligned, the caches 16-byte (e4m3: 8-byte) aligned");
  for (int i = 0; i < n; ++i) {
    ITTS_REQUIRE(slots[i] >= 0 && slots[i] < Bcache, "kv_admit: slot outside [0, Bcache)");
    for (int j = 0; j < i; ++j) ITTS_REQUIRE(slots[i] != slots[j], "kv_admit: a slot is written twice");
  }
  return OK;
}

int kv_admit(void* kc, void* vc, const void* qkv, int n, int S, int H, int dh, int Smax, int Bcache, int tq, int tc, const int* slots,
             hipStream_t s) {
  ITTS_TRY(kv_admit_check(kc, vc, qkv, n, S, H, dh, Smax, Bcache, tq, tc, slots));
  KvAdmitArgs a;
  a.kc = kc;
  a.vc = vc;
  a.qkv = qkv;
  a.n = n;
  a.S = S;
  a.H = H;
  a.dh = dh;
  a.Smax = Smax;
  for (int i = 0; i < n; ++i) a.slot[i] = (unsigned short)slots[i];
  const int epl = tc == FP8 ? 8 : tc == F32 ? 4 : 8;
  const unsigned long long total = (unsigned long long)n * H * S * (dh / epl);
  const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
  if (tq == F32 && tc == F32)
    hipLaunchKernelGGL((kv_admit_kernel<float, float>), grid, blk, 0, s, a);
  else if (tq == BF16 && tc == BF16)
    hipLaunchKernelGGL((kv_admit_kernel<bf16_t, bf16_t>), grid, blk, 0, s, a);
  else if (tq == BF16 && tc == FP8)
    hipLaunchKernelGGL((kv_admit_kernel<bf16_t, fp8_t>), grid, blk, 0, s, a);
  else
    hipLaunchKernelGGL((kv_admit_kernel<float, fp8_t>), grid, blk, 0, s, a);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// everything rows_admit refuses, without a HIP call.  slots / kvs: host lists of a.n entries
int rows_admit_check(const RowsAdmitArgs& a, const int* slots, const int* kvs) {
  ITTS_REQUIRE(a.seen && a.unfinished && a.cur_tok && a.len && a.kv_start && a.ids && slots && kvs, "rows_admit: null pointer");
  ITTS_REQUIRE(a.n >= 1 && a.n <= ROWS_MOVE_MAX, "rows_admit: 1 <= n <= 128 rows");
  ITTS_REQUIRE(a.B >= 1 && a.B <= 65536 && a.V >= 1 && a.max_gen >= 1, "rows_admit: need 1 <= B <= 65536, V >= 1, max_gen >= 1");
  ITTS_REQUIRE(!a.forced_src || a.forced, "rows_admit: forced tokens without a forced table");
  ITTS_REQUIRE(!a.uniforms_src || a.uniforms, "rows_admit: uniforms without a uniforms table");
  for (int i = 0; i < a.n; ++i) {
    ITTS_REQUIRE(slots[i] >= 0 && slots[i] < a.B, "rows_admit: slot outside [0, B)");
    ITTS_REQUIRE(kvs[i] >= 0 && kvs[i] < 65536, "rows_admit: kv_start outside [0, 65536)");
    for (int j = 0; j < i; ++j) ITTS_REQUIRE(slots[i] != slots[j], "rows_admit: a slot is written twice");
  }
  return OK;
}

int rows_admit(RowsAdmitArgs a, const int* slots, const int* kvs, hipStream_t s) {
  ITTS_TRY(rows_admit_check(a, slots, kvs));
  for (int i = 0; i < a.n; ++i) {
    a.slot[i] = (unsigned short)slots[i];
    a.kvs[i] = (unsigned short)kvs[i];
  }
  const int lim = a.V > a.max_gen ? a.V : a.max_gen;
  const int bx = (lim + 255) / 256;
  hipLaunchKernelGGL(rows_admit_kernel, dim3((unsigned)(bx < 64 ? bx : 64), (unsigned)a.n), dim3(256), 0, s, a);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// The slots an admission may take: a slot is finished when unfinished == 0 or len >= max_gen.  The min(n, *n_free) lowest finished
// slots go to slots[] in ascending order; *n_free is the number of finished slots of all B
int admit_plan(const int* unfinished, const int* len, int B, int max_gen, int n, int* slots, int* n_free) {
  ITTS_REQUIRE(unfinished && len && n_free && B >= 0 && n >= 0 && (n == 0 || slots), "admit_plan: bad arguments");
  int f = 0;
  for (int b = 0; b < B; ++b) {
    if (unfinished[b] != 0 && len[b] < max_gen) continue;
    if (f < n) slots[f] = b;
    ++f;
  }
  *n_free = f;
  return OK;
}

// everything beam_admit refuses, without a HIP call.  items: host list of a.n batch items
int beam_admit_check(const BeamAdmitArgs& a, const int* items) {
  ITTS_REQUIRE(a.beam_scores && a.anc && a.hyp_order && a.hyp_n && a.hyp_worst && a.hyp_counter && a.done && items, "beam_admit: null pointer");
  ITTS_REQUIRE(a.n >= 1 && a.n <= ROWS_MOVE_MAX, "beam_admit: 1 <= n <= 128 items");
  ITTS_REQUIRE(a.nb >= 2 && a.nb <= 10, "beam_admit: 2 <= num_beams <= 10");
  ITTS_REQUIRE(a.n * a.nb <= ROWS_MOVE_MAX, "beam_admit: more than 128 rows (n * num_beams) in one admission");
  ITTS_REQUIRE(a.items >= 1 && a.items <= 65536 / a.nb && a.max_gen >= 1 && a.max_gen <= 65536 && a.Smax >= 16 && a.Smax <= 65536,
               "beam_admit: need 1 <= items * num_beams <= 65536, 1 <= max_gen <= 65536, 16 <= Smax <= 65536");
  ITTS_REQUIRE(a.Smax % 16 == 0 && (uintptr_t)a.anc % 16 == 0, "beam_admit: Smax must be a multiple of 16 and anc 16-byte aligned");
  ITTS_REQUIRE(!a.uniforms_src || a.uniforms, "beam_admit: uniforms without a uniforms table");
  for (int i = 0; i < a.n; ++i) {
    ITTS_REQUIRE(items[i] >= 0 && items[i] < a.items, "beam_admit: item outside [0, items)");
    for (int j = 0; j < i; ++j) ITTS_REQUIRE(items[i] != items[j], "beam_admit: an item is written twice");
  }
  return OK;
}

int beam_admit(BeamAdmitArgs a, const int* items, hipStream_t s) {
  ITTS_TRY(beam_admit_check(a, items));
  for (int i = 0; i < a.n; ++i) a.item[i] = (unsigned short)items[i];
  const int n_anc = 2 * a.nb * (a.Smax / 16), n_u = (a.uniforms && a.uniforms_src) ? a.max_gen * 2 * a.nb : 0;
  const int bx = (std::max(n_anc, n_u) + 255) / 256;
  hipLaunchKernelGGL(beam_admit_kernel, dim3((unsigned)(bx < 64 ? bx : 64), (unsigned)a.n), dim3(256), 0, s, a);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace itts

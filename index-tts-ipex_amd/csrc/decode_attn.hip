// ---------------------------------------------------------------------------------------------
// decode_attn2: single-query attention over the KV cache with this step's K/V append fused in.
// One 1024-thread workgroup per (head, row).  LPK lanes share one key row with 16-byte loads (a wave reads
// 1 KiB of contiguous K and 1 KiB of V per step); every key slot runs an online softmax (running max, sum,
// partial context) so K and V are read in ONE pass with both loads of a step in flight together; slots are
// merged with max-rescaling through shuffles and LDS.  Output type TO: fp32 or bf16 (feeds the proj GEMV).
// Cache type TC: fp32, the 16-bit type, or (opt-in, whole forms only) OCP e4m3 bytes without a scale - fp8_t, itts_common.h;
// CacheVec<fp8_t> keeps the 16-bit form's thread <-> key mapping with 8-byte loads, the append is one 8-byte store per lane.
// ---------------------------------------------------------------------------------------------
#include "itts_decode.h"
#include "itts_attn_dev.h"
#include "itts_wave_dev.h"

namespace itts {
namespace {

// NIT = key pairs per slot held in registers (NIT * 2 * SLOTS keys: 768 with bf16 at NIT = 3).  The first pair is
// requested before any device scalar is read, the rest as soon as the sequence length is known, all before the first
// use: the whole cache read costs two overlapped memory latencies instead of one per iteration.
#ifdef ITTS_GEMV_STAMPS
__device__ unsigned long long* g_attn_stamp = nullptr;
#define ATTN_STAMP(i)                                                                                  \
  {                                                                                                    \
    unsigned long long t_;                                                                             \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                        \
    if (threadIdx.x == 0 && g_attn_stamp) g_attn_stamp[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8 + (i)] = t_; \
  }
#else
#define ATTN_STAMP(i)
#endif

// NT = threads per (row, head): 1024 for the latency-bound small batches (one workgroup per CU), 256 once there are
// enough (row, head) pairs to fill the CUs several times over - 5 workgroups per CU overlap their load / softmax /
// merge phases, where the 86-VGPR 1024-thread form runs its 5 rounds per CU back to back.
// NSPLIT > 1: the keys of one (row, head) are dealt round-robin, SLOTS rows at a time, to NSPLIT workgroups
// (blockIdx.z); each writes an un-normalised partial (max, sum, weighted V) and the consumer - the attention-projection
// GEMV, prologue 3 - merges them while it loads its activations.  At 2 rows x 20 heads this turns 40 workgroups of 16
// waves (4 waves per SIMD: the softmax phase is issue-bound and the last wave trails the first by 1.4 us on the phase
// timeline) into 160 workgroups of 4 waves, one per SIMD, on 160 CUs.
// ANC (beam-sample): the cache is NOT re-ordered when the beams are (HF `_reorder_cache` copies every layer's K/V by
// beam_idx each step, model.py:194-207).  Instead every beam row b carries an ancestry row anc[b][j] = which of the nb
// physical rows of its batch item holds position j of ITS history; the beam sampler rewrites those few KB per step
// (ping-pong by the parity of the step count) and this kernel gathers K/V rows through it.  The row appended by this
// step always goes to the beam's own physical row.
template <typename TC, typename TO, int NIT, int NT, int NSPLIT = 1, bool ANC = false>
__global__ __launch_bounds__(NT) void decode_attn2_kernel(TO* __restrict__ ctx, const float* __restrict__ qkv,
                                                          TC* __restrict__ kc, TC* __restrict__ vc,
                                                          const int* __restrict__ len, const int* __restrict__ kv_start,
                                                          const int* __restrict__ prefix, int H, int Smax, float scale,
                                                          int ctx_bt, float* __restrict__ part_o = nullptr,
                                                          float* __restrict__ part_ml = nullptr,
                                                          const uint8_t* __restrict__ anc = nullptr, int nb = 1) {
  constexpr int DH = 64, VEC = CacheVec<TC>::VEC, LPK = CacheVec<TC>::LPK, NW = NT / 64, SLOTS = NT / LPK;
  constexpr int SD = NT >= 1024 ? 2 : 4;  // rows per slot in flight beyond the register window
  ATTN_STAMP(0)
  __shared__ float sm[NW], sl[NW];
  __shared__ float so[NW][DH];
  const int h = blockIdx.x, b = blockIdx.y, sp = NSPLIT > 1 ? blockIdx.z : 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = H * DH;
  TC* kb = kc + ((size_t)b * H + h) * Smax * DH;
  TC* vb = vc + ((size_t)b * H + h) * Smax * DH;
  const int slot = tid / LPK, sub = tid % LPK;
  // cache row of key j: own row, or (ANC) the physical row the beam's ancestry names for that position
  const uint8_t* arow = nullptr;
  int rowbase = 0;
  if constexpr (ANC) {
    arow = anc + ((size_t)(len[b] & 1) * gridDim.y + b) * Smax;
    rowbase = (b / nb) * nb;
  }
  auto krow = [&](int j) -> const TC* {
    if constexpr (ANC) return kc + ((size_t)(rowbase + min((int)arow[j], nb - 1)) * H + h) * Smax * DH + (size_t)j * DH;
    return kb + (size_t)j * DH;
  };
  auto vrow = [&](int j) -> const TC* {
    if constexpr (ANC) return vc + ((size_t)(rowbase + min((int)arow[j], nb - 1)) * H + h) * Smax * DH + (size_t)j * DH;
    return vb + (size_t)j * DH;
  };
  // (a) the first pair of key/value rows of this slot, requested before ANYTHING else: their addresses depend on no
  //     device scalar (rows are clamped to the cache capacity; rows >= S are masked out below)
  CacheVec<TC> kr[2 * NIT], vr[2 * NIT];
  // UNC pairs are requested blind (rows past S cost their bytes but nothing waits for the length): 2 pairs cover every
  // prefix; with 1024 threads 4 pairs = 512 rows cover the sequence for most of a generation, so the device-scalar
  // -> load chain (a second full memory latency) only remains for the late steps
  constexpr int UNC = 2;  // 4 blind pairs (512 rows) measured slower: 0.602 vs 0.593 ms per step - the extra bytes cost more than the chain
#pragma unroll
  for (int u = 0; u < UNC; ++u) {
    const int j = min((u * NSPLIT + sp) * SLOTS + slot, Smax - 1);
    kr[u].load(krow(j) + sub * VEC);
    vr[u].load(vrow(j) + sub * VEC);
  }
  // (a') this thread's slice of the step's q / k / v (addresses depend on no device scalar either): straight to
  //      registers - no LDS round trip, no barrier between the query and the cache reads
  const float* qv = qkv + (size_t)b * 3 * D + h * DH + sub * VEC;
  float4 qraw[VEC / 4], kraw[VEC / 4], vraw[VEC / 4];
#pragma unroll
  for (int i = 0; i < VEC / 4; ++i) {
    qraw[i] = *reinterpret_cast<const float4*>(qv + 4 * i);
    kraw[i] = *reinterpret_cast<const float4*>(qv + D + 4 * i);
    vraw[i] = *reinterpret_cast<const float4*>(qv + 2 * D + 4 * i);
  }
  // (b) per-row scalars and the K/V append of this step
  const int pos = prefix[0] + len[b];
  const int S = pos + 1;
  const int ks = kv_start[b];
  // (c) now that S is known: request every remaining row of the sequence at once (one more memory latency in total).
  //     This comes BEFORE anything that consumes the q/k/v slice - vmcnt is in-order, and the K/V append below would
  //     otherwise make the wave sit out the first loads' latency before these are even issued
#pragma unroll
  for (int u = UNC; u < 2 * NIT; ++u)
    if ((u * NSPLIT + sp) * SLOTS < S) {  // block-uniform
      const int j = min((u * NSPLIT + sp) * SLOTS + slot, Smax - 1);
      kr[u].load(krow(j) + sub * VEC);
      vr[u].load(vrow(j) + sub * VEC);
    }
  ATTN_STAMP(1)
  // (d) the step's own q / k / v: scale, round as the cache does, append
  float qr[VEC], kown[VEC], vown[VEC];  // the appended row with the cache's rounding, never read back from HBM
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    qr[i] = (&qraw[i >> 2].x)[i & 3] * scale;
    kown[i] = (float)(TC)(&kraw[i >> 2].x)[i & 3];
    vown[i] = (float)(TC)(&vraw[i >> 2].x)[i & 3];
  }
  if (tid < LPK && sp == 0) {  // slot 0 (of split 0): its LPK lanes cover the 64 dims
    if constexpr (sizeof(TC) == 1) {  // e4m3 cache: the lane's 8 bytes as one store (kown / vown hold e4m3 values: packing them is exact)
      static_assert(VEC == 8, "fp8 cache: 8 dims per lane");
      *reinterpret_cast<u32x2*>(kb + (size_t)pos * DH + sub * VEC) =
          u32x2{fp8_pack4(kown[0], kown[1], kown[2], kown[3]), fp8_pack4(kown[4], kown[5], kown[6], kown[7])};
      *reinterpret_cast<u32x2*>(vb + (size_t)pos * DH + sub * VEC) =
          u32x2{fp8_pack4(vown[0], vown[1], vown[2], vown[3]), fp8_pack4(vown[4], vown[5], vown[6], vown[7])};
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        stf(kb + (size_t)pos * DH + sub * VEC + i, kown[i]);
        stf(vb + (size_t)pos * DH + sub * VEC + i, vown[i]);
      }
    }
  }
  ATTN_STAMP(2)
  float m = -INFINITY, l = 0.f, acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  auto score = [&](const CacheVec<TC>& kk) { return attn_score<LPK>(qr, kk); };  // itts_attn_dev.h; the lambda stays
  // (e) the register window in two phases, as torch.softmax does it: all scores, their maximum, then one exp per key and
  //     the weighted sum - half the VALU work of a per-key online update (no rescale of the accumulator per key), and the
  //     16 waves of a workgroup share 4 SIMDs, so this phase is issue-bound.  The row appended by this step (j == pos)
  //     is masked out of the window and enters as one extra key of slot 0, from registers.  Rows past S multiply by
  //     p = 0: the cache is zero-filled at allocation, so whatever they hold is finite.
  {
    float sc[2 * NIT + 1];
#pragma unroll
    for (int u = 0; u < 2 * NIT; ++u) {
      const int j = (u * NSPLIT + sp) * SLOTS + slot;
      const bool live = u < UNC || (u * NSPLIT + sp) * SLOTS < S;  // block-uniform: was this pair requested
      const float t = live ? score(kr[u]) : 0.f;
      sc[u] = (live && j < S && j >= ks && j != pos) ? t : -INFINITY;
    }
    {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) t = fmaf(qr[i], kown[i], t);
      t = dpp_add<0xB1>(t);
      t = dpp_add<0x4E>(t);
      t = dpp_add<0x141>(t);
      if (LPK == 16) t = dpp_add<0x140>(t);
      sc[2 * NIT] = (slot == 0 && sp == 0) ? t : -INFINITY;
    }
    float mw = sc[0];
#pragma unroll
    for (int u = 1; u <= 2 * NIT; ++u) mw = fmaxf(mw, sc[u]);
    if (mw > -INFINITY) {
#pragma unroll
      for (int u = 0; u < 2 * NIT; ++u)
        if (u < UNC || (u * NSPLIT + sp) * SLOTS < S) {  // block-uniform: pairs that were never requested hold no data at all
          const float p = __expf(sc[u] - mw);  // exp(-inf) = 0 for masked rows
          l += p;
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = fmaf(p, vr[u].get(i), acc[i]);
        }
      const float p = __expf(sc[2 * NIT] - mw);
      l += p;
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fmaf(p, vown[i], acc[i]);
      m = mw;
    }
  }
  // online update for rows beyond the window (never the appended row when it lies inside the window)
  auto consume = [&](const CacheVec<TC>& kk, const CacheVec<TC>& vv, int j) {
    attn_consume<LPK>(m, l, acc, qr, kk, vv, j < S && j >= ks && j != pos);
  };
  // sequences longer than the register-resident window: stream the rest two rows at a time
  for (int cb = 2 * NIT; (cb * NSPLIT + sp) * SLOTS < S; cb += SD) {  // chunk cb of this split = rows (cb*NSPLIT+sp)*SLOTS ..
    CacheVec<TC> k2[SD], v2[SD];
#pragma unroll
    for (int u = 0; u < SD; ++u) {
      const int j = min(((cb + u) * NSPLIT + sp) * SLOTS + slot, Smax - 1);
      k2[u].load(krow(j) + sub * VEC);
      v2[u].load(vrow(j) + sub * VEC);
    }
#pragma unroll
    for (int u = 0; u < SD; ++u) consume(k2[u], v2[u], ((cb + u) * NSPLIT + sp) * SLOTS + slot);
  }
  ATTN_STAMP(3)
  // merge the 64/LPK key slots of this wave (lanes with equal `sub`)
  // (wave_bfly_max / wave_bfly_sum, itts_wave_dev.h: no LDS crossbar)
  float M = m;
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) M = wave_bfly_max(M, o);
  const float sc0 = M > -INFINITY ? __expf(m - M) : 0.f;
  l *= sc0;
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] *= sc0;
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) {
    l = wave_bfly_sum(l, o);
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = wave_bfly_sum(acc[i], o);
  }
  if (lane < LPK)
#pragma unroll
    for (int i = 0; i < VEC; ++i) so[wave][lane * VEC + i] = acc[i];
  if (lane == 0) {
    sm[wave] = M;
    sl[wave] = l;
  }
  ATTN_STAMP(4)
  __syncthreads();
  ATTN_STAMP(5)
  if (tid < DH) {
    float MM = sm[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) MM = fmaxf(MM, sm[i]);
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const float e = sm[i] > -INFINITY ? __expf(sm[i] - MM) : 0.f;
      o = fmaf(e, so[i][tid], o);
      L = fmaf(e, sl[i], L);
    }
    if constexpr (NSPLIT > 1) {
      // partial of this split: [row][head][split][64] un-normalised, and [row][head][2][NSPLIT] = (max..., sum...)
      part_o[(((size_t)b * H + h) * NSPLIT + sp) * DH + tid] = o;
      if (tid == 0) {
        part_ml[((size_t)b * H + h) * 2 * NSPLIT + sp] = MM;
        part_ml[((size_t)b * H + h) * 2 * NSPLIT + NSPLIT + sp] = L;
      }
    } else {
      stf(ctx + (ctx_bt ? tile_off(b, h * DH + tid, ctx_bt) : (size_t)b * D + h * DH + tid), o / L);
    }
  }
  ATTN_STAMP(6)
}

}  // namespace

#ifndef ATTN_NIT_MANY
#define ATTN_NIT_MANY 8
#endif

int decode_attn2(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start,
                 const int* prefix_dev, int B, int H, int dh, int Smax, int tc, hipStream_t s, int ctx_tiled, float* part_o,
                 float* part_ml, const uint8_t* anc, int nb) {
  ITTS_REQUIRE(dh == 64, "decode_attn2: head dim must be 64");
  ITTS_REQUIRE(!anc || (nb >= 1 && nb <= 16 && B % nb == 0), "decode_attn2: beam ancestry needs B to be a multiple of 1 <= nb <= 16");
  const float scale = 1.f / sqrtf((float)dh);
  // every form is one launch of decode_attn2_kernel<TC, TO, NIT, NT, NSPLIT, ANC> with the same arguments (a form ignores the
  // ones it has no use for): NSPLIT workgroups of NT threads per (row, head), ANC when the beams carry an ancestry
  dim3 grid(H, B);
  int bt = 0;
#define ATTN_GO(TC, TO, NIT, NT, NSPLIT, ANC)                                                                                   \
  hipLaunchKernelGGL((decode_attn2_kernel<TC, TO, NIT, NT, NSPLIT, ANC>), grid, dim3(NT), 0, s, (TO*)ctx, qkv, (TC*)kc, (TC*)vc, \
                     len, kv_start, prefix_dev, H, Smax, scale, bt, part_o, part_ml, anc, nb)
#define ATTN_FORM(TC, TO, NIT, NT, NSPLIT)  \
  if (anc)                                  \
    ATTN_GO(TC, TO, NIT, NT, NSPLIT, true); \
  else                                      \
    ATTN_GO(TC, TO, NIT, NT, NSPLIT, false);
  if (part_o) {  // split form: 4 workgroups of 256 threads per (row, head), partials merged by the projection GEMV
    ITTS_REQUIRE(tc != FP8, "decode_attn2: the split form has no fp8 (e4m3) cache form - an fp8 cache runs the whole forms only");
    ITTS_REQUIRE(part_ml && tc == BF16, "decode_attn2: split form needs both partial buffers and a bf16 cache");
    grid.z = ATTN_NSPLIT;
    ctx = nullptr;
    ATTN_FORM(bf16_t, bf16_t, 3, 256, ATTN_NSPLIT)
    ITTS_HIP_CHECK(hipGetLastError());
    return OK;
  }
  ITTS_REQUIRE(!ctx_tiled || to == BF16, "decode_attn2: tiled ctx is bf16 only");
  bt = ctx_tiled ? (B + 15) / 16 : 0;
  const bool many = (long)B * H >= 512;
#define ATTN_WHOLE(TC, TO)                      \
  if (many) {                                   \
    ATTN_FORM(TC, TO, ATTN_NIT_MANY, 256, 1)    \
  } else {                                      \
    ATTN_FORM(TC, TO, 3, 1024, 1)               \
  }
  if (tc == F32 && to == F32) {
    ATTN_WHOLE(float, float)
  } else if (tc == BF16 && to == BF16) {
    ATTN_WHOLE(bf16_t, bf16_t)
  } else if (tc == BF16 && to == F32) {
    ATTN_WHOLE(bf16_t, float)
  } else if (tc == FP8 && to == BF16) {  // the opt-in e4m3 cache (whole forms only): caches are bytes, 8-byte aligned
    ATTN_WHOLE(fp8_t, bf16_t)
  } else if (tc == FP8 && to == F32) {
    ATTN_WHOLE(fp8_t, float)
  } else {
    set_error("decode_attn2: dtype combination");
    return E_INVALID;
  }
#undef ATTN_WHOLE
#undef ATTN_FORM
#undef ATTN_GO
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace itts

// ---------------------------------------------------------------------------------------------
// decode_attn_kv8: the single-query cache attention of a batched decode step, written for the e4m3 K/V cache (opt-in:
// itts_gpt_set_attn_kv8 / ITTS_ATTN_KV8).  decode_attn2_kernel<fp8_t, ..> is the 16-bit kernel with 8-byte loads put
// in (CacheVec<fp8_t>, VEC 8, LPK 8: bit-identical to the 16-bit form, half the bytes in flight per lane).  This kernel has the
// operation of its whole form - one token per (row, head) over kv_start <= j < pos plus this step's own key, the step's k / v
// rounded with fp8_pack4 and appended at pos, history gathered through the beam ancestry with ANC - and a work split of its own.
//
//   R = 64      keys per round and workgroup
//   D = 4       rounds in the register ring (W = D * R = 256 keys in flight per workgroup)
//   BLIND = 2   rounds (128 keys) requested before len / prefix are read
//
// Work split: grid (H, B), 256 threads = 4 waves per (row, head).  Lane (slot = tid >> 2, sub = tid & 3) owns dims 16 sub .. + 15
// of key 64 r + slot in round r: ONE nontemporal 16-byte load per lane for K and one for V, a wave-load is 16 consecutive keys =
// 1 KiB contiguous without ancestry.
// Ring: kr[D] / vr[D], 8 VGPRs per round and lane.  D = 4: 32 ring registers + 16 q + 16 acc + m, l, the batch's scores, the
// decode temporaries and addresses stay under the 96 VGPRs at which 5 workgroups (20 waves) share a CU - the occupancy the
// 256-thread form of decode_attn2 relies on: 94 VGPRs without ancestry.  The ANC instantiations come to 98 (4 workgroups per CU);
// forcing 96 on them spills (profiles/attn_kv8_resources.txt holds what the compiler made, DESIGN.md 5r what was tried).
// Rounds 0 and 1 are requested blind (rows clamped to Smax - 1), the rest of the ring as soon as pos is known.  The loop takes the
// ring one batch of D rounds at a time: all scores of the batch, the K requests of the next batch into the registers just freed,
// the batch maximum, ONE rescale of the state, then per round one __expf, the weighted V and the V request of the next batch
// into that register - the ring is full while the batch computes.  No LDS and no workgroup barrier inside the loop.
// ANC: the ancestry byte of a round is loaded one batch ahead of its K / V requests (never less than one round), so a request
// never waits for loads it has not waited for already (vmcnt is in order); K and V of a round are then requested together, when
// the V register frees, which keeps the rows out of registers (104 VGPRs otherwise).  The step's v is loaded behind the ring's
// requests for the same reason (48 raw q / k / v registers in flight next to the ring do not fit).
// Cache addresses are a scalar base plus a 32-bit byte offset: one layer's K (or V) must stay under 2 GiB.
// Arithmetic: exact decode (v_cvt_pk_f32_fp8), q * scale in fp32, 16 FMAs per lane and key, two quad_perm DPP adds (every lane
// of a quad holds the same score), one online-softmax state (m, l, acc[16]) per lane for its slot.  Masked keys (j < kv_start,
// j >= pos - the cache row at pos itself included) score -inf before the maximum; rows outside the sequence only have to be
// finite (their weight is 0).  Rounds at or past ceil(pos / 64) - never requested, or blind and wholly masked - are not touched.  This step's key is the initial state of slot 0
// of wave 0, from registers: m = its score, l = 1, acc = the rounded v, so every later key weighs in relative to the running
// maximum; alone it returns the rounded v to the bit.
// Merge: the 16 slots of a wave by butterflies at lane distances 4 (row_ror:4), 8, 16, 32 (wave_bfly_max / wave_bfly_sum), the
// four waves through LDS once, threads 0 .. 63 store o / L.  The summation order is this kernel's own: the result agrees with
// decode_attn2_kernel<fp8_t> to the bounds of the ctx type, not to the bit.
// Append: the four lanes of slot 0 of wave 0 store 16 bytes each of the packed k and v row - the bytes decode_attn2_kernel<fp8_t>
// and kv_scatter_kernel<.., fp8_t> write.  kc / vc must be 16-byte aligned (every row is 64 bytes).
// ---------------------------------------------------------------------------------------------
#include "itts_decode.h"
#include "itts_wave_dev.h"

namespace itts {
namespace {

constexpr int KV8_R = 64, KV8_D = 4, KV8_BLIND = 2;

__device__ __forceinline__ u32x4 ld16_nt(const uint8_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }

// the partner a quad away inside the 16-lane row (row_ror:4); with row_ror:8 after it every lane has met all four quads
__device__ __forceinline__ float quad_away(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xf, 0xf, true));
}

// q . k over the lane's 16 dims (k as 16 e4m3 bytes), summed over the quad
__device__ __forceinline__ float kv8_score(const float (&qr)[16], const u32x4& kk) {
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)kk[w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)kk[w], true);
    s = fmaf(qr[4 * w], lo[0], s);
    s = fmaf(qr[4 * w + 1], lo[1], s);
    s = fmaf(qr[4 * w + 2], hi[0], s);
    s = fmaf(qr[4 * w + 3], hi[1], s);
  }
  s = dpp_add<0xB1>(s);
  return dpp_add<0x4E>(s);
}

template <typename TO, bool ANC>
__global__ __launch_bounds__(256) void decode_attn_kv8_kernel(TO* __restrict__ ctx, const float* __restrict__ qkv,
                                                              uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                              const int* __restrict__ len, const int* __restrict__ kv_start,
                                                              const int* __restrict__ prefix, const uint8_t* __restrict__ anc, int nb,
                                                              int H, int Smax, float scale, int ctx_bt) {
  constexpr int DH = 64, NW = 4, R = KV8_R, D = KV8_D, BLIND = KV8_BLIND;
  static_assert(BLIND <= D, "the blind rounds are part of the first batch");
  __shared__ float sm[NW], sl[NW];
  __shared__ float so[NW][DH];
  const int h = blockIdx.x, b = blockIdx.y;
  // the wave number as a scalar, the lane from mbcnt: nothing keeps threadIdx.x alive across the loop (it cost the 97th VGPR)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = (int)__lane_id();
  const int slot = wave * 16 + (lane >> 2), sub = lane & 3;
  const int Dm = H * DH;
  // byte offsets into a layer's cache fit 32 bits (the launcher refuses larger caches): a scalar base plus one VGPR per address
  const uint32_t own = (uint32_t)((b * H + h) * Smax) * DH + sub * 16;  // this lane's 16 bytes of row 0 of the (row, head) block
  // ANC: byte offset of the lane's piece of key j in physical row `a` of the item; plain: in the row's own block
  const uint8_t* arow = nullptr;
  int rowbase = 0;
  if constexpr (ANC) {
    arow = anc + ((size_t)(len[b] & 1) * gridDim.y + b) * Smax;
    rowbase = (b / nb) * nb;
  }
  auto key_of = [&](int r) -> uint32_t { return (uint32_t)min(r * R + slot, Smax - 1); };  // (unsigned: scalar base + one VGPR)
  auto off_of = [&](int r, int a) -> uint32_t {
    if constexpr (ANC) return ((uint32_t)(((rowbase + a) * H + h) * Smax) + key_of(r)) * DH + sub * 16;
    return own + key_of(r) * DH;
  };
  // (a) the ring's first requests.  ANC: the ancestry bytes of batch 0 come first
  u32x4 kr[D], vr[D];
  int an[D];  // ANC: the ancestry bytes of the next rounds to request, one per ring register (entries at >= pos may be 255)
#pragma unroll
  for (int u = 0; u < D; ++u) an[u] = ANC ? (int)arow[key_of(u)] : 0;
#pragma unroll
  for (int u = 0; u < BLIND; ++u) {
    kr[u] = ld16_nt(kc + off_of(u, min(an[u], nb - 1)));
    vr[u] = ld16_nt(vc + off_of(u, min(an[u], nb - 1)));
  }
  // (a') this lane's slice of the step's q and k: no device scalar in their addresses either.  (v follows the ring: 48 raw
  //      registers in flight next to it are more than 96 VGPRs hold without a spill)
  const float* qp = qkv + (size_t)b * 3 * Dm + h * DH + sub * 16;
  f32x4 qraw[4], kraw[4], vraw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    qraw[i] = *reinterpret_cast<const f32x4*>(qp + 4 * i);
    kraw[i] = *reinterpret_cast<const f32x4*>(qp + Dm + 4 * i);
  }
  // (b) the row's scalars; (c) the rest of the ring, before anything consumes the q / k / v slice (vmcnt is in order)
  const int pos = prefix[0] + len[b];
  const int ks = kv_start[b];
  const int nr = (pos + R - 1) / R;  // rounds [0, nr) hold the keys < pos
#pragma unroll
  for (int u = BLIND; u < D; ++u)
    if (u < nr) {  // block-uniform
      kr[u] = ld16_nt(kc + off_of(u, min(an[u], nb - 1)));
      vr[u] = ld16_nt(vc + off_of(u, min(an[u], nb - 1)));
    }
  if constexpr (ANC) {  // the bytes of batch 1, right behind batch 0's requests
#pragma unroll
    for (int u = 0; u < D; ++u) an[u] = arow[key_of(D + u)];
  }
  // (d) q * scale; this step's k / v rounded as the cache rounds, appended, and taken as the initial state of slot 0
  float qr[16], acc[16];
  float m = -INFINITY, l = 0.f;
  {
    u32x4 kw, vw;
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kw[i] = fp8_pack4(kraw[i][0], kraw[i][1], kraw[i][2], kraw[i][3]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qr[4 * i + e] = qraw[i][e] * scale;
        dot = fmaf(qr[4 * i + e], fp8_get(kw[i], e), dot);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) vraw[i] = *reinterpret_cast<const f32x4*>(qp + 2 * Dm + 4 * i);
    dot = dpp_add<0xB1>(dot);
    dot = dpp_add<0x4E>(dot);
#pragma unroll
    for (int i = 0; i < 4; ++i) vw[i] = fp8_pack4(vraw[i][0], vraw[i][1], vraw[i][2], vraw[i][3]);
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    if (wave == 0 && lane < 4) {  // slot 0 of wave 0, its four lanes cover the 64 dims: the row's own physical cache row, whatever the ancestry says
      *reinterpret_cast<u32x4*>(kc + (own + (uint32_t)pos * DH)) = kw;
      *reinterpret_cast<u32x4*>(vc + (own + (uint32_t)pos * DH)) = vw;
      m = dot;
      l = 1.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = fp8_get(vw[i >> 2], i & 3);
    }
  }
  // (e) the key loop: one batch of D rounds per trip
  for (int base = 0; base < nr; base += D) {
    float sc[D];
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int r = base + u, j = r * R + slot;
      float t = 0.f;
      if (r < nr) t = kv8_score(qr, kr[u]);           // block-uniform: a round at or past nr holds no visible key, or no data at all
      sc[u] = (j >= ks && j < pos) ? t : -INFINITY;  // (j < pos implies r < nr)
    }
    // the next batch's K into the registers just freed (ANC: together with its V below, see there)
    if constexpr (!ANC) {
#pragma unroll
      for (int u = 0; u < D; ++u)
        if (base + D + u < nr) kr[u] = ld16_nt(kc + off_of(base + D + u, 0));
    }
    float mw = sc[0];
#pragma unroll
    for (int u = 1; u < D; ++u) mw = fmaxf(mw, sc[u]);
    const float mn = fmaxf(m, mw);
    const float mref = mn > -INFINITY ? mn : 0.f;  // a slot that has seen no key yet: every exp below is exp(-inf) = 0
    const float alpha = __expf(m - mref);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] *= alpha;
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int r = base + u;
      if (r < nr) {
        const float p = __expf(sc[u] - mref);
        l += p;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)vr[u][w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)vr[u][w], true);
          acc[4 * w] = fmaf(p, lo[0], acc[4 * w]);
          acc[4 * w + 1] = fmaf(p, lo[1], acc[4 * w + 1]);
          acc[4 * w + 2] = fmaf(p, hi[0], acc[4 * w + 2]);
          acc[4 * w + 3] = fmaf(p, hi[1], acc[4 * w + 3]);
        }
      }
      // ANC: the round's row from the byte loaded a batch ago, then the byte of the batch after it (clamped: always inside the
      // table).  That byte is older than every load the next trip's wait for it has not already waited for
      const int a = ANC ? min(an[u], nb - 1) : 0;
      if constexpr (ANC) an[u] = arow[key_of(base + 2 * D + u)];
      if (base + D + u < nr) {
        if constexpr (ANC) kr[u] = ld16_nt(kc + off_of(base + D + u, a));
        vr[u] = ld16_nt(vc + off_of(base + D + u, a));
      }
    }
    m = mn;
  }
  // (f) merge the 16 slots of the wave (lanes of equal `sub`), then the four waves
  float M = fmaxf(m, quad_away(m));
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) M = wave_bfly_max(M, o);
  const float sc0 = M > -INFINITY ? __expf(m - M) : 0.f;
  l *= sc0;
  l += quad_away(l);
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) l = wave_bfly_sum(l, o);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    acc[i] *= sc0;
    acc[i] += quad_away(acc[i]);
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) acc[i] = wave_bfly_sum(acc[i], o);
  }
  if (lane < 4)
#pragma unroll
    for (int i = 0; i < 16; ++i) so[wave][lane * 16 + i] = acc[i];
  if (lane == 0) {
    sm[wave] = M;
    sl[wave] = l;
  }
  __syncthreads();
  if (wave == 0) {
    const int tid = lane;  // threads 0 .. 63
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
    // wave 0 always holds the appended key: L >= exp(m0 - MM) > 0
    stf(ctx + (ctx_bt ? tile_off(b, h * DH + tid, ctx_bt) : (size_t)b * Dm + h * DH + tid), o / L);
  }
}

}  // namespace

int decode_attn_kv8(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start,
                    const int* prefix_dev, int B, int H, int dh, int Smax, int tc, hipStream_t s, int ctx_tiled, const uint8_t* anc,
                    int nb) {
  ITTS_REQUIRE(ctx && qkv && kc && vc && len && kv_start && prefix_dev, "decode_attn_kv8: null pointer (ctx, qkv, kc, vc, len, kv_start, prefix)");
  ITTS_REQUIRE(B >= 1 && H >= 1 && Smax >= 1, "decode_attn_kv8: B, H, Smax must be >= 1");
  ITTS_REQUIRE(tc == FP8, "decode_attn_kv8: the cache must be the fp8 (e4m3) type (the other caches have decode_attn2)");
  ITTS_REQUIRE(dh == 64, "decode_attn_kv8: head dim must be 64");
  ITTS_REQUIRE(to == BF16 || to == F32, "decode_attn_kv8: ctx must be the 16-bit type or fp32");
  ITTS_REQUIRE(!ctx_tiled || to == BF16, "decode_attn_kv8: tiled ctx is 16-bit only");
  ITTS_REQUIRE(!anc || (nb >= 1 && nb <= 16 && B % nb == 0), "decode_attn_kv8: beam ancestry needs B to be a multiple of 1 <= nb <= 16");
  ITTS_REQUIRE(((uintptr_t)kc | (uintptr_t)vc) % 16 == 0, "decode_attn_kv8: the caches must be 16-byte aligned");
  ITTS_REQUIRE((long long)B * H * Smax * 64 < (1ll << 31), "decode_attn_kv8: B * H * Smax * 64 bytes of cache must stay under 2 GiB (32-bit offsets)");
  const float scale = 1.f / sqrtf((float)dh);
  const dim3 grid(H, B);
  const int bt = ctx_tiled ? (B + 15) / 16 : 0;
#define KV8_GO(TO, ANC)                                                                                                         \
  hipLaunchKernelGGL((decode_attn_kv8_kernel<TO, ANC>), grid, dim3(256), 0, s, (TO*)ctx, qkv, (uint8_t*)kc, (uint8_t*)vc, len, \
                     kv_start, prefix_dev, anc, nb, H, Smax, scale, bt)
  if (to == BF16) {
    if (anc)
      KV8_GO(bf16_t, true);
    else
      KV8_GO(bf16_t, false);
  } else {
    if (anc)
      KV8_GO(float, true);
    else
      KV8_GO(float, false);
  }
#undef KV8_GO
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace itts

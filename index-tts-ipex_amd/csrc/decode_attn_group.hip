// ---------------------------------------------------------------------------------------------
// decode_attn_group: cache attention of one decode step under beams with the beam GROUP as the unit of work (opt-in:
// itts_gpt_set_group_attn / ITTS_GROUP_ATTN).  decode_attn2_kernel<.., ANC> runs one workgroup per (beam row, head)
// and every workgroup gathers its whole history through the row's ancestry, although the nb beams of an item share every
// position up to their common ancestor: each shared K / V row is fetched nb times.  Here one workgroup of 4 waves serves a
// (head, item): every needed (position, physical row) is fetched once and scored for all nb queries on the matrix cores.
// This file holds the family: ONE body (group_attn_body) behind the 16-bit kernel, its e4m3 form and its key-split form, and the
// split's merge.  A cache policy holds what depends on the bytes of a row, an output policy where the result goes, which units
// the workgroup walks and whether it takes the appended key (the e4m3 cache with the key split is not instantiated).
//
// Work split: the item's nb queries are the 16 columns of an MFMA tile (columns >= nb are zero and never stored).  Keys are
// dealt to the four waves in units of U positions (unit t to wave t & 3); a wave keeps its own online-softmax state for all
// queries and the waves merge once at the end through LDS.  No workgroup barrier inside the key loop.
// Which rows: need(j) = the set of physical rows that hold position j for some beam (a bit mask built from the nb ancestry
// bytes of the position).  A unit is read in passes: pass p takes, for every position, the p-th row of its set (positions with
// fewer rows are masked), until a ballot finds every set empty - one pass on the trunk, whichever rows the positions alternate
// between, up to nb passes behind the common ancestor.  Query q admits key (j, r) iff anc[q][j] == r and kv_start[q] <= j < pos_q.
// Data: K goes global -> registers in operand layout (lane (fr, fg): key 16 * hh + fr), S^T = K Q^T; a lane then owns query fr and
// keys 4 * fg + r of every 16-key part, and with k-slot (fg, e) = key 16 * (e / 4) + 4 * fg + e % 4 its eight probabilities of 32
// keys ARE the B operand of O^T = V^T P^T.  V is staged per wave in a private LDS tile, transposed on the way in ([dim][key]).
// The unit (t, pass) behind the current one is requested before the current one is computed; the ancestry bytes one unit ahead
// of that.
// Precision: q * scale and P each enter the MFMA as hi + lo of the 16-bit type (two MFMAs each), accumulation is fp32.
// This step's k / v: rounded to the cache type, appended to each beam's OWN row at pos (the bits decode_attn2_kernel writes) as
// 16-byte vector stores and taken into wave 0's state from registers (fp32 score over the rounded k, weight exp(0) at the start,
// the accumulator initialised with the rounded v); the cache row at pos is never admitted.
// Rows outside [kv_start, pos) may hold anything finite: they are masked before the maximum and get weight exp(-inf) = 0.
//
// 16-bit rows (GroupCache16, decode_attn_group_kernel<TILED>): U = 32.  A lane loads dims 32 * c + 8 * fg .. + 7 of its key for
// k-step c.  V: lane (kg = lane >> 3, dg = lane & 7) loads dims 8 * dg .. + 7 of keys 4 * kg .. + 3 and writes 8 bytes of four keys
// per dim into rows of 36 halves; lane (fr = dim, fg) reads them back as two 8-byte reads per dim tile.  Two lanes share an
// ancestry position (beams hq, hq + 2, ..).
//
// e4m3 rows (GroupCache8, decode_attn_group_kv8_kernel<TILED>; opt-in on top of group_attn and the fp8 cache:
// itts_gpt_set_group_attn_kv_fp8 / ITTS_GROUP_ATTN_KV_FP8).  A cache row is 64 bytes, not 128, so the mapping of
// lanes to bytes, the unit and the V transpose are its own.  U = 64: 4 KiB of K + 4 KiB of V, the bytes a unit of the 16-bit form
// has in flight; the four-wave deal is 256.
// K: lane (fr, fg) loads ONE 16-byte piece per 16-key quarter hh: dims 16 fg .. + 15 of key 16 hh + fr (a wave-load covers 16 whole
// rows, 1 KiB contiguous on the trunk).  The contraction of S^T = K Q^T runs over a permutation of the dims: k-step c takes bytes
// 8 c .. + 7 of the lane's load and qhi[c] / qlo[c] hold q dims 16 fg + 8 c .. + 7 - no second load, no shuffle.
// V: lane (kg = lane >> 2, dg = lane & 3) loads dims 16 dg .. + 15 of keys 4 kg .. + 3, transposes the four 4 x 4 byte blocks with
// v_perm_b32 and writes the tile in BYTES, one dword of four keys per dim; lane (fr = dim, fg) reads keys 4 fg .. + 3 of both
// halves of a 32-key k-step back as two dwords: the B-operand property above, twice per unit.
// LDS tile: 64 rows of 16 dwords, NO padding; dword column c of row d lies at c ^ (d & 14) ^ ((d >> 2) & 8), and a lane writes
// its four dims of a block in the order b ^ dg (the v_perm selectors are per lane, so that costs nothing).  A pure row stride
// cannot serve both sides: the writes need an odd stride in dwords, the reads need the sixteen row starts 4 banks apart.
// Checked by enumeration for 64 banks x 4 bytes over the wave and for 32 banks over each half wave: every dword write and every
// dword read touches 64 (32) distinct banks.
// Decoding: e4m3 is exact in bf16 and in binary16.  gfx950's one-step packed converts with a scale of 1 where the compiler has
// them, else v_cvt_pk_f32_fp8 and the upper halves (bf16) / a packed convert (binary16).  The MFMAs stay half_mfma16 on 16-bit
// operands (an fp8 MFMA would round q).  Rounding is fp8_pack4 (the bytes decode_attn2_kernel<fp8_t> and kv_scatter_kernel write).
// kc / vc must be 16-byte aligned (every row is 64 bytes).
//
// Key split (GroupOutPart, decode_attn_group_split_kernel + decode_attn_group_merge_kernel<TILED>; 16-bit rows, opt-in on top of
// group_attn: itts_gpt_set_group_attn_split / ITTS_GROUP_ATTN_SPLIT).  The unsplit grid is (H, items): at 3 to 6
// sentences and H = 20 that is 60 to 120 workgroups on 256 CUs, each walking its whole history.  Here the grid is (H, items, NS),
// 2 <= NS <= 8, and a second, small kernel merges the NS partials.  The host does not know S (the step is replayed from a
// captured graph, len lives on the device), so every workgroup derives its chunk from the item's ksmin / posmax, which it reduces
// anyway: t_first = ksmin >> 5, ntl = ceil(posmax / 32), n = max(ntl - t_first, 0), per = ceil(n / NS) rounded up to a multiple of
// 4 (each of the four waves of a split gets the same share), split z owns tiles [t_first + z * per, min(t_first + (z + 1) * per,
// ntl)).  Only split 0 appends this step's rows and only its wave 0 takes the appended key; the other splits neither read the
// cache row at pos nor write the cache.
// Epilogue: the four waves merge through LDS with max-rescaling, but nothing is normalised: per query q < nb the workgroup writes
// the fp32 accumulator to part_o[z][b][h][0 .. 63] and (m, l) to part_ml[z][b][h][0 .. 1] with plain vector stores.  A split that
// admitted no key for a row (an empty chunk, a chunk outside the row's [kv_start, pos)) writes exactly (-inf, 0) and zeros, and
// every (z, b, h) slot of a launch is written: the merge never reads stale data.
// Merge: 16 lanes per (row, head), four dims each; the NS partials in the fixed order z = 0 .. NS - 1: MM = max m,
// e_z = m_z > -inf ? exp(m_z - MM) : 0, o = sum e_z o_z, L = sum e_z l_z, ctx = o / L in the 16-bit type (row-major or tile_off).
// Split 0 always holds the appended key: L > 0.  No atomics, no tickets, no polling.
// ---------------------------------------------------------------------------------------------
#include "itts_decode.h"
#include "itts_wave_dev.h"

#if defined(__has_builtin)
#if !defined(ITTS_HALF_F16) && __has_builtin(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8)
#define ITTS_KV8_ONE_STEP 1
#elif defined(ITTS_HALF_F16) && __has_builtin(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8)
#define ITTS_KV8_ONE_STEP 1
#endif
#endif

namespace itts {
namespace {

constexpr int GA_DH = 64, GA_NW = 4;
constexpr int GA_VS = 36;  // 16-bit rows: halves per [dim] row of the transposed V tile: 32 keys + 4 (rows stay 8-byte aligned)

// LDS written by some lanes of a wave and read by others: the hardware runs a wave's LDS operations in order, the compiler must
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <typename T> __device__ __forceinline__ u32x4 ld16(const T* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ f32x4 ldf4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// x[0 .. 7] = hi + lo in the 16-bit type, as two MFMA operands
__device__ __forceinline__ void split_hi_lo(const float* x, half8_bits& hi, half8_bits& lo) {
  u32x4 h, l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bf16_t a = (bf16_t)x[2 * i], b = (bf16_t)x[2 * i + 1];
    h[i] = pack_bf16((float)a, (float)b);
    l[i] = pack_bf16(x[2 * i] - (float)a, x[2 * i + 1] - (float)b);
  }
  hi = __builtin_bit_cast(half8_bits, h);
  lo = __builtin_bit_cast(half8_bits, l);
}

// what a workgroup knows of its item and a lane of itself
struct GroupItem {
  const uint8_t* anc;
  int nb, B, b0, Smax, lane;
  unsigned parmask;   // bit q: live ancestry half of beam q
  int posmax, ksmin;  // the item's positions [ksmin, posmax)
  __device__ __forceinline__ uint32_t anc_byte(int q, int j) const {
    return anc[((size_t)((parmask >> q) & 1u) * B + b0 + q) * Smax + j];
  }
};

// ---- cache policy, 16-bit rows ----
struct GroupCache16 {
  using T = bf16_t;   // a cache element
  using VT = bf16_t;  // an element of the transposed V tile
  static constexpr int LOG_U = 5, U = 32, NT = 2, KS = 1, VT_N = GA_DH * GA_VS;  // NT 16-key score tiles, KS 32-key PV k-steps per unit
  const int jj, hq;          // ancestry duty: position jj of the tile, beams hq, hq + 2, ..
  uint32_t a0 = 0, a1 = 0;   // raw ancestry bytes of the next tile to prepare
  __device__ __forceinline__ explicit GroupCache16(int lane) : jj(lane & 31), hq(lane >> 5) {}
  // q dims of the lane's qs[4 * g .. + 3]
  static __device__ __forceinline__ int qdim(int fg, int g) { return 32 * (g >> 1) + 8 * fg + 4 * (g & 1); }
  static __device__ __forceinline__ f32x4 rounded(f32x4 v) {
    return f32x4{(float)(bf16_t)v[0], (float)(bf16_t)v[1], (float)(bf16_t)v[2], (float)(bf16_t)v[3]};
  }
  // this step's k / v rows (kp, vp: fp32) rounded and stored at krow / vrow; the lane's part of q . k over the rounded k
  static __device__ __forceinline__ float append(const float* kp, const float* vp, const float* qs, int fg, bool qok, T* krow, T* vrow) {
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      u32x4 kw, vw;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4 kf = ldf4(kp + qdim(fg, 2 * c + i)), vf = ldf4(vp + qdim(fg, 2 * c + i));
#pragma unroll
        for (int e = 0; e < 4; ++e) dot = fmaf(qs[8 * c + 4 * i + e], (float)(bf16_t)kf[e], dot);
        kw[2 * i] = pack_bf16(kf[0], kf[1]);
        kw[2 * i + 1] = pack_bf16(kf[2], kf[3]);
        vw[2 * i] = pack_bf16(vf[0], vf[1]);
        vw[2 * i + 1] = pack_bf16(vf[2], vf[3]);
      }
      if (qok) {  // the beam's own physical row, whatever the ancestry says
        *reinterpret_cast<u32x4*>(krow + 32 * c + 8 * fg) = kw;
        *reinterpret_cast<u32x4*>(vrow + 32 * c + 8 * fg) = vw;
      }
    }
    return dot;
  }
  __device__ __forceinline__ void load_anc(int tt, const GroupItem& it) {
    const int j = min(tt * U + jj, it.Smax - 1);
    a0 = a1 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      // every load is issued (beams >= nb re-read the last beam's byte, which prep ignores): a load under a lane-dependent
      // branch would wait for its result before the next one is requested
      const uint32_t v = it.anc_byte(min(hq + 2 * i, it.nb - 1), j);
      if (i < 4) a0 |= v << (8 * i);
      else a1 |= v << (8 * (i - 4));
    }
  }
  // a0 / a1 -> s_anc; returns need(j) of the lane's position
  __device__ __forceinline__ unsigned prep(int tt, const GroupItem& it, uint8_t (*s_anc)[U]) const {
    unsigned part = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q = hq + 2 * i;
      if (q < it.nb) {
        const int c = min((int)(((i < 4 ? a0 : a1) >> (8 * (i & 3))) & 255u), it.nb - 1);  // entries at >= pos may be 255
        s_anc[q][jj] = (uint8_t)c;
        part |= 1u << c;
      }
    }
    part |= (unsigned)__shfl_xor((int)part, 32, 64);
    const int j = tt * U + jj;
    return (j >= it.ksmin && j < it.posmax) ? part : 0u;
  }
  // K in operand layout: key 16 * hh + fr (row p), dims 32 * c + 8 * fg
  static __device__ __forceinline__ void load_k(u32x4 (&kk)[4], int hh, const T* p, int fg) {
    kk[2 * hh] = ld16(p + 8 * fg);
    kk[2 * hh + 1] = ld16(p + 8 * fg + 32);
  }
  static __device__ __forceinline__ half8_bits k_operand(const u32x4 (&kk)[4], int hh, int c) {
    return __builtin_bit_cast(half8_bits, kk[2 * hh + c]);
  }
  __device__ __forceinline__ void store_vt(const u32x4 (&vv)[4], VT* s_vt, int kg, int dg) const {
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // V, transposed: dim 8 * dg + i of keys 4 * kg .. + 3
      const int w = i >> 1;
      u32x2 x;
      if (i & 1) {
        x[0] = (vv[0][w] >> 16) | (vv[1][w] & 0xFFFF0000u);
        x[1] = (vv[2][w] >> 16) | (vv[3][w] & 0xFFFF0000u);
      } else {
        x[0] = (vv[0][w] & 0xFFFFu) | (vv[1][w] << 16);
        x[1] = (vv[2][w] & 0xFFFFu) | (vv[3][w] << 16);
      }
      *reinterpret_cast<u32x2*>(&s_vt[(8 * dg + i) * GA_VS + 4 * kg]) = x;
    }
  }
  static __device__ __forceinline__ half8_bits v_operand(const VT* s_vt, int d, int, int fg) {
    const bf16_t* vr = &s_vt[d * GA_VS + 4 * fg];
    const u32x2 v0 = *reinterpret_cast<const u32x2*>(vr), v1 = *reinterpret_cast<const u32x2*>(vr + 16);
    return __builtin_bit_cast(half8_bits, u32x4{v0[0], v0[1], v1[0], v1[1]});
  }
};

// four e4m3 bytes -> four values of the 16-bit type in byte order, exact in both builds
__device__ __forceinline__ u32x2 dec4(uint32_t w) {
  u32x2 r;
#ifdef ITTS_KV8_ONE_STEP
#ifdef ITTS_HALF_F16
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.f, false));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.f, true));
#else
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.f, false));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.f, true));
#endif
#else
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
#ifdef ITTS_HALF_F16
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(lo[0], lo[1]));  // exact: nothing to round
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(hi[0], hi[1]));
#else
  r[0] = __builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u);  // the upper halves
  r[1] = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
#endif
#endif
  return r;
}
__device__ __forceinline__ half8_bits dec8(uint32_t w0, uint32_t w1) {
  const u32x2 a = dec4(w0), b = dec4(w1);
  return __builtin_bit_cast(half8_bits, u32x4{a[0], a[1], b[0], b[1]});
}

// dword index of (dim d, key column c = key / 4) in a wave's transposed V tile of e4m3 rows
__device__ __forceinline__ int vt_idx(int d, int c) { return d * 16 + (c ^ (d & 14) ^ ((d >> 2) & 8)); }

// ---- cache policy, e4m3 rows ----
struct GroupCache8 {
  using T = uint8_t;
  using VT = uint32_t;  // the V tile in bytes, addressed by dwords of four keys
  static constexpr int LOG_U = 6, U = 64, NT = 4, KS = 2, VT_N = GA_DH * 16;
  // the lane writes dim 4 w + (b ^ dg) of block w as its b-th store: the selectors of the two v_perm stages, per lane
  const uint32_t selA, selB, selC, selD;
  uint32_t araw[4] = {0, 0, 0, 0};  // raw ancestry bytes of the next unit to prepare: beam q in byte q & 3 of word q >> 2
  __device__ __forceinline__ explicit GroupCache8(int lane)
      : selA((lane & 2) ? 0x07030602u : 0x05010400u), selB((lane & 2) ? 0x05010400u : 0x07030602u),
        selC((lane & 1) ? 0x07060302u : 0x05040100u), selD((lane & 1) ? 0x05040100u : 0x07060302u) {}
  static __device__ __forceinline__ int qdim(int fg, int g) { return 16 * fg + 4 * g; }
  static __device__ __forceinline__ f32x4 rounded(f32x4 v) {
    const uint32_t w = fp8_pack4(v[0], v[1], v[2], v[3]);
    return f32x4{fp8_get(w, 0), fp8_get(w, 1), fp8_get(w, 2), fp8_get(w, 3)};
  }
  static __device__ __forceinline__ float append(const float* kp, const float* vp, const float* qs, int fg, bool qok, T* krow, T* vrow) {
    float dot = 0.f;
    u32x4 kw, vw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 kf = ldf4(kp + qdim(fg, i)), vf = ldf4(vp + qdim(fg, i));
      kw[i] = fp8_pack4(kf[0], kf[1], kf[2], kf[3]);
      vw[i] = fp8_pack4(vf[0], vf[1], vf[2], vf[3]);
#pragma unroll
      for (int e = 0; e < 4; ++e) dot = fmaf(qs[4 * i + e], fp8_get(kw[i], e), dot);
    }
    if (qok) {  // the beam's own physical row, whatever the ancestry says
      *reinterpret_cast<u32x4*>(krow + 16 * fg) = kw;
      *reinterpret_cast<u32x4*>(vrow + 16 * fg) = vw;
    }
    return dot;
  }
  __device__ __forceinline__ void load_anc(int tt, const GroupItem& it) {
    const int j = min(tt * U + it.lane, it.Smax - 1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      araw[g] = 0;
      if (4 * g < it.nb) {  // wave-uniform; inside, every load is issued (beams >= nb re-read the last beam's byte, which prep ignores)
#pragma unroll
        for (int i = 0; i < 4; ++i) araw[g] |= it.anc_byte(min(4 * g + i, it.nb - 1), j) << (8 * i);
      }
    }
  }
  // araw -> s_anc; returns need(j) of the lane's position
  __device__ __forceinline__ unsigned prep(int tt, const GroupItem& it, uint8_t (*s_anc)[U]) const {
    unsigned part = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (q < it.nb) {  // wave-uniform
        const int c = min((int)((araw[q >> 2] >> (8 * (q & 3))) & 255u), it.nb - 1);  // entries at >= pos may be 255
        s_anc[q][it.lane] = (uint8_t)c;
        part |= 1u << c;
      }
    }
    const int j = tt * U + it.lane;
    return (j >= it.ksmin && j < it.posmax) ? part : 0u;
  }
  // K in operand layout: key 16 * hh + fr (row p), dims 16 * fg .. + 15
  static __device__ __forceinline__ void load_k(u32x4 (&kk)[4], int hh, const T* p, int fg) { kk[hh] = ld16(p + 16 * fg); }
  static __device__ __forceinline__ half8_bits k_operand(const u32x4 (&kk)[4], int hh, int c) {
    return dec8(kk[hh][2 * c], kk[hh][2 * c + 1]);
  }
  __device__ __forceinline__ void store_vt(const u32x4 (&vv)[4], VT* s_vt, int kg, int dg) const {
#pragma unroll
    for (int w = 0; w < 4; ++w) {  // V, transposed: the 4 x 4 byte block of dims 16 * dg + 4 * w .. + 3, keys 4 * kg .. + 3
      const uint32_t x0 = __builtin_amdgcn_perm(vv[1][w], vv[0][w], selA), x1 = __builtin_amdgcn_perm(vv[1][w], vv[0][w], selB);
      const uint32_t y0 = __builtin_amdgcn_perm(vv[3][w], vv[2][w], selA), y1 = __builtin_amdgcn_perm(vv[3][w], vv[2][w], selB);
      const uint32_t o[4] = {__builtin_amdgcn_perm(y0, x0, selC), __builtin_amdgcn_perm(y0, x0, selD),
                             __builtin_amdgcn_perm(y1, x1, selC), __builtin_amdgcn_perm(y1, x1, selD)};
#pragma unroll
      for (int b = 0; b < 4; ++b) s_vt[vt_idx(16 * dg + 4 * w + (b ^ dg), kg)] = o[b];
    }
  }
  // keys 32 * ks .. + 31: k-slot (fg, e) = key 32 * ks + 16 * (e / 4) + 4 * fg + e % 4
  static __device__ __forceinline__ half8_bits v_operand(const VT* s_vt, int d, int ks, int fg) {
    return dec8(s_vt[vt_idx(d, 8 * ks + fg)], s_vt[vt_idx(d, 8 * ks + 4 + fg)]);
  }
};

// ---- output policies.  VW: dims per thread in the combination of the four waves ----
template <bool TILED>
struct GroupOutCtx {  // the whole item; normalised ctx, row-major or tile_off
  static constexpr int VW = 1;
  bf16_t* ctx;
  int ctx_bt;
  __device__ __forceinline__ bool takes_append() const { return true; }
  __device__ __forceinline__ void range(int t_first, int ntl, int& t0, int& t_end) const { t0 = t_first, t_end = ntl; }
  // wave 0 always holds the appended key: L >= exp(m0 - MM) > 0
  __device__ __forceinline__ void store(int b, int B, int h, int H, int d, const float (&o)[1], float, float L) const {
    stf(ctx + (TILED ? tile_off(b, h * GA_DH + d, ctx_bt) : (size_t)b * H * GA_DH + h * GA_DH + d), o[0] / L);
  }
};
struct GroupOutPart {  // chunk z of NS; un-normalised partials.  part_o [NS][B][H][64], part_ml [NS][B][H][2] (m, l), fp32
  static constexpr int VW = 4;
  float *part_o, *part_ml;
  int z, NS;
  __device__ __forceinline__ bool takes_append() const { return z == 0; }
  __device__ __forceinline__ void range(int t_first, int ntl, int& t0, int& t_end) const {
    const int per = ((max(ntl - t_first, 0) + NS - 1) / NS + 3) & ~3;
    t0 = t_first + z * per;
    t_end = min(t_first + (z + 1) * per, ntl);
  }
  // a wave (a split) that admitted no key: m = -inf, weight 0 -> (-inf, 0) and zeros
  __device__ __forceinline__ void store(int b, int B, int h, int H, int d, const float (&o)[4], float MM, float L) const {
    const size_t slot = ((size_t)z * B + b) * H + h;
    *reinterpret_cast<f32x4*>(part_o + slot * GA_DH + d) = f32x4{o[0], o[1], o[2], o[3]};
    if (d == 0) *reinterpret_cast<float2*>(part_ml + slot * 2) = float2{MM, L};
  }
};

// ---- the body: grid (H, items[, NS]), 256 threads ----
template <class CP, class OP>
__device__ __forceinline__ void group_attn_body(const OP out, const float* __restrict__ qkv, typename CP::T* __restrict__ kc,
                                                typename CP::T* __restrict__ vc, const int* __restrict__ len,
                                                const int* __restrict__ kv_start, const int* __restrict__ prefix,
                                                const uint8_t* __restrict__ anc, int nb, int H, int Smax, float scale) {
  constexpr int DH = GA_DH, NW = GA_NW, U = CP::U, NT = CP::NT, NSC = 4 * NT;  // NSC scores per lane and unit
  constexpr int VE = 16 / sizeof(typename CP::T), LPK = DH / VE;  // V duty: 16 bytes = VE dims per lane, LPK lanes per key
  __shared__ __attribute__((aligned(16))) typename CP::VT s_vt[NW][CP::VT_N];  // per wave: V of the current unit, [dim][key]
  __shared__ __attribute__((aligned(4))) uint8_t s_anc[NW][16][U];  // per wave: clamped ancestry of the unit being issued
  __shared__ __attribute__((aligned(4))) uint8_t s_row[NW][U];      // per wave: physical row of each position in this pass
  __shared__ float s_m[NW][16], s_l[NW][16];
  __shared__ float s_o[NW][16][DH + 1];
  const int h = blockIdx.x, b0 = blockIdx.y * nb, B = gridDim.y * nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int D = H * DH;
  // ---- the lane's query (fr) and the item's range of positions ----
  const bool qok = fr < nb;
  const int qrow = b0 + (qok ? fr : 0);
  const int mylen = len[qrow], myks = kv_start[qrow];
  const int pos = prefix[0] + mylen;
  GroupItem it{anc, nb, B, b0, Smax, lane, (unsigned)__ballot(qok && fg == 0 && (mylen & 1)) & 0xFFFFu, qok ? pos : 0,
               qok ? myks : 0x7FFFFFFF};
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    it.posmax = max(it.posmax, __shfl_xor(it.posmax, o, 64));
    it.ksmin = min(it.ksmin, __shfl_xor(it.ksmin, o, 64));
  }
  // ---- q * scale as hi + lo operands; this step's k / v (wave 0 of the workgroup that takes it): rounded, appended, taken into the state ----
  const float* qp = qkv + (size_t)qrow * 3 * D + h * DH;
  CP cp(lane);
  half8_bits qhi[2], qlo[2];
  float m = -INFINITY, l = 0.f;
  f32x4 acc[4];
#pragma unroll
  for (int d0 = 0; d0 < 4; ++d0) acc[d0] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    float qs[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = ldf4(qp + CP::qdim(fg, g));
#pragma unroll
      for (int e = 0; e < 4; ++e) qs[4 * g + e] = qok ? v[e] * scale : 0.f;
    }
    split_hi_lo(qs, qhi[0], qlo[0]);
    split_hi_lo(qs + 8, qhi[1], qlo[1]);
    if (wave == 0 && out.takes_append()) {
      const size_t o = (((size_t)qrow * H + h) * Smax + pos) * DH;
      float dot = CP::append(qp + D, qp + 2 * D, qs, fg, qok, kc + o, vc + o);
      dot = wave_bfly_sum(dot, 16);
      dot = wave_bfly_sum(dot, 32);
      if (qok) {
        m = dot;
        l = fg == 0 ? 1.f : 0.f;  // l is summed over fg at the end
#pragma unroll
        for (int d0 = 0; d0 < 4; ++d0)  // the accumulator's dims of this lane: 16 * d0 + 4 * fg + r
          acc[d0] = CP::rounded(ldf4(qp + 2 * D + 16 * d0 + 4 * fg));
      }
    }
  }
  // ---- the workgroup's units and the key loop over them ----
  const int ntl = (it.posmax + U - 1) >> CP::LOG_U;  // units [0, ntl) hold the positions < posmax
  int t, t_end;
  out.range(it.ksmin >> CP::LOG_U, ntl, t, t_end);  // from the first unit that holds a position >= ksmin
  t += (wave - t) & 3;                              // the first unit of this wave in the range
  const int kg = lane / LPK, dg = lane % LPK;       // V duty: keys 4 * kg .. + 3, dims VE * dg .. + VE - 1
  unsigned rem = 0;                                 // rows of the lane's position not yet read
  auto prep = [&](int tt) {
    wave_lds_sync();
    rem = cp.prep(tt, it, s_anc[wave]);
  };
  auto issue = [&](int tt, u32x4 (&kk)[4], u32x4 (&vv)[4], uint32_t& adm) {
    wave_lds_sync();
    if (lane < U) s_row[wave][lane] = rem ? (uint8_t)__builtin_ctz(rem) : (uint8_t)255;
    rem &= rem - 1;
    wave_lds_sync();
#pragma unroll
    for (int hh = 0; hh < NT; ++hh) {
      const int j = min(tt * U + 16 * hh + fr, Smax - 1);
      int r = s_row[wave][16 * hh + fr];
      r = r == 255 ? 0 : r;
      CP::load_k(kk, hh, kc + (((size_t)(b0 + r) * H + h) * Smax + j) * DH, fg);
    }
    const uint32_t rv = *reinterpret_cast<const uint32_t*>(&s_row[wave][4 * kg]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = min(tt * U + 4 * kg + i, Smax - 1);
      int r = (rv >> (8 * i)) & 255u;
      r = r == 255 ? 0 : r;
      vv[i] = ld16(vc + (((size_t)(b0 + r) * H + h) * Smax + j) * DH + VE * dg);
    }
    adm = 0;  // the admission mask: bit 4 * hh + r for key 16 * hh + 4 * fg + r of the unit
#pragma unroll
    for (int hh = 0; hh < NT; ++hh) {
      const uint32_t aw = *reinterpret_cast<const uint32_t*>(&s_anc[wave][fr][16 * hh + 4 * fg]);
      const uint32_t rw = *reinterpret_cast<const uint32_t*>(&s_row[wave][16 * hh + 4 * fg]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = tt * U + 16 * hh + 4 * fg + r;
        const bool ok = qok && ((aw >> (8 * r)) & 255u) == ((rw >> (8 * r)) & 255u) && j >= myks && j < pos;
        adm |= (ok ? 1u : 0u) << (4 * hh + r);
      }
    }
  };
  auto compute = [&](const u32x4 (&kk)[4], const u32x4 (&vv)[4], uint32_t adm) {
    wave_lds_sync();
    cp.store_vt(vv, s_vt[wave], kg, dg);
    f32x4 s[NT];
#pragma unroll
    for (int hh = 0; hh < NT; ++hh) {
      s[hh] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const half8_bits kf = CP::k_operand(kk, hh, c);
        s[hh] = half_mfma16(kf, qhi[c], s[hh]);
        s[hh] = half_mfma16(kf, qlo[c], s[hh]);
      }
    }
    float sc[NSC], tmax = -INFINITY;  // the masked online-softmax update
#pragma unroll
    for (int e = 0; e < NSC; ++e) {
      sc[e] = ((adm >> e) & 1u) ? s[e >> 2][e & 3] : -INFINITY;  // masked before the maximum
      tmax = fmaxf(tmax, sc[e]);
    }
    tmax = wave_bfly_max(tmax, 16);
    tmax = wave_bfly_max(tmax, 32);
    const float mn = fmaxf(m, tmax);
    float p[NSC];
    if (mn > -INFINITY) {
      const float alpha = __expf(m - mn);  // exp(-inf) = 0 for a fresh state
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < NSC; ++e) {
        p[e] = __expf(sc[e] - mn);
        ps += p[e];
      }
      l = fmaf(l, alpha, ps);
#pragma unroll
      for (int d0 = 0; d0 < 4; ++d0) acc[d0] *= alpha;
      m = mn;
    } else {
#pragma unroll
      for (int e = 0; e < NSC; ++e) p[e] = 0.f;
    }
    wave_lds_sync();
#pragma unroll
    for (int ks = 0; ks < CP::KS; ++ks) {
      half8_bits phi, plo;
      split_hi_lo(p + 8 * ks, phi, plo);
#pragma unroll
      for (int d0 = 0; d0 < 4; ++d0) {
        const half8_bits vf = CP::v_operand(s_vt[wave], 16 * d0 + fr, ks, fg);
        acc[d0] = half_mfma16(vf, phi, acc[d0]);
        acc[d0] = half_mfma16(vf, plo, acc[d0]);
      }
    }
  };
  u32x4 kn[4], vn[4];
  uint32_t admn = 0;
  bool have = t < t_end;
  if (have) {
    cp.load_anc(t, it);
    prep(t);
    if (t + 4 < t_end) cp.load_anc(t + 4, it);
    issue(t, kn, vn, admn);
  }
  while (have) {
    u32x4 kcur[4], vcur[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kcur[i] = kn[i];
      vcur[i] = vn[i];
    }
    const uint32_t admc = admn;
    if (__ballot(rem != 0) == 0) {  // every position's rows are read: on to this wave's next unit
      t += 4;
      have = t < t_end;
      if (have) {
        prep(t);
        if (t + 4 < t_end) cp.load_anc(t + 4, it);
      }
    }
    if (have) issue(t, kn, vn, admn);
    compute(kcur, vcur, admc);
  }
  // ---- merge the four waves: thread (q, dv) combines VW dims of query q ----
  l = wave_bfly_sum(l, 16);
  l = wave_bfly_sum(l, 32);
  if (fg == 0) {
    s_m[wave][fr] = m;
    s_l[wave][fr] = l;
  }
#pragma unroll
  for (int d0 = 0; d0 < 4; ++d0)
#pragma unroll
    for (int r = 0; r < 4; ++r) s_o[wave][fr][16 * d0 + 4 * fg + r] = acc[d0][r];
  __syncthreads();
  constexpr int VW = OP::VW, TPQ = DH / VW;
  for (int idx = tid; idx < nb * TPQ; idx += 256) {
    const int q = idx / TPQ, d = (idx % TPQ) * VW;
    float MM = s_m[0][q];
#pragma unroll
    for (int w = 1; w < NW; ++w) MM = fmaxf(MM, s_m[w][q]);
    float o[VW], L = 0.f;
#pragma unroll
    for (int r = 0; r < VW; ++r) o[r] = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float e = s_m[w][q] > -INFINITY ? __expf(s_m[w][q] - MM) : 0.f;
#pragma unroll
      for (int r = 0; r < VW; ++r) o[r] = fmaf(e, s_o[w][q][d + r], o[r]);
      L = fmaf(e, s_l[w][q], L);
    }
    out.store(b0 + q, B, h, H, d, o, MM, L);
  }
}

template <bool TILED>
__global__ __launch_bounds__(256) void decode_attn_group_kernel(bf16_t* __restrict__ ctx, const float* __restrict__ qkv,
                                                                bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                                const int* __restrict__ len, const int* __restrict__ kv_start,
                                                                const int* __restrict__ prefix, const uint8_t* __restrict__ anc,
                                                                int nb, int H, int Smax, float scale, int ctx_bt) {
  group_attn_body<GroupCache16>(GroupOutCtx<TILED>{ctx, ctx_bt}, qkv, kc, vc, len, kv_start, prefix, anc, nb, H, Smax, scale);
}

template <bool TILED>
__global__ __launch_bounds__(256) void decode_attn_group_kv8_kernel(bf16_t* __restrict__ ctx, const float* __restrict__ qkv,
                                                                    uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                                    const int* __restrict__ len, const int* __restrict__ kv_start,
                                                                    const int* __restrict__ prefix, const uint8_t* __restrict__ anc,
                                                                    int nb, int H, int Smax, float scale, int ctx_bt) {
  group_attn_body<GroupCache8>(GroupOutCtx<TILED>{ctx, ctx_bt}, qkv, kc, vc, len, kv_start, prefix, anc, nb, H, Smax, scale);
}

// grid (H, items, NS)
__global__ __launch_bounds__(256) void decode_attn_group_split_kernel(float* __restrict__ part_o, float* __restrict__ part_ml,
                                                                      const float* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                                      bf16_t* __restrict__ vc, const int* __restrict__ len,
                                                                      const int* __restrict__ kv_start, const int* __restrict__ prefix,
                                                                      const uint8_t* __restrict__ anc, int nb, int H, int Smax,
                                                                      float scale) {
  group_attn_body<GroupCache16>(GroupOutPart{part_o, part_ml, (int)blockIdx.z, (int)gridDim.z}, qkv, kc, vc, len, kv_start, prefix,
                                anc, nb, H, Smax, scale);
}

// 256 threads = 16 (row, head) pairs of 16 lanes, lane dl owns dims 4 * dl .. + 3.  BH = B * H pairs
template <bool TILED>
__global__ __launch_bounds__(256) void decode_attn_group_merge_kernel(bf16_t* __restrict__ ctx, const float* __restrict__ part_o,
                                                                      const float* __restrict__ part_ml, int BH, int H, int NS,
                                                                      int ctx_bt) {
  const int pair = blockIdx.x * 16 + (threadIdx.x >> 4), dl = threadIdx.x & 15;
  if (pair >= BH) return;
  float MM = -INFINITY;
  for (int z = 0; z < NS; ++z) MM = fmaxf(MM, part_ml[((size_t)z * BH + pair) * 2]);
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  float L = 0.f;
  for (int z = 0; z < NS; ++z) {
    const size_t slot = (size_t)z * BH + pair;
    const float2 ml = *reinterpret_cast<const float2*>(part_ml + slot * 2);
    const f32x4 oz = *reinterpret_cast<const f32x4*>(part_o + slot * 64 + 4 * dl);
    const float e = ml.x > -INFINITY ? __expf(ml.x - MM) : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = fmaf(e, oz[r], o[r]);
    L = fmaf(e, ml.y, L);
  }
  const int b = pair / H, col = (pair - b * H) * 64 + 4 * dl;  // split 0 always holds the appended key: L > 0
  u32x2 w;
  w[0] = pack_bf16(o[0] / L, o[1] / L);
  w[1] = pack_bf16(o[2] / L, o[3] / L);
  // four neighbouring dims are neighbours in both layouts (tile_off keeps k % 8 together)
  *reinterpret_cast<u32x2*>(ctx + (TILED ? tile_off(b, col, ctx_bt) : (size_t)b * H * 64 + col)) = w;
}

// what the three entry points require alike; fn starts every message, want is the entry's cache type.  The 16-bit entries name the
// tiled ctx in a message of its own; decode_attn_group_kv8 never did and passes ctx_tiled = 0.  fn + ".." joins the std::string
// that ITTS_REQUIRE builds in its failing branch: a passing launch builds no string
int group_attn_check(const char* fn, int dh, int nb, int B, const uint8_t* anc, int tc, int want, int to, int ctx_tiled) {
  ITTS_REQUIRE(dh == 64, fn + ": head dim must be 64");
  ITTS_REQUIRE(nb >= 2 && nb <= 16, fn + ": needs 2 <= nb <= 16 beams per item");
  ITTS_REQUIRE(B % nb == 0, fn + ": B must be a multiple of nb");
  ITTS_REQUIRE(anc, fn + ": the beam ancestry is missing");
  if (want == FP8) ITTS_REQUIRE(tc == FP8, fn + ": the cache must be the fp8 (e4m3) type (a 16-bit cache has decode_attn_group)");
  else ITTS_REQUIRE(tc == BF16, fn + ": the cache must be the 16-bit type (no fp32, no fp8 cache)");
  ITTS_REQUIRE(!ctx_tiled || to == BF16, fn + ": tiled ctx is the 16-bit type only");
  ITTS_REQUIRE(to == BF16, fn + ": ctx must be the 16-bit type");
  return OK;
}

// one launch of the kernel's tiled or row-major instantiation; args end with the number of 16-row tiles of a tiled ctx (else 0)
template <class K, class... A>
int launch_tiled(K* tiled, K* plain, int ctx_tiled, int B, dim3 grid, hipStream_t s, A... args) {
  hipLaunchKernelGGL(ctx_tiled ? tiled : plain, grid, dim3(256), 0, s, args..., ctx_tiled ? (B + 15) / 16 : 0);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace

int decode_attn_group(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start,
                      const int* prefix_dev, int B, int H, int dh, int Smax, int tc, hipStream_t s, int ctx_tiled,
                      const uint8_t* anc, int nb) {
  if (int st = group_attn_check("decode_attn_group", dh, nb, B, anc, tc, BF16, to, ctx_tiled)) return st;
  return launch_tiled(decode_attn_group_kernel<true>, decode_attn_group_kernel<false>, ctx_tiled, B, dim3(H, B / nb), s, (bf16_t*)ctx,
                      qkv, (bf16_t*)kc, (bf16_t*)vc, len, kv_start, prefix_dev, anc, nb, H, Smax, 1.f / sqrtf((float)dh));
}

int decode_attn_group_kv8(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start,
                          const int* prefix_dev, int B, int H, int dh, int Smax, int tc, hipStream_t s, int ctx_tiled,
                          const uint8_t* anc, int nb) {
  if (int st = group_attn_check("decode_attn_group_kv8", dh, nb, B, anc, tc, FP8, to, 0)) return st;
  ITTS_REQUIRE(((uintptr_t)kc | (uintptr_t)vc) % 16 == 0, "decode_attn_group_kv8: the caches must be 16-byte aligned");
  return launch_tiled(decode_attn_group_kv8_kernel<true>, decode_attn_group_kv8_kernel<false>, ctx_tiled, B, dim3(H, B / nb), s,
                      (bf16_t*)ctx, qkv, (uint8_t*)kc, (uint8_t*)vc, len, kv_start, prefix_dev, anc, nb, H, Smax, 1.f / sqrtf((float)dh));
}

int decode_attn_group_split(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start,
                            const int* prefix_dev, int B, int H, int dh, int Smax, int tc, hipStream_t s, int ctx_tiled,
                            const uint8_t* anc, int nb, int nsplit, float* part_o, float* part_ml) {
  if (int st = group_attn_check("decode_attn_group_split", dh, nb, B, anc, tc, BF16, to, ctx_tiled)) return st;
  ITTS_REQUIRE(nsplit >= 2 && nsplit <= GROUP_SPLIT_MAX, "decode_attn_group_split: needs 2 <= nsplit <= 8 splits");
  ITTS_REQUIRE(part_o && part_ml, "decode_attn_group_split: the partial workspaces are missing");
  const int BH = B * H;
  hipLaunchKernelGGL(decode_attn_group_split_kernel, dim3(H, B / nb, nsplit), dim3(256), 0, s, part_o, part_ml, qkv, (bf16_t*)kc,
                     (bf16_t*)vc, len, kv_start, prefix_dev, anc, nb, H, Smax, 1.f / sqrtf((float)dh));
  ITTS_HIP_CHECK(hipGetLastError());
  return launch_tiled(decode_attn_group_merge_kernel<true>, decode_attn_group_merge_kernel<false>, ctx_tiled, B, dim3((BH + 15) / 16),
                      s, (bf16_t*)ctx, (const float*)part_o, (const float*)part_ml, BH, H, nsplit);
}

// NS for H * items workgroups of the unsplit kernel (1: do not split).  Measured (profiles/group_attn_split.txt): the rule wants the
// largest NS of a band that is not slower than the unsplit kernel at S = 200, 500 AND 900 on the trunk, and the host cannot see S.
// At 60 to 240 workgroups every NS loses at S = 200 (1.15 to 1.9 of the time: the second launch and the partials cost more than
// the short history gives back), so no band has such an NS: the switch at 1 keeps the unsplit kernel, 2 .. 8 force the split
int group_split_rule(int H, int items) {
  (void)H;
  (void)items;
  return 1;
}

}  // namespace itts

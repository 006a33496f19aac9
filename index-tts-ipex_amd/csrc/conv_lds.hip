// LDS-tiled 1-D convolution on the matrix cores for the narrow BigVGAN stages (AMPBlock1 convs with C = 24 / 48 / 96
// channels, k = 3 / 7 / 11, dilation 1 / 3 / 5; indextts/BigVGAN/models.py:20-81).
//
// The generic shift-GEMM (gemm_mfma.hip) re-fetches the activation rows once per tap; with K = k*C this small the
// kernel is bound by that global->LDS traffic, not by MFMA.  Here one workgroup owns a time tile of one batch item:
// the BM + (k-1)*dil input rows it needs (halo included, zero padded) are brought into LDS ONCE with contiguous
// 16-byte loads (channels-last rows are adjacent in memory), every tap then reads its MFMA A-fragments from that
// resident tile at a row offset.  Only the small weight slab streams (32-channel chunks, register-staged pairs).
// The epilogue goes back through LDS so residual / accumulate reads and the output store are 16-byte row-contiguous
// (C = 24 rows are 48 bytes: per-lane scalar stores would waste most of every HBM burst).
// v_mfma_f32_16x16x32_bf16; fp32 accumulation; bf16 in / out.
//
// LDS image (r04): one PLANE per 32-channel k-step, rows of 64 bytes (four 16-byte slots), slot g of row r at physical slot
// g ^ ((r >> 1) & 2).  A ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH
// LDS table): eight fragment rows at k-slot g beside the eight others at g + 1 - with any LINEAR row pitch two of those sixteen
// 16-byte reads always share a bank quartet (r03 counters: 6.9 M conflict cycles on 3.8 M active ones; the "odd multiple of
// 16 bytes" pitch was derived for contiguous 16-lane groups), with this key the sixteen land on sixteen different quartets for
// every row offset a tap adds.  The staged weight rows use the same 64-byte image.
//
// ACT (r04): Activation1d - the anti-aliased SnakeBeta that precedes EVERY one of these convolutions (a -> conv, models.py:65-74) -
// runs inside this kernel: the raw rows (tile + halo + 6 on either side for the FIR windows, replicate-clamped) are staged once,
// every lane slides down one channel (itts_snake_dev.h: the stand-alone kernel's loop, same operations) and writes the bf16
// result straight into the MFMA planes.  The stand-alone pass read and wrote the whole tensor once more per convolution: on these
// stages (HBM-bound convolutions, VALU-bound activation) that was 4 of the 10 tensor passes of an AMP iteration.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "itts_kernels.h"
#include "itts_snake_dev.h"

namespace itts {
namespace {

constexpr int WROW = 32;  // bf16 per staged weight row: 64 bytes = four 16-byte slots, slot q of row r at q ^ ((r >> 1) & 2)
constexpr int PROWE = 32;  // bf16 per activation-plane row (64 bytes)
__device__ __forceinline__ int swz4(int row) { return (row >> 1) & 2; }

// conv_lds_kernel<MT, NT, WAVES_M, WAVES_N, ACT>: its text lives in conv_lds_kernel_text.h and is compiled here in both forms
#define ITTS_CONV_RAG 0
#include "conv_lds_kernel_text.h"
#undef ITTS_CONV_RAG
#define ITTS_CONV_RAG 1  // conv_lds_rag_kernel: the fused-activation form over a padded ragged batch
#include "conv_lds_kernel_text.h"
#undef ITTS_CONV_RAG
#define ITTS_CONV_RAG 2  // conv_lds_seg_kernel: the fused-activation form over packed sentences
#include "conv_lds_kernel_text.h"
#undef ITTS_CONV_RAG

// LDS bytes per activation row over all planes (bf16 elements): channels rounded up to whole 32-channel k-steps
inline int row_pitch(int C) { return (C + 31) / 32 * 32; }

// dynamic LDS of one workgroup: planes + (staged weights | raw tile), or the fp32 epilogue tile
template <int BM, int NP, bool ACT>
size_t lds_bytes(const GemmArgs& g, int HR, int CP) {
  const size_t lds_w = (size_t)2 * NP * WROW * 2, lds_raw = ACT ? (size_t)(HR + 12) * g.Cin * 2 : 0;
  const size_t lds_main = (size_t)HR * CP * 2 + (lds_w > lds_raw ? lds_w : lds_raw);
  const size_t lds_epi = (size_t)BM * (NP + 4) * 4;
  return lds_main > lds_epi ? lds_main : lds_epi;
}

template <int MT, int NT, int WAVES_M, int WAVES_N, bool ACT>
int launch(const GemmArgs& g, hipStream_t s, const int* lens = nullptr, int mul = 1) {
  constexpr int BM = WAVES_M * MT * 16, NP = WAVES_N * NT * 16;
  const int HR = BM + (g.taps - 1) * g.dil, CP = row_pitch(g.Cin);
  const size_t lds = lds_bytes<BM, NP, ACT>(g, HR, CP);
  const int B = g.M / g.T, tiles = (g.T + BM - 1) / BM;
  if constexpr (ACT) {
    if (lens) {
      static DynLdsLatch rag_latch;
      ITTS_TRY(allow_dynamic_lds(rag_latch, (const void*)conv_lds_rag_kernel<MT, NT, WAVES_M, WAVES_N, true>, 160 * 1024));
      hipLaunchKernelGGL((conv_lds_rag_kernel<MT, NT, WAVES_M, WAVES_N, true>), dim3(B * tiles), dim3(256), lds, s, g, tiles, HR, CP, lens, mul);
      ITTS_HIP_CHECK(hipGetLastError());
      return OK;
    }
  }
  static DynLdsLatch latch;  // one per instantiation
  ITTS_TRY(allow_dynamic_lds(latch, (const void*)conv_lds_kernel<MT, NT, WAVES_M, WAVES_N, ACT>, 160 * 1024));
  hipLaunchKernelGGL((conv_lds_kernel<MT, NT, WAVES_M, WAVES_N, ACT>), dim3(B * tiles), dim3(256), lds, s, g, tiles, HR, CP);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// the segment form: grid (tiles of the longest capacity, sentences)
template <int MT, int NT, int WAVES_M, int WAVES_N>
int launch_seg(const GemmArgs& g, hipStream_t s, const SegTable& seg, int mul) {
  constexpr int BM = WAVES_M * MT * 16, NP = WAVES_N * NT * 16;
  const int HR = BM + (g.taps - 1) * g.dil, CP = row_pitch(g.Cin);
  const size_t lds = lds_bytes<BM, NP, true>(g, HR, CP);
  int cap = 0;
  for (int b = 0; b < seg.n; ++b) cap = std::max(cap, seg.off[b + 1] - seg.off[b]);
  const int tiles = (int)(((long)cap * mul + BM - 1) / BM);
  static DynLdsLatch latch;
  ITTS_TRY(allow_dynamic_lds(latch, (const void*)conv_lds_seg_kernel<MT, NT, WAVES_M, WAVES_N, true>, 160 * 1024));
  hipLaunchKernelGGL((conv_lds_seg_kernel<MT, NT, WAVES_M, WAVES_N, true>), dim3(tiles, seg.n), dim3(256), lds, s, g, tiles, HR, CP, seg, mul);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

}  // namespace

// conv_lds_supported apart from the row count: what the pinned selector of the packed vocoder asks (a sentence alone and the same
// sentence in a pack of 64 take one family; the pass pads the pack to the kernel's 256 rows where it has to)
bool conv_lds_shape_supported(const GemmArgs& g, int ta, int tw, int tc) {
  GemmArgs q = g;
  q.M = q.T = 256;
  return conv_lds_supported(q, ta, tw, tc);
}

bool conv_lds_supported(const GemmArgs& g, int ta, int tw, int tc) {
  if (ta != BF16 || tw != BF16 || tc != BF16) return false;
  if (g.nphase != 1 || g.in_up != 1 || g.pad_mode != PAD_ZERO || g.taps < 3) return false;
  if (g.Cin % 8 != 0 || g.Cin > 96 || g.Cin < 16 || g.N % 8 != 0 || g.N > 96) return false;
  if (g.T <= 0 || g.M % g.T != 0 || g.T < 256) return false;
  if (g.lda % 8 || g.ldc % 8 || (g.R && g.ldr % 8) || (g.ADD && g.ldadd % 8)) return false;
  if (((uintptr_t)g.A | (uintptr_t)g.W | (uintptr_t)g.C | (uintptr_t)g.R | (uintptr_t)g.ADD) & 15) return false;
  if ((g.taps - 1) * g.dil > 64) return false;
  return true;
}

// Activation1d inside the kernel: one lane per channel and run, at least two runs (Cin <= 96 of 256 threads)
bool conv_lds_act_supported(const GemmArgs& g, int ta, int tw, int tc) {
  const bool off = getenv("ITTS_NO_CONV_ACT") != nullptr;  // A/B switch (read per call): Activation1d as its own launch
  return !off && g.pre_alpha && g.pre_beta && g.pre_filt && conv_lds_supported(g, ta, tw, tc) && g.lda == g.Cin;
}

// lens (device, one per batch item) / mul: the ragged form of the fused activation (conv_lds_rag_kernel); null = every item is T rows
int conv_lds(const GemmArgs& g, hipStream_t s, const int* lens, int mul) {
  ITTS_REQUIRE(g.A && g.W && g.C, "conv_lds: null pointer");
  ITTS_REQUIRE(conv_lds_supported(g, BF16, BF16, BF16), "conv_lds: unsupported shape");
  ITTS_REQUIRE(!lens || (g.pre_alpha && mul >= 1), "conv_lds: per-item lengths go with the fused activation only");
  if (g.pre_alpha) {
    ITTS_REQUIRE(conv_lds_act_supported(g, BF16, BF16, BF16), "conv_lds: fused activation unsupported for this shape");
    // Tile heights measured on 64 x 480 frames (r04): C = 48 gains from 128-row tiles (3 workgroups per CU instead of 2: the
    // activation phase of one overlaps the matrix phase of another; 248.9 -> 242.5 ms per vocoder pass), C = 24 loses with them
    // (257.5) and C = 96 is indifferent to 64-row tiles (244.1 vs 243.4)
    if (g.N <= 32) return launch<4, 2, 4, 1, true>(g, s, lens, mul);
    if (g.N <= 48) return launch<2, 3, 4, 1, true>(g, s, lens, mul);
    return launch<4, 3, 2, 2, true>(g, s, lens, mul);
  }
  if (g.N <= 32) return launch<4, 2, 4, 1, false>(g, s);
  if (g.N <= 48) return launch<4, 3, 4, 1, false>(g, s);
  return launch<4, 3, 2, 2, false>(g, s);
}

// The fused activation + convolution over packed sentences (conv_lds_seg_kernel): g.M = g.T = the rows of the pack (off[n] * mul),
// sentence b the rows [off[b] * mul, off[b + 1] * mul) of A, C, R and ADD.  Any row count: the 256-row rule of conv_lds_supported is
// about where the family pays, the kernel tiles a sentence of one row as well.
int conv_lds_seg(const GemmArgs& g, hipStream_t s, const SegTable& seg, int mul) {
  ITTS_REQUIRE(g.A && g.W && g.C, "conv_lds_seg: null pointer");
  const char* why = seg_table_refusal(seg, mul, 0);
  ITTS_REQUIRE(!why, (std::string("conv_lds_seg: ") + why).c_str());
  ITTS_REQUIRE(g.pre_alpha && g.pre_beta && g.pre_filt && g.lda == g.Cin && conv_lds_shape_supported(g, BF16, BF16, BF16),
               "conv_lds_seg: not a fused-activation shape of the LDS-tiled narrow conv");
  ITTS_REQUIRE(g.M == g.T && (long)g.T >= (long)seg.off[seg.n] * mul, "conv_lds_seg: the pack is longer than the operands");
  ITTS_REQUIRE(!g.bias || g.bias_bstride == 0, "conv_lds_seg: one item, one bias row (bias_bstride == 0)");
  if (g.N <= 32) return launch_seg<4, 2, 4, 1>(g, s, seg, mul);
  if (g.N <= 48) return launch_seg<2, 3, 4, 1>(g, s, seg, mul);
  return launch_seg<4, 3, 2, 2>(g, s, seg, mul);
}

}  // namespace itts

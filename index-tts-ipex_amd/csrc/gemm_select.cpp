// Which kernel of the shift-GEMM family runs a shape (gemm_which), the dispatcher on top of it (gemm), and the K-split planner
// of the few-tile deep-K shapes (gemm_ksplit_plan).  Pure host code: no HIP call before the launch itself.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "itts_kernels.h"

namespace itts {

// what every matrix-core kernel of the family needs of its operands: 16-bit A and W read as 16-byte fragments, 16-bit or fp32 C
bool gemm_operands_ok(const GemmArgs& g, int ta, int tw, int tc) {
  if (ta != BF16 || tw != BF16 || (tc != BF16 && tc != F32)) return false;
  return g.lda % 8 == 0 && !((uintptr_t)g.A & 15) && !((uintptr_t)g.W & 15);
}

// N = 192 (BigVGAN stage 3): two 128-wide column tiles would waste a quarter of the MFMA work, three 64-wide tiles none
bool gemm_ragged128(const GemmArgs& g) { return g.N % 128 != 0 && g.N % 64 == 0 && g.N < 256; }

namespace {

// The A/B switches of the selector, read once per call (tests and tools/bench_gemm.py flip them between two calls of one process).
// The planner and the selector both ask this struct, so they cannot disagree about which kernels are allowed.
struct Switches {
  bool conv_lds = !getenv("ITTS_NO_CONV_LDS");                               // the LDS-tiled narrow conv
  bool lds_dma = !getenv("ITTS_NO_GEMM_GLDS") && !getenv("ITTS_GEMM_FORCE_OLD");  // gemm_glds / gemm_p8; off = the register-staged kernel everywhere
  bool p8 = lds_dma;                                                        // ITTS_GEMM_P8=0: without the 256 x 256 eight-phase kernel
  int ksplit = -1;                                                          // ITTS_GEMM_KSPLIT: 0 = off, n = forced where eligible, -1 = measured rule
  Switches() {
    const char* e = getenv("ITTS_GEMM_P8");
    if (e && atoi(e) == 0) p8 = false;
    if ((e = getenv("ITTS_GEMM_KSPLIT"))) ksplit = atoi(e);
  }
};

}  // namespace

// K split for the few-tile, deep-K shapes (batch-1 latent pass: 1242 rows x 1280 features over K = 5120 is 25 tiles of 256 x 256 - a
// tenth of the CUs, each MFMA-bound for 70 us; BigVGAN conv_pre and stage 0 likewise): the tile's K-tiles go to S workgroups that
// write raw fp32 sums to the caller's workspace, a second launch adds them in split order (deterministic) and runs the epilogue.
// Returns S (1 = no split).  ITTS_GEMM_KSPLIT=0 turns it off, =n forces n where the shape is eligible (A/B).
int gemm_ksplit_plan(const GemmArgs& g, int ta, int tw, int tc, size_t ws_bytes) {
  const Switches sw;
  const int forced = sw.ksplit;
  if (forced == 0 || g.nphase != 1 || !sw.p8) return 1;
  if (sw.conv_lds && conv_lds_supported(g, ta, tw, tc)) return 1;
  const long tiles = gemm_p8_tiles(g, ta, tw, tc);
  const long nk = (long)g.taps * (g.Cin / 64);
  // measured (tools/bench_gemm.py --batch 1 --ksplit, profiles/r04_gemm_ksplit_b1.txt): pays below 64 tiles with K >= 2048 (conv_pre
  // 126 -> 50 us, stage-0 k = 11 conv 146 -> 67, latent mlp.c_proj 70 -> 41); at 75 - 100 tiles or K = 1280 the reduction launch
  // costs more than the idle CUs did (c_attn 34 -> 36, c_proj 23 -> 27)
  if (tiles <= 0 || tiles >= (forced > 0 ? 128 : 64) || nk < (forced > 0 ? 16 : 32)) return 1;
  long S = forced > 0 ? forced : 224 / tiles;
  S = std::min(S, 8L);
  S = std::min(S, nk / 4);                                            // at least four K-tiles per split (the pipeline's fill)
  S = std::min(S, (long)(ws_bytes / ((size_t)g.M * g.N * 4)));
  while (S > 1 && (S - 1) * ((nk + S - 1) / S) >= nk) --S;            // every split owns at least one K-tile
  return S < 2 ? 1 : (int)S;
}

// which kernel family the dispatcher takes for a shape: 0 vector ALU, 1 register-staged MFMA (gemm_mfma), 2 LDS-DMA staged 128-wide
// tiles (gemm_glds), 3 256 x 256 eight-phase (gemm_p8), 4 LDS-tiled narrow conv (conv_lds)
int gemm_which(const GemmArgs& g, int ta, int tw, int tc) {
  if (g.ksplit > 1) return 3;  // planned by gemm_ksplit_plan (Engine::conv): gemm_p8 with its reduction launch
  const Switches sw;
  if (sw.conv_lds && conv_lds_supported(g, ta, tw, tc)) return 4;
  const long p8_tiles = sw.p8 ? gemm_p8_tiles(g, ta, tw, tc) : 0;
  if (p8_tiles >= 200) return 3;
  if (sw.lds_dma && gemm_glds_supported(g, ta, tw, tc)) return 2;
  if (p8_tiles >= 64) return 3;  // a quarter of the CUs busy with the deep pipeline still beats the register-staged kernel
  if (gemm_mfma_supported(g, ta, tw, tc)) return 1;
  return 0;
}

// Does a call that carries g.pre_* run with Activation1d applied INSIDE the convolution?  Only family 4 has that form.  The one rule
// behind the engine's a -> conv (model_vocoder.hip act_conv), itts_act_conv / itts_act_conv_supported and the guard in gemm() below.
bool gemm_act_fused(const GemmArgs& g, int ta, int tw, int tc) {
  return gemm_which(g, ta, tw, tc) == 4 && conv_lds_act_supported(g, ta, tw, tc);
}

int gemm(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s, const int* lens, int mul) {
  // the other families do not read pre_*: they would convolve the raw input without a word
  ITTS_REQUIRE(!(g.pre_alpha || g.pre_beta || g.pre_filt) || gemm_act_fused(g, ta, tw, tc),
               "gemm: pre_alpha / pre_beta / pre_filt set on a call that does not run the fused Activation1d kernel");
  // ... and only the fused activation knows a per-item signal length
  ITTS_REQUIRE(!lens || (g.pre_alpha && mul >= 1), "gemm: per-item lengths on a call that does not run the fused Activation1d kernel");
  switch (gemm_which(g, ta, tw, tc)) {
    case 4: return conv_lds(g, s, lens, mul);
    case 3: return gemm_p8(g, ta, tw, tc, s);
    case 2: return gemm_glds(g, ta, tw, tc, s);
    case 1: return gemm_mfma(g, ta, tw, tc, s);
    default: return gemm_simple(g, ta, tw, tc, s);
  }
}

// The PINNED selector of the packed latent pass (Engine::gpt_latent_packed): one family per projection, picked from the operand types,
// N, K and alignment - never from M.  A sequence alone and the same sequence among 127 others must run the same kernel family (the
// families sum K in one order inside a family; across families the bits differ), and gemm_which moves with the tile count.  gemm_p8
// wherever it can run the shape (every GPT projection at full dims; it is the family gemm_which takes at the row counts a packed pass
// is for), else gemm_mfma (M >= 16: the caller's duty), else the vector ALU.  Never a K split.
int gemm_which_pinned(const GemmArgs& g, int ta, int tw, int tc) {
  const Switches sw;
  if (sw.p8 && g.nphase == 1 && gemm_p8_tiles(g, ta, tw, tc) > 0) return 3;
  if (gemm_mfma_supported(g, ta, tw, tc)) return 1;
  return 0;
}

int gemm_pinned(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s) {
  ITTS_REQUIRE(!(g.pre_alpha || g.pre_beta || g.pre_filt) && g.ksplit == 1, "gemm_pinned: no fused activation, no K split");
  switch (gemm_which_pinned(g, ta, tw, tc)) {
    case 3: return gemm_p8(g, ta, tw, tc, s);
    case 1: return gemm_mfma(g, ta, tw, tc, s);
    default: return gemm_simple(g, ta, tw, tc, s);
  }
}

// The pinned selector of the packed vocoder's convolutions (Engine::bigvgan_packed): as above, with the LDS-tiled narrow conv in front
// where the shape - apart from its row count - is one of its own.  The pass pads a short pack to that kernel's 256 rows, so a one-frame
// sentence alone takes the family it takes inside a pack of 64.  gemm_glds is never an answer: its gate is a tile count.
int gemm_which_pinned_conv(const GemmArgs& g, int ta, int tw, int tc) {
  const Switches sw;
  if (sw.conv_lds && conv_lds_shape_supported(g, ta, tw, tc)) return 4;
  return gemm_which_pinned(g, ta, tw, tc);
}

bool gemm_pinned_conv_fused(const GemmArgs& g, int ta, int tw, int tc) {
  const bool off = getenv("ITTS_NO_CONV_ACT") != nullptr;
  return !off && g.pre_alpha && g.pre_beta && g.pre_filt && g.lda == g.Cin && gemm_which_pinned_conv(g, ta, tw, tc) == 4;
}

// seg / mul: the sentences of a fused-activation call (g.pre_*), which only family 4 runs - in its segment form
int gemm_pinned_conv(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s, const SegTable* seg, int mul) {
  ITTS_REQUIRE(g.ksplit == 1, "gemm_pinned_conv: no K split");
  const bool pre = g.pre_alpha || g.pre_beta || g.pre_filt;
  ITTS_REQUIRE(!pre || (seg && gemm_pinned_conv_fused(g, ta, tw, tc)),
               "gemm_pinned_conv: pre_alpha / pre_beta / pre_filt set on a call that does not run the fused segment kernel");
  ITTS_REQUIRE(pre || !seg, "gemm_pinned_conv: a segment table on a call without the fused activation");
  if (pre) return conv_lds_seg(g, s, *seg, mul);
  switch (gemm_which_pinned_conv(g, ta, tw, tc)) {
    case 4: return conv_lds(g, s);  // (plain form on the whole pack: its own 256-row rule applies, the pass has padded for it)
    case 3: return gemm_p8(g, ta, tw, tc, s);
    case 1: return gemm_mfma(g, ta, tw, tc, s);
    default: return gemm_simple(g, ta, tw, tc, s);
  }
}

// ---- one family by name (itts_gemm_family: the operator tests run each kernel at the smallest shapes that reach its paths, far below
//      the performance gates of gemm_which).  The refusal repeats, in words, every condition of that family's launcher, so that the
//      entry answers on the host before any HIP call; the launchers keep their own ITTS_REQUIREs behind it. ----
const char* gemm_family_refusal(const GemmArgs& g, int ta, int tw, int tc, int family, int variant) {
  if (!g.A || !g.W || !g.C) return "null pointer";
  if (g.pre_alpha || g.pre_beta || g.pre_filt) return "pre_alpha / pre_beta / pre_filt: only family 4 (itts_act_conv) has the fused activation";
  if (family < 0 || family > 3) return "unknown family (0 vector ALU, 1 gemm_mfma, 2 gemm_glds, 3 gemm_p8; family 4 runs through itts_gemm / itts_act_conv)";
  if (variant != 0 && family != 1) return "unknown variant: only family 1 has variants";
  if (g.ksplit < 1) return "ksplit < 1";
  if (g.ksplit > 1 && family != 3) return "ksplit > 1: only family 3 splits K";
  if (g.M < 1 || g.N < 1 || g.Cin < 1 || g.taps < 1) return "bad dims: M, N, Cin and taps must be >= 1";
  if (g.nphase < 1 || g.nphase > 8 || g.in_up < 1) return "bad phase/upsample: 1 <= nphase <= 8, in_up >= 1";
  if (g.lda < g.Cin || (long)g.ldc < (long)g.N * g.nphase) return "bad leading dims: lda >= Cin and ldc >= N * nphase";
  const int T = g.T > 0 ? g.T : g.M;
  if (g.M % T != 0 || T % g.in_up != 0) return "M must be a multiple of T (and T of in_up)";
  if (family == 0) {
    const bool combo = (ta == F32 && (tw == F32 || tw == BF16)) || (ta == BF16 && tw == BF16);  // gemm_simple's six instantiations
    return combo && (tc == F32 || tc == BF16) ? nullptr : "dtype: not a combination the vector-ALU kernel is built for";
  }
  if (ta != BF16 || tw != BF16 || (tc != BF16 && tc != F32)) return "dtype: A and W must be the 16-bit type of the library, C that or fp32";
  if (!gemm_operands_ok(g, ta, tw, tc)) return "operands: lda % 8 == 0, A and W 16-byte aligned";
  if (family == 1) {
    if (!gemm_mfma_supported(g, ta, tw, tc)) return "shape: gemm_mfma needs Cin % 8 == 0 and M >= 16";
    if (!gemm_mfma_variant_ok(g, variant)) return "unknown variant: tile 1 - 4 | depth 1, 2 or 4 << 4 | nbuf 1 or 2 << 8; tiles 1 - 3 need N >= 64";
    return nullptr;
  }
  if (family == 2) return gemm_glds_can_run(g, ta, tw, tc) ? nullptr : "shape: gemm_glds needs Cin % 64 == 0, in_up == 1, nphase == 1, N >= 64 and M >= 256";
  if (gemm_p8_tiles(g, ta, tw, tc) <= 0) return "shape: gemm_p8 needs Cin % 64 == 0, in_up == 1, N >= 192, N % 64 == 0 and taps * Cin >= 256";
  if (!gemm_p8_ksplit_ok(g)) return "ksplit: a K split needs a 16-byte aligned workspace, one phase and a K-tile for every split";
  return nullptr;
}

int gemm_family(const GemmArgs& g, int ta, int tw, int tc, int family, int variant, hipStream_t s) {
  const char* why = gemm_family_refusal(g, ta, tw, tc, family, variant);
  ITTS_REQUIRE(!why, (std::string("gemm_family: ") + why).c_str());
  switch (family) {
    case 3: return gemm_p8(g, ta, tw, tc, s);
    case 2: return gemm_glds(g, ta, tw, tc, s);
    case 1: return gemm_mfma(g, ta, tw, tc, s, variant);
    default: return gemm_simple(g, ta, tw, tc, s);
  }
}

}  // namespace itts

// Host-side launchers of every HIP kernel in libitts_hip.  All tensors are channels-last / row-major,
// all launches are asynchronous on the given stream, no launcher allocates or synchronises
// (graph-capture safe).  dtype arguments are itts::DType values.
#pragma once
#include "itts_common.h"

namespace itts {

// ---- packed sentences (the packed vocoder): one item whose sentences lie back to back in time ----
// Sentence b owns frames [off[b], off[b + 1]) - its capacity - of which the first len[b] are signal and the rest zeros; a tensor at
// up-sampling mul holds mul rows per frame.  The table travels BY VALUE in the argument block of every segment kernel (host-checked,
// no upload: nothing of the caller's outlives the call).
constexpr int SEG_MAX = 128;
struct SegTable {
  int n = 0;
  int off[SEG_MAX + 1] = {0};
  int len[SEG_MAX] = {0};
};
// why a table cannot run (null = it can), no HIP call: n in [1, SEG_MAX], mul >= 1, off[0] >= 0, every len >= 1, offsets increasing,
// every capacity >= len + gap, off[n] * mul below 2^31
const char* seg_table_refusal(const SegTable& seg, int mul, int gap);
int seg_table_fill(SegTable& seg, const int* off_host, const int* lens_host, int n);

// ---- GEMM / conv family (gemm_simple.hip, gemm_mfma.hip, gemm_glds.hip, gemm_p8.hip, conv_lds.hip; selector: gemm_select.cpp) ----
int gemm_simple(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s);
bool gemm_operands_ok(const GemmArgs& g, int ta, int tw, int tc);  // the operand gate of the three matrix-core GEMMs: half A / W, half or fp32 C, lda % 8, 16-byte aligned
bool gemm_ragged128(const GemmArgs& g);                             // N = 192-like shapes: 64-wide column tiles instead of 128-wide
bool gemm_mfma_supported(const GemmArgs& g, int ta, int tw, int tc);
int gemm_mfma(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s);
// ... with the instantiation named: variant = tile | depth << 4 | nbuf << 8 (tile 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 128x32; depth 1 / 2 / 4;
// nbuf 1 / 2), 0 = the launcher's own pick.  Tiles 1 - 3 need N >= 64.  For gemm_family and the operator tests; production passes 0.
bool gemm_mfma_variant_ok(const GemmArgs& g, int variant);
int gemm_mfma(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s, int variant);
bool gemm_glds_can_run(const GemmArgs& g, int ta, int tw, int tc);    // what gemm_glds needs of a shape (structural) ...
bool gemm_glds_supported(const GemmArgs& g, int ta, int tw, int tc);  // ... and where it pays: LDS-DMA staged 128 x 128 / 128 x 64 tiles (gemm_glds.hip)
int gemm_glds(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s);
long gemm_p8_tiles(const GemmArgs& g, int ta, int tw, int tc);      // 0 = cannot run the shape
int gemm_p8(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s);  // 256 x 256 tile, 8-phase LDS-DMA pipeline (gemm_p8.hip)
bool gemm_p8_ksplit_ok(const GemmArgs& g);                          // g.ksplit / g.ws as gemm_p8 can run them (1 = no split)
int gemm_ksplit_plan(const GemmArgs& g, int ta, int tw, int tc, size_t ws_bytes);  // K split of the few-tile deep-K shapes; 1 = none
bool conv_lds_supported(const GemmArgs& g, int ta, int tw, int tc);
bool conv_lds_act_supported(const GemmArgs& g, int ta, int tw, int tc);  // ... with Activation1d fused into the tile load (g.pre_*)
// lens / mul (ragged batches, next to the args so that GemmArgs - a by-value argument of every GEMM kernel - does not grow): item b of
// a fused-activation call is the signal of its first lens[b] * mul rows (device ints, one per batch item); null = all T rows
int conv_lds(const GemmArgs& g, hipStream_t s, const int* lens = nullptr, int mul = 1);
bool conv_lds_shape_supported(const GemmArgs& g, int ta, int tw, int tc);  // conv_lds_supported apart from the row count
// the fused activation + conv over packed sentences (conv_lds_seg_kernel): g.M = g.T >= off[n] * mul rows, any row count
int conv_lds_seg(const GemmArgs& g, hipStream_t s, const SegTable& seg, int mul);
int gemm(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s, const int* lens = nullptr, int mul = 1);  // dispatcher
int gemm_which(const GemmArgs& g, int ta, int tw, int tc);           // the kernel family the dispatcher takes: 0 VALU, 1 mfma, 2 glds, 3 p8, 4 conv_lds
// One family (0 - 3) by name, whatever the selector would take: why it cannot run the call (null = it can; no HIP call), and the
// launch.  g.ksplit / g.ws as the caller set them (family 3 only).  Never another family.  itts_gemm_family, the operator tests.
const char* gemm_family_refusal(const GemmArgs& g, int ta, int tw, int tc, int family, int variant);
int gemm_family(const GemmArgs& g, int ta, int tw, int tc, int family, int variant, hipStream_t s);
bool gemm_act_fused(const GemmArgs& g, int ta, int tw, int tc);      // a call with g.pre_* runs Activation1d inside the conv: family 4 and conv_lds_act_supported
// The packed latent pass's selector: the family by operand types, N, K and alignment, never by M (1, 3 or 0); no K split
int gemm_which_pinned(const GemmArgs& g, int ta, int tw, int tc);
int gemm_pinned(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s);
// The packed vocoder's selector for convolutions: 4 where conv_lds_shape_supported holds (the shape apart from its row count), then
// gemm_which_pinned's order (3, 1, 0); never gemm_glds, never by M or T.  A family-4 answer for a call with g.pre_* means the
// fused segment form (gemm_pinned_conv_fused: also conv_lds_act's own rule), else the caller activates first.
int gemm_which_pinned_conv(const GemmArgs& g, int ta, int tw, int tc);
bool gemm_pinned_conv_fused(const GemmArgs& g, int ta, int tw, int tc);
int gemm_pinned_conv(const GemmArgs& g, int ta, int tw, int tc, hipStream_t s, const SegTable* seg = nullptr, int mul = 1);

// ---- anti-aliased SnakeBeta (snake.hip); x,y [B,T,C] ----
int snake_aa(void* y, const void* x, const float* log_alpha, const float* log_beta, const float* up12,
             const float* down12, int B, int T, int C, int dt, hipStream_t s);
// ... on a padded ragged batch: item b is the signal of its first lens[b] * mul rows (clamped to [0, T]; replicate clamp at its own
// end), the rows behind it are written as zeros; lens: device ints [B]
int snake_aa_len(void* y, const void* x, const float* log_alpha, const float* log_beta, const float* up12, const float* down12,
                 int B, int T, int C, const int* lens, int mul, int dt, hipStream_t s);
// ... over packed sentences: sentence b is rows [off[b] * mul, off[b + 1] * mul) of x / y, its signal the first len[b] * mul of them;
// the rest of its capacity is written as zeros, rows outside the pack are not touched
int snake_aa_seg(void* y, const void* x, const float* log_alpha, const float* log_beta, const float* up12, const float* down12,
                 int C, const SegTable& seg, int mul, int dt, hipStream_t s);
// same op on the reference's [B,C,T] layout (drop-in for anti_alias_activation_cuda.forward)
int snake_aa_bct(void* y, const void* x, const float* log_alpha, const float* log_beta, const float* up12,
                 const float* down12, int B, int C, int T, int dt, hipStream_t s);

// ---- row-wise ops (elementwise.hip) ----
int layernorm(void* y, int ty, const void* x, int tx, const float* gamma, const float* beta, int rows, int D,
              int ldx, int ldy, float eps, int act, hipStream_t s);
int rmsnorm_unit(void* y, int ty, const void* x, int tx, const float* gamma, int rows, int D, hipStream_t s);
int glu(void* y, const void* x, int rows, int C, int dt, hipStream_t s);
int geglu(void* y, const void* x, int rows, int inner, int ldy, int dt, hipStream_t s);
int dwconv(void* y, const void* x, const float* w, const float* bias, int B, int T, int C, int k, int dt, hipStream_t s);
int conv2d_sub2(void* y, const void* mel, const float* w, const float* bias, int B, int F, int idim, int odim, int dt,
                hipStream_t s);
int gather_add(void* y, int ty, int ldy, const void* ta, const int* ia, const void* tb, const int* ib, int ttab,
               int rows, int D, hipStream_t s);
int transpose_brc(void* y, const void* x, int B, int R, int C, int dt, hipStream_t s);
int cast_copy(void* y, int ty, const void* x, int tx, long n, hipStream_t s);
int copy_rows(void* y, int ldy, const void* x, int ldx, int rows, int D, int dt, hipStream_t s);
int add_strided(void* y, int ldy, const void* a, int lda, const void* b, int ldb, int rows, int D, int dt, hipStream_t s);
int col_mean(float* mean, const void* x, int B, int T, int C, int ldx, int dt, hipStream_t s);
int col_mean_std(float* out, const void* x, int B, int T, int C, int ldx, int dt, hipStream_t s);
int scale_cols_add(void* y, int ldy, const void* x, int ldx, const float* sc, const void* res, int ldr, int B, int T,
                   int C, int dt, hipStream_t s);
int asp_pool(float* out, const void* logits, const void* x, const float* bn_scale, const float* bn_shift, int B, int T,
             int C, int dt, hipStream_t s);
int relpos_pack(void* qc, void* kc, const void* qkv, const void* p, const float* bu, const float* bv, int T, int H,
                int dk, int dt, hipStream_t s);
int tanh_rows(void* y, const void* x, long n, int dt, hipStream_t s);
// x [B, T, C]: rows [lens[b] * mul, T) of item b become zeros (the padding of a ragged batch and nothing else is written)
int zero_tail_rows(void* x, int B, int T, int C, const int* lens, int mul, int dt, hipStream_t s);
// x [off[n] * mul, C] over packed sentences: the signal rows of sentence b get bias[b][:] (fp32 [n, C]; null = left alone) added, the
// rest of its capacity becomes zeros; rows outside the pack are not touched
int seg_bias_mask(void* x, const float* bias, int C, const SegTable& seg, int mul, int dt, hipStream_t s);

// ---- the DVAE encoder's small kernels (model_vocoder.hip) ----
// y[B][(Tin + 1) / 2][2 C] = x[B][2t][:] | x[B][2t + 1][:], zero past Tin (the row pairs of a stride-2 convolution)
int pair_rows(void* y, const void* x, int B, int Tin, int C, int dt, hipStream_t s);
// codes[r] = the first n that minimises esq[n] - 2 dots[r][n]; dots fp32 [rows][N]
int dvae_argmin(int* codes, const float* dots, const float* esq, int rows, int N, hipStream_t s);

// ---- attention (attention.hip) ----
struct AttnArgs {
  const void* q = nullptr;  // [B, Sq] rows, element (b,i,h,d) at q[(b*Sq+i)*ldq + h*dqk + d]
  const void* k = nullptr;  // (b,j,h,d) at k[(b*Sk+j)*ldk + h*dqk + d]
  const void* v = nullptr;  // (b,j,h,d) at v[(b*Sk+j)*ldv + h*dv + d]
  void* o = nullptr;        // (b,i,h,d) at o[(b*Sq+i)*ldo + h*dv + d]
  int B = 1, H = 1, Sq = 0, Sk = 0, dqk = 64, dv = 64;
  int ldq = 0, ldk = 0, ldv = 0, ldo = 0;
  float scale = 1.f;
  int causal = 0;                 // key j visible to query i iff j <= i + (Sk - Sq)
  const int* kv_start = nullptr;  // per batch row: keys < kv_start[b] are masked (left padding)
};
int attention_simple(const AttnArgs& a, int dt, hipStream_t s);
bool attention_mfma_supported(const AttnArgs& a, int dt);
int attention_mfma(const AttnArgs& a, int dt, hipStream_t s);
int attention(const AttnArgs& a, int dt, hipStream_t s);  // dispatcher
// The host-side check of the C ABI entries (itts_attention, itts_attention_kernel, itts_attention_which): why the call cannot run
// (null = it can), no HIP call.  kernel 0 = the dispatcher, 1 = attention_simple, 2 = attention_mfma (then also its own rule).
const char* attention_refusal(const AttnArgs& a, int dt, int kernel);
int attention_which(const AttnArgs& a, int dt);  // 1 / 2: the kernel attention() takes (ITTS_ATTN_SIMPLE honoured), no launch

// ---- causal self-attention over packed sequences (attention_varlen.hip) ----
constexpr int VARLEN_MAX_SEQ = 128;
// Sequence b owns rows [off[b], off[b + 1]) of q, k, v and o (row r, head h, dim d at q[r*ldq + h*dqk + d] and alike); query i of a
// sequence sees keys 0 .. i of that sequence.  The offsets travel by value in the argument block (host-checked, no upload).
struct VarlenArgs {
  const void* q = nullptr;
  const void* k = nullptr;
  const void* v = nullptr;
  void* o = nullptr;
  int ldq = 0, ldk = 0, ldv = 0, ldo = 0;
  float scale = 1.f;
  int H = 1, dqk = 64, dv = 64, nseq = 0;
  int off[VARLEN_MAX_SEQ + 1] = {0};
};
// why the call cannot run (null = it can), no HIP call.  kernel 0 = the dispatcher, 1 = attn_varlen_simple_kernel (fp32 or the 16-bit
// type, dqk <= 128, dv <= 64), 2 = attn_varlen_mfma_kernel (then also attention_varlen_mfma_supported)
const char* attention_varlen_refusal(const VarlenArgs& a, int dt, int kernel);
bool attention_varlen_mfma_supported(const VarlenArgs& a, int dt);  // type, head dims, leading dims, alignment: never a length
int attention_varlen_which(const VarlenArgs& a, int dt);            // 1 / 2: the dispatcher's pick (ITTS_ATTN_SIMPLE honoured), no launch
int attention_varlen(const VarlenArgs& a, int dt, int kernel, hipStream_t s);  // the named kernel runs or nothing does

// ---- causal self-attention for APPENDED rows (attention_append.hip; the incremental packed latent pass) ----
// Sequence b: its n_new[b] new queries are positions pos0[b] .. pos0[b] + n_new[b] - 1, rows q_off[b] .. of q and o (the chunk's
// buffers; q_off[b + 1] - q_off[b] >= n_new[b]); its keys / values are rows 0 .. pos0[b] + n_new[b] - 1 of its block of a K/V history,
// which starts at row kv_off[b] of k / v and holds kv_off[b + 1] - kv_off[b] rows - the new rows' k / v already written.  Query at
// position i sees keys 0 .. i.  A delivered row has the bits attn_varlen_* of the same family gives it in a pass over the complete
// sequence: the query tiles stay aligned to the sequence's key 0, rows of a tile in front of pos0 are never stored, no key row at or
// behind pos0 + n_new is read.  n_new[b] = 0 leaves sequence b alone.  The four arrays travel by value (host-checked, no upload).
struct AppendArgs {
  const void* q = nullptr;
  const void* k = nullptr;
  const void* v = nullptr;
  void* o = nullptr;
  int ldq = 0, ldk = 0, ldv = 0, ldo = 0;
  float scale = 1.f;
  int H = 1, dqk = 64, dv = 64, nseq = 0;
  int q_off[VARLEN_MAX_SEQ + 1] = {0};
  int kv_off[VARLEN_MAX_SEQ + 1] = {0};
  int pos0[VARLEN_MAX_SEQ + 1] = {0};
  int n_new[VARLEN_MAX_SEQ + 1] = {0};
};
// why the call cannot run (null = it can): host memory only, no HIP call (append_check.cpp).  kernel 0 = the dispatcher, 1 =
// attn_append_simple_kernel, 2 = attn_append_mfma_kernel (then also attention_append_mfma_supported)
const char* attention_append_refusal(const AppendArgs& a, int dt, int kernel);
bool attention_append_mfma_supported(const AppendArgs& a, int dt);  // attention_varlen_mfma_supported's rule: never a length or a count
int attention_append_which(const AppendArgs& a, int dt);            // 1 / 2: the dispatcher's pick (ITTS_ATTN_SIMPLE honoured), no launch
int attention_append(const AppendArgs& a, int dt, int kernel, hipStream_t s);  // the named kernel runs or nothing does
// The history write that goes in front of it: columns [0, wk) of ksrc row q_off[b] + r go to k row kv_off[b] + pos0[b] + r, columns
// [0, wv) of vsrc likewise to v, r < n_new[b] (a.k / a.v are written; a.q / a.o / H / dqk / dv are not used).  fp32 or the 16-bit
// type, no conversion.  why it cannot run: kv_rows_append_refusal (host only).
const char* kv_rows_append_refusal(const AppendArgs& a, const void* ksrc, const void* vsrc, int lds, int wk, int wv, int dt);
int kv_rows_append(const AppendArgs& a, const void* ksrc, const void* vsrc, int lds, int wk, int wv, int dt, hipStream_t s);

// ---- the latent stream's argument checks (append_check.cpp): host memory only, no HIP call ----
// The state a stream entry judges a call against; Engine keeps one (engine.h LatentStream).
struct LatentStreamState {
  bool open = false;
  int nseq = 0, max_codes = 0, number_mel_codes = 0;
  const int* done = nullptr;  // [nseq] codes taken so far
};
const char* latent_stream_open_refusal(const LatentStreamState& st, const void* cond, const int32_t* cond_index, int n_cond,
                                       const int32_t* text_ids, const int32_t* text_lens, int nseq, int max_codes, int max_text_tokens,
                                       int max_mel_tokens, int number_text_tokens);
const char* latent_stream_append_refusal(const LatentStreamState& st, const int32_t* codes, const int32_t* counts, const void* latent_out);

}  // namespace itts

// Decode-step kernels: decode.hip (first generation), decode_gemv / decode_attn / decode_fused / decode_sampler.hip, decode_mfma.hip.
#pragma once
#include "itts_common.h"

namespace itts {

struct Lin;

struct GemvArgs {
  const float* X = nullptr;  // [B, K] fp32
  const void* W = nullptr;   // [N, K] (fp32 or bf16)
  float* Y = nullptr;        // [B, ldy] fp32
  const float* bias = nullptr;
  int B = 0, N = 0, K = 0, ldy = 0;
  int act = ACT_NONE;
  int accumulate = 0;                // Y += result (residual stream)
  int prologue = 0;                  // 0 plain, 1 LayerNorm(X), 2 LN2(LN(X)), 3 merge split-attention partials
  int x_bf16 = 0;                    // X is bf16 [B, K] (gemv_bf16 only)
  int y_bf16 = 0;                    // Y is bf16 [B, ldy] (gemv_bf16 only; no accumulate)
  const float* ln_gamma = nullptr;
  const float* ln_beta = nullptr;
  const float* ln2_gamma = nullptr;
  const float* ln2_beta = nullptr;
  float ln_eps = 1e-5f;
  int ksplit = 1;            // skinny_mfma: K split across workgroups; > 1 writes raw sums to partial[split][B][ldy]
  float* partial = nullptr;
  const struct Lin* w8src = nullptr;  // engine-internal: projection whose fp8 copy may replace W (decode GEMV)
  // prologue 3 (gemv_bf16): x = the attention output merged from ATTN_NSPLIT partials of decode_attn2 (K = heads * 64)
  const float* attn_o = nullptr;   // [B][heads][ATTN_NSPLIT][64] un-normalised weighted V
  const float* attn_ml = nullptr;  // [B][heads][2][ATTN_NSPLIT] partial max / sum
  const void* W8 = nullptr;      // gemv_bf16: [N, K] OCP fp8 e4m3 bytes (instead of W) ...
  const float* wscale = nullptr; // ... with one scale per output row: y = scale[n] * (x . w8[n]) + bias[n]
  unsigned long long* stamp = nullptr;  // -DITTS_GEMV_STAMPS builds only (tools/ubench_gemv2.hip): s_memtime per phase
  int x_tiled = 0, y_tiled = 0;  // skinny_mfma: bf16 X / Y in MFMA-fragment tiles (tile_off) instead of row-major
  const void* Wt = nullptr;      // skinny_mfma: W as bf16 fragment tiles (wtile_off) - used instead of W when set
  const void* W8t = nullptr;     // skinny_mfma: the fp8 bytes in the same tile order - used instead of W8 when set
  int half_tiles = 0;            // skinny_mfma, <= 16 rows: 8 features per workgroup (narrow projections, no K split)
};

// bf16 activations of the batched decode step live in the operand order of v_mfma_f32_16x16x32_bf16: element (b, k) of a
// [B, K] matrix at ((k/32) * BT + b/16) * 512 + ((k%32)/8 * 16 + b%16) * 8 + k%8, BT = ceil(B/16) - every (k-step, batch
// tile) fragment is one contiguous KiB, which the L2 -> CU path streams ~2.4x faster than 16 rows x 64 B.
__host__ __device__ inline size_t tile_off(int b, int k, int BT) {
  return ((size_t)(k >> 5) * BT + (b >> 4)) * 512 + ((((k & 31) >> 3) << 4) + (b & 15)) * 8 + (k & 7);
}

// bf16 weights of the batched decode step in the same operand order: element (n, k) of W[N, K] at
// ((n/16) * (K/32) + k/32) * 512 + ((k%32)/8 * 16 + n%16) * 8 + k%8 - every wave-load of a (16 features x 32 k) fragment is
// one contiguous KiB (8 whole 128-B lines) instead of 16 half lines 2*K bytes apart, and the K/32 fragments of a feature
// tile are contiguous: the HBM weight stream of the skinny GEMMs runs 1.3x faster (tools/ubench_skinny.hip).
// Rows N .. 16*ceil(N/16) are zero.
__host__ __device__ inline size_t wtile_off(int n, int k, int K) {
  return ((size_t)(n >> 4) * (K >> 5) + (k >> 5)) * 512 + ((((k & 31) >> 3) << 4) + (n & 15)) * 8 + (k & 7);
}
int retile_weights_bf16(void* dst, const void* src, int N, int K, hipStream_t s);
int retile_weights_fp8(void* dst, const void* src, int N, int K, hipStream_t s);  // same order, one byte per element

// one row of a mixed decode batch (SamplerArgs::rows; the layout of itts_row_sampling, include/itts_hip.h)
struct RowSampling {
  int mode;   // 0 greedy, 1 sample
  int top_k;  // <= 0: TopK warper off
  float top_p, temperature, penalty;
};
// the kernel that owns a row: 0 greedy (sampler2_kernel), 1 narrow (sampler_sample_kernel), 2 wide (sampler_wide_kernel)
enum { ROWCLS_GREEDY = 0, ROWCLS_NARROW = 1, ROWCLS_WIDE = 2 };
__host__ __device__ inline int row_class(int mode, int top_k) {
  return mode == 0 ? ROWCLS_GREEDY : (top_k >= 1 && top_k <= 128 ? ROWCLS_NARROW : ROWCLS_WIDE);
}

struct SamplerArgs {
  const float* logits = nullptr;  // [B, V]
  uint8_t* seen = nullptr;        // [B, V]
  int* ids = nullptr;             // [B, max_gen]
  int* cur_tok = nullptr;         // [B]
  int* unfinished = nullptr;      // [B]
  int* step = nullptr;            // [B] tokens generated so far, per row
  int V = 0, max_gen = 0, stop = 0, suppress_stop = 0;
  float penalty = 1.f;
  // fused input embedding of the next step: h_next[b] = emb[tok] + pos[k + 2]
  float* h_next = nullptr;
  const void* emb = nullptr;
  const void* pos = nullptr;
  int D = 0, pos_rows = 0, emb_bf16 = 0;
  // multinomial sampling (HF GenerationMixin.sample: processors -> Temperature -> TopK -> TopP -> softmax -> draw);
  // the draw is an inverse-CDF lookup of uniforms[k * B + b] over the kept tokens in descending-score order
  int do_sample = 0, top_k = 0, B = 0;
  float top_p = 1.f, temperature = 1.f;
  const float* uniforms = nullptr;  // [max_gen][B]
  // forced tokens (HF `input_tokens` continuation, model.py:672-686 / teacher forcing): forced[b][k] >= 0 replaces the
  // choice of step k for row b; nullptr = nothing forced (the table is only read when it exists)
  const int* forced = nullptr;  // [B][max_gen]
  int input_n = 0;  // the first input_n forced tokens are HF `input_tokens`: token k is fed at mel position k + 1, not k + 2
  int preprocessed = 0;  // logits already went through typical_filter (penalty, stop suppression done)
  int* kept = nullptr;   // [B] sampler_wide_kernel writes the number of kept ranks here (the operator entry point sets it)
  // mixed batches (sampler_rows_step): row b takes rows[b] in place of do_sample / top_k / top_p / temperature / penalty above.
  // nullptr = the scalars.  Last, so that no offset of an existing field moves
  const RowSampling* rows = nullptr;  // [B]
};

// one beam-sample step for every batch item (beam.hip): HF 4.36.2 beam_sample + BeamSearchScorer.process on the device
struct BeamArgs {
  const float* logits = nullptr;  // [B * nb, V]
  int V = 0, max_gen = 0, stop = 0, suppress_stop = 0, nb = 0, B = 0;  // B = batch items (rows = B * nb)
  int top_k = 0, start_tok = 0, fake_id = 1, Smax = 0;
  float penalty = 1.f, top_p = 1.f, temperature = 1.f;
  const float* uniforms = nullptr;  // [max_gen][B][2 * nb]
  int *len = nullptr, *cur_tok = nullptr, *unfinished = nullptr;  // per row
  int* ids = nullptr;          // [2][B * nb][max_gen] id histories, ping-pong by the parity of the step count
  uint8_t* anc = nullptr;      // [2][B * nb][Smax] cache ancestry rows (decode_attn2 ANC), same ping-pong
  const int* prefix_dev = nullptr;
  float* beam_scores = nullptr;  // [B * nb]
  // finished hypotheses per batch item: nb + 1 slots (one spare while the worst is being replaced)
  int* hyp_tok = nullptr;      // [B][nb + 1][max_gen]
  float* hyp_score = nullptr;  // [B][nb + 1]
  int* hyp_len = nullptr;      // [B][nb + 1]
  int* hyp_order = nullptr;    // [B][nb + 1] insertion counter, -1 = free
  int* hyp_n = nullptr;        // [B]
  float* hyp_worst = nullptr;  // [B]
  int* hyp_counter = nullptr;  // [B]
  int* done = nullptr;         // [B]
  float* h_next = nullptr;     // next step's input rows [B * nb][D]
  const void* emb = nullptr;
  const void* pos = nullptr;
  int D = 0, pos_rows = 0, emb_bf16 = 0;
  int preprocessed = 0;  // logits already went through typical_filter (log_softmax, penalty, stop suppression done)
  int do_sample = 1;     // 1: beam_sample (warpers + draws from uniforms); 0: beam_search (top 2 * nb, no warpers)
  float length_penalty = 0.f;  // BeamHypotheses score = sum_logprobs / generated_len ** length_penalty
  // scratch between the two launches of a step: every beam's kept candidates (token-ascending, beam score included)
  float* cand_sc = nullptr;  // [B * nb][BEAM_MAX_CAND]
  int* cand_tok = nullptr;   // [B * nb][BEAM_MAX_CAND]
  int* cand_n = nullptr;     // [B * nb]
  // HF `input_tokens` under beams (model.py:672-686): the first input_n steps of every beam row take forced[row][k] (all >= 0)
  // with the beam scores, the ancestry and the hypotheses untouched; they belong to the decoder prompt, so generated_len
  // (length penalty, is_done) counts from input_n and token k < input_n is fed at mel position k + 1
  const int* forced = nullptr;  // [B * nb][max_gen]
  int input_n = 0;
  // host-side warpers + draws (top_k outside [1, 128] under beams): the 2 * nb picks of every batch item IN DRAW ORDER
  // [B][2 * nb] - score (running beam score included), token, beam; beam_select_kernel then only sorts them and runs the
  // BeamSearchScorer bookkeeping + the history / ancestry swap
  const float* host_sc = nullptr;
  const int* host_tok = nullptr;
  const int* host_beam = nullptr;
};
constexpr int BEAM_MAX_CAND = 128;
// scratch and results of the whole-vocabulary beam sampler (beam.hip beam_wide_cand_kernel / beam_wide_pick_kernel: beam_sample
// with top_k < 1 or > BEAM_MAX_CAND); a second kernel argument, so that BeamArgs and the kernels that take it alone stay as they are
struct BeamWide {
  float* sc = nullptr;         // [B * nb][V] warped score + running beam score of the kept tokens, -inf everywhere else
  int* kept = nullptr;         // [B * nb] tokens of the row that survived the warpers
  float* pick_sc = nullptr;    // [B][2 * nb] the picks in draw order: what beam_select_kernel takes as host_sc / host_tok / host_beam
  int* pick_tok = nullptr;
  int* pick_beam = nullptr;
  int one_step = 0;  // the stateless operator (itts_beam_sample_rows): ids is ONE [B * nb][max_gen] table, uniforms [B][2 * nb]
};
constexpr int BEAM_WIDE_MAX_V = 16384;  // NP * 6 bytes of LDS: 96 KiB
// bytes of all five buffers for rows = B * nb beam rows of V tokens
inline size_t beam_wide_bytes(int rows, int nb, int V) { return ((size_t)rows * V + rows + (size_t)(rows / nb) * 2 * nb * 3) * 4; }
int beam_wide_prepare();  // once per device ordinal, outside graph capture: beam_wide_cand_kernel's dynamic LDS limit
// the two wide launches alone (no BeamSearchScorer step): w.sc, w.kept and the picks are written, nothing of `a` is
int beam_wide_pair(const BeamArgs& a, const BeamWide& w, hipStream_t s);
// w: needed when a.do_sample and a.top_k < 1 or > BEAM_MAX_CAND (the wide pair + beam_select_kernel on its picks)
int beam_sample_step(const BeamArgs& a, hipStream_t s, const BeamWide* w = nullptr);
int beam_commit_step(const BeamArgs& a, hipStream_t s);  // host picks -> scorer bookkeeping (beam_select_kernel only)
// the same step for batch item `item` alone (grid of one item, pointers advanced to it, a.B the full item count): the first token
// of an admitted beam group.  No typical pre-pass, no host picks
int beam_item_step(const BeamArgs& a, int item, hipStream_t s, const BeamWide* w = nullptr);

// TypicalLogitsWarper pre-pass (beam.hip): processed scores of every row -> out [rows, V] with the filtered ones at -inf
struct TypicalArgs {
  const float* logits = nullptr;
  float* out = nullptr;
  int V = 0, stop = 0, suppress_stop = 0, min_keep = 1, log_softmax_first = 0, npad = 0;
  float penalty = 1.f, mass = 0.9f;
  const uint8_t* seen = nullptr;   // [rows, V] byte bitmap (single-beam modes) ...
  const int* beam_ids = nullptr;   // ... or the beam id histories [2][rows][max_gen] with len[] (beam-sample)
  const int* len = nullptr;
  int max_gen = 0, start_tok = 0, fake_id = 1;
};
int typical_filter(const TypicalArgs& a, int rows, hipStream_t s);

int gemv(const GemvArgs& g, int tw, hipStream_t s);
int double_ln(float* y, const float* x, const float* g1, const float* b1, const float* g2, const float* b2, int rows,
              int D, float eps, hipStream_t s);
int kv_scatter(void* kc, void* vc, const void* qkv, int B, int S, int H, int dh, int Smax, int tq, int tc, hipStream_t s);

// decode_rows.hip: rows_move_kernel, the strided row copy behind the row retirement of a running batch (Engine::gpt_retire_rows).
// The moves travel by value in the argument block: at most ROWS_MOVE_MAX of them (itts_skinny_gemm's row limit), no device upload
constexpr int ROWS_MOVE_MAX = 128;
struct RowsMoveArgs {
  char* base = nullptr;
  size_t outer_stride = 0, row_stride = 0, chunk_stride = 0, chunk_bytes = 0;
  int n_outer = 0, n_moves = 0, n_chunks = 0;
  unsigned short src[ROWS_MOVE_MAX], dst[ROWS_MOVE_MAX];
};
int rows_move_check(const void* base, size_t outer_stride, int n_outer, size_t row_stride, size_t chunk_stride, int n_chunks,
                    size_t chunk_bytes, const int* src, const int* dst, int n_moves);  // host only: no HIP call
int rows_move(void* base, size_t outer_stride, int n_outer, size_t row_stride, size_t chunk_stride, int n_chunks, size_t chunk_bytes,
              const int* src, const int* dst, int n_moves, hipStream_t s);
int retire_plan(const int* unfinished, int B, int* n_live, int* src, int* dst, int* n_moves);  // host only
// rows_gather_kernel, the out-of-place row gather behind the retirement of finished beam groups: row j of every destination plane
// takes row src_rows[j] of the same source plane.  The source and destination byte ranges of one launch do not intersect
struct RowsGatherArgs {
  char* dst = nullptr;
  const char* src = nullptr;
  size_t dst_plane_stride = 0, src_plane_stride = 0, row_bytes = 0;
  int n_planes = 0, n_rows = 0;
  unsigned short src_rows[ROWS_MOVE_MAX];
};
int rows_gather_check(const void* dst, size_t dst_plane_stride, const void* src, size_t src_plane_stride, int n_planes, size_t row_bytes,
                      const int* src_rows, int n_rows);  // host only: no HIP call
int rows_gather(void* dst, size_t dst_plane_stride, const void* src, size_t src_plane_stride, int n_planes, size_t row_bytes,
                const int* src_rows, int n_rows, hipStream_t s);

// decode_admit.hip: the two kernels behind the row admission into a running batch (Engine::gpt_admit_rows).  The slots travel by
// value in the argument blocks, at most ROWS_MOVE_MAX of them, as the moves of rows_move_kernel do
struct KvAdmitArgs {
  void *kc = nullptr, *vc = nullptr;  // [Bcache][H][Smax][dh] of one layer
  const void* qkv = nullptr;          // [n][S][3 * H * dh]
  int n = 0, S = 0, H = 0, dh = 0, Smax = 0;
  unsigned short slot[ROWS_MOVE_MAX];
};
int kv_admit_check(const void* kc, const void* vc, const void* qkv, int n, int S, int H, int dh, int Smax, int Bcache, int tq, int tc,
                   const int* slots);  // host only: no HIP call
int kv_admit(void* kc, void* vc, const void* qkv, int n, int S, int H, int dh, int Smax, int Bcache, int tq, int tc, const int* slots,
             hipStream_t s);
struct RowsAdmitArgs {
  uint8_t* seen = nullptr;                                                   // [B][V]
  int *unfinished = nullptr, *cur_tok = nullptr, *len = nullptr, *kv_start = nullptr;  // [B]
  int* ids = nullptr;                                                        // [B][max_gen]
  int* forced = nullptr;                                                     // [B][max_gen] or null
  float* uniforms = nullptr;                                                 // [max_gen][B] or null
  const int* forced_src = nullptr;                                           // [n][max_gen] device, or null: -1
  const float* uniforms_src = nullptr;                                       // [n][max_gen] device, or null: the column stays
  int n = 0, B = 0, V = 0, max_gen = 0, fake_id = 1, start_tok = 0, stop = 0;
  unsigned short slot[ROWS_MOVE_MAX], kvs[ROWS_MOVE_MAX];                    // filled by rows_admit from its host lists
};
int rows_admit_check(const RowsAdmitArgs& a, const int* slots, const int* kvs);  // host only
int rows_admit(RowsAdmitArgs a, const int* slots, const int* kvs, hipStream_t s);
int admit_plan(const int* unfinished, const int* len, int B, int max_gen, int n, int* slots, int* n_free);  // host only
// beam_admit_kernel: the beam state of a fresh generation for n batch items of a running beam generation (the beam branch of
// Engine::gpt_admit_rows).  The items travel by value, n * nb <= ROWS_MOVE_MAX rows; rows_admit does the per-row part
struct BeamAdmitArgs {
  float* beam_scores = nullptr;                                        // [items * nb]
  uint8_t* anc = nullptr;                                              // [2][items * nb][Smax]
  int *hyp_order = nullptr, *hyp_n = nullptr, *hyp_counter = nullptr;  // [items][nb + 1], [items], [items]
  float* hyp_worst = nullptr;                                          // [items]
  int* done = nullptr;                                                 // [items]
  float* uniforms = nullptr;                                           // [max_gen][items][2 * nb] or null
  const float* uniforms_src = nullptr;                                 // [n][max_gen][2 * nb] device, or null: the columns stay
  int n = 0, nb = 0, items = 0, Smax = 0, max_gen = 0, do_sample = 0;
  unsigned short item[ROWS_MOVE_MAX];                                  // filled by beam_admit from its host list
};
int beam_admit_check(const BeamAdmitArgs& a, const int* items);  // host only
int beam_admit(BeamAdmitArgs a, const int* items, hipStream_t s);

// second generation, one file per kernel family.  decode_gemv.hip:
bool gemv2_supported(const GemvArgs& g);
int gemv2(const GemvArgs& g, int tw, hipStream_t s);
// the bf16 GEMV's selector: false = gemv_bf16 has no kernel for this call, else the instantiation it launches (the prologue and
// the two element types stay what GemvArgs says).  w5: the ITTS_GEMV_W5 rows.  No GPU work (itts_gemv_which)
struct GemvPick { int nb, rpw, nch, waves; };
bool gemv_bf16_pick(const GemvArgs& g, bool w5, GemvPick* p);
bool gemv_bf16_supported(const GemvArgs& g);  // gemv_bf16_pick(g, false, ..)
int gemv_bf16(const GemvArgs& g, hipStream_t s);
// decode_attn.hip
constexpr int ATTN_NSPLIT = 4;  // workgroups per (row, head) in the split form of decode_attn2
int decode_attn2(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start,
                 const int* prefix_dev, int B, int H, int dh, int Smax, int tc, hipStream_t s, int ctx_tiled = 0,
                 float* part_o = nullptr, float* part_ml = nullptr, const uint8_t* anc = nullptr, int nb = 1);
// decode_fused.hip: LN + c_attn projection and the cache attention of one layer in one launch (qkv_attn_fused_kernel)
bool qkv_attn_fused_supported(const GemvArgs& g, int H, int dh);
int qkv_attn_fused(const GemvArgs& g, unsigned long long* gran, int* err, void* kc, void* vc, const int* len,
                   const int* kv_start, const int* prefix_dev, int H, int dh, int Smax, float* part_o, float* part_ml,
                   const uint8_t* anc, int nb, hipStream_t s);
// decode_sampler.hip
int sampler2_step(const SamplerArgs& a, int B, hipStream_t s);
int sampler_wide_prepare();  // once per device ordinal, outside graph capture: sampler_wide_kernel's dynamic LDS limit
// a.rows set: one launch per class in `classes` (bit ROWCLS_*), grid B each; a block whose row another class owns returns at once
int sampler_rows_step(const SamplerArgs& a, int B, int classes, hipStream_t s);
// the token choice of ONE row of a batch (row admission): the per-row pointers of `a` are advanced to `slot` - uniforms by slot
// with the stride a.B kept - and the kernel of class `cls` runs with a grid of one block; no other row is read or written
int sampler_slot_step(const SamplerArgs& a, int slot, int cls, hipStream_t s);
int decode_embed2(float* h, const void* emb, const void* pos, const int* tok, const int* len, int B, int D, int tw,
                  hipStream_t s);

// larger decode batches (decode_mfma.hip): X bf16 [B,K], W bf16 [N,K]; Y fp32 (store / accumulate) or bf16
bool skinny_mfma_shape_ok(const GemvArgs& g);   // the shape rule alone, no pointer is looked at
bool skinny_mfma_supported(const GemvArgs& g);  // the shape rule and what the pointers have to satisfy
int skinny_mfma(const GemvArgs& g, hipStream_t s);
int ln_rows_bf16(void* y, float* x, const float* g1, const float* b1, int rows, int D, float eps, int passes,
                 const float* partial, int nsplit, const float* pbias, int y_tiled, hipStream_t s);

}  // namespace itts

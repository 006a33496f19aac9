// The inference engine behind the C ABI: owns nothing but scratch/state memory; weights stay in the
// caller's arena and are bound by name (itts_engine_bind_tensor).
#pragma once
#include <map>
#include <utility>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/itts_hip.h"
#include "itts_decode.h"
#include "itts_engine_kernel.h"
#include "itts_kernels.h"

namespace itts {

struct Tensor {
  const void* p = nullptr;
  int dt = 0, nd = 0;
  int64_t d[4] = {0, 0, 0, 0};
  int64_t numel() const {
    int64_t n = 1;
    for (int i = 0; i < nd; ++i) n *= d[i];
    return n;
  }
};

// a linear / conv layer: W [nphase][N][taps*Cin] in `dt`, bias fp32 [N] (optional), BN-eval affine (optional)
struct Lin {
  const void* w = nullptr;
  const float* b = nullptr;
  const float* bn_scale = nullptr;
  const float* bn_shift = nullptr;
  int N = 0, Cin = 0, taps = 1, nphase = 1, dt = 0;
  const void* w8 = nullptr;       // optional fp8 e4m3 copy of w (decode GEMV of the GPT), one scale per output row
  const float* wscale = nullptr;
  void* wt = nullptr;             // bf16 copy in MFMA-fragment tiles (wtile_off) for the batched decode step, made on first use
  void* wt8 = nullptr;            // the same for the fp8 copy (8 bytes per lane: half-KiB fragments)
};
struct Norm {
  const float* g = nullptr;
  const float* b = nullptr;
};

struct ConformerLayerW {
  Norm norm_mha, norm_conv, norm_ff, norm_final, conv_norm;
  Lin qkv, pos, out, pw1, pw2, w1, w2;
  const float *bu = nullptr, *bv = nullptr, *dw_w = nullptr, *dw_b = nullptr;
};
struct CondW {
  bool ok = false;
  const float *conv_w = nullptr, *conv_b = nullptr;
  Lin embed_out;
  const void* pe = nullptr;  // [max_len, od] activation dtype
  int pe_len = 0;
  std::vector<ConformerLayerW> layers;
  Norm after_norm;
  // perceiver
  const float* latents = nullptr;
  Lin proj;
  struct PL {
    Lin to_q, to_kv, to_out, ff1, ff2;
  };
  std::vector<PL> pl;
  const float* gamma = nullptr;
  int ffi = 0, ffi_pad = 0, inner = 0;
};
struct GptLayerW {
  Norm ln1, ln2;
  Lin attn, proj, fc, proj2;
};
struct GptW {
  bool ok = false;
  std::vector<GptLayerW> layers;
  Norm ln_f, final_norm;
  Lin head;
  const void *text_emb = nullptr, *mel_emb = nullptr, *mel_pos = nullptr, *text_pos = nullptr;
};
struct AmpW {
  Lin c1[4], c2[4];
  const float *a1[4], *b1[4], *a2[4], *b2[4];
};
struct BigvganW {
  bool ok = false;
  Lin conv_pre, cond_layer, conv_post;
  std::vector<Lin> ups, conds;
  std::vector<AmpW> res;
  const float *post_alpha = nullptr, *post_beta = nullptr, *filter = nullptr;
};
struct EcapaW {
  bool ok = false;
  Lin b0;
  struct Blk {
    Lin tdnn1, tdnn2, se1, se2;
    std::vector<Lin> res;
  };
  std::vector<Blk> blks;
  Lin mfa, asp_x, asp_ms, asp_conv, fc;
  const float *aspbn_scale = nullptr, *aspbn_shift = nullptr;
};
struct DvaeW {
  bool ok = false;
  const void* codebook = nullptr;
  Lin in_conv, out_conv;
  struct RB {
    Lin c0, c2, c4;
  };
  std::vector<RB> rbs;
  std::vector<Lin> ups;
  // encoder of get_codebook_indices (optional: only when the checkpoint carries it)
  bool enc_ok = false;
  std::vector<Lin> enc;   // stride-2 convs as 2-tap convs over paired rows
  std::vector<RB> erbs;
  Lin eout, quant;        // 1x1 to the codebook dim; quant = the codebook as a [tokens, dim] projection
  const float* codebook_sq = nullptr;
};

// What a captured decode step has baked into its nodes: the graph is replayed only while this compares equal.
// Everything SamplerArgs carries by value is baked into the captured nodes: max_gen is the ids row stride and the
// `k < max_gen` bound, so a per-request max_mel_tokens must re-capture (same B / Smax notwithstanding).
// Whatever SamplerArgs, BeamArgs or EngArgs come to carry by value belongs here (and in Engine::graph_key()).
struct GraphKey {
  int B = 0, Smax = 0, max_gen = 0, use_forced = 0, input_n = 0, host_sample = 0;
  int Bcache = 0;  // rows the cache was laid out for (DecodeState::Bcache): the per-layer cache offsets after a row retirement
  int fuse = 0, eng = 0;  // derived: fuse && !fuse_failed, engine_usable()
  int nb = 1, beam_sample = 1, suppress_stop = 0, do_sample = 0, top_k = 0;
  int ct = 0;  // element type of the K/V cache (DecodeState::ct): the attention form and every per-layer cache offset
  float length_penalty = 0.f, typical_mass = 0.f, penalty = 0.f, top_p = 1.f, temperature = 1.f;  // compared as floats: a NaN re-captures
  // mixed batch (DecodeState::rows_active): the step launches one sampler kernel per class present (bits ROWCLS_*).  The entries
  // themselves live in device memory behind a pointer that only changes together with dropped graphs
  int rows_active = 0, rows_classes = 0;
  bool operator==(const GraphKey& o) const {
    return rows_active == o.rows_active && rows_classes == o.rows_classes && B == o.B &&Bcache == o.Bcache && Smax == o.Smax && max_gen == o.max_gen && use_forced == o.use_forced && input_n == o.input_n &&
           host_sample == o.host_sample && fuse == o.fuse && eng == o.eng && nb == o.nb && beam_sample == o.beam_sample && ct == o.ct &&
           length_penalty == o.length_penalty && typical_mass == o.typical_mass && penalty == o.penalty &&
           suppress_stop == o.suppress_stop && do_sample == o.do_sample && top_k == o.top_k && top_p == o.top_p &&
           temperature == o.temperature;
  }
};

struct DecodeState {
  int B = 0, Smax = 0, prefix = 0, max_gen = 0;
  // Row retirement (Engine::gpt_retire_rows, opt-in): B is the row count the steps run at, Bcache the one the cache of this
  // generation was laid out for and B0 the one the caller sees - all three are what the prefill set until a retirement shrinks B.
  // orig[slot]: the original row a slot holds.  Retired rows live on the host: their codes (stop-padded) and last logits
  int Bcache = 0, B0 = 0;
  std::vector<int> orig;
  std::vector<uint8_t> retired;       // [B0]
  std::vector<int32_t> ret_codes;     // [B0][max_gen]
  std::vector<float> ret_logits;      // [B0][V]
  // Retirement of finished beam groups (gpt_set_retire_beams, opt-in): a group of nb rows moves as a unit.  retired / ret_logits /
  // orig stay per row; ret_codes is then [B0 / nb][ret_keep][max_gen] by original item, the finalised hypotheses of a retired item
  int retire_beams = 0;               // the sticky switch (ITTS_RETIRE_BEAMS overrides it per call)
  int ret_keep = 1;                   // beam_returns when the first group retired: the fetch returns as many per item
  // Row admission (Engine::gpt_admit_rows, opt-in): finished slots take new requests, which get the original rows B0, B0 + 1, ..
  // - so B0 grows while B and Bcache stay.  What the generation then owns by ORIGINAL row: the per-row settings (a table
  // generation; row_table is the caller's setting for the next prefill and keeps its size) and the draws [B0][max_gen]
  int admitted = 0;                   // rows admitted so far (0: everything as before)
  std::vector<RowSampling> adm_rows;  // [B0], empty in a scalar generation
  std::vector<float> adm_uniforms;    // [B0][max_gen], empty when no row of the generation draws
  // Admission under beams (gpt_set_admit_beams, opt-in): whole batch items are admitted, nb rows each, so B0 grows by nb per item
  // and the groups run at different steps from then on (the host reads every item's own len).  adm_uniforms is then
  // [B0 / nb][max_gen][2 * nb] by original item, ret_codes [B0 / nb][ret_keep][max_gen]
  int admit_beams = 0;                // the sticky switch (ITTS_ADMIT_BEAMS overrides it per call)
  size_t cache_bytes = 0;
  void *kc = nullptr, *vc = nullptr;  // [layers][B][H][Smax][dh], elements of type ct
  // element type of the cache: the engine's own (F32 / BF16) or, opt-in on a 16-bit engine, FP8 = e4m3 bytes (itts_gpt_set_kv_fp8 /
  // ITTS_KV_FP8).  kv_fp8 is the sticky request; ct / ces are what the prefill latched for the whole generation
  // (ensure_decode_state), ct_held the type whose values the allocation last held (-1: fresh).  An fp8 cache keeps the launch
  // path's whole-form attention at every row count (no split form, no fused qkv + attention launch) unless the engine object
  // opted into the persistent engine's fp8-cache form (eng_kv8 below; <= 6 rows).
  int kv_fp8 = 0, ct = 0, ct_held = -1;
  size_t ces = 4;
  float *h = nullptr, *qkv = nullptr, *ctx = nullptr, *act = nullptr, *hn = nullptr, *logits = nullptr;
  float *attn_o = nullptr, *attn_ml = nullptr;  // split decode attention partials (decode_attn.hip, ATTN_NSPLIT), small batches
  float* partial = nullptr;           // [4][B][D] split-K partial sums of the residual projections (batched decode)
  int pend_split = 0;                 // launch-time bookkeeping: partials waiting to be absorbed by the next LayerNorm
  const float* pend_bias = nullptr;
  int *len = nullptr, *prefix_dev = nullptr;  // len[b]: tokens generated so far by row b
  int *kv_start = nullptr, *cur_tok = nullptr, *ids = nullptr, *unfinished = nullptr;
  uint8_t* seen = nullptr;
  int cap_B = 0, cap_gen = 0;
  float penalty = 1.f;
  int suppress_stop = 0;
  hipGraphExec_t graph = nullptr, graphK = nullptr;  // one decode step / ITTS_GRAPH_STEPS (8) steps per launch
  GraphKey graph_key;                                // what they were captured with
  int graph_captures = 0;                            // times the step was captured (itts_gpt_graph_captures: tests)
  void drop_graphs() {                               // (the caller synchronises the stream first where a replay may be in flight)
    for (hipGraphExec_t* ge : {&graph, &graphK})
      if (*ge) {
        (void)hipGraphExecDestroy(*ge);
        *ge = nullptr;
      }
  }
  // multinomial sampling (itts_gpt_set_sampling): parameters baked into the captured step, uniforms [max_gen][B]
  int do_sample = 0, top_k = 0;
  float top_p = 1.f, temperature = 1.f;
  float* uniforms = nullptr;
  size_t uniforms_cap = 0;
  int have_uniforms = 0;  // this generation's prefill set the buffer up for its own [max_gen][B] draws (else it may be an earlier one's)
  // mixed batch (itts_gpt_set_sampling_rows, a table that is not uniform): what the prefill latched for this generation.
  // rows [B] on the device, in slot order; rows_classes: the classes its live rows hold (bits ROWCLS_*, sampler_rows_step)
  RowSampling* rows = nullptr;
  int rows_cap = 0, rows_active = 0, rows_classes = 0;
  // beam-sample (itts_gpt_set_beam_sample): B = batch items * nb rows; state of beam.hip
  int nb = 1;                         // beams per batch item (1 = off)
  int beam_sample = 1;                // 1: beam_sample (draws), 0: beam_search (deterministic top-2nb)
  float length_penalty = 0.f;
  int* beam_ids = nullptr;           // [2][B][max_gen]
  uint8_t* anc = nullptr;            // [2][B][Smax]
  float* beam_scores = nullptr;      // [B]
  float* cand_sc = nullptr;          // beam sampler scratch [rows][BEAM_MAX_CAND]
  int *cand_tok = nullptr, *cand_n = nullptr;
  int *hyp_tok = nullptr, *hyp_len = nullptr, *hyp_order = nullptr, *hyp_n = nullptr, *hyp_counter = nullptr, *beam_done = nullptr;
  float *hyp_score = nullptr, *hyp_worst = nullptr;
  size_t beam_cap = 0;               // bytes-independent capacity key: rows * max_gen * Smax the beam buffers were sized for
  int beam_rows = 0, beam_gen = 0, beam_smax = 0;
  // whole-vocabulary beam sampler (beam_sample with top_k < 1 or > 128 on the device): one block, carved up by beam_wide_bytes' order
  void* wide_buf = nullptr;
  size_t wide_cap = 0;
  BeamWide wide;                     // pointers into wide_buf for the current request
  int wide_valid = 0;                // a device-sampled wide step of this generation has written wide.pick_* / wide.kept
  // LN + c_attn + cache attention in one launch (decode_fused.hip qkv_attn_fused): per-layer granule buffers + error flag
  unsigned long long* gran = nullptr;  // [layers][cap_B <= 4][3 * D]
  int* fuse_err = nullptr;
  int fuse_failed = 0;                 // a hand-off timed out: two launches from then on
  int fuse = 0;                        // opt-in (ITTS_FUSE_QKV_ATTN=1 / debug bit 3): measured 1.5 % slower than two launches; 0 again after a hand-off timeout
  // persistent decode engine (decode_engine.hip): the step as one launch, <= 6 rows (beam rows included), bf16 weights - or,
  // opt-in (eng_fp8 / ITTS_ENGINE_FP8), the fp8 copies of every projection and the head (bf16 build only)
  unsigned long long* eng_gran = nullptr;
  unsigned* eng_ctr = nullptr;           // [0] step counter, [1] abort word
  int eng_off = 0;                       // debug bit 4 / ITTS_ENGINE=0: keep the five-launches-per-layer path (A/B)
  int eng_force = 0;                     // debug bit 5: use the engine whatever ITTS_ENGINE / the default says
  int eng_failed = 0;                    // a hand-off timed out: launch path from then on
  int eng_fp8 = 0;                       // itts_gpt_set_engine_fp8: a model with fp8 GPT weights may use the engine (sticky; default: launch path)
  int eng_kv8 = 0;                       // itts_gpt_set_engine_kv_fp8: a generation with an fp8 K/V cache may use the engine (sticky; default: launch path)
  int graph_mode = 0;                    // last_mode of the captured step
  float typical_mass = 0.f;                        // TypicalLogitsWarper pre-pass (0 = off)
  float* scores2 = nullptr;                        // [cap_B][V] its output
  int* forced = nullptr;  // [cap_B][cap_gen] forced token per (row, step) or -1; allocated with ids
  int use_forced = 0;
  int host_sample = 0;  // the caller picks every token (itts_gpt_commit): the step stops behind the head
  int input_n = 0;      // forced steps that are HF input_tokens (positions k + 1 instead of k + 2)
  int last_mode = 0;                   // 1: the last captured / launched decode step ran on the persistent engine
  bool active = false;
};

int bigvgan_packed_gap(const itts_config& c);  // zero frames a packed sentence needs behind its signal: the convolutions' largest reach
const char* bigvgan_packed_refusal(const itts_config& c, const void* latent, const float* spk, const int* off_host, const int* lens_host,
                                   int n, const float* wav);  // null = the call can run; host memory only

struct Engine {
  itts_config cfg;
  int adt = 0;  // activation / weight dtype
  size_t es = 4;
  std::unordered_map<std::string, Tensor> tensors;
  bool finalized = false;
  CondW cond;
  GptW gpt;
  BigvganW bv;
  EcapaW ec;
  DvaeW dv;
  DecodeState ds;
  bool use_graph = true;
  bool force_simple = false;

  // scratch workspace (bump allocator, two-pass: dry run sizes it, real run uses it)
  char* ws = nullptr;
  size_t ws_cap = 0, ws_off = 0;
  bool dry = false;
  void ws_reset() { ws_off = 0; }
  void* alloc(size_t bytes) {
    const size_t a = (ws_off + 255) & ~size_t(255);
    ws_off = a + bytes;
    return dry ? (void*)(uintptr_t)(0x1000 + a) : (void*)(ws + a);
  }
  int ws_reserve(size_t bytes, hipStream_t s);
  // A second scratch arena for the speaker encoder: Engine::ecapa swaps it in for the duration of the call, so that the caller may
  // run it on a side stream beside the conditioning encoder / the prefill (both are chains of small kernels that leave most of the
  // chip idle; itts_hip/engine.py ecapa(overlap=True)).  K-split GEMMs are off inside the swap (one split workspace per engine).
  char* ws_b = nullptr;
  size_t ws_b_cap = 0;
  bool ksplit_off = false;
  struct ArenaSwap {
    Engine& e;
    explicit ArenaSwap(Engine& en) : e(en) { flip(); e.ksplit_off = true; }
    ~ArenaSwap() { flip(); e.ksplit_off = false; }
    void flip() {
      std::swap(e.ws, e.ws_b);
      std::swap(e.ws_cap, e.ws_b_cap);
    }
  };
  // The packed latent pass (gpt_latent_packed) runs its GEMMs under both: no K split (ksplit_off, the flag above) and the kernel
  // family picked without looking at M (gemm_pin -> gemm_pinned) - what makes a sequence's latent independent of its companions.
  bool gemm_pin = false;
  struct PackedPass {
    Engine& e;
    explicit PackedPass(Engine& en) : e(en) { e.ksplit_off = e.gemm_pin = true; }
    ~PackedPass() { e.ksplit_off = e.gemm_pin = false; }
  };
  // The packed vocoder (bigvgan_packed) likewise: no K split, and every convolution through gemm_pinned_conv (conv_pin) - the narrow
  // conv where the shape apart from its row count is one of its own, else gemm_which_pinned's order; never gemm_glds.
  bool conv_pin = false;
  struct PackedVocoderPass {
    Engine& e;
    explicit PackedVocoderPass(Engine& en) : e(en) { e.ksplit_off = e.conv_pin = true; }
    ~PackedVocoderPass() { e.ksplit_off = e.conv_pin = false; }
  };
  // raw partial sums of K-split GEMMs (Engine::conv): [split][M][N] fp32, allocated at the first split launch
  static constexpr size_t KSPLIT_WS_BYTES = size_t(64) << 20;
  float* ksplit_ws = nullptr;

  // debug taps
  bool debug = false;
  std::map<std::string, std::vector<float>> taps;
  int tap(const char* name, const void* p, int dt, int64_t n, hipStream_t s);

  void* gpt_tiles = nullptr;  // one allocation: Lin::wt of every GPT projection + head (batched decode, bf16)
  int ensure_decode_tiles(hipStream_t s);
  ~Engine();

  // the GemmArgs fields a layer determines (W, N, Cin, taps, bias, BN affine) and the operand geometry; callers set only what differs
  static GemmArgs conv_args(const void* A, int lda, const Lin& w, void* C, int ldc, int M, int T);
  // op wrappers (skip launches in dry mode)
  int lin(void* C, int tc, const void* A, int ta, int lda, const Lin& w, int M, int ldc, hipStream_t s, int act = ACT_NONE,
          const void* R = nullptr, int ldr = 0, float alpha = 1.f);
  int conv(GemmArgs& g, int ta, int tw, int tc, hipStream_t s, const int* lens = nullptr, int mul = 1);  // lens / mul: gemm()
  // a fused-activation call (g.pre_*) of the packed vocoder: the segment form of the narrow conv or nothing (gemm_pinned_conv)
  int conv_seg(GemmArgs& g, int ta, int tw, int tc, hipStream_t s, const SegTable& seg, int mul);
  int ln(void* y, int ty, const void* x, int tx, const Norm& n, int rows, int D, hipStream_t s, int act = ACT_NONE,
         float eps = 1e-5f);

  // model entry points
  int finalize();
  int conditioning(const void* mel, int F, float* cond_out, hipStream_t s, int F_total = 0);
  int ecapa(const void* mel, int B, int F, float* spk_out, hipStream_t s);
  int gpt_prefill(const float* cond, const int32_t* text_ids, int B, int L, int max_gen, float penalty, int suppress,
                  hipStream_t s);
  int gpt_decode(int nsteps, hipStream_t s);
  int gpt_decode_steps(int nsteps, hipStream_t s);
  int gpt_set_sampling(int do_sample, int top_k, float top_p, float temperature, const float* uniforms_host, long n);
  std::vector<float> sample_uniforms;  // host copy, uploaded by the next prefill
  // per-row settings of the following generations (B = 0 clears); uniforms as gpt_set_sampling.  A table whose rows are all
  // equal IS the scalar setting (gpt_set_sampling is called with it) and only its penalty and row count are kept here
  int gpt_set_sampling_rows(const RowSampling* rows_host, int B, const float* uniforms_host, long n);
  std::vector<RowSampling> row_table;  // [B] by original row; empty = no table
  bool row_table_uniform = false;
  bool row_table_keep = false;  // gpt_keep_row_table: a uniform table stays a table generation (so that it can admit rows of other settings)
  int gpt_keep_row_table(int on);
  int upload_row_table(hipStream_t s);  // ds.rows / ds.rows_classes from row_table by ds.orig (or the identity)
  int gpt_set_forced(const int32_t* ids_host, int B, int n);
  int gpt_set_input_tokens(const int32_t* ids_host, int B, int n);
  int gpt_set_host_sampling(int on);
  int cond_per_row = 0;  // itts_gpt_set_cond_per_row: the cond passed to prefill holds one [latents, D] block per batch item
  int gpt_commit(const int32_t* tokens_host, hipStream_t s);
  int gpt_beam_state(int32_t* ids_host, float* scores_host, int32_t* done_host, int* step_host, hipStream_t s);
  int gpt_commit_beams(const float* pick_score_host, const int32_t* pick_tok_host, const int32_t* pick_beam_host, hipStream_t s);
  BeamArgs beam_args(const float* lg_in, bool typical) const;
  int forced_input = 0;  // the forced tokens are HF `input_tokens`: token k sits at mel position k + 1 (model.py:141-144)
  int gpt_set_typical(float mass);
  int gpt_set_beam_sample(int num_beams, int top_k, float top_p, float temperature, const float* uniforms_host, long n);
  int gpt_set_beams(int num_beams, int do_sample, int top_k, float top_p, float temperature, float length_penalty,
                    const float* uniforms_host, long n);
  int gpt_set_beam_returns(int n);
  int beam_do_sample = 1;
  float beam_length_penalty = 0.f;
  int gen_epoch = 0;   // generation counter: high bits of the hand-off tags (never 0)
  int beam_beams = 1;  // requested beams for the following generations (1 = off)
  int beam_returns = 1;  // hypotheses returned per batch item (generate()'s num_return_sequences = num_beam_hyps_to_keep)
  int ensure_beam_state(int rows, int max_gen, int Smax, hipStream_t s);
  int ensure_beam_wide_state(int rows, int nb, int V, hipStream_t s);
  int gpt_beam_picks(float* score_host, int32_t* tok_host, int32_t* beam_host, int32_t* kept_host, hipStream_t s);
  int beam_finalize(int32_t* codes_host, hipStream_t s);
  // the scorer's state on the host (beam_read_state) and BeamSearchScorer.finalize for one batch item of it: what beam_finalize
  // runs over every item at the fetch and gpt_retire_rows over the retiring items
  struct BeamHost {
    int k = 0;  // the common step (of row 0 once beam groups were admitted: item b then reads len[b * nb])
    bool both = false;     // groups were admitted: ids holds BOTH halves [2][rows][max_gen], an item's live half is len & 1
    std::vector<int> len;  // [rows]
    std::vector<int> done, hlen, hord;
    std::vector<float> bscore, hscore;
    std::vector<int32_t> ids, htok;  // the live half of beam_ids [rows][max_gen], hyp_tok [items][nb + 1][max_gen]
  };
  int beam_read_state(BeamHost& st, hipStream_t s);
  int beam_finalize_item(const BeamHost& st, int b, int32_t* out) const;  // out [beam_returns][max_gen]
  std::vector<int32_t> forced_host;  // [forced_B][forced_n], uploaded by the next prefill
  int forced_B = 0, forced_n = 0;
  int gpt_status(int* steps, int* n_unf, hipStream_t s);
  int gpt_fetch(int32_t* codes, float* logits, hipStream_t s);
  int fetch_retired(int32_t* codes, float* logits, hipStream_t s);  // gpt_fetch after a retirement: original row order
  int gpt_retire_rows(int* rows_now, hipStream_t s);  // compact a running single-beam generation to its unfinished rows (opt-in)
  int gpt_set_retire_beams(int on);                   // opt-in: gpt_retire_rows also retires the finished groups of a beam generation
  int retire_beam_groups(int* rows_now, hipStream_t s);  // its beam branch
  // refill n finished slots of the running generation with new requests (opt-in); slots_out [n]: the slots they took
  int gpt_admit_rows(const float* cond, int cond_rows, const int32_t* text_ids, int n, int L, const RowSampling* rows_host,
                     const float* uniforms_host, const int32_t* forced_host, int n_forced, int32_t* slots_out, hipStream_t s);
  int gpt_set_admit_beams(int on);  // opt-in: gpt_admit_rows admits whole batch items into a beam generation
  // its beam branch: n items, text_ids [n][L], uniforms_host [n][max_gen][2 * nb]; items_out [n]: the item slots they took
  int admit_beam_groups(const float* cond, int cond_rows, const int32_t* text_ids, int n, int L, const float* uniforms_host,
                        int32_t* items_out, hipStream_t s);
  int gpt_row_status(int32_t* orig_host, int32_t* len_host, int32_t* unf_host, hipStream_t s);  // per slot, [B] each
  int gpt_latent(const float* cond, const int32_t* text_ids, int L, const int32_t* codes, int T, void* latent_out,
                 hipStream_t s);
  int gpt_latent_batch(const float* cond, const int32_t* text_ids, const int* Ls, const int32_t* codes, const int* Ts,
                       int nseq, void* latent_out, hipStream_t s, const int32_t* cond_index = nullptr, int n_cond = 1);
  // the same interface on PACKED rows [sum S_i, D]: no pad rows, varlen attention, pinned GEMM family, no K split, no K/V cache;
  // nseq <= VARLEN_MAX_SEQ.  A sequence's latent has the same bits alone, with any companions, in any order.
  int gpt_latent_packed(const float* cond, const int32_t* text_ids, const int* Ls, const int32_t* codes, const int* Ts,
                        int nseq, void* latent_out, hipStream_t s, const int32_t* cond_index = nullptr, int n_cond = 1);
  // The INCREMENTAL packed latent pass (opt-in): up to VARLEN_MAX_SEQ sequences opened together, each fed its codes in
  // pieces.  The state below lives from open to close; the K/V history is allocated at open and freed at close (never inside a pass,
  // and nothing of it is known to a captured decode step, whose buffers are DecodeState's).  After any sequence of appends the rows
  // delivered so far are, bit for bit, the first rows of gpt_latent_packed over the final codes.
  struct LatentStream {
    bool open = false;
    int nseq = 0, max_codes = 0;
    int cap = 0;           // history rows per sequence: the longest prefix + max_codes
    int kernel = 1;        // the attention family gpt_latent_packed takes on this engine (1 simple, 2 mfma), fixed at open
    void* hist = nullptr;  // [layers][nseq * cap][2 D] in the engine's activation type: k | v of every computed row
    const float* cond = nullptr;  // the caller's conditioning (device), read by every first append
    std::vector<int> prefix;      // [nseq] rows in front of the start-mel row: cond_latents + L + 2
    std::vector<int> done;        // [nseq] codes taken so far = latent rows delivered
    std::vector<int> computed;    // [nseq] rows whose k / v the history holds (0, or prefix + done)
    std::vector<std::vector<int>> rd;  // [nseq] the row descriptors of [cond, text, start-mel, codes so far], 4 ints per row
  };
  LatentStream lstream;
  int gpt_latent_stream_open(const float* cond, const int32_t* cond_index, int n_cond, const int32_t* text_ids, const int* Ls, int nseq,
                             int max_codes, hipStream_t s);
  // codes [sum counts], counts [nseq] (0 leaves a sequence alone); latent_out [sum counts, D] in the engine dtype, sequence after sequence
  int gpt_latent_stream_append(const int32_t* codes, const int* counts, void* latent_out, hipStream_t s);
  int gpt_latent_stream_close(hipStream_t s);
  // gpt_layers_packed with kv_rows_append + attention_append in place of attention_varlen: h fp32 [M, D] holds the chunk's rows
  // (sequence b's at rows app.q_off[b] ..; rows that belong to no sequence are carried along and ignored)
  int gpt_layers_append(float* h, int M, const AppendArgs& app, hipStream_t s);
  int latent_stream_pass(const int* rd_host, int M, const AppendArgs& app, const int* out_row, const int* out_n, long Ttot, void* latent_out,
                         hipStream_t s);
  // lens_host (optional, [B], each in [1, T]): a padded ragged batch - item b is a latent of lens_host[b] frames, whatever its rows
  // behind them hold; its waveform is that of the item alone, zeros from sample lens_host[b] * up on
  int bigvgan(const void* latent, const float* spk, int B, int T, float* wav, hipStream_t s, const int* lens_host = nullptr);
  // The sentences of a call back to back as ONE item (opt-in): latent [off_host[n], D], sentence b the frames
  // [off_host[b], off_host[b + 1]) of which the first lens_host[b] are signal and at least bigvgan_packed_gap(cfg) are left over;
  // spk fp32 [n, E]; wav fp32 [off_host[n] * up], zeros in every gap.  A sentence's samples do not depend on its companions, their
  // order or the chunking.  n <= SEG_MAX; every refusal (bigvgan_packed_refusal) is made on the host before any HIP call.
  int bigvgan_packed(const void* latent, const float* spk, const int* off_host, const int* lens_host, int n, float* wav, hipStream_t s);
  int dvae_decode(const int32_t* codes, int B, int T, void* mel_out, hipStream_t s);
  int dvae_encode(const void* mel, int B, int T, int32_t* codes_host, hipStream_t s);

  // internals
  // admit_slots (host, [B]): the cache rows the B rows of this pass go to (kv_admit); nullptr: rows 0 .. B - 1 (kv_scatter)
  int gpt_layers_full(float* h, int B, int S, const int* kv_start_dev, bool write_cache, hipStream_t s, const int* admit_slots = nullptr);
  // gpt_layers_full's sibling for the packed latent pass: the 24 blocks over h fp32 [M = seqs.off[nseq], D] (in place), attention
  // per sequence (attention_varlen's dispatcher; seqs carries nseq and off, the rest is filled here); writes no cache
  int gpt_layers_packed(float* h, const VarlenArgs& seqs, hipStream_t s);
  int decode_step_launch(hipStream_t s);
  GraphKey graph_key() const;
  EngArgs engine_args(int& eng_first, bool& fold_head, bool& fold_samp) const;
  bool rows_on_mfma(int B) const;  // the batched decode step: weights streamed once, batch on MFMA
  bool engine_usable() const;
  int gpt_set_engine_kv_fp8(int on);  // opt-in: the persistent engine reads and appends an fp8 K/V cache (decode_engine_kernel<.., KV8>)
  bool engine_fp8_model() const;  // every projection of every block and the head carry an fp8 copy + row scales
  int ensure_engine_state(hipStream_t s);
  int engine_check(hipStream_t s);
  int head_and_sample(hipStream_t s, bool have_logits = false, bool sampled = false);
  int head_rows(float* h, float* hn, float* logits, int B, hipStream_t s);  // ln_f -> final_norm -> mel_head of B rows
  int sample_from_logits(hipStream_t s, bool sampled = false);
  SamplerArgs greedy_sampler_args(const float* lg_in, bool typical) const;
  int ensure_decode_state(int B, int Smax, int max_gen, hipStream_t s);
  template <typename F>
  int two_pass(F&& body, hipStream_t s) {
    dry = true;
    ws_reset();
    int st = body();
    dry = false;
    if (st != OK) return st;
    ITTS_TRY(ws_reserve(ws_off + 4096, s));
    ws_reset();
    return body();
  }
};

}  // namespace itts

// GPT-2 acoustic LM: prefix assembly + prefill (step 0), per-token decode (hipGraph-captured), latent pass.
// Reference: UnifiedVoice.inference_speech / prepare_gpt_inputs / forward(return_latent) and
// GPT2InferenceModel.forward (indextts/gpt/model.py:115-192,521-708); HF transformers 4.36.2 GPT2Model /
// greedy_search semantics (not vendored; restated in oracle/gpt.py and pinned by tests/golden).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <mutex>

#include <cstdlib>

#include "engine.h"

namespace itts {

namespace {

// row descriptor for the embedding assembly: kind 0 zero, 1 cond row, 2 text (emb+pos), 3 mel (emb+pos)
struct RowDesc {
  int kind, a, b, pad;
};

template <typename TW>
__global__ void gpt_embed_rows_kernel(float* __restrict__ h, const RowDesc* __restrict__ rd, const float* __restrict__ cond,
                                      const TW* __restrict__ text_emb, const TW* __restrict__ text_pos,
                                      const TW* __restrict__ mel_emb, const TW* __restrict__ mel_pos, int D) {
  const int r = blockIdx.x;
  const RowDesc d = rd[r];
  for (int i = threadIdx.x; i < D; i += blockDim.x) {
    float v = 0.f;
    if (d.kind == 1) v = cond[(size_t)d.a * D + i];
    else if (d.kind == 2) v = ldf(text_emb + (size_t)d.a * D + i) + ldf(text_pos + (size_t)d.b * D + i);
    else if (d.kind == 3) v = ldf(mel_emb + (size_t)d.a * D + i) + ldf(mel_pos + (size_t)d.b * D + i);
    h[(size_t)r * D + i] = v;
  }
}

__global__ void init_decode_state_kernel(uint8_t* seen, int* unfinished, int* cur_tok, int* len, int* prefix_dev,
                                         int B, int V, int fake_id, int start_tok, int prefix, int epoch) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (long)B * V) {
    const int v = (int)(i % V);
    seen[i] = (v == fake_id || v == start_tok) ? 1 : 0;
  }
  if (i < B) {
    unfinished[i] = 1;
    cur_tok[i] = start_tok;
    len[i] = 0;
  }
  if (i == 0) {
    prefix_dev[0] = prefix;
    prefix_dev[1] = epoch;  // generation epoch: the high bits of the in-launch hand-off tags (qkv_attn_fused)
  }
}

// beam-sample state of a fresh generation: identity cache ancestry (every beam row reads its own prefix copy), zero
// running scores (beam_sample starts all beams at 0, unlike beam_search), no finished hypotheses
__global__ void beam_init_kernel(uint8_t* anc, float* beam_scores, int* hyp_order, int* hyp_n, float* hyp_worst,
                                 int* hyp_counter, int* done, int rows, int nb, int Smax, int do_sample) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)rows * Smax;
  if (i < 2 * n) anc[i] = (uint8_t)(((i % n) / Smax) % nb);
  // beam_sample starts every beam at 0; beam_search starts beams 1.. at -1e9 so that step 0 expands beam 0 only
  if (i < rows) beam_scores[i] = (do_sample || i % nb == 0) ? 0.f : -1e9f;
  const int B = rows / nb;
  if (i < (long)B * (nb + 1)) hyp_order[i] = -1;
  if (i < B) {
    hyp_n[i] = 0;
    hyp_worst[i] = 1e9f;
    hyp_counter[i] = 0;
    done[i] = 0;
  }
}

}  // namespace

#define K(call)               \
  do {                        \
    if (!dry) ITTS_TRY(call); \
  } while (0)

// full-sequence pass of the 24 blocks over h fp32 [B*S, D] (in place); optional KV-cache fill
int Engine::gpt_layers_full(float* h, int B, int S, const int* kv_start_dev, bool write_cache, hipStream_t s, const int* admit_slots) {
  const itts_config& c = cfg;
  const int D = c.model_dim, H = c.heads, dh = D / H, M = B * S;
  void* xn = alloc((size_t)M * D * es);
  void* qkv = alloc((size_t)M * 3 * D * es);
  void* ctx = alloc((size_t)M * D * es);
  void* act = alloc((size_t)M * 4 * D * es);
  for (int l = 0; l < c.layers; ++l) {
    const GptLayerW& L = gpt.layers[l];
    ITTS_TRY(ln(xn, adt, h, F32, L.ln1, M, D, s));
    ITTS_TRY(lin(qkv, adt, xn, adt, D, L.attn, M, 3 * D, s));
    if (write_cache) {
      const size_t lo = (size_t)l * ds.Bcache * H * ds.Smax * dh * ds.ces;  // the cache's element size, not the engine's
      if (admit_slots)  // a row admission: the B rows of this pass go to chosen rows of the running generation's cache
        K(kv_admit((char*)ds.kc + lo, (char*)ds.vc + lo, qkv, B, S, H, dh, ds.Smax, ds.Bcache, adt, ds.ct, admit_slots, s));
      else
        K(kv_scatter((char*)ds.kc + lo, (char*)ds.vc + lo, qkv, B, S, H, dh, ds.Smax, adt, ds.ct, s));
    }
    AttnArgs a;
    a.q = qkv;
    a.k = (const char*)qkv + (size_t)D * es;
    a.v = (const char*)qkv + (size_t)2 * D * es;
    a.o = ctx;
    a.B = B;
    a.H = H;
    a.Sq = a.Sk = S;
    a.dqk = a.dv = dh;
    a.ldq = a.ldk = a.ldv = 3 * D;
    a.ldo = D;
    a.scale = 1.f / std::sqrt((float)dh);
    a.causal = 1;
    a.kv_start = kv_start_dev;
    K(force_simple ? attention_simple(a, adt, s) : attention(a, adt, s));
    ITTS_TRY(lin(h, F32, ctx, adt, D, L.proj, M, D, s, ACT_NONE, h, D));
    ITTS_TRY(ln(xn, adt, h, F32, L.ln2, M, D, s));
    ITTS_TRY(lin(act, adt, xn, adt, D, L.fc, M, 4 * D, s, ACT_GELU_NEW));
    ITTS_TRY(lin(h, F32, act, adt, 4 * D, L.proj2, M, D, s, ACT_NONE, h, D));
  }
  return OK;
}

// the same 24 blocks over PACKED rows: sequence b is rows [seqs.off[b], seqs.off[b + 1]) of h; no pad rows, no cache
int Engine::gpt_layers_packed(float* h, const VarlenArgs& seqs, hipStream_t s) {
  const itts_config& c = cfg;
  const int D = c.model_dim, H = c.heads, dh = D / H, M = seqs.off[seqs.nseq];
  void* xn = alloc((size_t)M * D * es);
  void* qkv = alloc((size_t)M * 3 * D * es);
  void* ctx = alloc((size_t)M * D * es);
  void* act = alloc((size_t)M * 4 * D * es);
  VarlenArgs a = seqs;
  a.q = qkv;
  a.k = (const char*)qkv + (size_t)D * es;
  a.v = (const char*)qkv + (size_t)2 * D * es;
  a.o = ctx;
  a.H = H;
  a.dqk = a.dv = dh;
  a.ldq = a.ldk = a.ldv = 3 * D;
  a.ldo = D;
  a.scale = 1.f / std::sqrt((float)dh);
  for (int l = 0; l < c.layers; ++l) {
    const GptLayerW& L = gpt.layers[l];
    ITTS_TRY(ln(xn, adt, h, F32, L.ln1, M, D, s));
    ITTS_TRY(lin(qkv, adt, xn, adt, D, L.attn, M, 3 * D, s));
    K(attention_varlen(a, adt, force_simple ? 1 : 0, s));
    ITTS_TRY(lin(h, F32, ctx, adt, D, L.proj, M, D, s, ACT_NONE, h, D));
    ITTS_TRY(ln(xn, adt, h, F32, L.ln2, M, D, s));
    ITTS_TRY(lin(act, adt, xn, adt, D, L.fc, M, 4 * D, s, ACT_GELU_NEW));
    ITTS_TRY(lin(h, F32, act, adt, 4 * D, L.proj2, M, D, s, ACT_NONE, h, D));
  }
  return OK;
}

static int dev_alloc(void** p, size_t bytes) {
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  if (hipMalloc(p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("device allocation of " + std::to_string(bytes) + " bytes failed");
    return E_NOMEM;
  }
  return OK;
}

// The batched decode step (B > 4, bf16) streams its weights from fragment-tiled copies (wtile_off): made once per loaded
// checkpoint, on the first batched generation (+ 2 bytes per GPT weight; ITTS_NO_TILED_W=1 keeps the row-major stream).
bool Engine::rows_on_mfma(int B) const {
  const int D = cfg.model_dim;
  return adt == BF16 && B > 4 && D % 32 == 0 && D <= 2048;
}
int Engine::ensure_decode_tiles(hipStream_t s) {
  static const bool off = getenv("ITTS_NO_TILED_W") != nullptr;
  if (gpt_tiles || off || !gpt.ok) return OK;
  std::vector<Lin*> lins;
  for (GptLayerW& L : gpt.layers)
    for (Lin* l : {&L.attn, &L.proj, &L.fc, &L.proj2}) lins.push_back(l);
  lins.push_back(&gpt.head);
  size_t total = 0;
  for (Lin* l : lins) {
    if (l->dt != BF16 || l->Cin % 32 != 0 || l->taps != 1) return OK;  // not a bf16 checkpoint: nothing to tile
    total += (size_t)((l->N + 15) / 16) * 16 * l->Cin * (l->w8 ? 3 : 2);
  }
  ITTS_TRY(dev_alloc(&gpt_tiles, total));
  size_t o = 0;
  for (Lin* l : lins) {
    const size_t elems = (size_t)((l->N + 15) / 16) * 16 * l->Cin;
    l->wt = (char*)gpt_tiles + o;
    ITTS_TRY(retile_weights_bf16(l->wt, l->w, l->N, l->Cin, s));
    o += elems * 2;
    if (l->w8) {  // BASELINE config 5: the fp8 bytes in the same order
      l->wt8 = (char*)gpt_tiles + o;
      ITTS_TRY(retile_weights_fp8(l->wt8, l->w8, l->N, l->Cin, s));
      o += elems;
    }
  }
  return OK;
}

// The persistent decode engine (decode_engine.hip) replaces the 120 per-layer launches of a step when the step is the
// launch-bound small-batch bf16 one it was built for: IndexTTS-1.5 GPT dims, <= 6 rows (beam rows included: cache ancestry),
// a whole MI355X (256 CUs) to itself.  ITTS_ENGINE=0 (or debug bit 4) keeps the launch path.
// fp8 weight copies (BASELINE config 5) keep the launch path unless the engine object opted in (itts_gpt_set_engine_fp8, or
// ITTS_ENGINE_FP8=1 for every engine; ITTS_ENGINE_FP8=0 overrides the setter) AND this is the bf16 build AND all four projections
// of every block and the head carry an fp8 copy with its row scales - a mixed model stays on the launch path.
bool Engine::engine_fp8_model() const {
  if (!gpt.head.w8 || !gpt.head.wscale) return false;
  for (const GptLayerW& L : gpt.layers)
    for (const Lin* l : {&L.attn, &L.proj, &L.fc, &L.proj2})
      if (!l->w8 || !l->wscale) return false;
  return true;
}
bool Engine::engine_usable() const {
  const char* ev = getenv("ITTS_ENGINE");  // read per call: tests flip it inside one process
  const bool env_off = ev ? atoi(ev) == 0 : !ENG_DEFAULT_ON;
  // CU count of the device this call runs on (a process may drive engines on several ordinals, and a partitioned MI355X
  // exposes fewer CUs on some of them): cached per ordinal, the same key EngineGate uses
  static std::atomic<int> ncu_of[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  int ncu = ncu_of[dev & 63].load(std::memory_order_relaxed);
  if (ncu == 0) {
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = -1;
    ncu_of[dev & 63].store(ncu, std::memory_order_relaxed);
  }
  const itts_config& c = cfg;
  if ((env_off && !ds.eng_force) || ds.eng_off || ds.eng_failed || ncu != ENG_NCU) return false;
  if (ds.fuse && !ds.fuse_failed) return false;  // A/B switch of the fused projection + attention launch: a launch-path variant
  if (ds.B != ds.Bcache) return false;  // rows were retired: the engine computes its layer stride from its row count
  if (ds.ct == FP8) {  // the fp8 K/V cache keeps the launch path (decode_attn2_kernel<fp8_t>) unless the engine object opted in
    const char* k8 = getenv("ITTS_ENGINE_KV_FP8");  // read per call, like ITTS_ENGINE_FP8: =1 opts in, =0 overrides the setter
    if (!(k8 ? atoi(k8) != 0 : ds.eng_kv8 != 0)) return false;  // opted in: decode_engine_kernel<.., KV8>, both builds
  }
  if (adt != BF16 || ds.B < 1 || ds.B > ENG_MAX_ROWS || ds.nb < 1 || ds.B % ds.nb != 0 || (ds.nb > 1 && !ds.anc)) return false;
  if (c.model_dim != ENG_D || c.heads != ENG_H || c.layers < 1 || c.layers > ENG_MAX_LAYERS || ds.Smax > 2048 || ds.Smax % 256 != 0) return false;
  for (const GptLayerW& L : gpt.layers)
    for (const Lin* l : {&L.attn, &L.proj, &L.fc, &L.proj2})
      if (l->dt != BF16 || !l->b || l->taps != 1) return false;
  bool any8 = false;  // (an fp8 head alone, as before, only keeps the head out of the launch)
  for (const GptLayerW& L : gpt.layers)
    for (const Lin* l : {&L.attn, &L.proj, &L.fc, &L.proj2}) any8 = any8 || l->w8;
  if (any8) {
#ifdef ITTS_HALF_F16
    return false;  // the fp8 readers expand to bf16 pairs
#else
    const char* e8 = getenv("ITTS_ENGINE_FP8");  // read per call, like ITTS_ENGINE
    const bool opted = e8 ? atoi(e8) != 0 : ds.eng_fp8 != 0;
    if (!opted || !engine_fp8_model()) return false;
#endif
  }
  return true;
}

// Opt-in (sticky; ITTS_ENGINE_KV_FP8 overrides it per call): a generation whose cache type latched as FP8 may run on the
// persistent engine.  engine_usable() is part of the graph key, so a change re-captures the step of a running engine object.
int Engine::gpt_set_engine_kv_fp8(int on) {
  ds.eng_kv8 = on != 0;
  return OK;
}

int Engine::ensure_engine_state(hipStream_t s) {
  DecodeState& d = ds;
  if (d.eng_gran) return OK;
  const itts_config& c = cfg;
  for (int l = 0; l < c.layers; ++l) {
    const GptLayerW& L = gpt.layers[l];
    ITTS_REQUIRE(L.attn.N == 3 * ENG_D && L.attn.Cin == ENG_D && L.proj.N == ENG_D && L.proj.Cin == ENG_D &&
                     L.fc.N == 4 * ENG_D && L.fc.Cin == ENG_D && L.proj2.N == ENG_D && L.proj2.Cin == 4 * ENG_D,
                 "decode engine: projection shapes");
  }
  const size_t gb = eng_gran_count(c.layers) * 8;
  ITTS_TRY(dev_alloc((void**)&d.eng_gran, gb));
  ITTS_TRY(dev_alloc((void**)&d.eng_ctr, 64));
  const unsigned ctr0[16] = {1u, 0u};
  ITTS_HIP_CHECK(hipMemsetAsync(d.eng_gran, 0, gb, s));  // tag 0 is never issued
  ITTS_HIP_CHECK(hipMemcpyAsync(d.eng_ctr, ctr0, 64, hipMemcpyHostToDevice, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));  // ctr0 is a host stack buffer
  return OK;
}

int Engine::ensure_decode_state(int B, int Smax, int max_gen, hipStream_t s) {
  const itts_config& c = cfg;
  const int D = c.model_dim, H = c.heads, dh = D / H, V = c.number_mel_codes;
  DecodeState& d = ds;
  if (rows_on_mfma(B)) ITTS_TRY(ensure_decode_tiles(s));
  // the cache type of this generation, latched here (by the prefill): the engine's own, or e4m3 bytes when a 16-bit engine opted
  // in - ITTS_KV_FP8 (read per prefill: tests flip it inside one process) overrides the setter in both directions; fp32 engines
  // ignore both
  int ct = adt;
  if (adt == BF16) {
    const char* ev = getenv("ITTS_KV_FP8");
    if (ev ? atoi(ev) != 0 : d.kv_fp8 != 0) ct = FP8;
  }
  const size_t ces = dtype_size(ct);
  const size_t need = (size_t)c.layers * B * H * Smax * dh * ces;
  const bool regrow = B > d.cap_B || max_gen > d.cap_gen;
  // bytes left by the other type are not values of this one: bf16 halves read as e4m3 hold NaN encodings (0x7F / 0xFF), e4m3
  // bytes read as 16-bit pairs hold Inf / NaN - and rows past the sequence end have to be finite (below)
  const bool retype = d.cache_bytes && d.ct_held != ct;
  if (need > d.cache_bytes || regrow || B != d.B || Smax != d.Smax || retype) {
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
    d.drop_graphs();
  }
  d.ct = ct;
  d.ces = ces;
  d.ct_held = ct;
  if (need <= d.cache_bytes && retype) {  // the whole allocation, not just this request's share
    ITTS_HIP_CHECK(hipMemsetAsync(d.kc, 0, d.cache_bytes, s));
    ITTS_HIP_CHECK(hipMemsetAsync(d.vc, 0, d.cache_bytes, s));
  }
  if (need > d.cache_bytes) {
    ITTS_TRY(dev_alloc(&d.kc, need));
    ITTS_TRY(dev_alloc(&d.vc, need));
    // zero-filled once: the decode attention multiplies rows past the sequence end by p = 0 instead of selecting them
    // away, so whatever such a row holds has to be finite
    ITTS_HIP_CHECK(hipMemsetAsync(d.kc, 0, need, s));
    ITTS_HIP_CHECK(hipMemsetAsync(d.vc, 0, need, s));
    d.cache_bytes = need;
  }
  if (regrow) {
    // rows rounded up to 16: the batched decode keeps its bf16 activations in 16-row MFMA tiles
    const int cb = (std::max(B, d.cap_B) + 15) / 16 * 16, cg = std::max(max_gen, d.cap_gen);
    ITTS_TRY(dev_alloc((void**)&d.h, (size_t)cb * D * 4));
    ITTS_TRY(dev_alloc((void**)&d.qkv, (size_t)cb * 3 * D * 4));
    ITTS_TRY(dev_alloc((void**)&d.ctx, (size_t)cb * D * 4));
    ITTS_TRY(dev_alloc((void**)&d.act, (size_t)cb * 4 * D * 4));
    ITTS_TRY(dev_alloc((void**)&d.hn, (size_t)cb * D * 4));
    ITTS_TRY(dev_alloc((void**)&d.partial, (size_t)8 * cb * D * 4));
    ITTS_TRY(dev_alloc((void**)&d.attn_o, (size_t)cb * D * ATTN_NSPLIT * 4));
    ITTS_TRY(dev_alloc((void**)&d.attn_ml, (size_t)cb * H * 2 * ATTN_NSPLIT * 4));
    ITTS_TRY(dev_alloc((void**)&d.logits, (size_t)cb * V * 4));
    ITTS_TRY(dev_alloc((void**)&d.scores2, (size_t)cb * V * 4));
    ITTS_TRY(dev_alloc((void**)&d.kv_start, (size_t)cb * 4));
    ITTS_TRY(dev_alloc((void**)&d.cur_tok, (size_t)cb * 4));
    ITTS_TRY(dev_alloc((void**)&d.unfinished, (size_t)cb * 4));
    ITTS_TRY(dev_alloc((void**)&d.ids, (size_t)cb * cg * 4));
    ITTS_TRY(dev_alloc((void**)&d.forced, (size_t)cb * cg * 4));
    {
      const size_t gb = (size_t)c.layers * 4 * 3 * D * 8;
      ITTS_TRY(dev_alloc((void**)&d.gran, gb));
      ITTS_HIP_CHECK(hipMemsetAsync(d.gran, 0, gb, s));  // tag 0 is never issued
      ITTS_TRY(dev_alloc((void**)&d.fuse_err, 64));
      ITTS_HIP_CHECK(hipMemsetAsync(d.fuse_err, 0, 64, s));
    }
    ITTS_TRY(dev_alloc((void**)&d.seen, (size_t)cb * V));
    ITTS_TRY(dev_alloc((void**)&d.len, (size_t)cb * 4));
    if (!d.prefix_dev) ITTS_TRY(dev_alloc((void**)&d.prefix_dev, 64));
    d.cap_B = cb;
    d.cap_gen = cg;
  }
  d.B = d.Bcache = d.B0 = B;  // a fresh generation: nothing retired
  d.orig.clear();
  d.retired.clear();
  d.ret_codes.clear();
  d.ret_logits.clear();
  d.admitted = 0;
  d.adm_rows.clear();
  d.adm_uniforms.clear();
  d.Smax = Smax;
  d.max_gen = max_gen;
  return OK;
}

int Engine::ensure_beam_state(int rows, int max_gen, int Smax, hipStream_t s) {
  DecodeState& d = ds;
  if (rows <= d.beam_rows && max_gen <= d.beam_gen && Smax <= d.beam_smax && d.beam_ids) return OK;
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  d.drop_graphs();  // captured nodes hold the old pointers
  const int r = std::max(rows, d.beam_rows), g = std::max(max_gen, d.beam_gen), sm = std::max(Smax, d.beam_smax);
  ITTS_TRY(dev_alloc((void**)&d.beam_ids, (size_t)2 * r * g * 4));
  ITTS_TRY(dev_alloc((void**)&d.anc, (size_t)2 * r * sm));
  ITTS_TRY(dev_alloc((void**)&d.beam_scores, (size_t)r * 4));
  ITTS_TRY(dev_alloc((void**)&d.cand_sc, (size_t)r * BEAM_MAX_CAND * 4));
  ITTS_TRY(dev_alloc((void**)&d.cand_tok, (size_t)r * BEAM_MAX_CAND * 4));
  ITTS_TRY(dev_alloc((void**)&d.cand_n, (size_t)r * 4));
  ITTS_TRY(dev_alloc((void**)&d.hyp_tok, (size_t)r * 2 * g * 4));  // [B][nb + 1][g] <= rows * 2 * g
  ITTS_TRY(dev_alloc((void**)&d.hyp_score, (size_t)r * 2 * 4));
  ITTS_TRY(dev_alloc((void**)&d.hyp_len, (size_t)r * 2 * 4));
  ITTS_TRY(dev_alloc((void**)&d.hyp_order, (size_t)r * 2 * 4));
  ITTS_TRY(dev_alloc((void**)&d.hyp_n, (size_t)r * 4));
  ITTS_TRY(dev_alloc((void**)&d.hyp_worst, (size_t)r * 4));
  ITTS_TRY(dev_alloc((void**)&d.hyp_counter, (size_t)r * 4));
  ITTS_TRY(dev_alloc((void**)&d.beam_done, (size_t)r * 4));
  d.beam_rows = r;
  d.beam_gen = g;
  d.beam_smax = sm;
  return OK;
}

// scratch of the whole-vocabulary beam sampler (beam_wide_cand_kernel / beam_wide_pick_kernel): scores [rows][V], kept [rows], the
// picks [items][2 * nb] x 3.  Allocated with the decode state at prefill, never inside a captured step
int Engine::ensure_beam_wide_state(int rows, int nb, int V, hipStream_t s) {
  DecodeState& d = ds;
  const size_t need = beam_wide_bytes(rows, nb, V);
  if (need > d.wide_cap) {
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
    d.drop_graphs();  // captured nodes hold the old pointers
    ITTS_TRY(dev_alloc(&d.wide_buf, need));
    d.wide_cap = need;
  }
  BeamWide w;
  w.sc = (float*)d.wide_buf;
  w.kept = (int*)(w.sc + (size_t)rows * V);
  w.pick_sc = (float*)(w.kept + rows);
  w.pick_tok = (int*)(w.pick_sc + (size_t)(rows / nb) * 2 * nb);
  w.pick_beam = w.pick_tok + (size_t)(rows / nb) * 2 * nb;
  if (w.sc != d.wide.sc || w.kept != d.wide.kept || w.pick_sc != d.wide.pick_sc) {  // another carving: the nodes hold the old one
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
    d.drop_graphs();
  }
  d.wide = w;
  return OK;
}

// HF beam_sample configuration for the following generations (num_beams <= 1 switches it off): the generate() mode of
// the reference's default kwargs (infer.py:116-124).  uniforms_host: row-major [max_gen][B][2 * num_beams] draws in [0, 1).
// generate()'s num_return_sequences under beams: the n best hypotheses of every batch item (1 <= n <= num_beams, checked
// against the beam count when the generation starts)
int Engine::gpt_set_beam_returns(int n) {
  ITTS_REQUIRE(n >= 1 && n <= 10, "gpt_set_beam_returns: num_return_sequences must be in [1, 10]");
  beam_returns = n;
  return OK;
}

int Engine::gpt_set_beam_sample(int num_beams, int top_k, float top_p, float temperature, const float* uniforms_host, long n) {
  return gpt_set_beams(num_beams, 1, top_k, top_p, temperature, 0.f, uniforms_host, n);
}

// do_sample = 1: beam_sample as above; do_sample = 0: HF beam_search (deterministic: per step the 2 * num_beams best of
// log_softmax + repetition penalty + running beam score, no warpers, no uniforms).  length_penalty as BeamHypotheses
// uses it (score = sum_logprobs / generated_len ** length_penalty; the reference passes 0.0).
int Engine::gpt_set_beams(int num_beams, int do_sample, int top_k, float top_p, float temperature, float length_penalty,
                          const float* uniforms_host, long n) {
  if (num_beams <= 1) {
    beam_beams = 1;
    if (!ds.do_sample) sample_uniforms.clear();
    return OK;
  }
  ITTS_REQUIRE(num_beams <= 10, "gpt_set_beams: num_beams must be in [2, 10]");
  if (do_sample && !ds.host_sample) {  // (host sampling: the caller warps and draws itself, any top_k - gpt_commit_beams)
    // any top_k: < 1 is HF's "TopK warper off" (stored as 0); 0 and > 128 run on the whole-vocabulary pair (beam_sample_step)
    ITTS_REQUIRE(top_k <= BEAM_MAX_CAND || cfg.number_mel_codes <= BEAM_WIDE_MAX_V,
                 "gpt_set_beams: top_k > 128 needs number_mel_codes <= 16384");
    ITTS_REQUIRE(top_p > 0.f && top_p <= 1.f && temperature > 0.f, "gpt_set_beams: need 0 < top_p <= 1 and temperature > 0");
    ITTS_REQUIRE(uniforms_host && n > 0, "gpt_set_beams: uniforms missing");
    sample_uniforms.assign(uniforms_host, uniforms_host + n);
  }
  beam_beams = num_beams;
  beam_do_sample = do_sample ? 1 : 0;
  beam_length_penalty = length_penalty;
  ds.do_sample = 0;
  ds.top_k = (do_sample && !ds.host_sample && top_k < 1) ? 0 : top_k;
  ds.top_p = top_p;
  ds.temperature = temperature;
  return OK;
}

// BeamSearchScorer.finalize (beam_search.py, 4.36.2) on the host: open beams of unfinished batch items join their
// hypotheses with the running scores, the beam_returns best hypotheses (num_beam_hyps_to_keep = generate()'s
// num_return_sequences, model.py:655,698-703; highest score first, the later one on ties) are returned per batch item as
// codes [B * beam_returns][max_gen] padded with the stop token (eos = pad = stop_mel_token, model.py:698-700).
int Engine::beam_finalize(int32_t* codes, hipStream_t s) {
  BeamHost st;
  ITTS_TRY(beam_read_state(st, s));
  for (int b = 0; b < ds.B / ds.nb; ++b) ITTS_TRY(beam_finalize_item(st, b, codes + (size_t)b * beam_returns * ds.max_gen));
  return OK;
}

// the scorer's state of the running rows: done flags, running scores, the hypothesis store and the live half of the beam ids
int Engine::beam_read_state(BeamHost& st, hipStream_t s) {
  DecodeState& d = ds;
  const int nb = d.nb, rows = d.B, B = rows / nb, mg = d.max_gen;
  std::vector<int>& len = st.len;
  len.resize(rows);
  st.done.resize(B);
  st.hlen.resize((size_t)B * (nb + 1));
  st.hord.resize((size_t)B * (nb + 1));
  st.bscore.resize(rows);
  st.hscore.resize((size_t)B * (nb + 1));
  ITTS_HIP_CHECK(hipMemcpyAsync(len.data(), d.len, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(st.done.data(), d.beam_done, (size_t)B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(st.bscore.data(), d.beam_scores, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(st.hscore.data(), d.hyp_score, st.hscore.size() * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(st.hlen.data(), d.hyp_len, st.hlen.size() * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(st.hord.data(), d.hyp_order, st.hord.size() * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  const int k = st.k = len[0];
  // admitted groups (admit_beam_groups) started later: every item then has its own step and its own live half - both are read
  st.both = d.admitted > 0;
  st.ids.resize((size_t)(st.both ? 2 : 1) * rows * mg);
  st.htok.resize((size_t)B * (nb + 1) * mg);
  ITTS_HIP_CHECK(hipMemcpyAsync(st.ids.data(), d.beam_ids + (st.both ? 0 : (size_t)(k & 1) * rows * mg), st.ids.size() * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(st.htok.data(), d.hyp_tok, st.htok.size() * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  return OK;
}

// BeamSearchScorer.finalize for batch item b of the state st -> codes [beam_returns][max_gen].  A done item is read from its
// hypothesis store alone: its result is final from the step at which it became done
int Engine::beam_finalize_item(const BeamHost& st, int b, int32_t* codes) const {
  const DecodeState& d = ds;
  const int nb = d.nb, mg = d.max_gen;
  const int k = st.both ? std::min(std::max(st.len[(size_t)b * nb], 0), mg) : st.k;  // the item's own step: parity and lpdiv
  const int32_t* ids = st.ids.data() + (st.both ? (size_t)(k & 1) * st.len.size() * mg : 0);
  struct Hyp {
    float score;
    int order, len;
    const int32_t* tok;
  };
  std::vector<Hyp> hy;
  for (int q = 0; q <= nb; ++q) {
    const size_t i = (size_t)b * (nb + 1) + q;
    if (st.hord[i] >= 0) hy.push_back({st.hscore[i], st.hord[i], st.hlen[i], st.htok.data() + i * mg});
  }
  if (!st.done[b]) {
    // beam_hyp.add(final_tokens, final_score, generated_len) for every open beam, with BeamHypotheses.add's eviction
    std::sort(hy.begin(), hy.end(), [](const Hyp& x, const Hyp& y) { return x.order < y.order; });
    float worst = 1e9f;
    for (const Hyp& h : hy) worst = std::min(worst, h.score);
    int counter = 1 << 20;
    const float lpdiv = d.length_penalty == 0.f ? 1.f : std::pow((float)(k - d.input_n), d.length_penalty);  // generated_len = k - given tokens
    for (int q = 0; q < nb; ++q) {
      const int row = b * nb + q;
      const float score = st.bscore[row] / lpdiv;
      if ((int)hy.size() < nb || score > worst) {
        hy.push_back({score, counter++, k, ids + (size_t)row * mg});
        if ((int)hy.size() > nb) {
          size_t lo = 0;
          for (size_t i = 1; i < hy.size(); ++i)
            if (hy[i].score < hy[lo].score || (hy[i].score == hy[lo].score && hy[i].order < hy[lo].order)) lo = i;
          hy.erase(hy.begin() + lo);
          worst = 1e9f;
          for (const Hyp& h : hy) worst = std::min(worst, h.score);
        } else {
          worst = std::min(worst, score);
        }
      }
    }
  }
  const int keep = beam_returns;
  ITTS_REQUIRE((int)hy.size() >= keep, "beam_finalize: fewer hypotheses than num_return_sequences for a batch item");
  for (int r = 0; r < keep; ++r) {
    size_t best = 0;  // sorted(key=score).pop(): highest score, the later insertion on ties
    for (size_t i = 1; i < hy.size(); ++i)
      if (hy[i].score > hy[best].score || (hy[i].score == hy[best].score && hy[i].order > hy[best].order)) best = i;
    int32_t* out = codes + (size_t)r * mg;
    for (int i = 0; i < mg; ++i) out[i] = i < hy[best].len ? hy[best].tok[i] : cfg.stop_mel_token;
    hy.erase(hy.begin() + best);
  }
  return OK;
}

int Engine::gpt_prefill(const float* cond_dev, const int32_t* text_ids_in, int B_items, int L, int max_gen, float penalty,
                        int suppress, hipStream_t s) {
  // beam-sample: every batch item becomes nb rows (HF _expand_inputs_for_generation: repeat_interleave)
  const int nbeam = beam_beams > 1 ? beam_beams : 1;
  const int B = B_items * nbeam;
  std::vector<int32_t> text_exp;
  const int32_t* text_ids = text_ids_in;
  if (nbeam > 1 && text_ids_in && B_items > 0 && L > 0) {
    text_exp.resize((size_t)B * L);
    for (int b = 0; b < B; ++b) std::memcpy(text_exp.data() + (size_t)b * L, text_ids_in + (size_t)(b / nbeam) * L, (size_t)L * 4);
    text_ids = text_exp.data();
  }
  if (!finalized || !gpt.ok) {
    set_error("gpt_prefill: GPT weights not bound");
    return E_STATE;
  }
  const itts_config& c = cfg;
  ITTS_REQUIRE(cond_dev && text_ids && B > 0 && L > 0 && max_gen > 0, "gpt_prefill: bad arguments");
  ITTS_REQUIRE(B <= c.max_batch, "gpt_prefill: batch larger than max_batch");
  ITTS_REQUIRE(L + 2 <= c.max_text_tokens + 2, "gpt_prefill: text longer than max_text_tokens");
  ITTS_REQUIRE(max_gen + 2 <= c.max_mel_tokens + 3, "gpt_prefill: max_gen exceeds the mel position table");
  const int D = c.model_dim, nl = c.cond_latents, V = c.number_mel_codes;
  const int sp = nl + L + 2;  // prefix length s (model.py:614)
  const int S0 = sp + 1;      // + start_mel_token
  const int Smax = (S0 + max_gen + 255) / 256 * 256;  // coarse, so one captured graph serves many L
  ITTS_REQUIRE(Smax <= 2048, "gpt_prefill: sequence too long for the decode attention kernel");
  ITTS_REQUIRE(max_gen < 4095, "gpt_prefill: max_gen must stay below 4095 (12-bit step field of the fused hand-off tags)");
  // per-row settings (gpt_set_sampling_rows): single-beam device modes only, and for exactly this batch
  if (!row_table.empty()) {
    ITTS_REQUIRE((int)row_table.size() == B_items, "gpt_prefill: the per-row sampling table was set for another batch size");
    ITTS_REQUIRE(nbeam == 1, "gpt_prefill: per-row sampling settings do not run under beams");
    ITTS_REQUIRE(!(ds.typical_mass > 0.f), "gpt_prefill: per-row sampling settings do not run with typical filtering");
    ITTS_REQUIRE(!ds.host_sample, "gpt_prefill: per-row sampling settings do not run with host sampling");
    penalty = row_table[0].penalty;  // a uniform table: the scalar path with its values; else every row reads its own
  }
  ITTS_TRY(ensure_decode_state(B, Smax, max_gen, s));
  ds.rows_active = !row_table.empty() && (!row_table_uniform || row_table_keep);  // (kept: a generation that will admit other settings)
  ds.rows_classes = 0;
  ds.prefix = sp;
  ds.penalty = penalty;
  ds.suppress_stop = suppress;
  gen_epoch = (gen_epoch % 0xFFFFF) + 1;  // 1 .. 2^20 - 1
  ds.nb = nbeam;
  ds.beam_sample = beam_do_sample;
  ds.length_penalty = beam_length_penalty;
  if (nbeam > 1) {
    ITTS_REQUIRE(forced_n == 0 || forced_input, "gpt_prefill: teacher forcing (gpt_set_forced) is not supported together with beams; `input_tokens` is");
    for (size_t i = 0; i < forced_host.size() && forced_n > 0; ++i)
      ITTS_REQUIRE(forced_host[i] >= 0, "gpt_prefill: `input_tokens` under beams must not hold free (-1) entries");
    ITTS_REQUIRE(beam_returns <= nbeam, "`num_return_sequences` has to be smaller or equal to `num_beams`.");
    ITTS_TRY(ensure_beam_state(B, max_gen, Smax, s));
    const long n_init = std::max<long>(2L * B * Smax, 64);
    hipLaunchKernelGGL(beam_init_kernel, dim3((unsigned)((n_init + 255) / 256)), dim3(256), 0, s, ds.anc, ds.beam_scores,
                       ds.hyp_order, ds.hyp_n, ds.hyp_worst, ds.hyp_counter, ds.beam_done, B, nbeam, Smax, beam_do_sample);
    ITTS_HIP_CHECK(hipGetLastError());
  }
  if (engine_usable()) ITTS_TRY(ensure_engine_state(s));  // allocations must not happen inside the graph capture of the step
  if (ds.do_sample && nbeam == 1 && (ds.top_k < 1 || ds.top_k > BEAM_MAX_CAND)) ITTS_TRY(sampler_wide_prepare());  // nor this
  if (ds.rows_active) {
    ITTS_TRY(upload_row_table(s));  // (may allocate)
    if (ds.rows_classes >> ROWCLS_NARROW & 1)
      ITTS_REQUIRE((size_t)V * 4 <= 60 * 1024, "gpt_prefill: a row with 1 <= top_k <= 128 needs number_mel_codes <= 15360");
    if (ds.rows_classes >> ROWCLS_WIDE & 1) {
      ITTS_REQUIRE(V <= 16384, "gpt_prefill: a sampled row with top_k outside [1, 128] needs number_mel_codes <= 16384");
      ITTS_TRY(sampler_wide_prepare());
    }
  }
  const bool rows_sample = ds.rows_active && (ds.rows_classes & ~(1 << ROWCLS_GREEDY));
  ds.wide_valid = 0;
  if (nbeam > 1 && beam_do_sample && !ds.host_sample && (ds.top_k < 1 || ds.top_k > BEAM_MAX_CAND)) {  // nor these two
    ITTS_REQUIRE(cfg.number_mel_codes <= BEAM_WIDE_MAX_V, "gpt_prefill: beam_sample with top_k outside [1, 128] needs number_mel_codes <= 16384");
    ITTS_TRY(beam_wide_prepare());
    ITTS_TRY(ensure_beam_wide_state(B, nbeam, cfg.number_mel_codes, s));
    ds.wide_valid = 1;  // this generation's steps leave their picks in ds.wide (gpt_beam_picks)
  }
  // a kept table whose rows are all greedy: room for the draws of sampled rows it may admit (gpt_admit_rows fills their columns)
  const bool keep_u = ds.rows_active && row_table_keep && !ds.do_sample && !rows_sample;
  ds.have_uniforms = 0;
  if (ds.do_sample || rows_sample || (nbeam > 1 && beam_do_sample && !ds.host_sample) || keep_u) {
    const size_t need_u = nbeam > 1 ? (size_t)max_gen * B_items * 2 * nbeam : (size_t)max_gen * B;
    ITTS_REQUIRE(keep_u || sample_uniforms.size() >= need_u,
                 "gpt_prefill: sampling enabled but fewer uniforms than max_gen * B (* 2 * num_beams) were supplied");
    if (need_u > ds.uniforms_cap) {
      ITTS_HIP_CHECK(hipStreamSynchronize(s));
      ds.drop_graphs();  // the captured samplers hold the old pointer
      ITTS_TRY(dev_alloc((void**)&ds.uniforms, need_u * 4));
      ds.uniforms_cap = need_u;
    }
    if (keep_u)
      ITTS_HIP_CHECK(hipMemsetAsync(ds.uniforms, 0, need_u * 4, s));
    else
      ITTS_HIP_CHECK(hipMemcpyAsync(ds.uniforms, sample_uniforms.data(), need_u * 4, hipMemcpyHostToDevice, s));
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
    ds.have_uniforms = nbeam == 1;
  }
  ds.use_forced = forced_n > 0;
  ds.input_n = forced_input ? forced_n : 0;
  if (ds.host_sample) {
    ITTS_REQUIRE(forced_n == 0 && !ds.do_sample, "gpt_prefill: host sampling excludes forced tokens and the device sampler");
    if (nbeam == 1) ITTS_HIP_CHECK(hipMemsetAsync(ds.forced, 0xFF, (size_t)B * max_gen * 4, s));  // -1: nothing forced yet
  }
  if (ds.use_forced) {
    ITTS_REQUIRE(forced_B == B_items || forced_B == 1, "gpt_prefill: forced tokens were set for a different batch size");
    ITTS_REQUIRE(forced_n <= max_gen, "gpt_prefill: more forced tokens than max_gen");
    std::vector<int32_t> tab((size_t)B * max_gen, -1);
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < forced_n; ++k) tab[(size_t)b * max_gen + k] = forced_host[(size_t)(forced_B == 1 ? 0 : b / nbeam) * forced_n + k];
    ITTS_HIP_CHECK(hipMemcpyAsync(ds.forced, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
  }
  // host: row descriptors (prepare_gpt_inputs, model.py:615-639)
  std::vector<RowDesc> rd((size_t)B * S0);
  std::vector<int> kvs(B);
  for (int b = 0; b < B; ++b) {
    std::vector<int> ids;
    for (int i = 0; i < L; ++i) {
      const int t = text_ids[(size_t)b * L + i];
      if (t != c.start_text_token && t != c.stop_text_token) {
        ITTS_REQUIRE(t >= 0 && t <= c.number_text_tokens, "gpt_prefill: text id out of range");
        ids.push_back(t);
      }
    }
    const int n = (int)ids.size();
    const int pad = L - n;
    kvs[b] = pad;
    RowDesc* r = rd.data() + (size_t)b * S0;
    int k = 0;
    for (int i = 0; i < pad; ++i) r[k++] = {0, 0, 0, 0};
    // conditioning latents: one set for every row (infer.py), or one per batch item (model.py:599-602 takes [b, 32, D])
    for (int i = 0; i < nl; ++i) r[k++] = {1, (cond_per_row ? (b / nbeam) * nl : 0) + i, 0, 0};
    r[k++] = {2, c.start_text_token, 0, 0};
    for (int i = 0; i < n; ++i) r[k++] = {2, ids[i], i + 1, 0};
    r[k++] = {2, c.stop_text_token, n + 1, 0};
    r[k++] = {3, c.start_mel_token, 0, 0};
  }
  auto body = [&]() -> int {
    RowDesc* rd_dev = (RowDesc*)alloc(rd.size() * sizeof(RowDesc));
    float* h = (float*)alloc((size_t)B * S0 * D * 4);
    if (!dry) {
      ITTS_HIP_CHECK(hipMemcpyAsync(rd_dev, rd.data(), rd.size() * sizeof(RowDesc), hipMemcpyHostToDevice, s));
      ITTS_HIP_CHECK(hipMemcpyAsync(ds.kv_start, kvs.data(), B * 4, hipMemcpyHostToDevice, s));
      const long n = (long)B * V;
      hipLaunchKernelGGL(init_decode_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ds.seen,
                         ds.unfinished, ds.cur_tok, ds.len, ds.prefix_dev, B, V, 1, c.start_mel_token, sp, gen_epoch);
      if (adt == F32)
        hipLaunchKernelGGL(gpt_embed_rows_kernel<float>, dim3(B * S0), dim3(256), 0, s, h, rd_dev, cond_dev,
                           (const float*)gpt.text_emb, (const float*)gpt.text_pos, (const float*)gpt.mel_emb,
                           (const float*)gpt.mel_pos, D);
      else
        hipLaunchKernelGGL(gpt_embed_rows_kernel<bf16_t>, dim3(B * S0), dim3(256), 0, s, h, rd_dev, cond_dev,
                           (const bf16_t*)gpt.text_emb, (const bf16_t*)gpt.text_pos, (const bf16_t*)gpt.mel_emb,
                           (const bf16_t*)gpt.mel_pos, D);
      ITTS_HIP_CHECK(hipGetLastError());
    }
    ITTS_TRY(tap("prefix_emb", h, F32, (int64_t)B * S0 * D, s));
    ITTS_TRY(gpt_layers_full(h, B, S0, ds.kv_start, true, s));
    // logits of the last position only (generate takes logits[:, -1, :])
    K(copy_rows(ds.h, D, h + (size_t)(S0 - 1) * D, S0 * D, B, D, F32, s));
    if (!dry) ITTS_TRY(head_and_sample(s));
    return OK;
  };
  ITTS_TRY(two_pass(body, s));
  // rd/kvs are host stack buffers read by async copies
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  ds.active = true;
  return OK;
}

// ln_f -> final_norm -> mel_head -> repetition penalty / argmax / bookkeeping (lm_head, model.py:48,180)
int Engine::head_and_sample(hipStream_t s, bool have_logits, bool sampled) {
  if (have_logits) return sample_from_logits(s, sampled);  // the persistent engine ran ln_f / final_norm / mel_head itself
  ITTS_TRY(head_rows(ds.h, ds.hn, ds.logits, ds.B, s));
  return sample_from_logits(s);
}

// the head of B rows: h [B][D] fp32 -> logits [B][V]; hn: [ceil(B / 16) * 16][D] floats of scratch (the decode step's own buffers,
// or those of a row admission)
int Engine::head_rows(float* h, float* hn, float* logits, int B, hipStream_t s) {
  const itts_config& c = cfg;
  const int D = c.model_dim, V = c.number_mel_codes;
  GemvArgs g;
  g.W = gpt.head.w;
  g.Y = logits;
  g.bias = gpt.head.b;
  g.B = B;
  g.N = V;
  g.K = D;
  g.ldy = V;
  g.X = h;
  g.prologue = 2;
  g.ln_gamma = gpt.ln_f.g;
  g.ln_beta = gpt.ln_f.b;
  g.ln2_gamma = nullptr;  // final_norm's affine is folded into mel_head by the packer
  g.ln2_beta = nullptr;
  if (rows_on_mfma(B)) {
    // batched decode: ln_f -> final_norm as a row kernel (bf16), head on the matrix cores
    ITTS_TRY(ln_rows_bf16(hn, h, gpt.ln_f.g, gpt.ln_f.b, B, D, 1e-5f, 2, ds.partial, ds.pend_split, ds.pend_bias, 1, s));
    ds.pend_split = 0;
    g.X = hn;
    g.x_bf16 = 1;
    g.x_tiled = 1;
    g.prologue = 0;
    g.W8 = gpt.head.w8;
    g.wscale = gpt.head.wscale;
    g.Wt = gpt.head.wt;
    g.W8t = gpt.head.wt8;
    ITTS_TRY(skinny_mfma(g, s));
  } else if (adt == BF16 && gemv_bf16_supported(g)) {
    g.W8 = gpt.head.w8;
    g.wscale = gpt.head.wscale;
    ITTS_TRY(gemv_bf16(g, s));
  } else if (gemv2_supported(g) && !(adt == BF16 && D <= 2048)) {
    ITTS_TRY(gemv2(g, gpt.head.dt, s));
  } else {
    // (also the bf16 engine at a width the bf16 GEMV refuses: gemv2 hands the elements of its LayerNorm rows to the threads by
    // their position in the batch, so identical rows would differ in the last ulp; these two kernels treat every row alike)
    ITTS_TRY(double_ln(hn, h, gpt.ln_f.g, gpt.ln_f.b, nullptr, nullptr, B, D, 1e-5f, s));
    g.X = hn;
    g.prologue = 0;
    ITTS_TRY(gemv(g, gpt.head.dt, s));
  }
  return OK;
}

// arguments of the beam kernels (beam_sample_step / beam_commit_step) from the decode state
BeamArgs Engine::beam_args(const float* lg_in, bool typical) const {
  const itts_config& c = cfg;
  const int D = c.model_dim, V = c.number_mel_codes, B = ds.B;
  BeamArgs ba;
  ba.logits = lg_in;
  ba.preprocessed = typical;
  ba.do_sample = ds.beam_sample;
  ba.length_penalty = ds.length_penalty;
  ba.cand_sc = ds.cand_sc;
  ba.cand_tok = ds.cand_tok;
  ba.cand_n = ds.cand_n;
  ba.V = V;
  ba.max_gen = ds.max_gen;
  ba.stop = c.stop_mel_token;
  ba.suppress_stop = ds.suppress_stop;
  ba.nb = ds.nb;
  ba.B = B / ds.nb;
  ba.top_k = ds.top_k;
  ba.top_p = ds.top_p;
  ba.temperature = ds.temperature;
  ba.penalty = ds.penalty;
  ba.start_tok = c.start_mel_token;
  ba.fake_id = 1;  // prepare_gpt_inputs: fake ids are all 1 with last = start_mel_token (model.py:644-653)
  ba.Smax = ds.Smax;
  ba.uniforms = ds.uniforms;
  ba.len = ds.len;
  ba.cur_tok = ds.cur_tok;
  ba.unfinished = ds.unfinished;
  ba.ids = ds.beam_ids;
  ba.anc = ds.anc;
  ba.prefix_dev = ds.prefix_dev;
  ba.beam_scores = ds.beam_scores;
  ba.hyp_tok = ds.hyp_tok;
  ba.hyp_score = ds.hyp_score;
  ba.hyp_len = ds.hyp_len;
  ba.hyp_order = ds.hyp_order;
  ba.hyp_n = ds.hyp_n;
  ba.hyp_worst = ds.hyp_worst;
  ba.hyp_counter = ds.hyp_counter;
  ba.done = ds.beam_done;
  ba.h_next = ds.h;
  ba.emb = gpt.mel_emb;
  ba.pos = gpt.mel_pos;
  ba.D = D;
  ba.pos_rows = c.max_mel_tokens + 3;
  ba.emb_bf16 = adt == BF16;
  ba.forced = ds.use_forced ? ds.forced : nullptr;
  ba.input_n = ds.use_forced ? ds.input_n : 0;
  return ba;
}

// repetition penalty / argmax or the sampling / beam modes / bookkeeping on ds.logits [B][V]
int Engine::sample_from_logits(hipStream_t s, bool sampled) {
  const itts_config& c = cfg;
  const int V = c.number_mel_codes, B = ds.B;
  ITTS_TRY(tap("logits0", ds.logits, F32, (int64_t)B * V, s));
  if (sampled) return OK;  // the persistent engine's in-launch greedy sampler committed this step's tokens
  if (ds.host_sample) return OK;  // the caller reads the logits, picks the tokens and commits them (gpt_commit)
  const float* lg_in = ds.logits;
  // (a logits PROCESSOR in the reference, model.py:690-697: greedy search and beam search run it too, not only the sampling modes)
  const bool typical = ds.typical_mass > 0.f;
  if (typical) {  // TypicalLogitsWarper sits in HF's logits_processor list, right after the repetition penalty
    TypicalArgs ta;
    ta.logits = ds.logits;
    ta.out = ds.scores2;
    ta.V = V;
    ta.stop = c.stop_mel_token;
    ta.suppress_stop = ds.suppress_stop;
    ta.penalty = ds.penalty;
    ta.mass = ds.typical_mass;
    ta.min_keep = ds.nb > 1 ? 2 : 1;  // model.py:693-694
    ta.log_softmax_first = ds.nb > 1;  // beam_sample processes log-probs, sample() raw logits
    if (ds.nb > 1) {
      ta.beam_ids = ds.beam_ids;
      ta.len = ds.len;
      ta.max_gen = ds.max_gen;
      ta.start_tok = c.start_mel_token;
      ta.fake_id = 1;
    } else {
      ta.seen = ds.seen;
    }
    ITTS_TRY(typical_filter(ta, B, s));
    ITTS_TRY(tap("typical0", ds.scores2, F32, (int64_t)B * V, s));
    lg_in = ds.scores2;
  }
  if (ds.nb > 1) {  // beam-sample: one workgroup per batch item over its nb rows
    const BeamArgs ba = beam_args(lg_in, typical);
    const bool wide = ba.do_sample && (ba.top_k < 1 || ba.top_k > BEAM_MAX_CAND);
    return beam_sample_step(ba, s, wide ? &ds.wide : nullptr);
  }
  SamplerArgs sa = greedy_sampler_args(lg_in, typical);
  if (ds.rows_active) {  // a mixed batch: one launch per class present, every row in its own class's kernel
    sa.rows = ds.rows;
    return sampler_rows_step(sa, B, ds.rows_classes, s);
  }
  return sampler2_step(sa, B, s);
}

// arguments of the greedy / sampling kernels (sampler2_step) - also what the persistent engine's in-launch sampler runs on
SamplerArgs Engine::greedy_sampler_args(const float* lg_in, bool typical) const {
  const itts_config& c = cfg;
  const int D = c.model_dim, V = c.number_mel_codes, B = ds.B;
  SamplerArgs sa;
  sa.logits = lg_in;
  sa.preprocessed = typical;
  sa.seen = ds.seen;
  sa.ids = ds.ids;
  sa.cur_tok = ds.cur_tok;
  sa.unfinished = ds.unfinished;
  sa.step = ds.len;
  sa.V = V;
  sa.max_gen = ds.max_gen;
  sa.stop = c.stop_mel_token;
  sa.suppress_stop = ds.suppress_stop;
  sa.penalty = ds.penalty;
  sa.h_next = ds.h;  // the sampler also prepares the next step's input embedding
  sa.emb = gpt.mel_emb;
  sa.pos = gpt.mel_pos;
  sa.D = D;
  sa.pos_rows = c.max_mel_tokens + 3;
  sa.emb_bf16 = adt == BF16;
  sa.do_sample = ds.do_sample;
  sa.top_k = ds.top_k;
  sa.top_p = ds.top_p;
  sa.temperature = ds.temperature;
  sa.uniforms = ds.uniforms;
  sa.forced = ds.use_forced ? ds.forced : nullptr;
  sa.input_n = ds.use_forced ? ds.input_n : 0;
  sa.B = B;
  return sa;
}

// arguments of the persistent decode engine's launch (decode_engine_layers) from the decode state.  eng_first: the blocks
// [0, eng_first) run on the engine; fold_head / fold_samp: the head / the greedy sampler run inside the same launch
EngArgs Engine::engine_args(int& eng_first, bool& fold_head, bool& fold_samp) const {
  const itts_config& c = cfg;
  const int dh = c.model_dim / c.heads, B = ds.B;
  EngArgs ea;
  const bool w8 = gpt.layers[0].attn.w8 != nullptr;  // engine_usable(): then every projection and the head carry an fp8 copy
  ea.w8 = w8;
  for (int l = 0; l < c.layers; ++l) {
    const GptLayerW& L = gpt.layers[l];
    if (w8) {
      ea.L[l] = {(const bf16_t*)L.attn.w8, (const bf16_t*)L.proj.w8, (const bf16_t*)L.fc.w8, (const bf16_t*)L.proj2.w8,
                 L.attn.b, L.proj.b, L.fc.b, L.proj2.b};
      ea.S[l] = {L.attn.wscale, L.proj.wscale, L.fc.wscale, L.proj2.wscale};
    } else {
      ea.L[l] = {(const bf16_t*)L.attn.w, (const bf16_t*)L.proj.w, (const bf16_t*)L.fc.w, (const bf16_t*)L.proj2.w,
                 L.attn.b, L.proj.b, L.fc.b, L.proj2.b};
    }
  }
  ea.gran = ds.eng_gran;
  ea.h = ds.h;
  // engine_usable(): a 16-bit cache (ds.ces == 2), or - opted in - e4m3 bytes (ds.ces == 1, kv8); the kernel's per-layer offsets
  // count elements of the cache's type either way
  ea.kc = (bf16_t*)ds.kc;
  ea.vc = (bf16_t*)ds.vc;
  ea.kv8 = ds.ct == FP8;
  ea.len = ds.len;
  ea.kv_start = ds.kv_start;
  ea.prefix = ds.prefix_dev;
  ea.ctr = ds.eng_ctr;
  ea.anc = ds.nb > 1 ? ds.anc : nullptr;  // beam rows gather their keys through the ancestry table (no cache re-ordering)
  ea.nb = ds.nb;
  // ITTS_ENGINE_LAYERS=n (debugging aid): blocks [0, n) on the engine, the rest as launches
  static const int e_nl = getenv("ITTS_ENGINE_LAYERS") ? atoi(getenv("ITTS_ENGINE_LAYERS")) : -1;
  eng_first = e_nl >= 0 && e_nl < c.layers ? e_nl : c.layers;
  ea.NL = eng_first;
  ea.B = B;
  ea.Smax = ds.Smax;
  ea.scale = 1.f / std::sqrt((float)dh);
#ifdef ITTS_PROBES  // the probes library (make probes): the product kernels have no tap, stamp or divisor code to switch on
  static const int e_tap = getenv("ITTS_TAP_LAYER") ? atoi(getenv("ITTS_TAP_LAYER")) : -1;
  if (debug && e_tap >= 0 && e_tap < eng_first && !dry) {  // debugging aid: the engine's view of one block's edges
    ea.dbg = ds.act;  // [16][4D] fp32 scratch of the launch path, unused by the engine: room for the 9 B D floats of the dump
    ea.dbg_layer = e_tap;
  }
  static const int e_fake = getenv("ITTS_ENG_FAKE_DIV") ? atoi(getenv("ITTS_ENG_FAKE_DIV")) : 1;
  ea.fake_div = e_fake < 1 ? 1 : e_fake;
  static const bool e_stamps = getenv("ITTS_ENGINE_STAMPS") != nullptr;
  if (debug && e_stamps && !dry) ea.stamp = (unsigned*)ds.scores2;  // [16][V] fp32 scratch of the typical filter (off in this mode) >= 256 * 24 * 16 words
#endif
  // gather pacing (s_sleep units of 64 clocks): a publish needs ~0.4 us to become visible; earlier passes fail AND slow the
  // stores down.  Defaults from tools/eng_pacing_rows.sh (profiles/r03_engine_pacing_sweep.txt): 14 / 16 at <= 2 rows, 12 / 8
  // at 3 - 4 rows, 12 / 4 at 5 - 6 (more granules per pass: the first pass itself takes longer)
  static const int e_fd_env = getenv("ITTS_ENGINE_FIRST_DELAY") ? atoi(getenv("ITTS_ENGINE_FIRST_DELAY")) : -1;
  static const int e_ad_env = getenv("ITTS_ENGINE_ACT_DELAY") ? atoi(getenv("ITTS_ENGINE_ACT_DELAY")) : -1;
  const int e_fd = e_fd_env >= 0 ? e_fd_env : (B <= 2 ? 14 : 12);
  const int e_ad = e_ad_env >= 0 ? e_ad_env : (B <= 2 ? 16 : B <= 4 ? 8 : 4);
  static const int e_ps = getenv("ITTS_ENGINE_PASS_SLEEP") ? atoi(getenv("ITTS_ENGINE_PASS_SLEEP")) : 1;
  static const int e_thin = getenv("ITTS_ENGINE_THIN_FC") ? atoi(getenv("ITTS_ENGINE_THIN_FC")) : 0;
  ea.thin_fc = e_thin;
  static const int e_early = getenv("ITTS_ENGINE_EARLY_FC") ? atoi(getenv("ITTS_ENGINE_EARLY_FC")) : -1;
  ea.early_fc = e_early >= 0 ? e_early : 74;  // tools/ab_early.sh, tools/eng_pacing_rows.sh (profiles/r03_engine_early_fc.txt)
  ea.first_delay = e_fd;
  static const int e_ekv = getenv("ITTS_ENGINE_EARLY_KV") ? atoi(getenv("ITTS_ENGINE_EARLY_KV")) : 1;
  ea.early_kv = e_ekv;
  static const int e_cd = getenv("ITTS_ENGINE_CTX_DELAY") ? atoi(getenv("ITTS_ENGINE_CTX_DELAY")) : 0;
  ea.ctx_delay = e_cd;
  ea.act_delay = e_ad;
  ea.pass_sleep = e_ps;
  if (const char* tt = getenv("ITTS_ENGINE_TIMEOUT_TICKS")) ea.timeout_ticks = (unsigned)atol(tt);  // tests: force the give-up path (read per call)
  // the head (ln_f -> final_norm -> mel_head) inside the same launch when the engine runs every block (ITTS_ENGINE_HEAD=0: own launch)
  // (read per call - i.e. whenever an engine object captures its step -, so one process can compare both forms on fresh engine objects)
  const char* e_head_env = getenv("ITTS_ENGINE_HEAD");
  const bool e_head = !(e_head_env && atoi(e_head_env) == 0);
  fold_head = e_head && eng_first == c.layers && gpt.head.dt == BF16 && (gpt.head.w8 != nullptr) == w8 && gpt.head.b && gpt.head.Cin == ENG_D &&
              gpt.ln_f.g && gpt.ln_f.b && (c.number_mel_codes + ENG_NCU - 1) / ENG_NCU <= 33;
  // ... and the greedy sampler behind it (ITTS_ENGINE_SAMPLER=0: own launch): plain greedy search only - sampling, beams,
  // typical filtering and host-side sampling keep their kernels
  static const bool e_samp = !(getenv("ITTS_ENGINE_SAMPLER") && atoi(getenv("ITTS_ENGINE_SAMPLER")) == 0);
  fold_samp = fold_head && e_samp && !ds.do_sample && !ds.rows_active && ds.nb == 1 && !ds.host_sample && !(ds.typical_mass > 0.f);
  if (fold_samp) {
    ea.fold_sampler = 1;
    ea.samp = greedy_sampler_args(ds.logits, false);
    ea.cand = ds.eng_gran + eng_gran_count(c.layers) - ENG_CAND_WORDS;
  }
  if (fold_head) {
    ea.head_w = (const bf16_t*)(w8 ? gpt.head.w8 : gpt.head.w);
    ea.head_s = w8 ? gpt.head.wscale : nullptr;
    ea.head_b = gpt.head.b;
    ea.lnf_g = gpt.ln_f.g;
    ea.lnf_b = gpt.ln_f.b;
    ea.logits = ds.logits;
    ea.V = c.number_mel_codes;
  }
  return ea;
}

// a projection's GEMV arguments from its Lin; the call site adds X / Y, the prologue, the activation and the activation formats
static GemvArgs lin_gemv(const Lin& w, int B) {
  GemvArgs g;
  g.B = B;
  g.W = w.w;
  g.bias = w.b;
  g.N = g.ldy = w.N;
  g.K = w.Cin;
  g.w8src = w.w8 ? &w : nullptr;
  g.Wt = w.wt;
  return g;
}

// fp8 copy of the projection (BASELINE config 5) in place of W: the same weight bytes on every path (decode only; prefill /
// latent use the bf16 dequantisation of it), fragment-tiled for skinny_mfma
static void attach_fp8(GemvArgs& g, bool tiled) {
  if (!g.w8src) return;
  g.W8 = g.w8src->w8;
  g.wscale = g.w8src->wscale;
  if (tiled) g.W8t = g.w8src->wt8;
}

// one decode step: 24 x {LN+QKV gemv, cache attention (+append), proj gemv (+res),
// LN+FC gemv (gelu), proj2 gemv (+res)} -> head.  Every length / position is read from device memory, so the
// captured graph is identical for every step and every prefix length.
int Engine::decode_step_launch(hipStream_t s) {
  const itts_config& c = cfg;
  const int D = c.model_dim, H = c.heads, dh = D / H, B = ds.B;
  // ds.h already holds mel_emb[tok] + mel_pos[...] of this step (written by the previous step's sampler)
  const bool fast = adt == BF16 && B <= 4;  // bf16 activations between the decode kernels (ctx, act)
  const bool skinny = rows_on_mfma(B);      // weights once, batch on MFMA
  ds.pend_split = 0;
  ds.last_mode = 0;
  int eng_first = 0;
  if (engine_usable()) {  // <= 6 rows: the 24 blocks (+ head, + greedy sampler) as ONE persistent launch
    ITTS_REQUIRE(ds.eng_gran && ds.eng_ctr, "decode engine: state not allocated (prefill first)");
    bool fold_head = false, fold_samp = false;
    const EngArgs ea = engine_args(eng_first, fold_head, fold_samp);
    ds.last_mode = eng_first > 0;
    if (eng_first > 0) ITTS_TRY(decode_engine_layers(ea, s));
    if (ea.stamp) ITTS_TRY(tap("eng_stamps", ea.stamp, F32, (int64_t)ENG_NCU * eng_first * 16, s));
    if (ea.dbg) {
      ITTS_TRY(tap("eng_qkv", ea.dbg, F32, (int64_t)B * 3 * D, s));
      ITTS_TRY(tap("eng_h1", ea.dbg + (size_t)B * 3 * D, F32, (int64_t)B * D, s));
      ITTS_TRY(tap("eng_act", ea.dbg + (size_t)B * 4 * D, F32, (int64_t)B * 4 * D, s));
      ITTS_TRY(tap("eng_h2", ea.dbg + (size_t)B * 8 * D, F32, (int64_t)B * D, s));
    }
    if (eng_first == c.layers) return head_and_sample(s, fold_head, fold_samp);
  }
  // 5-16 rows: the step is launch-bound, so the two LayerNorm launches of a layer fold into the projections they feed
  // (skinny_mfma_kernel<LNP>) and the residual projections run as half tiles without a K split (<HALF>): 5 launches a
  // layer instead of 7 (ITTS_NO_SKINNY16=1 keeps the 7-launch form)
  static const bool no_s16 = getenv("ITTS_NO_SKINNY16") != nullptr;
  const bool small16 = skinny && B <= 16 && D <= 1280 && !no_s16;
  auto run = [&](GemvArgs& g, int dt) -> int {
    if (small16 && ((g.prologue == 1 && !g.ln_gamma) || (g.prologue == 0 && g.accumulate && g.Y == ds.h && g.N == D))) {
      if (g.prologue != 1) {
        g.half_tiles = 1;
        g.x_tiled = 1;
      }
      g.y_tiled = g.y_bf16;
      attach_fp8(g, true);
      return skinny_mfma(g, s);
    }
    if (skinny) {
      if (g.prologue == 1) {  // LayerNorm as a row kernel (its affine lives in the projection); it also absorbs the
                              // split-K partial sums of the projection that fed the residual stream
        ITTS_TRY(ln_rows_bf16(ds.hn, ds.h, g.ln_gamma, g.ln_beta, B, g.K, g.ln_eps, 1, ds.partial, ds.pend_split, ds.pend_bias, 1, s));
        ds.pend_split = 0;
        g.X = ds.hn;
        g.x_bf16 = 1;
        g.prologue = 0;
      } else if (g.accumulate && g.Y == ds.h && g.N == D) {
        // residual projections have few 16-feature tiles (D/16 = 80 on 256 CUs): split K over workgroups, reduced by
        // the LayerNorm that follows.  3 / 5 splits (240 / 200 workgroups): best of tools/split_sweep.sh
        static const int e_s1 = getenv("ITTS_SKINNY_SPLIT_PROJ") ? atoi(getenv("ITTS_SKINNY_SPLIT_PROJ")) : 3;
        static const int e_s2 = getenv("ITTS_SKINNY_SPLIT_PROJ2") ? atoi(getenv("ITTS_SKINNY_SPLIT_PROJ2")) : 5;
        g.ksplit = g.K >= 4 * D ? e_s2 : e_s1;
        g.partial = ds.partial;
        ds.pend_split = g.ksplit;
        ds.pend_bias = g.bias;
      }
      g.x_tiled = 1;           // every bf16 activation of this path (hn, ctx, act) is fragment-tiled
      g.y_tiled = g.y_bf16;
      attach_fp8(g, true);
      return skinny_mfma(g, s);
    }
    if (fast && gemv_bf16_supported(g)) {
      attach_fp8(g, false);
      return gemv_bf16(g, s);
    }
    ITTS_REQUIRE(!g.x_bf16 && !g.y_bf16, "decode: bf16 activation without the bf16 GEMV");
    // the bf16 engine's rows do not depend on their place in the batch: gemv2 maps the elements of its LayerNorm rows to threads
    // by batch position (its sums differ in the last ulp between identical rows), the generic kernel maps every row alike
    if (adt == BF16 && g.prologue == 1) return gemv(g, dt, s);
    return gemv2_supported(g) ? gemv2(g, dt, s) : gemv(g, dt, s);
  };
  GemvArgs probe;
  probe.B = B;
  probe.K = 4 * D;
  probe.x_bf16 = 1;
  probe.N = D;
  const bool bf_act = skinny || (fast && gemv_bf16_supported(probe));
  probe.K = D;
  const bool bf_ctx = skinny || (fast && gemv_bf16_supported(probe));
  for (int l = eng_first; l < c.layers; ++l) {
    const GptLayerW& L = gpt.layers[l];
    GemvArgs g = lin_gemv(L.attn, B);  // qkv = LN1(h) Wqkv + b
    g.X = ds.h;
    g.Y = ds.qkv;
    g.prologue = 1;
    g.ln_gamma = L.ln1.g;
    g.ln_beta = L.ln1.b;
    const size_t lo = (size_t)l * ds.Bcache * H * ds.Smax * dh * ds.ces;  // the cache's element size, not the engine's; the rows the cache was laid out for
    // few (row, head) pairs: the keys of each pair go to ATTN_NSPLIT workgroups and the projection merges the partials
    static const bool no_split = getenv("ITTS_ATTN_NOSPLIT") != nullptr;
    static const bool env_fuse = getenv("ITTS_FUSE_QKV_ATTN") != nullptr && atoi(getenv("ITTS_FUSE_QKV_ATTN")) != 0;
    // (an fp8 K/V cache has the whole forms only: neither the split form nor the fused launch below)
    const bool split = fast && bf_ctx && !no_split && (long)B * H <= 128 && D % 64 == 0 && ds.ct != FP8;
    // projection + attention of the layer as ONE launch (the attention workgroups poll for q / k / v): bf16 weights only
    const bool fused = split && (ds.fuse || env_fuse) && !ds.fuse_failed && !g.w8src && gemv_bf16_supported(g) && qkv_attn_fused_supported(g, H, dh);
    if (fused) {
      ITTS_TRY(qkv_attn_fused(g, ds.gran + (size_t)l * 4 * 3 * D, ds.fuse_err, (char*)ds.kc + lo, (char*)ds.vc + lo, ds.len,
                              ds.kv_start, ds.prefix_dev, H, dh, ds.Smax, ds.attn_o, ds.attn_ml, ds.nb > 1 ? ds.anc : nullptr,
                              ds.nb, s));
    } else {
      ITTS_TRY(run(g, L.attn.dt));
    }
#ifdef ITTS_PROBES
    static const int l_tap = getenv("ITTS_TAP_LAYER") ? atoi(getenv("ITTS_TAP_LAYER")) : -1;
#else
    constexpr int l_tap = -1;  // (the launch path's side of tools/eng_tap.py: probes library only)
#endif
    if (l == l_tap) ITTS_TRY(tap("lp_qkv", ds.qkv, F32, (int64_t)B * 3 * D, s));
    if (fused) {
    } else if (split)
      ITTS_TRY(decode_attn2(nullptr, BF16, ds.qkv, (char*)ds.kc + lo, (char*)ds.vc + lo, ds.len, ds.kv_start, ds.prefix_dev, B, H,
                            dh, ds.Smax, ds.ct, s, 0, ds.attn_o, ds.attn_ml, ds.nb > 1 ? ds.anc : nullptr, ds.nb));
    else
      ITTS_TRY(decode_attn2(ds.ctx, bf_ctx ? BF16 : F32, ds.qkv, (char*)ds.kc + lo, (char*)ds.vc + lo, ds.len, ds.kv_start,
                            ds.prefix_dev, B, H, dh, ds.Smax, ds.ct, s, skinny ? 1 : 0, nullptr, nullptr,
                            ds.nb > 1 ? ds.anc : nullptr, ds.nb));
    GemvArgs p = lin_gemv(L.proj, B);  // h += ctx Wproj + b
    p.X = ds.ctx;
    p.x_bf16 = bf_ctx;
    p.Y = ds.h;
    p.accumulate = 1;
    if (split) {
      p.prologue = 3;
      p.attn_o = ds.attn_o;
      p.attn_ml = ds.attn_ml;
      ITTS_REQUIRE(gemv_bf16_supported(p), "decode: split attention needs the bf16 GEMV with prologue 3");
    }
    ITTS_TRY(run(p, L.proj.dt));
    if (l == l_tap) ITTS_TRY(tap("lp_h1", ds.h, F32, (int64_t)B * D, s));
    GemvArgs f = lin_gemv(L.fc, B);  // act = gelu_new(LN2(h) Wfc + b)
    f.X = ds.h;
    f.Y = ds.act;
    f.y_bf16 = bf_act;
    f.act = ACT_GELU_NEW;
    f.prologue = 1;
    f.ln_gamma = L.ln2.g;
    f.ln_beta = L.ln2.b;
    ITTS_TRY(run(f, L.fc.dt));
    if (l == l_tap) ITTS_TRY(tap("lp_act", ds.act, bf_act ? BF16 : F32, (int64_t)B * 4 * D, s));
    GemvArgs q = lin_gemv(L.proj2, B);  // h += act Wproj2 + b
    q.X = ds.act;
    q.x_bf16 = bf_act;
    q.Y = ds.h;
    q.accumulate = 1;
    ITTS_TRY(run(q, L.proj2.dt));
    if (l == l_tap) ITTS_TRY(tap("lp_h2", ds.h, F32, (int64_t)B * D, s));
  }
  return head_and_sample(s);
}

// HF GenerationMixin.sample configuration of infer.py:116-124 (do_sample, top_k, top_p, temperature); the random
// draws are supplied by the caller as uniforms in [0, 1), one per (step, row): row-major [max_gen][B].  Any top_k: <= 0 is HF's
// "TopK warper off"
int Engine::gpt_set_sampling(int do_sample, int top_k, float top_p, float temperature, const float* uniforms_host, long n) {
  if (!do_sample) {
    ds.do_sample = 0;
    sample_uniforms.clear();
    return OK;
  }
  ITTS_REQUIRE(top_p > 0.f && top_p <= 1.f && temperature > 0.f, "gpt_set_sampling: need 0 < top_p <= 1 and temperature > 0");
  ITTS_REQUIRE(uniforms_host && n > 0, "gpt_set_sampling: uniforms missing");
  ds.do_sample = 1;
  ds.top_k = top_k < 1 ? 0 : top_k;  // 0: HF's TopK warper off; 0 and > 128 run on sampler_wide_kernel (sampler2_step)
  ds.top_p = top_p;
  ds.temperature = temperature;
  sample_uniforms.assign(uniforms_host, uniforms_host + n);
  return OK;
}

// Per-row settings of the following single-beam generations: row b of a batch of B takes rows_host[b] (B = 0 clears the table;
// the scalar setting then is whatever gpt_set_sampling last said, or greedy after a table that was not uniform).  The prefill
// latches it.  A table whose rows are all equal is the scalar setting with those values: gpt_set_sampling is called with it here
// and the steps take the scalar path, the persistent engine's in-launch greedy sampler included.  Any other table makes the step
// choose its tokens with sampler_rows_step; uniforms_host [max_gen][B] as in gpt_set_sampling, needed when any row samples.
int Engine::gpt_set_sampling_rows(const RowSampling* rows_host, int B, const float* uniforms_host, long n) {
  if (B == 0) {
    row_table.clear();
    row_table_uniform = false;
    return OK;
  }
  ITTS_REQUIRE(rows_host && B > 0, "gpt_set_sampling_rows: row table missing");
  bool uniform = true, samples = false;
  for (int b = 0; b < B; ++b) {
    const RowSampling& r = rows_host[b];
    ITTS_REQUIRE(r.mode == 0 || r.mode == 1, "gpt_set_sampling_rows: mode is 0 (greedy) or 1 (sample)");
    ITTS_REQUIRE(r.top_p > 0.f && r.top_p <= 1.f && r.temperature > 0.f && r.penalty > 0.f,
                 "gpt_set_sampling_rows: need 0 < top_p <= 1, temperature > 0 and penalty > 0");
    samples = samples || r.mode == 1;
    const RowSampling& r0 = rows_host[0];
    uniform = uniform && r.mode == r0.mode && r.penalty == r0.penalty &&
              (r.mode == 0 || ((r.top_k < 1 ? 0 : r.top_k) == (r0.top_k < 1 ? 0 : r0.top_k) && r.top_p == r0.top_p && r.temperature == r0.temperature));
  }
  ITTS_REQUIRE(!samples || (uniforms_host && n > 0), "gpt_set_sampling_rows: a sampled row needs uniforms");
  if (uniform) {
    ITTS_TRY(gpt_set_sampling(rows_host[0].mode, rows_host[0].top_k, rows_host[0].top_p, rows_host[0].temperature, uniforms_host, n));
  } else {
    ds.do_sample = 0;  // no scalar sampling beside the table
    if (samples)
      sample_uniforms.assign(uniforms_host, uniforms_host + n);
    else
      sample_uniforms.clear();
  }
  row_table.assign(rows_host, rows_host + B);
  for (RowSampling& r : row_table) r.top_k = r.top_k < 1 ? 0 : r.top_k;
  row_table_uniform = uniform;
  return OK;
}

// ds.rows [ds.B] <- row_table by the original row of every slot; ds.rows_classes <- the classes those rows hold
int Engine::upload_row_table(hipStream_t s) {
  DecodeState& d = ds;
  // after an admission the generation owns its table (adm_rows, by original row; B0 has grown, the slots have not)
  const std::vector<RowSampling>& row_table = d.admitted ? d.adm_rows : this->row_table;
  ITTS_REQUIRE((int)row_table.size() == d.B0 && d.B >= 1 && d.B <= d.B0 && (d.orig.empty() ? d.B == d.B0 : (int)d.orig.size() == d.B),
               "per-row sampling table: it does not belong to this generation");
  const int room = d.admitted ? d.Bcache : d.B0;  // entries: one per slot
  if (room > d.rows_cap) {
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
    d.drop_graphs();  // the captured samplers hold the old pointer
    ITTS_TRY(dev_alloc((void**)&d.rows, (size_t)room * sizeof(RowSampling)));
    d.rows_cap = room;
  }
  std::vector<RowSampling> tab((size_t)d.B);
  int classes = 0;
  for (int b = 0; b < d.B; ++b) {
    tab[b] = row_table[d.orig.empty() ? b : d.orig[b]];
    classes |= 1 << row_class(tab[b].mode, tab[b].top_k);
  }
  ITTS_HIP_CHECK(hipMemcpyAsync(d.rows, tab.data(), tab.size() * sizeof(RowSampling), hipMemcpyHostToDevice, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));  // tab is a host buffer of this call
  d.rows_classes = classes;
  return OK;
}

// TypicalLogitsWarper(mass) in front of the warpers of the sampling modes (typical_sampling=True, model.py:690-697); 0 = off
int Engine::gpt_set_typical(float mass) {
  ITTS_REQUIRE(mass == 0.f || (mass > 0.f && mass < 1.f), "gpt_set_typical: `typical_mass` has to be a float > 0 and < 1");
  ds.typical_mass = mass;
  return OK;
}

// Tokens that replace the sampler's choice for the first n steps of every following generation (n = 0 clears):
// the HF `input_tokens` continuation of inference_speech (model.py:672-686) and teacher forcing for parity tests.
// HF `input_tokens` (inference_speech, model.py:672-686): the given mel tokens are appended to the fake input ids, so the
// reference's FIRST forward embeds [start_mel, t1 .. tn] with mel positions 0 .. n (model.py:141-144) and the first
// generated token is fed at position n + 2 (model.py:151-155).  Same forcing as gpt_set_forced, but token k (0-based) is fed
// at position k + 1 instead of k + 2.
int Engine::gpt_set_input_tokens(const int32_t* ids_host, int B, int n) {
  ITTS_TRY(gpt_set_forced(ids_host, B, n));
  forced_input = forced_n > 0;
  return OK;
}

// Host-side token choice for the generate() modes the device samplers do not cover (HF warpers over the FULL vocabulary:
// top_k = 0 / None): prefill / decode(1) stop behind the head GEMV, the caller fetches the logits, applies the processors and
// warpers itself and hands the chosen token of every row back with gpt_commit, which runs the sampler's bookkeeping (ids,
// repetition bitmap, eos state, step counter, next step's input embedding) with those tokens.
int Engine::gpt_set_host_sampling(int on) {
  ds.host_sample = on ? 1 : 0;
  return OK;
}

int Engine::gpt_commit(const int32_t* tokens_host, hipStream_t s) {
  if (!ds.active || !ds.host_sample) {
    set_error("gpt_commit: needs an active generation in host-sampling mode");
    return E_STATE;
  }
  ITTS_REQUIRE(tokens_host && ds.nb == 1, "gpt_commit: tokens missing (or beams active)");
  std::vector<int> lens(ds.B);
  ITTS_HIP_CHECK(hipMemcpyAsync(lens.data(), ds.len, (size_t)ds.B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  for (int b = 0; b < ds.B; ++b) {
    ITTS_REQUIRE(tokens_host[b] >= 0 && tokens_host[b] < cfg.number_mel_codes, "gpt_commit: token id out of range");
    ITTS_REQUIRE(lens[b] < ds.max_gen, "gpt_commit: generation already at max length");
    ITTS_HIP_CHECK(hipMemcpyAsync(ds.forced + (size_t)b * ds.max_gen + lens[b], tokens_host + b, 4, hipMemcpyHostToDevice, s));
  }
  ITTS_HIP_CHECK(hipStreamSynchronize(s));  // tokens_host is the caller's buffer
  // the sampler's commit path with the forced table: argmax is computed and overridden, bookkeeping as in every other mode
  SamplerArgs sa = greedy_sampler_args(ds.logits, false);
  sa.forced = ds.forced;
  sa.input_n = 0;
  // plain greedy arguments whatever an earlier sampled generation left in the decode state (sampler2_kernel reads none of them)
  sa.do_sample = sa.top_k = 0;
  sa.top_p = sa.temperature = 1.f;
  sa.uniforms = nullptr;
  return sampler2_step(sa, ds.B, s);
}

// Host-side beam_sample (the generate() kwargs the device beam sampler does not cover: top_k = 0 / None or > 128 with several
// beams, infer.py:116-124 + webui.py:393-402).  The step stops behind the head GEMV (host sampling mode); the caller reads the
// logits and gpt_beam_state (every beam's id history, running scores, the done flags), does log_softmax -> processors ->
// warpers -> + beam scores -> the 2 * num_beams draws itself and hands the picks IN DRAW ORDER to gpt_commit_beams, which runs
// BeamSearchScorer.process and the history / cache-ancestry swap on the device exactly as the device-sampled mode does
// (beam_select_kernel with the draw skipped), so hypotheses, finalize and the engine's beam rows are shared.
int Engine::gpt_beam_state(int32_t* ids_host, float* scores_host, int32_t* done_host, int* step_host, hipStream_t s) {
  if (!ds.active || ds.nb <= 1) {
    set_error("gpt_beam_state: needs an active beam generation");
    return E_STATE;
  }
  int k = 0;
  ITTS_HIP_CHECK(hipMemcpyAsync(&k, ds.len, 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  const size_t rows = (size_t)ds.B, mg = (size_t)ds.max_gen;
  if (ids_host) ITTS_HIP_CHECK(hipMemcpyAsync(ids_host, ds.beam_ids + (size_t)(k & 1) * rows * mg, rows * mg * 4, hipMemcpyDeviceToHost, s));
  if (scores_host) ITTS_HIP_CHECK(hipMemcpyAsync(scores_host, ds.beam_scores, rows * 4, hipMemcpyDeviceToHost, s));
  if (done_host) ITTS_HIP_CHECK(hipMemcpyAsync(done_host, ds.beam_done, (size_t)(ds.B / ds.nb) * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  if (step_host) *step_host = k;
  return OK;
}

int Engine::gpt_commit_beams(const float* pick_score_host, const int32_t* pick_tok_host, const int32_t* pick_beam_host, hipStream_t s) {
  if (!ds.active || !ds.host_sample || ds.nb <= 1) {
    set_error("gpt_commit_beams: needs an active beam generation in host-sampling mode");
    return E_STATE;
  }
  ITTS_REQUIRE(pick_score_host && pick_tok_host && pick_beam_host, "gpt_commit_beams: picks missing");
  const int items = ds.B / ds.nb, nd = 2 * ds.nb;
  for (int i = 0; i < items * nd; ++i) {
    ITTS_REQUIRE(pick_tok_host[i] >= 0 && pick_tok_host[i] < cfg.number_mel_codes, "gpt_commit_beams: token id out of range");
    ITTS_REQUIRE(pick_beam_host[i] >= 0 && pick_beam_host[i] < ds.nb, "gpt_commit_beams: beam index out of range");
  }
  // the candidate scratch of the device sampler is idle in this mode: [0, items * nd) of cand_sc / cand_tok, beams behind the tokens
  static_assert(BEAM_MAX_CAND >= 4, "pick scratch fits the candidate scratch");
  ITTS_HIP_CHECK(hipMemcpyAsync(ds.cand_sc, pick_score_host, (size_t)items * nd * 4, hipMemcpyHostToDevice, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(ds.cand_tok, pick_tok_host, (size_t)items * nd * 4, hipMemcpyHostToDevice, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(ds.cand_tok + (size_t)items * nd, pick_beam_host, (size_t)items * nd * 4, hipMemcpyHostToDevice, s));
  BeamArgs ba = beam_args(ds.logits, false);
  ba.host_sc = ds.cand_sc;
  ba.host_tok = ds.cand_tok;
  ba.host_beam = ds.cand_tok + (size_t)items * nd;
  const int st = beam_commit_step(ba, s);
  ITTS_HIP_CHECK(hipStreamSynchronize(s));  // the picks are the caller's buffers
  return st;
}

// The last device-sampled whole-vocabulary beam step's picks in draw order [items][2 * num_beams] (score with the running beam
// score, token, beam) and the kept count of every beam row [items * num_beams]: they sit in the sampler's buffers until the
// next step overwrites them.  Items that were done (or a given-token step) keep what an earlier step left there.
int Engine::gpt_beam_picks(float* score_host, int32_t* tok_host, int32_t* beam_host, int32_t* kept_host, hipStream_t s) {
  if (!ds.active || ds.nb <= 1 || !ds.wide_valid || !ds.wide.sc) {
    set_error("gpt_beam_picks: needs an active beam generation that samples over the whole vocabulary on the device");
    return E_STATE;
  }
  const size_t np = (size_t)(ds.B / ds.nb) * 2 * ds.nb;
  if (score_host) ITTS_HIP_CHECK(hipMemcpyAsync(score_host, ds.wide.pick_sc, np * 4, hipMemcpyDeviceToHost, s));
  if (tok_host) ITTS_HIP_CHECK(hipMemcpyAsync(tok_host, ds.wide.pick_tok, np * 4, hipMemcpyDeviceToHost, s));
  if (beam_host) ITTS_HIP_CHECK(hipMemcpyAsync(beam_host, ds.wide.pick_beam, np * 4, hipMemcpyDeviceToHost, s));
  if (kept_host) ITTS_HIP_CHECK(hipMemcpyAsync(kept_host, ds.wide.kept, (size_t)ds.B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  return OK;
}

int Engine::gpt_set_forced(const int32_t* ids_host, int B, int n) {
  forced_input = 0;
  if (n <= 0 || !ids_host) {
    forced_host.clear();
    forced_B = forced_n = 0;
    return OK;
  }
  ITTS_REQUIRE(B >= 1, "gpt_set_forced: B < 1");
  for (long i = 0; i < (long)B * n; ++i)
    ITTS_REQUIRE(ids_host[i] >= -1 && ids_host[i] < cfg.number_mel_codes, "gpt_set_forced: token id out of range");
  forced_host.assign(ids_host, ids_host + (size_t)B * n);
  forced_B = B;
  forced_n = n;
  return OK;
}

// The persistent decode engine keeps one workgroup on EVERY CU for a whole token step and its workgroups wait for each other:
// two such launches in flight together (two Engine objects decoding on two streams of one device) could each hold part of
// the CUs and wait for workgroups that cannot become resident - until the 20 ms bound of the waits fires.  So engine launches
// of one device are chained across streams: a decode call first makes its stream wait for the event behind the last engine
// launch of the device (a no-op on the same stream), then records its own.  Other kernels may share the device freely: they
// finish on their own and the engine's workgroups simply start later.
namespace {
struct EngineGate {
  std::mutex mu;
  hipEvent_t ev = nullptr;
};
EngineGate& engine_gate(int dev) {
  static EngineGate gates[64];
  return gates[dev & 63];
}
}  // namespace

int Engine::gpt_decode(int nsteps, hipStream_t s) {
  if (!ds.active) {
    set_error("gpt_decode: call itts_gpt_prefill first");
    return E_STATE;
  }
  static const bool no_gate = getenv("ITTS_ENGINE_NO_GATE") != nullptr;  // debugging aid: show what the chaining prevents
  if (!engine_usable() || dry || no_gate) return gpt_decode_steps(nsteps, s);
  int dev = 0;
  ITTS_HIP_CHECK(hipGetDevice(&dev));
  EngineGate& g = engine_gate(dev);
  std::lock_guard<std::mutex> lk(g.mu);
  if (!g.ev) ITTS_HIP_CHECK(hipEventCreateWithFlags(&g.ev, hipEventDisableTiming));
  else ITTS_HIP_CHECK(hipStreamWaitEvent(s, g.ev, 0));
  const int rc = gpt_decode_steps(nsteps, s);
  ITTS_HIP_CHECK(hipEventRecord(g.ev, s));
  return rc;
}

// the values a captured step depends on (GraphKey, engine.h), from the decode state of the current request
GraphKey Engine::graph_key() const {
  const DecodeState& d = ds;
  GraphKey k;
  k.B = d.B;
  k.Bcache = d.Bcache;
  k.Smax = d.Smax;
  k.max_gen = d.max_gen;
  k.use_forced = d.use_forced;
  k.input_n = d.input_n;
  k.host_sample = d.host_sample;
  k.fuse = d.fuse && !d.fuse_failed;
  k.eng = (int)engine_usable();
  k.ct = d.ct;
  k.nb = d.nb;
  k.beam_sample = d.beam_sample;
  k.length_penalty = d.length_penalty;
  k.typical_mass = d.typical_mass;
  k.penalty = d.penalty;
  k.suppress_stop = d.suppress_stop;
  k.do_sample = d.do_sample;
  k.top_k = d.top_k;
  k.top_p = d.top_p;
  k.temperature = d.temperature;
  k.rows_active = d.rows_active;
  k.rows_classes = d.rows_classes;
  return k;
}

int Engine::gpt_decode_steps(int nsteps, hipStream_t s) {
  ITTS_REQUIRE(nsteps >= 0, "gpt_decode: nsteps < 0");
  if (use_graph && s != nullptr) {
    DecodeState& d = ds;
    const GraphKey key = graph_key();
    const bool stale = !d.graph || !(d.graph_key == key);
    // two executables: one step, and GK steps back to back (one launch per GK tokens: the gap between consecutive graph
    // launches is paid once per GK steps; every step reads its lengths from device memory, so any mix is valid)
    static const int GK = [] {
      const char* e = getenv("ITTS_GRAPH_STEPS");
      const int v = e ? atoi(e) : 8;
      return v < 1 ? 1 : (v > 32 ? 32 : v);
    }();
    if (stale && nsteps > 0) {
      d.drop_graphs();
      for (int which = 0; which < (GK > 1 ? 2 : 1); ++which) {
        hipGraph_t g = nullptr;
        ITTS_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        int st = OK;
        for (int k = 0; k < (which ? GK : 1) && st == OK; ++k) st = decode_step_launch(s);
        const hipError_t ee = hipStreamEndCapture(s, &g);
        if (st != OK) {
          if (g) (void)hipGraphDestroy(g);
          return st;
        }
        ITTS_HIP_CHECK(ee);
        ITTS_HIP_CHECK(hipGraphInstantiate(which ? &d.graphK : &d.graph, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
      }
      d.graph_key = key;
      d.graph_mode = d.last_mode;  // what the captured step runs on
      ++d.graph_captures;
    }
    d.last_mode = d.graph_mode;  // a replayed graph: the mode it was captured with
    int left = nsteps;
    if (d.graphK)
      for (; left >= GK; left -= GK) ITTS_HIP_CHECK(hipGraphLaunch(d.graphK, s));
    for (; left > 0; --left) ITTS_HIP_CHECK(hipGraphLaunch(d.graph, s));
    return OK;
  }
  for (int i = 0; i < nsteps; ++i) ITTS_TRY(decode_step_launch(s));
  return OK;
}

// abort word of the persistent decode engine: a hand-off wait gave up, so the codes of this generation are not valid.
// The engine is switched off for this Engine (launch path from the next generation on) and its state re-initialised.
int Engine::engine_check(hipStream_t s) {
  if (ds.fuse_err && (ds.fuse || ds.graph_key.fuse)) {  // the opt-in fused projection + attention launch: checked at fetch too
    int ferr = 0;
    ITTS_HIP_CHECK(hipMemcpyAsync(&ferr, ds.fuse_err, 4, hipMemcpyDeviceToHost, s));
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
    if (ferr) {  // an attention workgroup gave up waiting for its q / k / v: the codes of this generation are not valid
      ds.fuse_failed = 1;  // later generations take the two-launch path
      ITTS_HIP_CHECK(hipMemsetAsync(ds.fuse_err, 0, 4, s));
      set_error("in-launch q/k/v hand-off timed out (fused projection + attention disabled for this engine; the codes of this generation are not valid)");
      return E_HANDOFF;
    }
  }
  if (!ds.eng_ctr) return OK;
  unsigned host[2] = {0, 0};
  ITTS_HIP_CHECK(hipMemcpyAsync(host, ds.eng_ctr, 8, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  if (!host[1]) return OK;
  ds.eng_failed = 1;
  // The drained launches computed on hand-offs that never arrived: what they appended to the K/V cache is arbitrary bits, and the
  // decode attention multiplies rows past the sequence end by p = 0 instead of selecting them away (ensure_decode_state) - a NaN
  // or infinity left there would poison the next generation's first steps.  Back to the zero fill of a fresh allocation.
  if (ds.kc && ds.vc && ds.cache_bytes) {
    ITTS_HIP_CHECK(hipMemsetAsync(ds.kc, 0, ds.cache_bytes, s));
    ITTS_HIP_CHECK(hipMemsetAsync(ds.vc, 0, ds.cache_bytes, s));
  }
  const unsigned ctr0[2] = {host[0] ? host[0] : 1u, 0u};
  ITTS_HIP_CHECK(hipMemcpyAsync(ds.eng_ctr, ctr0, 8, hipMemcpyHostToDevice, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  set_error("decode engine: an in-launch hand-off timed out (persistent engine disabled for this engine; the codes of this generation are not valid)");
  fprintf(stderr, "[itts_hip] persistent decode engine: a hand-off wait gave up (another process or kernel held CUs of this GPU?); "
                  "this engine object uses the five-launches-per-block decode path from now on\n");
  return E_HANDOFF;
}

int Engine::gpt_status(int* steps, int* n_unf, hipStream_t s) {
  if (!ds.active) {
    set_error("gpt_status: no active generation");
    return E_STATE;
  }
  std::vector<int> host(ds.B + 1);
  ITTS_HIP_CHECK(hipMemcpyAsync(host.data(), ds.len, 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(host.data() + 1, ds.unfinished, (size_t)ds.B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  ITTS_TRY(engine_check(s));
  if (steps) *steps = host[0];
  if (n_unf) {
    int n = 0;
    for (int b = 0; b < ds.B; ++b) n += host[1 + b] != 0;
    *n_unf = n;
  }
  return OK;
}

int Engine::gpt_fetch(int32_t* codes, float* logits, hipStream_t s) {
  if (!ds.active) {
    set_error("gpt_fetch: no active generation");
    return E_STATE;
  }
  ITTS_TRY(engine_check(s));
  if (ds.B != ds.B0) return fetch_retired(codes, logits, s);
  if (codes && ds.nb > 1)
    ITTS_TRY(beam_finalize(codes, s));  // [B / nb * beam_returns][max_gen]
  else if (codes)
    ITTS_HIP_CHECK(hipMemcpyAsync(codes, ds.ids, (size_t)ds.B * ds.max_gen * 4, hipMemcpyDeviceToHost, s));
  if (logits)
    ITTS_HIP_CHECK(hipMemcpyAsync(logits, ds.logits, (size_t)ds.B * cfg.number_mel_codes * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  return OK;
}

// gpt_fetch after a row retirement: [B0] rows in the ORIGINAL order - live rows from their slot, retired rows from the host store
// (their codes followed by stop, as an unretired run holds them, and the logits of their last step before the retirement).
// Under beams the codes come per batch item, ret_keep hypotheses each: live items from beam_finalize over the live state
int Engine::fetch_retired(int32_t* codes, float* logits, hipStream_t s) {
  const DecodeState& d = ds;
  const size_t mg = (size_t)d.max_gen, V = (size_t)cfg.number_mel_codes;
  const int nb = d.nb, keep = nb > 1 ? d.ret_keep : 1;  // an item: nb rows, keep code rows
  ITTS_REQUIRE(nb == 1 || beam_returns == d.ret_keep, "gpt_fetch: num_return_sequences changed after a beam group was retired");
  const size_t item = (size_t)keep * mg;
  std::vector<int32_t> ids(codes ? (size_t)(d.B / nb) * item : 0);
  std::vector<float> lg(logits ? (size_t)d.B * V : 0);
  if (codes && nb > 1) ITTS_TRY(beam_finalize(ids.data(), s));
  if (codes && nb == 1) ITTS_HIP_CHECK(hipMemcpyAsync(ids.data(), d.ids, ids.size() * 4, hipMemcpyDeviceToHost, s));
  if (logits) ITTS_HIP_CHECK(hipMemcpyAsync(lg.data(), d.logits, lg.size() * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  for (int r = 0; r < d.B0; ++r) {
    if (!d.retired[r]) continue;
    if (codes && r % nb == 0) std::memcpy(codes + (size_t)(r / nb) * item, d.ret_codes.data() + (size_t)(r / nb) * item, item * 4);
    if (logits) std::memcpy(logits + (size_t)r * V, d.ret_logits.data() + (size_t)r * V, V * 4);
  }
  for (int slot = 0; slot < d.B; ++slot) {
    const size_t r = (size_t)d.orig[slot];
    if (codes && slot % nb == 0) std::memcpy(codes + r / nb * item, ids.data() + (size_t)(slot / nb) * item, item * 4);
    if (logits) std::memcpy(logits + r * V, lg.data() + (size_t)slot * V, V * 4);
  }
  return OK;
}

// Row retirement (opt-in): compact the decode state of a running single-beam generation to its unfinished rows, so that the
// following steps run - and are captured - at the smaller row count.  A finished row's output is fixed (the sampler writes stop
// for it), a row's results do not depend on its slot, so the caller sees the same generation.  The plan (retire_plan) moves live
// rows from slots >= n into dead slots < n; rows_move_kernel copies their K/V history (the positions that hold history only:
// what lies behind stays the dead row's finite bytes, which the attention multiplies by p = 0) and their state arrays.
// No-op (the row count stays) without an active generation, under beams (unless gpt_set_retire_beams opted in: retire_beam_groups)
// or host sampling, while the step runs on the persistent
// engine or the fused qkv + attention launch, and when no row or every row has finished.
int Engine::gpt_retire_rows(int* rows_now, hipStream_t s) {
  DecodeState& d = ds;
  if (rows_now) *rows_now = d.active ? d.B : 0;
  if (!d.active) return OK;
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  static const bool env_fuse = getenv("ITTS_FUSE_QKV_ATTN") != nullptr && atoi(getenv("ITTS_FUSE_QKV_ATTN")) != 0;
  if (d.nb > 1) {  // opt-in on its own (gpt_set_retire_beams; ITTS_RETIRE_BEAMS, read per call, overrides the setter both ways)
    const char* rb = getenv("ITTS_RETIRE_BEAMS");
    if (!(rb ? atoi(rb) != 0 : d.retire_beams != 0) || d.input_n > 0) return OK;
  }
  if (d.host_sample || engine_usable() || ((d.fuse || env_fuse) && !d.fuse_failed)) return OK;
  if (d.nb > 1) return retire_beam_groups(rows_now, s);
  const itts_config& c = cfg;
  const int B = d.B, D = c.model_dim, H = c.heads, dh = D / H, V = c.number_mel_codes, mg = d.max_gen;
  std::vector<int> unf(B), lens(B), src(B), dst(B);
  int k = 0, n = 0, nm = 0;
  ITTS_HIP_CHECK(hipMemcpyAsync(unf.data(), d.unfinished, (size_t)B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(lens.data(), d.len, (size_t)B * 4, hipMemcpyDeviceToHost, s));  // (admitted rows started later)
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  ITTS_TRY(retire_plan(unf.data(), B, &n, src.data(), dst.data(), &nm));
  if (n == B || n == 0) return OK;
  for (int b = 0; b < B; ++b) {
    ITTS_REQUIRE(lens[b] >= 0 && lens[b] <= mg, "gpt_retire_rows: decode state out of range");
    k = std::max(k, lens[b]);  // the longest history: what the K/V moves copy
  }
  ITTS_REQUIRE(nm <= ROWS_MOVE_MAX, "gpt_retire_rows: decode state out of range");
  // 1. the retiring rows' codes and last logits go to the host store, by original row
  if (d.orig.empty()) {
    d.orig.resize(B);
    for (int b = 0; b < B; ++b) d.orig[b] = b;
    d.retired.assign((size_t)d.B0, 0);
    d.ret_codes.assign((size_t)d.B0 * mg, c.stop_mel_token);
    d.ret_logits.assign((size_t)d.B0 * V, 0.f);
  }
  {
    std::vector<int32_t> ids((size_t)B * mg);
    std::vector<float> lg((size_t)B * V);
    ITTS_HIP_CHECK(hipMemcpyAsync(ids.data(), d.ids, ids.size() * 4, hipMemcpyDeviceToHost, s));
    ITTS_HIP_CHECK(hipMemcpyAsync(lg.data(), d.logits, lg.size() * 4, hipMemcpyDeviceToHost, s));
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
      if (unf[b]) continue;
      const size_t r = (size_t)d.orig[b];
      d.retired[r] = 1;
      std::memcpy(d.ret_codes.data() + r * mg, ids.data() + (size_t)b * mg, (size_t)lens[b] * 4);  // stop behind them (the fill above)
      std::memcpy(d.ret_logits.data() + r * V, lg.data() + (size_t)b * V, (size_t)V * 4);
    }
  }
  // 2. the moves: K and V over all layers (heads as chunks, the positions that hold history), then the per-row state arrays
  const size_t head = (size_t)d.Smax * dh * d.ces, row = (size_t)H * head;
  const size_t hist = (size_t)std::min(d.Smax, d.prefix + k) * dh * d.ces;
  for (void* cache : {d.kc, d.vc})
    ITTS_TRY(rows_move(cache, (size_t)d.Bcache * row, c.layers, row, head, H, hist, src.data(), dst.data(), nm, s));
  const std::pair<void*, size_t> arrays[] = {{d.h, (size_t)D * 4},      {d.logits, (size_t)V * 4}, {d.ids, (size_t)mg * 4},
                                             {d.forced, (size_t)mg * 4}, {d.seen, (size_t)V},       {d.len, 4},
                                             {d.kv_start, 4},            {d.cur_tok, 4},            {d.unfinished, 4}};
  for (const auto& a : arrays)
    ITTS_TRY(rows_move(a.first, 0, 1, a.second, a.second, 1, a.second, src.data(), dst.data(), nm, s));
  for (int i = 0; i < nm; ++i) d.orig[dst[i]] = d.orig[src[i]];
  d.orig.resize(n);
  // 3. the sampler reads uniforms[k * B + b]: re-packed to [max_gen][n] by original row
  std::vector<float> u;
  if (d.do_sample || (d.rows_active && (d.rows_classes & ~(1 << ROWCLS_GREEDY)))) {
    ITTS_REQUIRE(d.admitted ? d.adm_uniforms.size() == (size_t)mg * d.B0 : sample_uniforms.size() >= (size_t)mg * d.B0,
                 "gpt_retire_rows: the uniforms of this generation are gone");
    u.resize((size_t)mg * n);
    for (int q = 0; q < mg; ++q)
      for (int b = 0; b < n; ++b)
        u[(size_t)q * n + b] = d.admitted ? d.adm_uniforms[(size_t)d.orig[b] * mg + q] : sample_uniforms[(size_t)q * d.B0 + d.orig[b]];
    ITTS_HIP_CHECK(hipMemcpyAsync(d.uniforms, u.data(), u.size() * 4, hipMemcpyHostToDevice, s));
  }
  d.B = n;
  // 4. the per-row settings travel with their rows, and the classes are those of the rows that are left (GraphKey::rows_classes)
  if (d.rows_active) ITTS_TRY(upload_row_table(s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  d.drop_graphs();  // every later step re-captures at the smaller row count (GraphKey::B / Bcache)
  if (rows_now) *rows_now = n;
  return OK;
}

int Engine::gpt_set_retire_beams(int on) {
  ds.retire_beams = on != 0;
  return OK;
}

// The beam branch of gpt_retire_rows (opt-in, gpt_set_retire_beams): compact a running beam generation to the rows of its
// unfinished batch items.  Why a group may move as a unit: its nb rows are contiguous and aligned to nb, the cache ancestry names
// a key's row relative to the group (decode_attn2_kernel<ANC>: (b / nb) * nb + anc[b][j]), and a done group is a no-op in every
// beam kernel while beam_finalize reads nothing of it but its hypothesis store - so its result is final, taken here, and kept on
// the host by original item.  With group-uniform flags retire_plan moves whole groups into whole holes and a beam keeps its index
// inside its group (asserted below before anything changes).  The live groups share one step k, so len[0] stays the common step - unless groups
// were admitted (admit_beam_groups): then every group has its own step, the host reads len per item, and both halves of step 3 move.
//   1. the retiring items' hypotheses (beam_finalize_item) and their rows' last logits -> the host store
//   2. rows_move with the row plan: K and V over all layers, h, logits, forced, len, kv_start, cur_tok, unfinished, beam_scores;
//      with the item plan: the hypothesis store and the scorer's per-item words
//   3. beam_ids [2][rows][max_gen] and anc [2][rows][Smax]: only the half of parity k & 1 is live (the next beam_select_kernel
//      rewrites the other one completely for every live group), and every kernel computes the base of half 1 from the CURRENT row
//      count.  Parity 0: rows_move in place.  Parity 1: the live rows go from base rows_old * row to base rows_new * row, ranges
//      that may overlap - two rows_gather launches through the dead half 0: old half 1 -> [0, rows_new), then -> [rows_new, 2 rows_new)
//   4. uniforms [max_gen][items][2 nb] re-packed from the host copy by original item
// cand_*, scores2 and the whole-vocabulary sampler's block are scratch between the launches of one step, indexed by row or item
// from pointers fixed at the prefill: nothing in them depends on the row count.
int Engine::retire_beam_groups(int* rows_now, hipStream_t s) {
  DecodeState& d = ds;
  const itts_config& c = cfg;
  const int nb = d.nb, B = d.B, items = B / nb, D = c.model_dim, H = c.heads, dh = D / H, V = c.number_mel_codes, mg = d.max_gen;
  const int keep = beam_returns, nd = 2 * nb, items0 = d.B0 / nb;
  std::vector<int> done(items), unf(B), lens(B), live(B), src(B), dst(B);
  ITTS_HIP_CHECK(hipMemcpyAsync(done.data(), d.beam_done, (size_t)items * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(unf.data(), d.unfinished, (size_t)B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(lens.data(), d.len, (size_t)B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  for (int b = 0; b < B; ++b) live[b] = !done[b / nb];
  int n = 0, nm = 0;
  ITTS_TRY(retire_plan(live.data(), B, &n, src.data(), dst.data(), &nm));
  if (n == B || n == 0) return OK;
  // everything that could refuse, before anything is changed
  // groups that were admitted (admit_beam_groups) started later: then every group has its own step and BOTH ping-pong halves are
  // live - k is the longest history (what the K/V moves copy), and step 3 moves both halves
  const bool mixed = d.admitted > 0;
  int k = lens[0];
  ITTS_REQUIRE(k >= 0 && k <= mg, "gpt_retire_rows: decode state out of range");
  for (int b = 0; b < B; ++b) {
    ITTS_REQUIRE(lens[b] == (mixed ? lens[b - b % nb] : k) && (live[b] || !unf[b]), "gpt_retire_rows: the beam groups do not share one step, or a done group has an unfinished row");
    ITTS_REQUIRE(lens[b] >= 0 && lens[b] <= mg, "gpt_retire_rows: decode state out of range");
  }
  for (int b = 0; b < B; ++b) k = std::max(k, lens[b]);
  ITTS_REQUIRE(n % nb == 0 && nm % nb == 0 && nm <= ROWS_MOVE_MAX && n <= ROWS_MOVE_MAX, "gpt_retire_rows: beam groups need at most 128 live rows");
  for (int i = 0; i < nm; ++i)  // whole groups into whole holes, a beam keeps its index inside its group
    ITTS_REQUIRE(src[i] % nb == i % nb && dst[i] % nb == i % nb && src[i] - src[i - i % nb] == i % nb && dst[i] - dst[i - i % nb] == i % nb,
                 "gpt_retire_rows: the plan splits a beam group");
  ITTS_REQUIRE(keep >= 1 && keep <= nb && (d.orig.empty() || keep == d.ret_keep), "gpt_retire_rows: num_return_sequences changed inside a generation");
  const bool draws = d.beam_sample && !d.host_sample;
  ITTS_REQUIRE(!draws || (mixed ? d.adm_uniforms.size() == (size_t)mg * items0 * nd : sample_uniforms.size() >= (size_t)mg * items0 * nd),
               "gpt_retire_rows: the uniforms of this generation are gone");
  std::vector<int> isrc(nm / nb), idst(nm / nb);  // the item plan
  for (int g = 0; g < nm / nb; ++g) {
    isrc[g] = src[g * nb] / nb;
    idst[g] = dst[g * nb] / nb;
  }
  // 1. the retiring items' hypotheses and last logits go to the host store, by original item / row
  {
    BeamHost st;
    ITTS_TRY(beam_read_state(st, s));
    std::vector<int32_t> fin((size_t)items * keep * mg);
    for (int b = 0; b < items; ++b)
      if (done[b]) ITTS_TRY(beam_finalize_item(st, b, fin.data() + (size_t)b * keep * mg));
    std::vector<float> lg((size_t)B * V);
    ITTS_HIP_CHECK(hipMemcpyAsync(lg.data(), d.logits, lg.size() * 4, hipMemcpyDeviceToHost, s));
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
    if (d.orig.empty()) {
      d.orig.resize(B);
      for (int b = 0; b < B; ++b) d.orig[b] = b;
      d.retired.assign((size_t)d.B0, 0);
      d.ret_keep = keep;
      d.ret_codes.assign((size_t)items0 * keep * mg, c.stop_mel_token);
      d.ret_logits.assign((size_t)d.B0 * V, 0.f);
    }
    for (int b = 0; b < B; ++b) {
      if (live[b]) continue;
      const size_t r = (size_t)d.orig[b];
      d.retired[r] = 1;
      if (b % nb == 0) std::memcpy(d.ret_codes.data() + r / nb * keep * mg, fin.data() + (size_t)(b / nb) * keep * mg, (size_t)keep * mg * 4);
      std::memcpy(d.ret_logits.data() + r * V, lg.data() + (size_t)b * V, (size_t)V * 4);
    }
  }
  // 2. K and V over all layers (heads as chunks, the positions that hold history), the per-row and the per-item arrays
  const size_t head = (size_t)d.Smax * dh * d.ces, row = (size_t)H * head;
  const size_t hist = (size_t)std::min(d.Smax, d.prefix + k + 1) * dh * d.ces;
  for (void* cache : {d.kc, d.vc})
    ITTS_TRY(rows_move(cache, (size_t)d.Bcache * row, c.layers, row, head, H, hist, src.data(), dst.data(), nm, s));
  const std::pair<void*, size_t> by_row[] = {{d.h, (size_t)D * 4}, {d.logits, (size_t)V * 4}, {d.forced, (size_t)mg * 4}, {d.len, 4},
                                             {d.kv_start, 4},      {d.cur_tok, 4},            {d.unfinished, 4},          {d.beam_scores, 4}};
  for (const auto& a : by_row)
    ITTS_TRY(rows_move(a.first, 0, 1, a.second, a.second, 1, a.second, src.data(), dst.data(), nm, s));
  const size_t slots = (size_t)(nb + 1) * 4;  // the nb + 1 hypothesis slots of an item
  const std::pair<void*, size_t> by_item[] = {{d.hyp_tok, slots * mg}, {d.hyp_score, slots}, {d.hyp_len, slots},  {d.hyp_order, slots},
                                              {d.hyp_n, 4},            {d.hyp_worst, 4},     {d.hyp_counter, 4}, {d.beam_done, 4}};
  for (const auto& a : by_item)
    ITTS_TRY(rows_move(a.first, 0, 1, a.second, a.second, 1, a.second, isrc.data(), idst.data(), nm / nb, s));
  // 3. the live half of the two ping-pong arrays
  const std::pair<void*, size_t> halves[] = {{d.beam_ids, (size_t)mg * 4}, {d.anc, (size_t)d.Smax}};
  if (mixed) {
    // both halves are live, so there is no dead half to stage through: half 0 moves in place, half 1 goes from base rows_old * row
    // to base rows_new * row through a staging block of the scratch arena (two rows_gather launches, stream-ordered)
    std::vector<int> from(n), iota(n);
    for (int j = 0; j < n; ++j) from[j] = B + j, iota[j] = j;
    for (int i = 0; i < nm; ++i) from[dst[i]] = B + src[i];
    const size_t stage_bytes = (size_t)n * std::max((size_t)mg * 4, (size_t)d.Smax);
    ITTS_TRY(ws_reserve(stage_bytes + 4096, s));
    ws_reset();
    void* stage = alloc(stage_bytes);
    for (const auto& a : halves) {
      ITTS_TRY(rows_move(a.first, 0, 1, a.second, a.second, 1, a.second, src.data(), dst.data(), nm, s));
      ITTS_TRY(rows_gather(stage, 0, a.first, 0, 1, a.second, from.data(), n, s));
      ITTS_TRY(rows_gather((char*)a.first + (size_t)n * a.second, 0, stage, 0, 1, a.second, iota.data(), n, s));
    }
  } else if ((k & 1) == 0) {
    for (const auto& a : halves)
      ITTS_TRY(rows_move(a.first, 0, 1, a.second, a.second, 1, a.second, src.data(), dst.data(), nm, s));
  } else {
    std::vector<int> from(n), iota(n);  // from[j]: the row of the old half 1 that slot j holds after the retirement
    for (int j = 0; j < n; ++j) from[j] = B + j, iota[j] = j;
    for (int i = 0; i < nm; ++i) from[dst[i]] = B + src[i];
    for (const auto& a : halves) {
      ITTS_TRY(rows_gather(a.first, 0, a.first, 0, 1, a.second, from.data(), n, s));
      ITTS_TRY(rows_gather((char*)a.first + (size_t)n * a.second, 0, a.first, 0, 1, a.second, iota.data(), n, s));
    }
  }
  for (int i = 0; i < nm; ++i) d.orig[dst[i]] = d.orig[src[i]];
  d.orig.resize(n);
  // 4. beam_select_kernel reads uniforms[(k * items + item) * 2 nb + j]: re-packed by original item
  std::vector<float> u;
  if (draws) {
    const int ni = n / nb;
    u.resize((size_t)mg * ni * nd);
    for (int q = 0; q < mg; ++q)
      for (int i = 0; i < ni; ++i)
        std::memcpy(u.data() + ((size_t)q * ni + i) * nd,
                    mixed ? d.adm_uniforms.data() + ((size_t)(d.orig[i * nb] / nb) * mg + q) * nd
                          : sample_uniforms.data() + ((size_t)q * items0 + d.orig[i * nb] / nb) * nd,
                    (size_t)nd * 4);
    ITTS_HIP_CHECK(hipMemcpyAsync(d.uniforms, u.data(), u.size() * 4, hipMemcpyHostToDevice, s));
  }
  d.B = n;
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  d.drop_graphs();  // every later step re-captures at the smaller row count (GraphKey::B / Bcache)
  if (rows_now) *rows_now = n;
  return OK;
}

// A uniform per-row table normally IS the scalar setting (gpt_set_sampling_rows).  With on = 1 the following prefills keep any
// table as a table generation - one sampler launch per class, room for draws - so that it can admit rows of other settings later.
int Engine::gpt_keep_row_table(int on) {
  row_table_keep = on != 0;
  return OK;
}

int Engine::gpt_row_status(int32_t* orig_host, int32_t* len_host, int32_t* unf_host, hipStream_t s) {
  if (!ds.active) {
    set_error("gpt_row_status: no active generation");
    return E_STATE;
  }
  if (len_host) ITTS_HIP_CHECK(hipMemcpyAsync(len_host, ds.len, (size_t)ds.B * 4, hipMemcpyDeviceToHost, s));
  if (unf_host) ITTS_HIP_CHECK(hipMemcpyAsync(unf_host, ds.unfinished, (size_t)ds.B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  ITTS_TRY(engine_check(s));
  if (orig_host)
    for (int b = 0; b < ds.B; ++b) orig_host[b] = ds.orig.empty() ? b : ds.orig[b];
  return OK;
}

// Row admission (opt-in): n finished slots of the running generation take n new requests.  A batched token step costs almost the
// same at every row count, so a slot that a finished row holds is better spent on the next waiting sentence than carried to the
// end of the slowest row.  Every kernel of the step reads a row's position from its own len / kv_start, so an admitted row is a row
// with len = 0 whose prefix sits in positions [kv_start, prefix] of its slot: the steps that follow are the steps of a fresh
// generation for it, and the running rows are neither stepped nor touched here.
//   1. synchronise; the n lowest finished slots (admit_plan); their codes and last logits go to the host store by original row
//   2. the new rows become original rows B0 .. B0 + n - 1 (gpt_fetch returns all of them, in that order)
//   3. embedding + the 24 blocks over the n rows in scratch (the prefill's kernels at n rows), K/V into the slots (kv_admit)
//   4. rows_admit_kernel: the slots' state of a fresh generation
//   5. the head on the n rows' last position in scratch, logits to the slots, one sampler launch (grid 1) per admitted row
//   6. a table generation: the row table for the new occupancy (a class that was not present re-captures the step)
// text_ids [n][L] with L the generation's own text length (stop ids pad a shorter text, which is left-padded as in the prefill).
// cond [cond_rows][latents, D], cond_rows 1 (shared) or n.  rows_host [n] (optional): in a table generation the rows' settings
// (missing: greedy with the generation's penalty); in a scalar generation only its own settings are accepted.  uniforms_host
// [n][max_gen]: the draws of a sampled row.  forced_host [n][n_forced] (optional, -1 free): needs a generation started with forced
// tokens.  Everything is refused before anything is changed.
int Engine::gpt_admit_rows(const float* cond_dev, int cond_rows, const int32_t* text_ids, int n, int L, const RowSampling* rows_host,
                           const float* uniforms_host, const int32_t* forced_host, int n_forced, int32_t* slots_out, hipStream_t s) {
  DecodeState& d = ds;
  if (!d.active) {
    set_error("gpt_admit_rows: no active generation");
    return E_STATE;
  }
  const itts_config& c = cfg;
  const int D = c.model_dim, nl = c.cond_latents, V = c.number_mel_codes, B = d.B, mg = d.max_gen;
  ITTS_REQUIRE(cond_dev && text_ids && n >= 1 && L >= 1 && (cond_rows == 1 || cond_rows == n), "gpt_admit_rows: bad arguments");
  ITTS_REQUIRE(n <= ROWS_MOVE_MAX, "gpt_admit_rows: more than 128 rows in one admission");
  if (d.nb > 1) {  // opt-in on its own (gpt_set_admit_beams; ITTS_ADMIT_BEAMS, read per call, overrides the setter both ways)
    const char* ab = getenv("ITTS_ADMIT_BEAMS");
    if (ab ? atoi(ab) != 0 : d.admit_beams != 0) {
      ITTS_REQUIRE(!rows_host && !forced_host, "gpt_admit_rows: under beams there are no per-row settings and no forced tokens (rows_host and forced_host must be null)");
      return admit_beam_groups(cond_dev, cond_rows, text_ids, n, L, uniforms_host, slots_out, s);
    }
  }
  ITTS_REQUIRE(d.nb == 1, "gpt_admit_rows: rows cannot be admitted under beams");
  ITTS_REQUIRE(!(d.typical_mass > 0.f), "gpt_admit_rows: rows cannot be admitted with typical filtering");
  ITTS_REQUIRE(!d.host_sample, "gpt_admit_rows: rows cannot be admitted with host sampling");
  static const bool env_fuse = getenv("ITTS_FUSE_QKV_ATTN") != nullptr && atoi(getenv("ITTS_FUSE_QKV_ATTN")) != 0;
  ITTS_REQUIRE(!((d.fuse || env_fuse) && !d.fuse_failed), "gpt_admit_rows: rows cannot be admitted with the fused qkv + attention launch");
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  ITTS_REQUIRE(!engine_usable(), "gpt_admit_rows: rows cannot be admitted while the step runs on the persistent engine (<= 6 rows)");
  ITTS_REQUIRE(d.B == d.Bcache, "gpt_admit_rows: rows cannot be admitted after a retirement");
  ITTS_REQUIRE(d.input_n == 0, "gpt_admit_rows: rows cannot be admitted into a generation with `input_tokens`");
  ITTS_REQUIRE(L == d.prefix - nl - 2, "gpt_admit_rows: L must be the text length of the running generation");
  // what kv_admit would refuse inside the launch sequence, asked here - before anything is changed (its slots come from admit_plan:
  // distinct, inside [0, B); the scratch and the per-layer cache offsets are 256-byte aligned)
  ITTS_REQUIRE((D / c.heads) % (d.ct == F32 ? 4 : 8) == 0 && d.Bcache <= 65536 && ((uintptr_t)d.kc | (uintptr_t)d.vc) % 16 == 0,
               "gpt_admit_rows: the cache write needs a head dim that is a multiple of 8 (4: fp32 cache) and at most 65536 cache rows");
  ITTS_REQUIRE(!forced_host || (d.use_forced && n_forced >= 1 && n_forced <= mg),
               "gpt_admit_rows: forced tokens need a generation started with forced tokens, and 1 <= n_forced <= max_gen");
  // the text rows, stripped and left-padded as gpt_prefill does
  const int sp = d.prefix, S0 = sp + 1;
  std::vector<RowDesc> rd((size_t)n * S0);
  std::vector<int> kvs(n);
  for (int b = 0; b < n; ++b) {
    std::vector<int> ids;
    for (int i = 0; i < L; ++i) {
      const int t = text_ids[(size_t)b * L + i];
      if (t != c.start_text_token && t != c.stop_text_token) {
        ITTS_REQUIRE(t >= 0 && t <= c.number_text_tokens, "gpt_admit_rows: text id out of range");
        ids.push_back(t);
      }
    }
    const int nt = (int)ids.size(), pad = L - nt;
    kvs[b] = pad;
    RowDesc* r = rd.data() + (size_t)b * S0;
    int k = 0;
    for (int i = 0; i < pad; ++i) r[k++] = {0, 0, 0, 0};
    for (int i = 0; i < nl; ++i) r[k++] = {1, (cond_rows == n && n > 1 ? b * nl : 0) + i, 0, 0};
    r[k++] = {2, c.start_text_token, 0, 0};
    for (int i = 0; i < nt; ++i) r[k++] = {2, ids[i], i + 1, 0};
    r[k++] = {2, c.stop_text_token, nt + 1, 0};
    r[k++] = {3, c.start_mel_token, 0, 0};
  }
  // the rows' settings and classes
  std::vector<RowSampling> rs(n);
  std::vector<int> cls(n);
  bool draws = false;
  for (int b = 0; b < n; ++b) {
    RowSampling r = rows_host ? rows_host[b] : RowSampling{d.rows_active ? 0 : d.do_sample, d.top_k, d.top_p, d.temperature, d.penalty};
    ITTS_REQUIRE(r.mode == 0 || r.mode == 1, "gpt_admit_rows: mode is 0 (greedy) or 1 (sample)");
    ITTS_REQUIRE(r.top_p > 0.f && r.top_p <= 1.f && r.temperature > 0.f && r.penalty > 0.f,
                 "gpt_admit_rows: need 0 < top_p <= 1, temperature > 0 and penalty > 0");
    r.top_k = r.top_k < 1 ? 0 : r.top_k;
    if (!d.rows_active)
      ITTS_REQUIRE(r.mode == d.do_sample && r.penalty == d.penalty &&
                       (r.mode == 0 || (r.top_k == d.top_k && r.top_p == d.top_p && r.temperature == d.temperature)),
                   "gpt_admit_rows: a scalar generation admits only rows that carry its own settings (start a table generation: itts_gpt_keep_row_table)");
    cls[b] = row_class(r.mode, r.top_k);
    if (cls[b] == ROWCLS_NARROW) ITTS_REQUIRE((size_t)V * 4 <= 60 * 1024, "gpt_admit_rows: a row with 1 <= top_k <= 128 needs number_mel_codes <= 15360");
    if (cls[b] == ROWCLS_WIDE) ITTS_REQUIRE(V <= 16384, "gpt_admit_rows: a sampled row with top_k outside [1, 128] needs number_mel_codes <= 16384");
    draws = draws || r.mode == 1;
    rs[b] = r;
  }
  ITTS_REQUIRE(!draws || uniforms_host, "gpt_admit_rows: uniforms missing for a sampled row");
  ITTS_REQUIRE(!draws || (d.have_uniforms && d.uniforms && d.uniforms_cap >= (size_t)mg * B),
               "gpt_admit_rows: this generation has no room for draws (start it with the row table kept: itts_gpt_keep_row_table)");
  if (forced_host)
    for (long i = 0; i < (long)n * n_forced; ++i)
      ITTS_REQUIRE(forced_host[i] >= -1 && forced_host[i] < V, "gpt_admit_rows: forced token id out of range");
  // 1. the slots
  std::vector<int> unf(B), lens(B), slots(n);
  ITTS_HIP_CHECK(hipMemcpyAsync(unf.data(), d.unfinished, (size_t)B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(lens.data(), d.len, (size_t)B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  int n_free = 0;
  ITTS_TRY(admit_plan(unf.data(), lens.data(), B, mg, n, slots.data(), &n_free));
  ITTS_REQUIRE(n_free >= n, "gpt_admit_rows: fewer finished slots than rows to admit");
  for (int i = 0; i < n; ++i) ITTS_REQUIRE(lens[slots[i]] >= 0 && lens[slots[i]] <= mg, "gpt_admit_rows: decode state out of range");
  if (std::find(cls.begin(), cls.end(), (int)ROWCLS_WIDE) != cls.end()) ITTS_TRY(sampler_wide_prepare());  // (outside any capture)
  // ---- nothing was changed up to here ----
  {  // the leaving rows' codes and last logits, by original row
    std::vector<int32_t> ids((size_t)n * mg);
    std::vector<float> lg((size_t)n * V);
    for (int i = 0; i < n; ++i) {
      ITTS_HIP_CHECK(hipMemcpyAsync(ids.data() + (size_t)i * mg, d.ids + (size_t)slots[i] * mg, (size_t)mg * 4, hipMemcpyDeviceToHost, s));
      ITTS_HIP_CHECK(hipMemcpyAsync(lg.data() + (size_t)i * V, d.logits + (size_t)slots[i] * V, (size_t)V * 4, hipMemcpyDeviceToHost, s));
    }
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
    if (d.orig.empty()) {
      d.orig.resize(B);
      for (int b = 0; b < B; ++b) d.orig[b] = b;
      d.retired.assign((size_t)d.B0, 0);
      d.ret_codes.assign((size_t)d.B0 * mg, c.stop_mel_token);
      d.ret_logits.assign((size_t)d.B0 * V, 0.f);
    }
    if (!d.admitted) {  // the generation takes its own copy of the per-row settings and the draws, by original row
      if (d.rows_active) d.adm_rows = row_table;
      if (d.do_sample || d.rows_active) {
        d.adm_uniforms.assign((size_t)d.B0 * mg, 0.f);
        if (sample_uniforms.size() >= (size_t)mg * d.B0)
          for (int q = 0; q < mg; ++q)
            for (int b = 0; b < d.B0; ++b) d.adm_uniforms[(size_t)b * mg + q] = sample_uniforms[(size_t)q * d.B0 + b];
      }
    }
    for (int i = 0; i < n; ++i) {
      const size_t r = (size_t)d.orig[slots[i]];
      d.retired[r] = 1;
      std::fill(d.ret_codes.begin() + r * mg, d.ret_codes.begin() + (r + 1) * mg, c.stop_mel_token);
      std::memcpy(d.ret_codes.data() + r * mg, ids.data() + (size_t)i * mg, (size_t)lens[slots[i]] * 4);  // stop behind them
      std::memcpy(d.ret_logits.data() + r * V, lg.data() + (size_t)i * V, (size_t)V * 4);
    }
  }
  // 2. the new original rows
  const int first = d.B0;
  d.B0 += n;
  d.admitted += n;
  d.retired.resize((size_t)d.B0, 0);
  d.ret_codes.resize((size_t)d.B0 * mg, c.stop_mel_token);
  d.ret_logits.resize((size_t)d.B0 * V, 0.f);
  for (int i = 0; i < n; ++i) d.orig[slots[i]] = first + i;
  if (d.rows_active) d.adm_rows.insert(d.adm_rows.end(), rs.begin(), rs.end());
  if (d.do_sample || d.rows_active) {
    d.adm_uniforms.resize((size_t)d.B0 * mg, 0.f);
    for (int i = 0; i < n; ++i)
      if (rs[i].mode == 1) std::memcpy(d.adm_uniforms.data() + (size_t)(first + i) * mg, uniforms_host + (size_t)i * mg, (size_t)mg * 4);
  }
  std::vector<int32_t> ftab;
  if (forced_host) {
    ftab.assign((size_t)n * mg, -1);
    for (int i = 0; i < n; ++i) std::memcpy(ftab.data() + (size_t)i * mg, forced_host + (size_t)i * n_forced, (size_t)n_forced * 4);
  }
  // 6 (first: the samplers of step 5 read the slot's own entry)
  if (d.rows_active) ITTS_TRY(upload_row_table(s));
  d.pend_split = 0;
  const int nr = (n + 15) / 16 * 16;  // the batched head keeps its bf16 rows in 16-row tiles
  auto body = [&]() -> int {
    RowDesc* rd_dev = (RowDesc*)alloc(rd.size() * sizeof(RowDesc));
    int* kvs_dev = (int*)alloc((size_t)n * 4);
    float* h = (float*)alloc((size_t)n * S0 * D * 4);
    float* h_last = (float*)alloc((size_t)nr * D * 4);
    float* hn = (float*)alloc((size_t)nr * D * 4);
    float* lg = (float*)alloc((size_t)nr * V * 4);
    int* f_dev = forced_host ? (int*)alloc(ftab.size() * 4) : nullptr;
    float* u_dev = draws ? (float*)alloc((size_t)n * mg * 4) : nullptr;
    if (!dry) {
      ITTS_HIP_CHECK(hipMemcpyAsync(rd_dev, rd.data(), rd.size() * sizeof(RowDesc), hipMemcpyHostToDevice, s));
      ITTS_HIP_CHECK(hipMemcpyAsync(kvs_dev, kvs.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
      if (f_dev) ITTS_HIP_CHECK(hipMemcpyAsync(f_dev, ftab.data(), ftab.size() * 4, hipMemcpyHostToDevice, s));
      if (u_dev) ITTS_HIP_CHECK(hipMemcpyAsync(u_dev, d.adm_uniforms.data() + (size_t)first * mg, (size_t)n * mg * 4, hipMemcpyHostToDevice, s));
      if (adt == F32)
        hipLaunchKernelGGL(gpt_embed_rows_kernel<float>, dim3(n * S0), dim3(256), 0, s, h, rd_dev, cond_dev,
                           (const float*)gpt.text_emb, (const float*)gpt.text_pos, (const float*)gpt.mel_emb,
                           (const float*)gpt.mel_pos, D);
      else
        hipLaunchKernelGGL(gpt_embed_rows_kernel<bf16_t>, dim3(n * S0), dim3(256), 0, s, h, rd_dev, cond_dev,
                           (const bf16_t*)gpt.text_emb, (const bf16_t*)gpt.text_pos, (const bf16_t*)gpt.mel_emb,
                           (const bf16_t*)gpt.mel_pos, D);
      ITTS_HIP_CHECK(hipGetLastError());
    }
    // 3.
    ITTS_TRY(gpt_layers_full(h, n, S0, kvs_dev, true, s, slots.data()));
    if (dry) return OK;
    // 4.
    RowsAdmitArgs ra;
    ra.seen = d.seen;
    ra.unfinished = d.unfinished;
    ra.cur_tok = d.cur_tok;
    ra.len = d.len;
    ra.kv_start = d.kv_start;
    ra.ids = d.ids;
    ra.forced = d.forced;
    ra.uniforms = u_dev ? d.uniforms : nullptr;
    ra.forced_src = f_dev;
    ra.uniforms_src = u_dev;
    ra.n = n;
    ra.B = B;
    ra.V = V;
    ra.max_gen = mg;
    ra.fake_id = 1;
    ra.start_tok = c.start_mel_token;
    ra.stop = c.stop_mel_token;
    ITTS_TRY(rows_admit(ra, slots.data(), kvs.data(), s));
    // 5. (the sampler writes the next step's input row h[slot] itself)
    ITTS_TRY(copy_rows(h_last, D, h + (size_t)(S0 - 1) * D, S0 * D, n, D, F32, s));
    ITTS_TRY(head_rows(h_last, hn, lg, n, s));
    SamplerArgs sa = greedy_sampler_args(d.logits, false);
    if (d.rows_active) sa.rows = d.rows;
    for (int i = 0; i < n; ++i) {
      ITTS_HIP_CHECK(hipMemcpyAsync(d.logits + (size_t)slots[i] * V, lg + (size_t)i * V, (size_t)V * 4, hipMemcpyDeviceToDevice, s));
      ITTS_TRY(sampler_slot_step(sa, slots[i], cls[i], s));
    }
    return OK;
  };
  ITTS_TRY(two_pass(body, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));  // rd / kvs / the tables are host buffers of this call
  if (slots_out)
    for (int i = 0; i < n; ++i) slots_out[i] = slots[i];
  return OK;
}

int Engine::gpt_set_admit_beams(int on) {
  ds.admit_beams = on != 0;
  return OK;
}

// The beam branch of gpt_admit_rows (opt-in, gpt_set_admit_beams): n finished batch items of a running beam generation take n new
// requests, nb rows each.  Why the device allows it: beam_cand_kernel, beam_select_kernel and the whole-vocabulary pair take their
// step from the item's own state (k = len[item * nb]), with it the ping-pong half (k & 1) and the draws (uniforms[(k * items +
// item) * 2 nb + j]); decode_attn2_kernel<ANC> takes its ancestry half from len[row] & 1.  So a group with len = 0, the beam state
// of a fresh generation and its prefix in its rows' cache is a fresh generation that happens to sit beside older ones.  What the
// host assumed - one common step, one live half (beam_read_state, beam_finalize_item, retire_beam_groups) - reads per item from
// the first admission on (DecodeState::admitted).
//   1. every refusal; synchronise; the n lowest finished items (admit_plan over per-item flags: done, or len >= max_gen)
//   2. the leaving items are finalised at their own step (beam_finalize_item) and kept, with their rows' last logits, by original
//      item / row; the new items become original items items0, items0 + 1, .. and their draws join the host copy by original item
//   3. embedding + the blocks over the n * nb rows in scratch, expanded as gpt_prefill expands them (the rows and kernels of a
//      fresh generation of those items), K/V into rows item * nb + q (kv_admit)
//   4. rows_admit_kernel on those rows, beam_admit_kernel on the items
//   5. the head on the rows' last position in scratch, logits to their rows, beam_item_step per admitted item: the running groups
//      are neither stepped nor touched, no pointer of the captured step changes
int Engine::admit_beam_groups(const float* cond_dev, int cond_rows, const int32_t* text_ids, int n, int L, const float* uniforms_host,
                              int32_t* items_out, hipStream_t s) {
  DecodeState& d = ds;
  const itts_config& c = cfg;
  const int D = c.model_dim, nl = c.cond_latents, V = c.number_mel_codes, B = d.B, mg = d.max_gen;
  const int nb = d.nb, items = B / nb, nd = 2 * nb, nr = n * nb, keep = beam_returns;
  ITTS_REQUIRE(nr <= ROWS_MOVE_MAX, "gpt_admit_rows: more than 128 rows (items * num_beams) in one admission");
  ITTS_REQUIRE(!(d.typical_mass > 0.f), "gpt_admit_rows: beam groups cannot be admitted with typical filtering");
  ITTS_REQUIRE(!d.host_sample, "gpt_admit_rows: beam groups cannot be admitted with host sampling (host-side beam warpers)");
  static const bool env_fuse = getenv("ITTS_FUSE_QKV_ATTN") != nullptr && atoi(getenv("ITTS_FUSE_QKV_ATTN")) != 0;
  ITTS_REQUIRE(!((d.fuse || env_fuse) && !d.fuse_failed), "gpt_admit_rows: beam groups cannot be admitted with the fused qkv + attention launch");
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  ITTS_REQUIRE(!engine_usable(), "gpt_admit_rows: beam groups cannot be admitted while the step runs on the persistent engine (<= 6 rows)");
  ITTS_REQUIRE(d.B == d.Bcache, "gpt_admit_rows: beam groups cannot be admitted after a retirement");
  ITTS_REQUIRE(d.input_n == 0 && !d.use_forced, "gpt_admit_rows: beam groups cannot be admitted into a generation with `input_tokens`");
  ITTS_REQUIRE(L == d.prefix - nl - 2, "gpt_admit_rows: L must be the text length of the running generation");
  ITTS_REQUIRE((D / c.heads) % (d.ct == F32 ? 4 : 8) == 0 && d.Bcache <= 65536 && ((uintptr_t)d.kc | (uintptr_t)d.vc) % 16 == 0,
               "gpt_admit_rows: the cache write needs a head dim that is a multiple of 8 (4: fp32 cache) and at most 65536 cache rows");
  ITTS_REQUIRE(B % nb == 0 && d.B0 % nb == 0 && d.Smax % 16 == 0 && d.beam_ids && d.anc, "gpt_admit_rows: beam state out of range");
  ITTS_REQUIRE(keep >= 1 && keep <= nb && (d.orig.empty() || keep == d.ret_keep), "gpt_admit_rows: num_return_sequences changed inside a generation");
  const bool draws = d.beam_sample != 0;
  const bool wide = draws && (d.top_k < 1 || d.top_k > BEAM_MAX_CAND);
  const size_t items0 = (size_t)d.B0 / nb;
  ITTS_REQUIRE(!draws || uniforms_host, "gpt_admit_rows: uniforms missing for beam_sample");
  ITTS_REQUIRE(!draws || (d.uniforms && d.uniforms_cap >= (size_t)mg * items * nd &&
                          (d.admitted ? d.adm_uniforms.size() == items0 * mg * nd : sample_uniforms.size() >= items0 * mg * nd)),
               "gpt_admit_rows: the uniforms of this generation are gone");
  ITTS_REQUIRE(!wide || (d.wide_valid && d.wide.sc), "gpt_admit_rows: the whole-vocabulary beam sampler's scratch is missing");
  // the text rows, stripped, left-padded and repeated per beam as gpt_prefill does
  const int sp = d.prefix, S0 = sp + 1;
  std::vector<RowDesc> rd((size_t)nr * S0);
  std::vector<int> kvs(nr);
  for (int b = 0; b < nr; ++b) {
    const int it = b / nb;
    std::vector<int> ids;
    for (int i = 0; i < L; ++i) {
      const int t = text_ids[(size_t)it * L + i];
      if (t != c.start_text_token && t != c.stop_text_token) {
        ITTS_REQUIRE(t >= 0 && t <= c.number_text_tokens, "gpt_admit_rows: text id out of range");
        ids.push_back(t);
      }
    }
    const int nt = (int)ids.size(), pad = L - nt;
    kvs[b] = pad;
    RowDesc* r = rd.data() + (size_t)b * S0;
    int k = 0;
    for (int i = 0; i < pad; ++i) r[k++] = {0, 0, 0, 0};
    for (int i = 0; i < nl; ++i) r[k++] = {1, (cond_rows == n && n > 1 ? it * nl : 0) + i, 0, 0};
    r[k++] = {2, c.start_text_token, 0, 0};
    for (int i = 0; i < nt; ++i) r[k++] = {2, ids[i], i + 1, 0};
    r[k++] = {2, c.stop_text_token, nt + 1, 0};
    r[k++] = {3, c.start_mel_token, 0, 0};
  }
  // 1. the items
  std::vector<int> unf(B), lens(B), done(items), iunf(items), ilen(items), took(n), rows(nr);
  ITTS_HIP_CHECK(hipMemcpyAsync(unf.data(), d.unfinished, (size_t)B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(lens.data(), d.len, (size_t)B * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipMemcpyAsync(done.data(), d.beam_done, (size_t)items * 4, hipMemcpyDeviceToHost, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  for (int b = 0; b < B; ++b)
    ITTS_REQUIRE(lens[b] >= 0 && lens[b] <= mg && lens[b] == lens[b - b % nb], "gpt_admit_rows: decode state out of range");
  for (int g = 0; g < items; ++g) {
    iunf[g] = !done[g];
    ilen[g] = lens[g * nb];
  }
  int n_free = 0;
  ITTS_TRY(admit_plan(iunf.data(), ilen.data(), items, mg, n, took.data(), &n_free));
  ITTS_REQUIRE(n_free >= n, "gpt_admit_rows: fewer finished items than items to admit");
  for (int i = 0; i < nr; ++i) rows[i] = took[i / nb] * nb + i % nb;
  // 2. the leaving items: finalised at their own step, before anything is changed
  std::vector<int32_t> fin((size_t)n * keep * mg);
  std::vector<float> lg_old((size_t)nr * V);
  {
    BeamHost st;
    ITTS_TRY(beam_read_state(st, s));
    for (int i = 0; i < n; ++i) {
      ITTS_TRY(beam_finalize_item(st, took[i], fin.data() + (size_t)i * keep * mg));
      ITTS_HIP_CHECK(hipMemcpyAsync(lg_old.data() + (size_t)i * nb * V, d.logits + (size_t)took[i] * nb * V, (size_t)nb * V * 4, hipMemcpyDeviceToHost, s));
    }
    ITTS_HIP_CHECK(hipStreamSynchronize(s));
  }
  // ---- nothing was changed up to here ----
  if (d.orig.empty()) {
    d.orig.resize(B);
    for (int b = 0; b < B; ++b) d.orig[b] = b;
    d.retired.assign((size_t)d.B0, 0);
    d.ret_keep = keep;
    d.ret_codes.assign(items0 * keep * mg, c.stop_mel_token);
    d.ret_logits.assign((size_t)d.B0 * V, 0.f);
  }
  if (!d.admitted && draws) {  // the generation takes its own copy of the draws, by original item
    d.adm_uniforms.resize(items0 * mg * nd);
    for (int q = 0; q < mg; ++q)
      for (size_t it = 0; it < items0; ++it)
        std::memcpy(d.adm_uniforms.data() + (it * mg + q) * nd, sample_uniforms.data() + ((size_t)q * items0 + it) * nd, (size_t)nd * 4);
  }
  for (int i = 0; i < n; ++i) {
    const size_t r = (size_t)d.orig[took[i] * nb];  // the group's first original row
    for (int q = 0; q < nb; ++q) d.retired[r + q] = 1;
    std::memcpy(d.ret_codes.data() + r / nb * keep * mg, fin.data() + (size_t)i * keep * mg, (size_t)keep * mg * 4);
    std::memcpy(d.ret_logits.data() + r * V, lg_old.data() + (size_t)i * nb * V, (size_t)nb * V * 4);
  }
  const int first = d.B0;  // the new original rows; original items first / nb ..
  d.B0 += nr;
  d.admitted += nr;
  d.retired.resize((size_t)d.B0, 0);
  d.ret_codes.resize((size_t)d.B0 / nb * keep * mg, c.stop_mel_token);
  d.ret_logits.resize((size_t)d.B0 * V, 0.f);
  for (int i = 0; i < nr; ++i) d.orig[rows[i]] = first + i;
  if (draws) {
    d.adm_uniforms.resize((size_t)d.B0 / nb * mg * nd, 0.f);
    std::memcpy(d.adm_uniforms.data() + (size_t)first / nb * mg * nd, uniforms_host, (size_t)n * mg * nd * 4);
  }
  d.pend_split = 0;
  const int nr16 = (nr + 15) / 16 * 16;  // the batched head keeps its bf16 rows in 16-row tiles
  auto body = [&]() -> int {
    RowDesc* rd_dev = (RowDesc*)alloc(rd.size() * sizeof(RowDesc));
    int* kvs_dev = (int*)alloc((size_t)nr * 4);
    float* h = (float*)alloc((size_t)nr * S0 * D * 4);
    float* h_last = (float*)alloc((size_t)nr16 * D * 4);
    float* hn = (float*)alloc((size_t)nr16 * D * 4);
    float* lg = (float*)alloc((size_t)nr16 * V * 4);
    float* u_dev = draws ? (float*)alloc((size_t)n * mg * nd * 4) : nullptr;
    if (!dry) {
      ITTS_HIP_CHECK(hipMemcpyAsync(rd_dev, rd.data(), rd.size() * sizeof(RowDesc), hipMemcpyHostToDevice, s));
      ITTS_HIP_CHECK(hipMemcpyAsync(kvs_dev, kvs.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s));
      if (u_dev) ITTS_HIP_CHECK(hipMemcpyAsync(u_dev, d.adm_uniforms.data() + (size_t)first / nb * mg * nd, (size_t)n * mg * nd * 4, hipMemcpyHostToDevice, s));
      if (adt == F32)
        hipLaunchKernelGGL(gpt_embed_rows_kernel<float>, dim3(nr * S0), dim3(256), 0, s, h, rd_dev, cond_dev,
                           (const float*)gpt.text_emb, (const float*)gpt.text_pos, (const float*)gpt.mel_emb,
                           (const float*)gpt.mel_pos, D);
      else
        hipLaunchKernelGGL(gpt_embed_rows_kernel<bf16_t>, dim3(nr * S0), dim3(256), 0, s, h, rd_dev, cond_dev,
                           (const bf16_t*)gpt.text_emb, (const bf16_t*)gpt.text_pos, (const bf16_t*)gpt.mel_emb,
                           (const bf16_t*)gpt.mel_pos, D);
      ITTS_HIP_CHECK(hipGetLastError());
    }
    // 3.
    ITTS_TRY(gpt_layers_full(h, nr, S0, kvs_dev, true, s, rows.data()));
    if (dry) return OK;
    // 4.
    RowsAdmitArgs ra;
    ra.seen = d.seen;
    ra.unfinished = d.unfinished;
    ra.cur_tok = d.cur_tok;
    ra.len = d.len;
    ra.kv_start = d.kv_start;
    ra.ids = d.ids;
    ra.n = nr;
    ra.B = B;
    ra.V = V;
    ra.max_gen = mg;
    ra.fake_id = 1;
    ra.start_tok = c.start_mel_token;
    ra.stop = c.stop_mel_token;
    ITTS_TRY(rows_admit(ra, rows.data(), kvs.data(), s));
    BeamAdmitArgs bg;
    bg.beam_scores = d.beam_scores;
    bg.anc = d.anc;
    bg.hyp_order = d.hyp_order;
    bg.hyp_n = d.hyp_n;
    bg.hyp_worst = d.hyp_worst;
    bg.hyp_counter = d.hyp_counter;
    bg.done = d.beam_done;
    bg.uniforms = u_dev ? d.uniforms : nullptr;
    bg.uniforms_src = u_dev;
    bg.n = n;
    bg.nb = nb;
    bg.items = items;
    bg.Smax = d.Smax;
    bg.max_gen = mg;
    bg.do_sample = d.beam_sample;
    ITTS_TRY(beam_admit(bg, took.data(), s));
    // 5. (beam_select_kernel writes the next step's input rows h[item * nb ..] itself)
    ITTS_TRY(copy_rows(h_last, D, h + (size_t)(S0 - 1) * D, S0 * D, nr, D, F32, s));
    ITTS_TRY(head_rows(h_last, hn, lg, nr, s));
    const BeamArgs ba = beam_args(d.logits, false);
    for (int i = 0; i < n; ++i) {
      ITTS_HIP_CHECK(hipMemcpyAsync(d.logits + (size_t)took[i] * nb * V, lg + (size_t)i * nb * V, (size_t)nb * V * 4, hipMemcpyDeviceToDevice, s));
      ITTS_TRY(beam_item_step(ba, took[i], s, wide ? &d.wide : nullptr));
    }
    return OK;
  };
  ITTS_TRY(two_pass(body, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));  // rd / kvs are host buffers of this call
  if (items_out)
    for (int i = 0; i < n; ++i) items_out[i] = took[i];
  return OK;
}

// UnifiedVoice.forward(return_latent=True) for one or more sentences in ONE pass.  The reference runs it at batch 1
// per sentence (infer.py:194-200); sentences are independent, so several are stacked here as left-padded rows
// ([pad.., cond, text, mel] with the pad keys masked exactly like prepare_gpt_inputs' left padding), which fills the
// MFMA tiles better without changing any row's result.  out = concatenated [sum T_i, D] latents in the engine dtype.
int Engine::gpt_latent_batch(const float* cond_dev, const int32_t* text_ids, const int* Ls, const int32_t* codes,
                             const int* Ts, int nseq, void* latent_out, hipStream_t s, const int32_t* cond_index, int n_cond) {
  if (!finalized || !gpt.ok) {
    set_error("gpt_latent: GPT weights not bound");
    return E_STATE;
  }
  const itts_config& c = cfg;
  ITTS_REQUIRE(cond_dev && text_ids && codes && latent_out && Ls && Ts && nseq > 0, "gpt_latent: bad arguments");
  const int D = c.model_dim, nl = c.cond_latents;
  int Smax = 0;
  long Ttot = 0;
  for (int i = 0; i < nseq; ++i) {
    ITTS_REQUIRE(Ls[i] > 0 && Ts[i] > 0, "gpt_latent: empty sentence");
    ITTS_REQUIRE(Ls[i] + 2 <= c.max_text_tokens + 2 && Ts[i] + 2 <= c.max_mel_tokens + 3, "gpt_latent: sequence too long");
    Smax = std::max(Smax, nl + Ls[i] + 2 + Ts[i] + 2);
    Ttot += Ts[i];
  }
  std::vector<RowDesc> rd((size_t)nseq * Smax);
  std::vector<int> kvs(nseq), mel_row(nseq);
  long to = 0, co = 0;
  for (int b = 0; b < nseq; ++b) {
    const int L = Ls[b], T = Ts[b];
    const int S = nl + L + 2 + T + 2, pad = Smax - S;
    kvs[b] = pad;
    RowDesc* r = rd.data() + (size_t)b * Smax;
    int k = 0;
    for (int i = 0; i < pad; ++i) r[k++] = {0, 0, 0, 0};
    // conditioning latents: one block for every sentence, or block cond_index[b] of cond [n_cond][nl, D] (several voices in one pass)
    const int cb = cond_index ? cond_index[b] : 0;
    ITTS_REQUIRE(cb >= 0 && cb < n_cond, "gpt_latent: conditioning index outside [0, n_cond)");
    for (int i = 0; i < nl; ++i) r[k++] = {1, cb * nl + i, 0, 0};
    r[k++] = {2, c.start_text_token, 0, 0};
    for (int i = 0; i < L; ++i) {
      const int t = text_ids[to + i];
      ITTS_REQUIRE(t >= 0 && t <= c.number_text_tokens, "gpt_latent: text id out of range");
      r[k++] = {2, t, i + 1, 0};
    }
    r[k++] = {2, c.stop_text_token, L + 1, 0};
    mel_row[b] = b * Smax + k;  // first mel row (the start token); model.py:578 keeps rows [0, T) of the mel part
    r[k++] = {3, c.start_mel_token, 0, 0};
    for (int i = 0; i < T; ++i) {
      const int m = codes[co + i];
      ITTS_REQUIRE(m >= 0 && m < c.number_mel_codes, "gpt_latent: mel code out of range");
      r[k++] = {3, m, i + 1, 0};
    }
    r[k++] = {3, c.stop_mel_token, T + 1, 0};
    to += L;
    co += T;
  }
  auto body = [&]() -> int {
    RowDesc* rd_dev = (RowDesc*)alloc(rd.size() * sizeof(RowDesc));
    int* kvs_dev = (int*)alloc((size_t)nseq * 4);
    float* h = (float*)alloc((size_t)nseq * Smax * D * 4);
    float* hn = (float*)alloc((size_t)Ttot * D * 4);
    if (!dry) {
      ITTS_HIP_CHECK(hipMemcpyAsync(rd_dev, rd.data(), rd.size() * sizeof(RowDesc), hipMemcpyHostToDevice, s));
      ITTS_HIP_CHECK(hipMemcpyAsync(kvs_dev, kvs.data(), (size_t)nseq * 4, hipMemcpyHostToDevice, s));
      if (adt == F32)
        hipLaunchKernelGGL(gpt_embed_rows_kernel<float>, dim3(nseq * Smax), dim3(256), 0, s, h, rd_dev, cond_dev,
                           (const float*)gpt.text_emb, (const float*)gpt.text_pos, (const float*)gpt.mel_emb,
                           (const float*)gpt.mel_pos, D);
      else
        hipLaunchKernelGGL(gpt_embed_rows_kernel<bf16_t>, dim3(nseq * Smax), dim3(256), 0, s, h, rd_dev, cond_dev,
                           (const bf16_t*)gpt.text_emb, (const bf16_t*)gpt.text_pos, (const bf16_t*)gpt.mel_emb,
                           (const bf16_t*)gpt.mel_pos, D);
      ITTS_HIP_CHECK(hipGetLastError());
    }
    ITTS_TRY(gpt_layers_full(h, nseq, Smax, nseq > 1 ? kvs_dev : nullptr, false, s));
    long off = 0;
    for (int b = 0; b < nseq; ++b) {
      K(double_ln(hn + off * D, h + (size_t)mel_row[b] * D, gpt.ln_f.g, gpt.ln_f.b, gpt.final_norm.g, gpt.final_norm.b,
                  Ts[b], D, 1e-5f, s));
      off += Ts[b];
    }
    K(cast_copy(latent_out, adt, hn, F32, Ttot * D, s));
    return OK;
  };
  ITTS_TRY(two_pass(body, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));  // rd / kvs are host buffers
  return OK;
}

// The latent pass on PACKED rows: [cond, text, mel] of every sentence back to back, no pad rows (RowDesc kinds 1 - 3 only).  Each
// sentence is tiled by the attention from its own key 0 (attention_varlen.hip), the GEMMs run without a K split on a kernel family
// that does not depend on the row count (PackedPass), LayerNorm and the embedding are row-wise: a sentence's latent has the same
// bits alone, with any companions, in any order.  Same interface and output as gpt_latent_batch; nseq <= VARLEN_MAX_SEQ.
int Engine::gpt_latent_packed(const float* cond_dev, const int32_t* text_ids, const int* Ls, const int32_t* codes,
                              const int* Ts, int nseq, void* latent_out, hipStream_t s, const int32_t* cond_index, int n_cond) {
  if (!finalized || !gpt.ok) {
    set_error("gpt_latent_packed: GPT weights not bound");
    return E_STATE;
  }
  const itts_config& c = cfg;
  ITTS_REQUIRE(cond_dev && text_ids && codes && latent_out && Ls && Ts, "gpt_latent_packed: null pointer");
  ITTS_REQUIRE(nseq >= 1 && nseq <= VARLEN_MAX_SEQ, "gpt_latent_packed: 1 <= nseq <= 128");
  ITTS_REQUIRE(n_cond >= 1, "gpt_latent_packed: n_cond >= 1");
  const int D = c.model_dim, nl = c.cond_latents;
  // the matrix-core GEMM of the pinned selector needs 16 rows: every sentence has nl + 6 or more, alone as in company
  ITTS_REQUIRE(adt == F32 || force_simple || nl + 6 >= 16, "gpt_latent_packed: a 16-bit engine needs cond_latents >= 10");
  VarlenArgs seqs;
  seqs.nseq = nseq;
  long Ttot = 0, Mtot = 0;
  for (int i = 0; i < nseq; ++i) {
    ITTS_REQUIRE(Ls[i] > 0 && Ts[i] > 0, "gpt_latent_packed: empty sentence");
    ITTS_REQUIRE(Ls[i] + 2 <= c.max_text_tokens + 2 && Ts[i] + 2 <= c.max_mel_tokens + 3, "gpt_latent_packed: sequence too long");
    const int cb = cond_index ? cond_index[i] : 0;
    ITTS_REQUIRE(cb >= 0 && cb < n_cond, "gpt_latent_packed: conditioning index outside [0, n_cond)");
    seqs.off[i] = (int)Mtot;
    Mtot += nl + Ls[i] + 2 + Ts[i] + 2;
    Ttot += Ts[i];
    ITTS_REQUIRE(Mtot < (1L << 24), "gpt_latent_packed: more than 2^24 rows in one pass");
  }
  seqs.off[nseq] = (int)Mtot;
  std::vector<RowDesc> rd((size_t)Mtot);
  std::vector<int> mel_row(nseq);
  long to = 0, co = 0;
  for (int b = 0; b < nseq; ++b) {
    const int L = Ls[b], T = Ts[b];
    RowDesc* r = rd.data() + seqs.off[b];
    int k = 0;
    const int cb = cond_index ? cond_index[b] : 0;
    for (int i = 0; i < nl; ++i) r[k++] = {1, cb * nl + i, 0, 0};
    r[k++] = {2, c.start_text_token, 0, 0};
    for (int i = 0; i < L; ++i) {
      const int t = text_ids[to + i];
      ITTS_REQUIRE(t >= 0 && t <= c.number_text_tokens, "gpt_latent_packed: text id out of range");
      r[k++] = {2, t, i + 1, 0};
    }
    r[k++] = {2, c.stop_text_token, L + 1, 0};
    mel_row[b] = seqs.off[b] + k;  // first mel row (the start token); model.py:578 keeps rows [0, T) of the mel part
    r[k++] = {3, c.start_mel_token, 0, 0};
    for (int i = 0; i < T; ++i) {
      const int m = codes[co + i];
      ITTS_REQUIRE(m >= 0 && m < c.number_mel_codes, "gpt_latent_packed: mel code out of range");
      r[k++] = {3, m, i + 1, 0};
    }
    r[k++] = {3, c.stop_mel_token, T + 1, 0};
    to += L;
    co += T;
  }
  PackedPass packed(*this);
  auto body = [&]() -> int {
    RowDesc* rd_dev = (RowDesc*)alloc(rd.size() * sizeof(RowDesc));
    float* h = (float*)alloc((size_t)Mtot * D * 4);
    float* hn = (float*)alloc((size_t)Ttot * D * 4);
    if (!dry) {
      ITTS_HIP_CHECK(hipMemcpyAsync(rd_dev, rd.data(), rd.size() * sizeof(RowDesc), hipMemcpyHostToDevice, s));
      if (adt == F32)
        hipLaunchKernelGGL(gpt_embed_rows_kernel<float>, dim3((unsigned)Mtot), dim3(256), 0, s, h, rd_dev, cond_dev,
                           (const float*)gpt.text_emb, (const float*)gpt.text_pos, (const float*)gpt.mel_emb,
                           (const float*)gpt.mel_pos, D);
      else
        hipLaunchKernelGGL(gpt_embed_rows_kernel<bf16_t>, dim3((unsigned)Mtot), dim3(256), 0, s, h, rd_dev, cond_dev,
                           (const bf16_t*)gpt.text_emb, (const bf16_t*)gpt.text_pos, (const bf16_t*)gpt.mel_emb,
                           (const bf16_t*)gpt.mel_pos, D);
      ITTS_HIP_CHECK(hipGetLastError());
    }
    ITTS_TRY(gpt_layers_packed(h, seqs, s));
    long off = 0;
    for (int b = 0; b < nseq; ++b) {
      K(double_ln(hn + off * D, h + (size_t)mel_row[b] * D, gpt.ln_f.g, gpt.ln_f.b, gpt.final_norm.g, gpt.final_norm.b,
                  Ts[b], D, 1e-5f, s));
      off += Ts[b];
    }
    K(cast_copy(latent_out, adt, hn, F32, Ttot * D, s));
    return OK;
  };
  ITTS_TRY(two_pass(body, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));  // rd is a host buffer
  return OK;
}

// ---- the incremental packed latent pass (engine.h LatentStream) ----

// gpt_layers_packed over the chunk's rows alone: every row-wise step is the packed pass's on those rows; each layer's k / v of the new
// rows go to the history (kv_rows_append) and the attention reads the history (attention_append, the family fixed at open)
int Engine::gpt_layers_append(float* h, int M, const AppendArgs& app, hipStream_t s) {
  const itts_config& c = cfg;
  const int D = c.model_dim, H = c.heads, dh = D / H;
  void* xn = alloc((size_t)M * D * es);
  void* qkv = alloc((size_t)M * 3 * D * es);
  void* ctx = alloc((size_t)M * D * es);
  void* act = alloc((size_t)M * 4 * D * es);
  if (!dry) ITTS_HIP_CHECK(hipMemsetAsync(ctx, 0, (size_t)M * D * es, s));  // rows of no sequence: the attention never stores them
  AppendArgs a = app;
  a.q = qkv;
  a.o = ctx;
  a.H = H;
  a.dqk = a.dv = dh;
  a.ldq = 3 * D;
  a.ldk = a.ldv = 2 * D;
  a.ldo = D;
  a.scale = 1.f / std::sqrt((float)dh);
  const size_t layer_bytes = (size_t)lstream.nseq * lstream.cap * 2 * D * es;
  for (int l = 0; l < c.layers; ++l) {
    const GptLayerW& L = gpt.layers[l];
    a.k = (const char*)lstream.hist + l * layer_bytes;
    a.v = (const char*)a.k + (size_t)D * es;
    ITTS_TRY(ln(xn, adt, h, F32, L.ln1, M, D, s));
    ITTS_TRY(lin(qkv, adt, xn, adt, D, L.attn, M, 3 * D, s));
    K(kv_rows_append(a, (const char*)qkv + (size_t)D * es, (const char*)qkv + (size_t)2 * D * es, 3 * D, D, D, adt, s));
    K(attention_append(a, adt, lstream.kernel, s));
    ITTS_TRY(lin(h, F32, ctx, adt, D, L.proj, M, D, s, ACT_NONE, h, D));
    ITTS_TRY(ln(xn, adt, h, F32, L.ln2, M, D, s));
    ITTS_TRY(lin(act, adt, xn, adt, D, L.fc, M, 4 * D, s, ACT_GELU_NEW));
    ITTS_TRY(lin(h, F32, act, adt, 4 * D, L.proj2, M, D, s, ACT_NONE, h, D));
  }
  return OK;
}

// embedding of the chunk's M rows, the blocks, then ln_f -> final_norm -> cast of out_n[b] rows from chunk row out_row[b] of every
// sequence, contiguously (what gpt_latent_packed does with a sentence's mel rows).  rd_host = nullptr: the sizing run of open.
int Engine::latent_stream_pass(const int* rd_host, int M, const AppendArgs& app, const int* out_row, const int* out_n, long Ttot,
                               void* latent_out, hipStream_t s) {
  const int D = cfg.model_dim;
  PackedPass packed(*this);
  auto body = [&]() -> int {
    RowDesc* rd_dev = (RowDesc*)alloc((size_t)M * sizeof(RowDesc));
    float* h = (float*)alloc((size_t)M * D * 4);
    float* hn = (float*)alloc((size_t)Ttot * D * 4);
    if (!dry) {
      ITTS_HIP_CHECK(hipMemcpyAsync(rd_dev, rd_host, (size_t)M * sizeof(RowDesc), hipMemcpyHostToDevice, s));
      if (adt == F32)
        hipLaunchKernelGGL(gpt_embed_rows_kernel<float>, dim3((unsigned)M), dim3(256), 0, s, h, rd_dev, lstream.cond,
                           (const float*)gpt.text_emb, (const float*)gpt.text_pos, (const float*)gpt.mel_emb,
                           (const float*)gpt.mel_pos, D);
      else
        hipLaunchKernelGGL(gpt_embed_rows_kernel<bf16_t>, dim3((unsigned)M), dim3(256), 0, s, h, rd_dev, lstream.cond,
                           (const bf16_t*)gpt.text_emb, (const bf16_t*)gpt.text_pos, (const bf16_t*)gpt.mel_emb,
                           (const bf16_t*)gpt.mel_pos, D);
      ITTS_HIP_CHECK(hipGetLastError());
    }
    ITTS_TRY(gpt_layers_append(h, M, app, s));
    long off = 0;
    for (int b = 0; b < app.nseq; ++b) {
      if (out_n[b] < 1) continue;
      K(double_ln(hn + off * D, h + (size_t)out_row[b] * D, gpt.ln_f.g, gpt.ln_f.b, gpt.final_norm.g, gpt.final_norm.b, out_n[b], D,
                  1e-5f, s));
      off += out_n[b];
    }
    K(cast_copy(latent_out, adt, hn, F32, Ttot * D, s));
    return OK;
  };
  if (!rd_host) {  // open: size the scratch for the largest pass this stream can ask for, so that no append allocates
    dry = true;
    ws_reset();
    const int st = body();
    dry = false;
    ITTS_TRY(st);
    return ws_reserve(ws_off + 4096, s);
  }
  return two_pass(body, s);
}

int Engine::gpt_latent_stream_open(const float* cond_dev, const int32_t* cond_index, int n_cond, const int32_t* text_ids, const int* Ls,
                                   int nseq, int max_codes, hipStream_t s) {
  if (!finalized || !gpt.ok) {
    set_error("itts_gpt_latent_stream_open: GPT weights not bound");
    return E_STATE;
  }
  const itts_config& c = cfg;
  LatentStream& st = lstream;
  LatentStreamState view;
  view.open = st.open;
  if (const char* why = latent_stream_open_refusal(view, cond_dev, cond_index, n_cond, text_ids, Ls, nseq, max_codes, c.max_text_tokens,
                                                   c.max_mel_tokens, c.number_text_tokens)) {
    set_error(std::string("itts_gpt_latent_stream_open: ") + why);
    return E_INVALID;
  }
  const int D = c.model_dim, nl = c.cond_latents, H = c.heads, dh = D / H;
  // gpt_latent_packed's rule: the matrix-core GEMM of the pinned selector needs 16 rows, and so does every append (the re-run rule)
  if (!(adt == F32 || force_simple || nl + 6 >= 16)) {
    set_error("itts_gpt_latent_stream_open: a 16-bit engine needs cond_latents >= 10");
    return E_INVALID;
  }
  // the attention family of the packed pass on this engine (its qkv: 256-byte aligned, ld 3 D) - the stream takes the same one
  VarlenArgs va;
  va.q = (const void*)(uintptr_t)0x1000;
  va.k = (const char*)va.q + (size_t)D * es;
  va.v = (const char*)va.q + (size_t)2 * D * es;
  va.dqk = va.dv = dh;
  va.ldq = va.ldk = va.ldv = 3 * D;
  const int kernel = force_simple ? 1 : attention_varlen_which(va, adt);
  AppendArgs pa;  // ... and it has to be able to read the history's layout (k | v rows of 2 D, 256-byte aligned)
  pa.q = va.q, pa.k = va.q, pa.v = va.k;
  pa.dqk = pa.dv = dh;
  pa.ldq = 3 * D, pa.ldk = pa.ldv = 2 * D;
  if (kernel == 2 && !attention_append_mfma_supported(pa, adt)) {
    set_error("itts_gpt_latent_stream_open: the packed pass runs attn_varlen_mfma on this engine, attn_append_mfma cannot read the history layout");
    return E_INVALID;
  }
  int pmax = 0;
  long rows_max = 0;
  std::vector<int> prefix(nseq);
  std::vector<std::vector<int>> rd(nseq);
  long to = 0;
  for (int b = 0; b < nseq; ++b) {
    const int L = Ls[b], cb = cond_index ? cond_index[b] : 0;
    prefix[b] = nl + L + 2;
    pmax = std::max(pmax, prefix[b]);
    rows_max += prefix[b] + max_codes;
    std::vector<int>& r = rd[b];
    r.reserve((size_t)(prefix[b] + 1 + max_codes) * 4);
    auto push = [&r](int kind, int a0, int b0) { r.insert(r.end(), {kind, a0, b0, 0}); };
    for (int i = 0; i < nl; ++i) push(1, cb * nl + i, 0);
    push(2, c.start_text_token, 0);
    for (int i = 0; i < L; ++i) push(2, text_ids[to + i], i + 1);
    push(2, c.stop_text_token, L + 1);
    push(3, c.start_mel_token, 0);
    to += L;
  }
  if (rows_max + 16 >= (1L << 24)) {
    set_error("itts_gpt_latent_stream_open: more than 2^24 rows in one pass");
    return E_INVALID;
  }
  const int cap = pmax + max_codes;
  ITTS_HIP_CHECK(hipStreamSynchronize(s));
  void* hist = nullptr;
  ITTS_TRY(dev_alloc(&hist, (size_t)c.layers * nseq * cap * 2 * D * es));
  st.nseq = nseq, st.max_codes = max_codes, st.cap = cap, st.kernel = kernel, st.hist = hist, st.cond = cond_dev;
  st.prefix = prefix;
  st.done.assign(nseq, 0);
  st.computed.assign(nseq, 0);
  st.rd = std::move(rd);
  // the scratch of the largest pass: every sequence's first append carrying all its codes at once
  AppendArgs none;
  none.nseq = nseq;
  std::vector<int> zero(nseq, 0);
  const int status = latent_stream_pass(nullptr, (int)rows_max + 16, none, zero.data(), zero.data(), (long)nseq * max_codes, nullptr, s);
  if (status != OK) {
    (void)hipFree(hist);
    st.hist = nullptr;
    return status;
  }
  st.open = true;
  return OK;
}

int Engine::gpt_latent_stream_append(const int32_t* codes, const int* counts, void* latent_out, hipStream_t s) {
  LatentStream& st = lstream;
  LatentStreamState view;
  view.open = st.open, view.nseq = st.nseq, view.max_codes = st.max_codes, view.number_mel_codes = cfg.number_mel_codes;
  view.done = st.done.data();
  if (const char* why = latent_stream_append_refusal(view, codes, counts, latent_out)) {
    set_error(std::string("itts_gpt_latent_stream_append: ") + why);
    return E_INVALID;
  }
  const int nseq = st.nseq;
  // the rows of this call: sequence b's new positions [computed, prefix + done + count) - the row of a code is computed by the append
  // that brings the NEXT code's latent (latent row j reads the start token and codes < j), so a first append carries the prefix, the
  // start-mel row and all but its last code, a later one the held code and all but its last
  AppendArgs app;
  app.nseq = nseq;
  std::vector<int> out_n(nseq, 0), out_row(nseq, 0);
  long co = 0, Ttot = 0, M = 0;
  for (int b = 0; b < nseq; ++b) {
    const int n = counts[b];
    for (int i = 0; i < n; ++i) st.rd[b].insert(st.rd[b].end(), {3, codes[co + i], st.done[b] + i + 1, 0});
    co += n;
    app.kv_off[b] = b * st.cap;
    app.pos0[b] = st.computed[b];
    app.n_new[b] = n > 0 ? st.prefix[b] + st.done[b] + n - st.computed[b] : 0;
    out_n[b] = n;
    M += app.n_new[b];
    Ttot += n;
  }
  app.kv_off[nseq] = nseq * st.cap;
  if (Ttot == 0) return OK;
  // The 16-row rule: below 16 GEMM rows the pinned selector of a 16-bit engine changes family, and with it the bits.  A short call
  // re-runs the last rows it already computed (their history rows are rewritten with the same bits, their outputs dropped); where a
  // sequence has too few of those, zero rows that belong to no sequence fill the rest (every step outside the attention is row-wise).
  long pad = 0;
  if (adt != F32 && !force_simple && M < 16) {
    long need = 16 - M;
    for (int b = 0; b < nseq && need > 0; ++b) {
      if (app.n_new[b] < 1) continue;
      const int back = (int)std::min<long>(need, app.pos0[b]);
      app.pos0[b] -= back, app.n_new[b] += back;
      need -= back;
    }
    M = 16 - need;
    pad = need;
  }
  std::vector<int> rd((size_t)(M + pad) * 4, 0);  // (kind 0 = a zero row)
  long row = 0;
  for (int b = 0; b < nseq; ++b) {
    app.q_off[b] = (int)row;
    if (app.n_new[b] > 0) {
      std::copy(st.rd[b].begin() + (size_t)app.pos0[b] * 4, st.rd[b].begin() + (size_t)(app.pos0[b] + app.n_new[b]) * 4, rd.begin() + row * 4);
      out_row[b] = (int)row + st.prefix[b] + st.done[b] - app.pos0[b];  // latent row j is position prefix + j
    }
    row += app.n_new[b];
  }
  app.q_off[nseq] = (int)row;
  const int status = latent_stream_pass(rd.data(), (int)(M + pad), app, out_row.data(), out_n.data(), Ttot, latent_out, s);
  if (status != OK) {  // the codes of a failed call are not taken
    for (int b = 0; b < nseq; ++b) st.rd[b].resize((size_t)(st.prefix[b] + 1 + st.done[b]) * 4);
    return status;
  }
  ITTS_HIP_CHECK(hipStreamSynchronize(s));  // rd is a host buffer
  for (int b = 0; b < nseq; ++b)
    if (counts[b] > 0) {
      st.done[b] += counts[b];
      st.computed[b] = st.prefix[b] + st.done[b];
    }
  return OK;
}

int Engine::gpt_latent_stream_close(hipStream_t s) {
  LatentStream& st = lstream;
  if (!st.open) return OK;
  (void)s;  // every append ends with a synchronise of its stream: nothing in flight reads the history (hipFree waits for the device anyway)
  if (st.hist) ITTS_HIP_CHECK(hipFree(st.hist));
  st = LatentStream();
  return OK;
}

int Engine::gpt_latent(const float* cond_dev, const int32_t* text_ids, int L, const int32_t* codes, int T,
                       void* latent_out, hipStream_t s) {
  return gpt_latent_batch(cond_dev, text_ids, &L, codes, &T, 1, latent_out, s);
}

}  // namespace itts

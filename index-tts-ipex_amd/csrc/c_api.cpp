// extern "C" boundary of libitts_hip (declared in include/itts_hip.h).
#include <algorithm>
#include <cstring>
#include <new>

#include "engine.h"

using namespace itts;

struct itts_engine {
  Engine e;
};

extern "C" {

const char* itts_last_error(void) { return last_error(); }
int itts_abi_version(void) { return 4; }
int itts_half_is_f16(void) {
#ifdef ITTS_HALF_F16
  return 1;
#else
  return 0;
#endif
}

int itts_snake_aa_fwd(void* dst, const void* src, const float* up12, const float* down12, const float* log_alpha,
                      const float* log_beta, int B, int C, int T, int dtype, int layout, itts_stream stream) {
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  if (layout == 1) return snake_aa(dst, src, log_alpha, log_beta, up12, down12, B, T, C, dtype, (hipStream_t)stream);
  if (layout == 0) return snake_aa_bct(dst, src, log_alpha, log_beta, up12, down12, B, C, T, dtype, (hipStream_t)stream);
  set_error("itts_snake_aa_fwd: layout must be 0 ([B,C,T]) or 1 ([B,T,C])");
  return E_INVALID;
}

static void to_gemm_args(const itts_gemm_args* a, GemmArgs& g) {
  g.A = a->A; g.W = a->W; g.C = a->C;
  g.M = a->M; g.N = a->N; g.Cin = a->Cin; g.taps = a->taps; g.lda = a->lda; g.ldc = a->ldc; g.T = a->T;
  g.dil = a->dil; g.pad_left = a->pad_left; g.pad_mode = a->pad_mode; g.in_up = a->in_up < 1 ? 1 : a->in_up;
  g.nphase = a->nphase < 1 ? 1 : a->nphase;
  for (int i = 0; i < 8; ++i) g.phase_shift[i] = a->phase_shift[i];
  g.bias = a->bias; g.bias_bstride = a->bias_bstride; g.act = a->act; g.scale = a->scale; g.shift = a->shift;
  g.act2 = a->act2; g.R = a->R; g.ldr = a->ldr; g.alpha = a->alpha; g.ADD = a->ADD; g.ldadd = a->ldadd; g.beta = a->beta;
}

int itts_gemm(const itts_gemm_args* a, itts_stream stream) {
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  if (!a) {
    set_error("itts_gemm: null args");
    return E_INVALID;
  }
  GemmArgs g;
  to_gemm_args(a, g);
  if (a->force_simple) return gemm_simple(g, a->dtype_a, a->dtype_w, a->dtype_c, (hipStream_t)stream);
  return gemm(g, a->dtype_a, a->dtype_w, a->dtype_c, (hipStream_t)stream);
}

int itts_gemm_ws(const itts_gemm_args* a, void* ws, size_t ws_bytes, itts_stream stream) {
  (void)hipGetLastError();
  if (!a) {
    set_error("itts_gemm_ws: null args");
    return E_INVALID;
  }
  GemmArgs g;
  to_gemm_args(a, g);
  if (a->force_simple) return gemm_simple(g, a->dtype_a, a->dtype_w, a->dtype_c, (hipStream_t)stream);
  if (ws && !((uintptr_t)ws & 15)) {
    const int S = gemm_ksplit_plan(g, a->dtype_a, a->dtype_w, a->dtype_c, ws_bytes);
    if (S > 1) {
      g.ws = (float*)ws;
      g.ksplit = S;
    }
  }
  return gemm(g, a->dtype_a, a->dtype_w, a->dtype_c, (hipStream_t)stream);
}

int itts_gemm_ksplit(const itts_gemm_args* a, size_t ws_bytes) {
  if (!a) return E_INVALID;
  GemmArgs g;
  to_gemm_args(a, g);
  return a->force_simple ? 1 : gemm_ksplit_plan(g, a->dtype_a, a->dtype_w, a->dtype_c, ws_bytes);
}

int itts_gemm_which(const itts_gemm_args* a) {
  if (!a) return E_INVALID;
  GemmArgs g;
  to_gemm_args(a, g);
  return a->force_simple ? 0 : gemm_which(g, a->dtype_a, a->dtype_w, a->dtype_c);
}

// Why itts_gemm_family cannot run a call (null = it can): the entry's own questions, then the family's rule (gemm_family_refusal).
// have_ws: the launch (its workspace pointer is judged) or itts_gemm_family_supported (only ws_bytes is known).
static const char* gemm_family_entry_refusal(const itts_gemm_args* a, int family, int variant, int ksplit, const void* ws, bool have_ws,
                                             size_t ws_bytes, GemmArgs& g) {
  static const float dummy_ws[4] __attribute__((aligned(16))) = {0.f, 0.f, 0.f, 0.f};  // stands for a workspace the rule only asks the presence of
  if (!a) return "null args";
  if (a->force_simple && family != 0) return "force_simple: that is family 0";
  to_gemm_args(a, g);
  if (ksplit > 1 && family == 3) {
    if (have_ws && !ws) return "ksplit: a K split needs a workspace";
    if (have_ws && ((uintptr_t)ws & 15)) return "ksplit: the workspace must be 16-byte aligned";
    if (a->M >= 1 && a->N >= 1 && ws_bytes < (size_t)ksplit * a->M * a->N * 4) return "ksplit: the workspace is shorter than ksplit * M * N * 4 bytes";
    g.ws = have_ws ? (float*)ws : const_cast<float*>(dummy_ws);
  }
  g.ksplit = ksplit;
  return gemm_family_refusal(g, a->dtype_a, a->dtype_w, a->dtype_c, family, variant);
}

int itts_gemm_family(const itts_gemm_args* a, int family, int variant, int ksplit, void* ws, size_t ws_bytes, itts_stream stream) {
  GemmArgs g;
  if (const char* why = gemm_family_entry_refusal(a, family, variant, ksplit, ws, true, ws_bytes, g)) {  // before any HIP call
    set_error(std::string("itts_gemm_family: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  return gemm_family(g, a->dtype_a, a->dtype_w, a->dtype_c, family, variant, (hipStream_t)stream);
}

int itts_gemm_family_supported(const itts_gemm_args* a, int family, int variant, int ksplit, size_t ws_bytes) {
  GemmArgs g;
  return gemm_family_entry_refusal(a, family, variant, ksplit, nullptr, false, ws_bytes, g) ? 0 : 1;
}

// Why itts_act_conv cannot run a call FUSED (null = it can).  The early answers only name the reason; the decision is gemm_act_fused.
static const char* act_conv_refusal(const itts_gemm_args* a, const float* log_alpha, const float* log_beta, const float* filt12) {
  if (!a) return "null args";
  if (!a->A || !a->W || !a->C || !log_alpha || !log_beta || !filt12) return "null pointer";
  if (a->force_simple) return "force_simple: the vector-ALU kernel has no fused activation";
  if (a->dtype_a != BF16 || a->dtype_w != BF16 || a->dtype_c != BF16) return "dtype: A, W and C must be the 16-bit type of the library";
  if (a->lda != a->Cin) return "lda != Cin: the fused form stages whole dense rows";
  GemmArgs g;
  to_gemm_args(a, g);
  g.pre_alpha = log_alpha, g.pre_beta = log_beta, g.pre_filt = filt12;
  if (gemm_which(g, BF16, BF16, BF16) != 4) return "shape: not the LDS-tiled narrow conv (itts_gemm_which != 4)";
  if (!gemm_act_fused(g, BF16, BF16, BF16)) return "the fused activation is switched off (ITTS_NO_CONV_ACT)";
  return nullptr;
}

int itts_act_conv(const itts_gemm_args* a, const float* log_alpha, const float* log_beta, const float* filt12, itts_stream stream) {
  if (const char* why = act_conv_refusal(a, log_alpha, log_beta, filt12)) {  // before any HIP call
    set_error(std::string("itts_act_conv: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  GemmArgs g;
  to_gemm_args(a, g);
  g.pre_alpha = log_alpha, g.pre_beta = log_beta, g.pre_filt = filt12;
  return gemm(g, BF16, BF16, BF16, (hipStream_t)stream);  // (gemm() itself refuses a pre_* call it would not run fused)
}

// ---- padded ragged batches: every block is judged on the host before any HIP call ----
static const char* ragged_refusal(const void* lens_dev, int mul) {
  if (!lens_dev) return "null pointer";
  if (mul < 1) return "mul < 1";
  return nullptr;
}

int itts_snake_aa_fwd_len(void* dst, const void* src, const float* up12, const float* down12, const float* log_alpha,
                          const float* log_beta, int B, int C, int T, const int* lens_dev, int mul, int dtype, itts_stream stream) {
  const char* why = (!dst || !src || !up12 || !down12 || !log_alpha || !log_beta) ? "null pointer" : ragged_refusal(lens_dev, mul);
  if (!why && (B < 1 || C < 1 || T < 1)) why = "B, C and T must be >= 1";
  if (!why && dtype != F32 && dtype != BF16 && dtype != F16) why = "unsupported dtype";
  if (why) {
    set_error(std::string("itts_snake_aa_fwd_len: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  return snake_aa_len(dst, src, log_alpha, log_beta, up12, down12, B, T, C, lens_dev, mul, dtype, (hipStream_t)stream);
}

int itts_act_conv_len(const itts_gemm_args* a, const float* log_alpha, const float* log_beta, const float* filt12, const int* lens_dev,
                      int mul, itts_stream stream) {
  const char* why = act_conv_refusal(a, log_alpha, log_beta, filt12);
  if (!why) why = ragged_refusal(lens_dev, mul);
  if (why) {
    set_error(std::string("itts_act_conv_len: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();
  GemmArgs g;
  to_gemm_args(a, g);
  g.pre_alpha = log_alpha, g.pre_beta = log_beta, g.pre_filt = filt12;
  return gemm(g, BF16, BF16, BF16, (hipStream_t)stream, lens_dev, mul);
}

int itts_zero_tail_rows(void* x, int B, int T, int C, const int* lens_dev, int mul, int dtype, itts_stream stream) {
  const char* why = !x ? "null pointer" : ragged_refusal(lens_dev, mul);
  if (!why && (B < 1 || B > 65535 || C < 1 || T < 1)) why = "B in [1, 65535], C and T >= 1";
  if (!why && dtype != F32 && dtype != BF16) why = "unsupported dtype";
  if (why) {
    set_error(std::string("itts_zero_tail_rows: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();
  return zero_tail_rows(x, B, T, C, lens_dev, mul, dtype, (hipStream_t)stream);
}

// ---- packed sentences: offsets and lengths are HOST arrays, so every entry judges the whole call before any HIP call ----
static const char* seg_entry_refusal(SegTable& seg, const int* off_host, const int* lens_host, int n, int mul) {
  if (!off_host || !lens_host) return "null pointer";
  if (n < 1 || n > SEG_MAX) return "n outside [1, 128]";
  (void)seg_table_fill(seg, off_host, lens_host, n);
  return seg_table_refusal(seg, mul, 0);
}

int itts_snake_aa_fwd_seg(void* dst, const void* src, const float* up12, const float* down12, const float* log_alpha,
                          const float* log_beta, int C, const int* off_host, const int* lens_host, int n, int mul, int dtype,
                          itts_stream stream) {
  SegTable seg;
  const char* why = (!dst || !src || !up12 || !down12 || !log_alpha || !log_beta) ? "null pointer" : seg_entry_refusal(seg, off_host, lens_host, n, mul);
  if (!why && C < 1) why = "C must be >= 1";
  if (!why && dtype != F32 && dtype != BF16 && dtype != F16) why = "unsupported dtype";
  if (why) {
    set_error(std::string("itts_snake_aa_fwd_seg: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  return snake_aa_seg(dst, src, log_alpha, log_beta, up12, down12, C, seg, mul, dtype, (hipStream_t)stream);
}

int itts_act_conv_seg(const itts_gemm_args* a, const float* log_alpha, const float* log_beta, const float* filt12, const int* off_host,
                      const int* lens_host, int n, int mul, itts_stream stream) {
  SegTable seg;
  GemmArgs g;
  const char* why = !a ? "null args" : (!a->A || !a->W || !a->C || !log_alpha || !log_beta || !filt12) ? "null pointer" : nullptr;
  if (!why && a->force_simple) why = "force_simple: the vector-ALU kernel has no fused activation";
  if (!why && (a->dtype_a != BF16 || a->dtype_w != BF16 || a->dtype_c != BF16)) why = "dtype: A, W and C must be the 16-bit type of the library";
  if (!why && a->lda != a->Cin) why = "lda != Cin: the fused form stages whole dense rows";
  // one item: the kernel would step the bias by SENTENCE with a stride (per-sentence rows are itts_seg_bias_mask's business)
  if (!why && a->bias && a->bias_bstride != 0) why = "bias_bstride != 0: the pack is one item, its bias is one row";
  if (!why) {
    to_gemm_args(a, g);
    g.pre_alpha = log_alpha, g.pre_beta = log_beta, g.pre_filt = filt12;
    if (gemm_which_pinned_conv(g, BF16, BF16, BF16) != 4) why = "shape: not the LDS-tiled narrow conv (itts_gemm_which_pinned_conv != 4)";
    else if (!gemm_pinned_conv_fused(g, BF16, BF16, BF16)) why = "the fused activation is switched off (ITTS_NO_CONV_ACT)";
  }
  if (!why) why = seg_entry_refusal(seg, off_host, lens_host, n, mul);
  if (!why && (a->M != a->T || (long)a->T < (long)seg.off[n] * mul)) why = "M == T >= off[n] * mul expected: one item that holds the whole pack";
  if (why) {
    set_error(std::string("itts_act_conv_seg: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();
  return gemm_pinned_conv(g, BF16, BF16, BF16, (hipStream_t)stream, &seg, mul);
}

int itts_seg_bias_mask(void* x, const float* bias, int C, const int* off_host, const int* lens_host, int n, int mul, int dtype,
                       itts_stream stream) {
  SegTable seg;
  const char* why = !x ? "null pointer" : seg_entry_refusal(seg, off_host, lens_host, n, mul);
  if (!why && C < 1) why = "C must be >= 1";
  if (!why && dtype != F32 && dtype != BF16) why = "unsupported dtype";
  if (!why) {
    long cap = 0;
    for (int b = 0; b < n; ++b) cap = std::max<long>(cap, seg.off[b + 1] - seg.off[b]);
    if (cap * mul * C > 0x7fffffffL) why = "a sentence of more than 2^31 - 1 elements";
  }
  if (why) {
    set_error(std::string("itts_seg_bias_mask: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();
  return seg_bias_mask(x, bias, C, seg, mul, dtype, (hipStream_t)stream);
}

int itts_gemm_which_pinned_conv(const itts_gemm_args* a) {
  if (!a) return E_INVALID;
  GemmArgs g;
  to_gemm_args(a, g);
  return a->force_simple ? 0 : gemm_which_pinned_conv(g, a->dtype_a, a->dtype_w, a->dtype_c);
}

int itts_bigvgan_packed_gap(const itts_config* cfg) { return cfg ? bigvgan_packed_gap(*cfg) : E_INVALID; }

int itts_bigvgan_packed_check(const itts_config* cfg, const void* latent, const float* spk, const int32_t* off_host,
                              const int32_t* lens_host, int n, const float* wav_out) {
  const char* why = !cfg ? "null config" : bigvgan_packed_refusal(*cfg, latent, spk, off_host, lens_host, n, wav_out);
  if (why) {
    set_error(std::string("itts_bigvgan_packed: ") + why);
    return E_INVALID;
  }
  return OK;
}

int itts_act_conv_supported(const itts_gemm_args* a) {
  static const float dummy = 0.f;  // a real call has its three parameter vectors; the rule only asks whether they are there
  return act_conv_refusal(a, &dummy, &dummy, &dummy) ? 0 : 1;
}

int itts_gemv_which(int B, int N, int K, int prologue, int x_bf16, int y_bf16, int w5) {
  static const float partials = 0.f;  // prologue 3: a real call has its two partial buffers; the selector only asks whether they are there
  GemvArgs g;
  g.B = B, g.N = N, g.K = K, g.prologue = prologue, g.x_bf16 = x_bf16, g.y_bf16 = y_bf16;
  if (prologue == 3) g.attn_o = g.attn_ml = &partials;
  GemvPick p;
  return gemv_bf16_pick(g, w5 != 0, &p) ? p.nb | p.rpw << 4 | p.nch << 8 | p.waves << 16 : -1;
}

int itts_layernorm(void* y, int dtype_y, const void* x, int dtype_x, const float* gamma, const float* beta, int rows,
                   int D, float eps, itts_stream stream) {
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  return layernorm(y, dtype_y, x, dtype_x, gamma, beta, rows, D, D, D, eps, ACT_NONE, (hipStream_t)stream);
}

static AttnArgs to_attn_args(void* o, const void* q, const void* k, const void* v, int B, int H, int Sq, int Sk, int dqk, int dv, int ldq,
                             int ldk, int ldv, int ldo, float scale, int causal, const int* kv_start) {
  AttnArgs a;
  a.q = q; a.k = k; a.v = v; a.o = o; a.B = B; a.H = H; a.Sq = Sq; a.Sk = Sk; a.dqk = dqk; a.dv = dv;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.scale = scale; a.causal = causal; a.kv_start = kv_start;
  return a;
}

// itts_attention (kernel 0) and itts_attention_kernel: one host-side check (attention_refusal) before any HIP call, then the
// dispatcher or the named kernel's own launcher - a named kernel is never replaced by the other one.
static int attention_entry(const char* entry, void* o, const void* q, const void* k, const void* v, int B, int H, int Sq, int Sk, int dqk,
                           int dv, int ldq, int ldk, int ldv, int ldo, float scale, int causal, const int* kv_start, int dtype, int kernel,
                           itts_stream stream) {
  const AttnArgs a = to_attn_args(o, q, k, v, B, H, Sq, Sk, dqk, dv, ldq, ldk, ldv, ldo, scale, causal, kv_start);
  if (const char* why = attention_refusal(a, dtype, kernel)) {
    set_error(std::string(entry) + ": " + why);
    return E_INVALID;
  }
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  if (kernel == 1) return attention_simple(a, dtype, (hipStream_t)stream);
  if (kernel == 2) return attention_mfma(a, dtype, (hipStream_t)stream);
  return attention(a, dtype, (hipStream_t)stream);
}

int itts_attention(void* o, const void* q, const void* k, const void* v, int B, int H, int Sq, int Sk, int dqk, int dv,
                   int ldq, int ldk, int ldv, int ldo, float scale, int causal, const int* kv_start, int dtype,
                   itts_stream stream) {
  return attention_entry("itts_attention", o, q, k, v, B, H, Sq, Sk, dqk, dv, ldq, ldk, ldv, ldo, scale, causal, kv_start, dtype, 0, stream);
}

int itts_attention_kernel(void* o, const void* q, const void* k, const void* v, int B, int H, int Sq, int Sk, int dqk, int dv,
                          int ldq, int ldk, int ldv, int ldo, float scale, int causal, const int* kv_start, int dtype, int kernel,
                          itts_stream stream) {
  return attention_entry("itts_attention_kernel", o, q, k, v, B, H, Sq, Sk, dqk, dv, ldq, ldk, ldv, ldo, scale, causal, kv_start, dtype, kernel,
                         stream);
}

int itts_attention_which(const void* q, const void* k, const void* v, int B, int H, int Sq, int Sk, int dqk, int dv, int ldq, int ldk,
                         int ldv, int ldo, float scale, int causal, const int* kv_start, int dtype) {
  static const float dummy_o = 0.f;  // a real call has its output; the rule only asks whether it is there
  const AttnArgs a = to_attn_args(const_cast<float*>(&dummy_o), q, k, v, B, H, Sq, Sk, dqk, dv, ldq, ldk, ldv, ldo, scale, causal, kv_start);
  return attention_refusal(a, dtype, 0) ? E_INVALID : attention_which(a, dtype);
}

// itts_attention_varlen / itts_attention_varlen_which: one host-side check (attention_varlen_refusal) before any HIP call
static const char* to_varlen_args(VarlenArgs& a, void* o, const void* q, const void* k, const void* v, const int32_t* seq_off_host, int nseq,
                                  int H, int dqk, int dv, int ldq, int ldk, int ldv, int ldo, float scale) {
  a.q = q; a.k = k; a.v = v; a.o = o; a.H = H; a.dqk = dqk; a.dv = dv;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.scale = scale; a.nseq = nseq;
  if (!seq_off_host) return "null pointer (q, k, v, o, seq_off_host)";
  if (nseq < 1 || nseq > VARLEN_MAX_SEQ) return "nseq outside 1 .. 128";  // (before the copy: the array holds nseq + 1 ints)
  for (int i = 0; i <= nseq; ++i) a.off[i] = seq_off_host[i];
  return nullptr;
}

int itts_attention_varlen(void* o, const void* q, const void* k, const void* v, const int32_t* seq_off_host, int nseq, int H, int dqk,
                          int dv, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, int kernel, itts_stream stream) {
  VarlenArgs a;
  const char* why = to_varlen_args(a, o, q, k, v, seq_off_host, nseq, H, dqk, dv, ldq, ldk, ldv, ldo, scale);
  if (!why) why = attention_varlen_refusal(a, dtype, kernel);
  if (why) {
    set_error(std::string("itts_attention_varlen: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  return attention_varlen(a, dtype, kernel, (hipStream_t)stream);
}

int itts_attention_varlen_which(const void* q, const void* k, const void* v, const int32_t* seq_off_host, int nseq, int H, int dqk,
                                int dv, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, int kernel) {
  static const float dummy_o = 0.f;  // a real call has its output; the rule only asks whether it is there
  VarlenArgs a;
  const char* why = to_varlen_args(a, const_cast<float*>(&dummy_o), q, k, v, seq_off_host, nseq, H, dqk, dv, ldq, ldk, ldv, ldo, scale);
  if (!why) why = attention_varlen_refusal(a, dtype, kernel);
  if (why) {
    set_error(std::string("itts_attention_varlen_which: ") + why);
    return E_INVALID;
  }
  return kernel ? kernel : attention_varlen_which(a, dtype);
}

// itts_attention_append / itts_attention_append_which / itts_kv_rows_append: one host-side check (append_check.cpp) before any HIP call
static const char* to_append_args(AppendArgs& a, void* o, const void* q, const void* k, const void* v, const int32_t* q_off_host,
                                  const int32_t* kv_off_host, const int32_t* pos0_host, const int32_t* n_new_host, int nseq, int H, int dqk,
                                  int dv, int ldq, int ldk, int ldv, int ldo, float scale) {
  a.q = q; a.k = k; a.v = v; a.o = o; a.H = H; a.dqk = dqk; a.dv = dv;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.scale = scale; a.nseq = nseq;
  if (!q_off_host || !kv_off_host || !pos0_host || !n_new_host) return "null pointer (q, k, v, o, q_off_host, kv_off_host, pos0_host, n_new_host)";
  if (nseq < 1 || nseq > VARLEN_MAX_SEQ) return "nseq outside 1 .. 128";  // (before the copy: the arrays hold nseq (+ 1) ints)
  for (int i = 0; i <= nseq; ++i) a.q_off[i] = q_off_host[i], a.kv_off[i] = kv_off_host[i];
  for (int i = 0; i < nseq; ++i) a.pos0[i] = pos0_host[i], a.n_new[i] = n_new_host[i];
  return nullptr;
}

int itts_attention_append(void* o, const void* q, const void* k_hist, const void* v_hist, const int32_t* q_off_host, const int32_t* kv_off_host,
                          const int32_t* pos0_host, const int32_t* n_new_host, int nseq, int H, int dqk, int dv, int ldq, int ldk, int ldv,
                          int ldo, float scale, int dtype, int kernel, itts_stream stream) {
  AppendArgs a;
  const char* why = to_append_args(a, o, q, k_hist, v_hist, q_off_host, kv_off_host, pos0_host, n_new_host, nseq, H, dqk, dv, ldq, ldk, ldv, ldo, scale);
  if (!why) why = attention_append_refusal(a, dtype, kernel);
  if (why) {
    set_error(std::string("itts_attention_append: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  return attention_append(a, dtype, kernel, (hipStream_t)stream);
}

int itts_attention_append_which(const void* q, const void* k_hist, const void* v_hist, const int32_t* q_off_host, const int32_t* kv_off_host,
                                const int32_t* pos0_host, const int32_t* n_new_host, int nseq, int H, int dqk, int dv, int ldq, int ldk,
                                int ldv, int ldo, float scale, int dtype, int kernel) {
  static const float dummy_o = 0.f;  // a real call has its output; the rule only asks whether it is there
  AppendArgs a;
  const char* why = to_append_args(a, const_cast<float*>(&dummy_o), q, k_hist, v_hist, q_off_host, kv_off_host, pos0_host, n_new_host, nseq, H, dqk,
                                   dv, ldq, ldk, ldv, ldo, scale);
  if (!why) why = attention_append_refusal(a, dtype, kernel);
  if (why) {
    set_error(std::string("itts_attention_append_which: ") + why);
    return E_INVALID;
  }
  return kernel ? kernel : attention_append_which(a, dtype);
}

int itts_kv_rows_append(void* k_hist, void* v_hist, const void* k_src, const void* v_src, const int32_t* q_off_host, const int32_t* kv_off_host,
                        const int32_t* pos0_host, const int32_t* n_new_host, int nseq, int ld_src, int ldk, int ldv, int wk, int wv, int dtype,
                        itts_stream stream) {
  AppendArgs a;
  const char* why = to_append_args(a, nullptr, nullptr, k_hist, v_hist, q_off_host, kv_off_host, pos0_host, n_new_host, nseq, 1, 1, 1, 0, ldk, ldv, 0, 1.f);
  if (!why) why = kv_rows_append_refusal(a, k_src, v_src, ld_src, wk, wv, dtype);
  if (why) {
    set_error(std::string("itts_kv_rows_append: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  return kv_rows_append(a, k_src, v_src, ld_src, wk, wv, dtype, (hipStream_t)stream);
}

int itts_gemv(float* Y, const float* X, const void* W, const float* bias, int B, int N, int K, int act, int accumulate,
              int prologue, const float* ln_gamma, const float* ln_beta, const float* ln2_gamma, const float* ln2_beta,
              int dtype_w, int version, itts_stream stream) {
  (void)hipGetLastError();
  GemvArgs g;
  g.X = X; g.W = W; g.Y = Y; g.bias = bias; g.B = B; g.N = N; g.K = K; g.ldy = N; g.act = act; g.accumulate = accumulate;
  g.prologue = prologue; g.ln_gamma = ln_gamma; g.ln_beta = ln_beta; g.ln2_gamma = ln2_gamma; g.ln2_beta = ln2_beta;
  if (version == 2 || (version == 0 && gemv2_supported(g))) return gemv2(g, dtype_w, (hipStream_t)stream);
  return gemv(g, dtype_w, (hipStream_t)stream);
}

int itts_gemv_bf16(void* Y, int y_bf16, const void* X, int x_bf16, const void* W, const float* bias, int B, int N, int K, int act,
                   int accumulate, int prologue, const float* ln_gamma, const float* ln_beta, const float* attn_o,
                   const float* attn_ml, const void* W8, const float* wscale, itts_stream stream) {
  (void)hipGetLastError();
  GemvArgs g;
  g.X = (const float*)X; g.x_bf16 = x_bf16; g.W = W; g.Y = (float*)Y; g.y_bf16 = y_bf16; g.bias = bias; g.B = B; g.N = N; g.K = K;
  g.ldy = N; g.act = act; g.accumulate = accumulate; g.prologue = prologue; g.ln_gamma = ln_gamma; g.ln_beta = ln_beta;
  g.attn_o = attn_o; g.attn_ml = attn_ml; g.W8 = W8; g.wscale = wscale;
  if (prologue == 2 && !(ln_gamma && ln_beta)) {  // the kernel reads both unconditionally
    set_error("itts_gemv_bf16: prologue 2 needs ln_gamma and ln_beta");
    return E_INVALID;
  }
  return gemv_bf16(g, (hipStream_t)stream);
}

int itts_decode_attn(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start, const int* prefix,
                     int B, int H, int dh, int Smax, int tc, int ctx_tiled, float* part_o, float* part_ml, const uint8_t* anc, int nb,
                     itts_stream stream) {
  (void)hipGetLastError();
  if (!qkv || !kc || !vc || !len || !kv_start || !prefix || B < 1 || H < 1 || Smax < 1 || (!ctx && !part_o)) {
    set_error("itts_decode_attn: bad arguments (qkv, kc, vc, len, kv_start, prefix; B, H, Smax >= 1; ctx unless part_o is given)");
    return E_INVALID;
  }
  return decode_attn2(ctx, to, qkv, kc, vc, len, kv_start, prefix, B, H, dh, Smax, tc, (hipStream_t)stream, ctx_tiled, part_o, part_ml,
                      anc, nb);
}

int itts_kv_scatter(void* kc, void* vc, const void* qkv, int B, int S, int H, int dh, int Smax, int tq, int tc, itts_stream stream) {
  (void)hipGetLastError();
  if (!kc || !vc || !qkv || B < 1 || S < 1 || H < 1 || dh < 1 || Smax < 1 || S > Smax) {
    set_error("itts_kv_scatter: bad arguments (kc, vc, qkv; B, S, H, dh, Smax >= 1; S <= Smax)");
    return E_INVALID;
  }
  if (!((tq == F32 && (tc == F32 || tc == FP8)) || (tq == BF16 && (tc == BF16 || tc == FP8)))) {
    set_error("itts_kv_scatter: type pair (tq, tc) must be fp32 -> fp32, 16-bit -> 16-bit, or either -> fp8 (e4m3) cache");
    return E_INVALID;
  }
  return kv_scatter(kc, vc, qkv, B, S, H, dh, Smax, tq, tc, (hipStream_t)stream);
}

int itts_rows_move(void* base, size_t outer_stride, int n_outer, size_t row_stride, size_t chunk_stride, int n_chunks, size_t chunk_bytes,
                   const int* src_host, const int* dst_host, int n_moves, itts_stream stream) {
  // refused before any HIP call
  ITTS_TRY(rows_move_check(base, outer_stride, n_outer, row_stride, chunk_stride, n_chunks, chunk_bytes, src_host, dst_host, n_moves));
  (void)hipGetLastError();
  return rows_move(base, outer_stride, n_outer, row_stride, chunk_stride, n_chunks, chunk_bytes, src_host, dst_host, n_moves,
                   (hipStream_t)stream);
}

int itts_rows_gather(void* dst, size_t dst_plane_stride, const void* src, size_t src_plane_stride, int n_planes, size_t row_bytes,
                     const int* src_rows_host, int n_rows, itts_stream stream) {
  // refused before any HIP call
  ITTS_TRY(rows_gather_check(dst, dst_plane_stride, src, src_plane_stride, n_planes, row_bytes, src_rows_host, n_rows));
  (void)hipGetLastError();
  return rows_gather(dst, dst_plane_stride, src, src_plane_stride, n_planes, row_bytes, src_rows_host, n_rows, (hipStream_t)stream);
}

int itts_retire_plan(const int* unfinished_host, int B, int* n_live, int* src_host, int* dst_host, int* n_moves) {
  return retire_plan(unfinished_host, B, n_live, src_host, dst_host, n_moves);
}

int itts_kv_admit(void* kc, void* vc, const void* qkv, int n, int S, int H, int dh, int Smax, int Bcache, int tq, int tc,
                  const int* slots_host, itts_stream stream) {
  // refused before any HIP call
  ITTS_TRY(kv_admit_check(kc, vc, qkv, n, S, H, dh, Smax, Bcache, tq, tc, slots_host));
  (void)hipGetLastError();
  return kv_admit(kc, vc, qkv, n, S, H, dh, Smax, Bcache, tq, tc, slots_host, (hipStream_t)stream);
}

int itts_rows_admit(const itts_rows_admit_args* p, itts_stream stream) {
  ITTS_REQUIRE(p, "itts_rows_admit: null argument block");
  RowsAdmitArgs a;
  a.seen = (uint8_t*)p->seen;
  a.unfinished = (int*)p->unfinished;
  a.cur_tok = (int*)p->cur_tok;
  a.len = (int*)p->len;
  a.kv_start = (int*)p->kv_start;
  a.ids = (int*)p->ids;
  a.forced = (int*)p->forced;
  a.uniforms = (float*)p->uniforms;
  a.forced_src = (const int*)p->forced_src;
  a.uniforms_src = (const float*)p->uniforms_src;
  a.n = p->n;
  a.B = p->B;
  a.V = p->V;
  a.max_gen = p->max_gen;
  a.fake_id = p->fake_id;
  a.start_tok = p->start_tok;
  a.stop = p->stop;
  ITTS_TRY(rows_admit_check(a, p->slots_host, p->kv_start_host));  // refused before any HIP call
  (void)hipGetLastError();
  return rows_admit(a, p->slots_host, p->kv_start_host, (hipStream_t)stream);
}

int itts_admit_plan(const int* unfinished_host, const int* len_host, int B, int max_gen, int n, int* slots_host, int* n_free) {
  return admit_plan(unfinished_host, len_host, B, max_gen, n, slots_host, n_free);
}

int itts_beam_admit(const itts_beam_admit_args* p, itts_stream stream) {
  ITTS_REQUIRE(p, "itts_beam_admit: null argument block");
  BeamAdmitArgs a;
  a.beam_scores = (float*)p->beam_scores;
  a.anc = (uint8_t*)p->anc;
  a.hyp_order = (int*)p->hyp_order;
  a.hyp_n = (int*)p->hyp_n;
  a.hyp_worst = (float*)p->hyp_worst;
  a.hyp_counter = (int*)p->hyp_counter;
  a.done = (int*)p->beam_done;
  a.uniforms = (float*)p->uniforms;
  a.uniforms_src = (const float*)p->uniforms_src;
  a.n = p->n;
  a.nb = p->nb;
  a.items = p->items;
  a.Smax = p->Smax;
  a.max_gen = p->max_gen;
  a.do_sample = p->do_sample;
  ITTS_TRY(beam_admit_check(a, p->items_host));  // refused before any HIP call
  (void)hipGetLastError();
  return beam_admit(a, p->items_host, (hipStream_t)stream);
}

int itts_sample_rows(int32_t* tok, int32_t* kept, const float* logits, const uint8_t* seen, int B, int V, float penalty, int stop,
                     int suppress_stop, int preprocessed, int top_k, float top_p, float temperature, const float* uniforms,
                     void* scratch, size_t scratch_bytes, itts_stream stream) {
  (void)hipGetLastError();
  if (!tok || !kept || !logits || !uniforms || !scratch || B < 1 || V < 1 || stop < 0 || stop >= V || ((uintptr_t)scratch & 3) ||
      scratch_bytes < (size_t)B * ((size_t)V + 16)) {
    set_error("itts_sample_rows: bad arguments (tok, kept, logits, uniforms, a 4-byte aligned scratch of B * (V + 16) bytes, 0 <= stop < V)");
    return E_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  // the samplers' bookkeeping of a one-step generation, on the caller's scratch: step 0, every row running, a private copy of
  // the seen bytes (the commit marks the drawn token in it)
  int* step = (int*)scratch;
  int* unfinished = step + B;
  int* ids = unfinished + B;
  uint8_t* seen_copy = (uint8_t*)(ids + B);
  ITTS_HIP_CHECK(hipMemsetAsync(step, 0, (size_t)B * 4, s));
  ITTS_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)unfinished, 1, (size_t)B, s));
  if (seen)
    ITTS_HIP_CHECK(hipMemcpyAsync(seen_copy, seen, (size_t)B * V, hipMemcpyDeviceToDevice, s));
  else
    ITTS_HIP_CHECK(hipMemsetAsync(seen_copy, 0, (size_t)B * V, s));
  ITTS_HIP_CHECK(hipMemsetAsync(kept, 0xFF, (size_t)B * 4, s));  // -1: the narrow kernel does not report it
  SamplerArgs a;
  a.logits = logits; a.seen = seen_copy; a.ids = ids; a.cur_tok = tok; a.unfinished = unfinished; a.step = step;
  a.V = V; a.max_gen = 1; a.stop = stop; a.suppress_stop = suppress_stop; a.penalty = penalty; a.preprocessed = preprocessed;
  a.do_sample = 1; a.top_k = top_k < 1 ? 0 : top_k; a.B = B; a.top_p = top_p; a.temperature = temperature; a.uniforms = uniforms;
  a.kept = kept;
  return sampler2_step(a, B, s);
}

int itts_beam_sample_rows(float* pick_score, int32_t* pick_tok, int32_t* pick_beam, int32_t* kept, const float* logits,
                          const int32_t* ids, int ids_stride, int k, const float* beam_scores, int items, int num_beams, int V,
                          float penalty, int stop, int suppress_stop, int start_tok, int fake_id, int preprocessed, int top_k,
                          float top_p, float temperature, const float* uniforms, void* scratch, size_t scratch_bytes,
                          itts_stream stream) {
  (void)hipGetLastError();
  if (!pick_score || !pick_tok || !pick_beam || !kept || !logits || !beam_scores || !uniforms || !scratch || items < 1 || k < 0 ||
      (k > 0 && (!ids || ids_stride < k)) || ((uintptr_t)scratch & 3)) {
    set_error("itts_beam_sample_rows: bad arguments (picks, kept, logits, beam_scores, uniforms, a 4-byte aligned scratch; ids [rows][ids_stride >= k])");
    return E_INVALID;
  }
  if (num_beams < 2 || num_beams > 10 || V < 2 || V > BEAM_WIDE_MAX_V || stop < 0 || stop >= V || start_tok < 0 || start_tok >= V ||
      fake_id < 0 || fake_id >= V || !(top_p > 0.f) || !(temperature > 0.f)) {
    set_error("itts_beam_sample_rows: 2 <= num_beams <= 10, 2 <= V <= 16384, stop / start_tok / fake_id inside the vocabulary, top_p > 0, temperature > 0");
    return E_INVALID;
  }
  const int rows = items * num_beams;
  if (scratch_bytes < ((size_t)rows * ((size_t)V + 1) + (size_t)items) * 4) {
    set_error("itts_beam_sample_rows: scratch shorter than (items * num_beams * (V + 1) + items) * 4 bytes");
    return E_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  // the kernels' view of a generation at step k on the caller's scratch: every beam row k tokens long, no item done
  BeamWide w;
  w.sc = (float*)scratch;
  int* len = (int*)(w.sc + (size_t)rows * V);
  int* done = len + rows;
  w.kept = kept;
  w.pick_sc = pick_score;
  w.pick_tok = pick_tok;
  w.pick_beam = pick_beam;
  w.one_step = 1;
  ITTS_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)len, k, (size_t)rows, s));
  ITTS_HIP_CHECK(hipMemsetAsync(done, 0, (size_t)items * 4, s));
  BeamArgs a;
  a.logits = logits; a.V = V; a.max_gen = ids_stride > 0 ? ids_stride : 1; a.stop = stop; a.suppress_stop = suppress_stop;
  a.nb = num_beams; a.B = items; a.top_k = top_k < 1 ? 0 : top_k; a.start_tok = start_tok; a.fake_id = fake_id; a.penalty = penalty;
  a.top_p = top_p; a.temperature = temperature; a.uniforms = uniforms; a.len = len; a.ids = (int*)ids; a.beam_scores = (float*)beam_scores;
  a.done = done; a.preprocessed = preprocessed; a.do_sample = 1;
  if (!a.ids) a.ids = len;  // k = 0: never read
  return beam_wide_pair(a, w, s);
}

// The argument block of the two skinny entries, without pointers: what itts_skinny_gemm_supported judges and the entries launch.
static bool skinny_args(GemvArgs& g, int y_bf16, int B, int N, int K, int act, int accumulate, int ksplit, int layout, int fp8) {
  if ((layout & ~31) || (fp8 && (layout & 4))) return false;  // fp8: tiling is said by W8t
  g.x_bf16 = 1; g.y_bf16 = y_bf16 ? 1 : 0; g.B = B; g.N = N; g.K = K; g.ldy = N; g.act = act; g.accumulate = accumulate ? 1 : 0;
  g.ksplit = ksplit;
  g.x_tiled = layout & 1; g.y_tiled = (layout >> 1) & 1;
  if (layout & 8) {  // X is fp32 [B, K]: LayerNorm (eps 1e-5, no affine) in the prologue, B <= 16
    g.x_bf16 = 0;
    g.prologue = 1;
  }
  g.half_tiles = (layout >> 4) & 1;
  return skinny_mfma_shape_ok(g);
}

int itts_skinny_gemm_supported(int y_bf16, int B, int N, int K, int act, int accumulate, int ksplit, int layout, int fp8) {
  GemvArgs g;
  return skinny_args(g, y_bf16, B, N, K, act, accumulate, ksplit, layout, fp8) ? 1 : 0;
}

#define SKINNY_REQUIRE(name, cond, msg)                 \
  do {                                                  \
    if (!(cond)) {                                      \
      set_error(std::string(name) + ": " msg " (" #cond ")"); \
      return E_INVALID;                                 \
    }                                                   \
  } while (0)

int itts_skinny_gemm(void* Y, int y_bf16, const void* X, const void* W, const float* bias, int B, int N, int K, int act,
                     int accumulate, int ksplit, float* partial, int layout, itts_stream stream) {
  (void)hipGetLastError();
  const char* me = "itts_skinny_gemm";
  SKINNY_REQUIRE(me, X && W && (Y || ksplit > 1), "null pointer (X, W; Y unless ksplit > 1)");
  SKINNY_REQUIRE(me, B > 0 && N > 0 && K > 0 && ksplit > 0, "non-positive B, N, K or ksplit");
  SKINNY_REQUIRE(me, ksplit == 1 || partial, "ksplit > 1 needs partial[ksplit][B][N]");
  GemvArgs g;
  SKINNY_REQUIRE(me, skinny_args(g, y_bf16, B, N, K, act, accumulate, ksplit, layout, 0), "unsupported shape (itts_skinny_gemm_supported)");
  g.X = (const float*)X; g.Y = (float*)Y; g.bias = bias; g.partial = partial;
  if (layout & 4)
    g.Wt = W;
  else
    g.W = W;
  return skinny_mfma(g, (hipStream_t)stream);
}

int itts_skinny_gemm_fp8(void* Y, int y_bf16, const void* X, const void* W8, const void* W8t, const float* wscale, const float* bias,
                         int B, int N, int K, int act, int accumulate, int ksplit, float* partial, int layout, itts_stream stream) {
  (void)hipGetLastError();
  const char* me = "itts_skinny_gemm_fp8";
  SKINNY_REQUIRE(me, X && W8 && wscale && (Y || ksplit > 1), "null pointer (X, W8, wscale; Y unless ksplit > 1)");
  SKINNY_REQUIRE(me, B > 0 && N > 0 && K > 0 && ksplit > 0, "non-positive B, N, K or ksplit");
  SKINNY_REQUIRE(me, ksplit == 1 || partial, "ksplit > 1 needs partial[ksplit][B][N]");
  SKINNY_REQUIRE(me, !(layout & 4), "layout bit 2 is the bf16 entry's: W8t says that the weights are tiled");
  GemvArgs g;
  SKINNY_REQUIRE(me, skinny_args(g, y_bf16, B, N, K, act, accumulate, ksplit, layout, 1), "unsupported shape (itts_skinny_gemm_supported)");
  g.X = (const float*)X; g.Y = (float*)Y; g.bias = bias; g.partial = partial;
  g.W8 = W8; g.W8t = W8t; g.wscale = wscale;  // g.W stays null: the fp8 instantiations read no bf16 weights
  return skinny_mfma(g, (hipStream_t)stream);
}

int itts_retile_weights(void* dst, const void* src, int N, int K, itts_stream stream) {
  (void)hipGetLastError();
  return retile_weights_bf16(dst, src, N, K, (hipStream_t)stream);
}

int itts_retile_weights_fp8(void* dst, const void* src, int N, int K, itts_stream stream) {
  (void)hipGetLastError();
  return retile_weights_fp8(dst, src, N, K, (hipStream_t)stream);
}

int itts_ln_rows_bf16(void* y, float* x, const float* gamma, const float* beta, int rows, int D, float eps, int passes,
                      const float* partial, int nsplit, const float* partial_bias, int y_tiled, itts_stream stream) {
  (void)hipGetLastError();
  const char* me = "itts_ln_rows_bf16";
  SKINNY_REQUIRE(me, y && x, "null pointer");
  SKINNY_REQUIRE(me, rows > 0 && D >= 1 && D <= 2048, "rows >= 1, 1 <= D <= 2048");
  SKINNY_REQUIRE(me, (gamma == nullptr) == (beta == nullptr), "one of gamma / beta alone");
  SKINNY_REQUIRE(me, passes >= 1 && passes <= 2, "1 or 2 passes");
  SKINNY_REQUIRE(me, nsplit >= 0 && nsplit <= 8 && (nsplit == 0 || partial), "0 .. 8 splits, partial[nsplit][rows][D] with them");
  SKINNY_REQUIRE(me, !y_tiled || D % 32 == 0, "tiled output needs D % 32 == 0");
  return ln_rows_bf16(y, x, gamma, beta, rows, D, eps, passes, partial, nsplit, partial_bias, y_tiled, (hipStream_t)stream);
}
#undef SKINNY_REQUIRE

int itts_transpose(void* y, const void* x, int B, int R, int C, int dtype, itts_stream stream) {
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  return transpose_brc(y, x, B, R, C, dtype, (hipStream_t)stream);
}

int itts_rowop(int op, const itts_rowop_args* a, itts_stream stream) {
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
#define ROWOP_REQUIRE(cond, msg)                  \
  do {                                            \
    if (!(cond)) {                                \
      set_error("itts_rowop: " msg " (" #cond ")"); \
      return E_INVALID;                           \
    }                                             \
  } while (0)
  ROWOP_REQUIRE(a, "null args");
  ROWOP_REQUIRE(op >= 0 && op < ITTS_ROWOP_COUNT, "unknown op");
  hipStream_t s = (hipStream_t)stream;
  const int tx = a->dtype_x, ty = a->dtype_y;
  const bool half_or_f32 = (tx == F32 || tx == BF16) && (ty == F32 || ty == BF16);
  const bool one_type = half_or_f32 && tx == ty;  // ops with a single element type
  const bool f32_out = half_or_f32 && ty == F32;  // statistics: fp32 results from either input type
  switch (op) {
    case ITTS_ROWOP_LAYERNORM:
      ROWOP_REQUIRE(a->y && a->x && (a->w == nullptr) == (a->b == nullptr), "layernorm: null pointer, or one of w / b alone");
      ROWOP_REQUIRE(a->rows > 0 && a->D > 0 && a->ldx >= a->D && a->ldy >= a->D, "layernorm: rows, D >= 1; ldx, ldy >= D");
      ROWOP_REQUIRE(half_or_f32, "layernorm: dtype");
      ROWOP_REQUIRE(a->act >= ACT_NONE && a->act <= ACT_SIGMOID, "layernorm: act");
      return layernorm(a->y, ty, a->x, tx, a->w, a->b, a->rows, a->D, a->ldx, a->ldy, a->eps, a->act, s);
    case ITTS_ROWOP_RMSNORM_UNIT:
      ROWOP_REQUIRE(a->y && a->x && a->w, "rmsnorm_unit: null pointer");
      ROWOP_REQUIRE(a->rows > 0 && a->D > 0, "rmsnorm_unit: rows, D >= 1");
      ROWOP_REQUIRE(f32_out, "rmsnorm_unit: dtype (fp32 output)");
      return rmsnorm_unit(a->y, ty, a->x, tx, a->w, a->rows, a->D, s);
    case ITTS_ROWOP_GLU:
      ROWOP_REQUIRE(a->y && a->x, "glu: null pointer");
      ROWOP_REQUIRE(a->rows > 0 && a->D > 0, "glu: rows, D >= 1");
      ROWOP_REQUIRE(one_type, "glu: dtype");
      return glu(a->y, a->x, a->rows, a->D, tx, s);
    case ITTS_ROWOP_GEGLU:
      ROWOP_REQUIRE(a->y && a->x, "geglu: null pointer");
      ROWOP_REQUIRE(a->rows > 0 && a->D > 0 && a->ldy >= a->D, "geglu: rows, D >= 1; ldy >= D");
      ROWOP_REQUIRE(one_type, "geglu: dtype");
      return geglu(a->y, a->x, a->rows, a->D, a->ldy, tx, s);
    case ITTS_ROWOP_DWCONV:
      ROWOP_REQUIRE(a->y && a->x && a->w, "dwconv: null pointer");
      ROWOP_REQUIRE(a->B > 0 && a->T > 0 && a->D > 0 && a->k > 0, "dwconv: B, T, D, k >= 1");
      ROWOP_REQUIRE(one_type, "dwconv: dtype");
      return dwconv(a->y, a->x, a->w, a->b, a->B, a->T, a->D, a->k, tx, s);
    case ITTS_ROWOP_CONV2D_SUB2:
      ROWOP_REQUIRE(a->y && a->x && a->w && a->b, "conv2d_sub2: null pointer");
      ROWOP_REQUIRE(a->B > 0 && a->N > 0, "conv2d_sub2: B, N >= 1");
      ROWOP_REQUIRE(a->T >= 3 && a->D >= 3, "conv2d_sub2: input below 3 x 3");
      ROWOP_REQUIRE(one_type, "conv2d_sub2: dtype");
      return conv2d_sub2(a->y, a->x, a->w, a->b, a->B, a->T, a->D, a->N, tx, s);
    case ITTS_ROWOP_CAST_COPY:
      ROWOP_REQUIRE(a->y && a->x, "cast_copy: null pointer");
      ROWOP_REQUIRE(a->rows > 0 && a->D > 0, "cast_copy: rows, D >= 1");
      ROWOP_REQUIRE(half_or_f32, "cast_copy: dtype");
      return cast_copy(a->y, ty, a->x, tx, (long)a->rows * a->D, s);
    case ITTS_ROWOP_COPY_ROWS:
      ROWOP_REQUIRE(a->y && a->x, "copy_rows: null pointer");
      ROWOP_REQUIRE(a->rows > 0 && a->D > 0 && a->ldx >= a->D && a->ldy >= a->D, "copy_rows: rows, D >= 1; ldx, ldy >= D");
      ROWOP_REQUIRE(one_type, "copy_rows: dtype");
      return copy_rows(a->y, a->ldy, a->x, a->ldx, a->rows, a->D, tx, s);
    case ITTS_ROWOP_ADD_STRIDED:
      ROWOP_REQUIRE(a->y && a->x && a->x2, "add_strided: null pointer");
      ROWOP_REQUIRE(a->rows > 0 && a->D > 0 && a->ldx >= a->D && a->ld2 >= a->D && a->ldy >= a->D,
                    "add_strided: rows, D >= 1; ldx, ld2, ldy >= D");
      ROWOP_REQUIRE(one_type, "add_strided: dtype");
      return add_strided(a->y, a->ldy, a->x, a->ldx, a->x2, a->ld2, a->rows, a->D, tx, s);
    case ITTS_ROWOP_COL_MEAN:
    case ITTS_ROWOP_COL_MEAN_STD:
      ROWOP_REQUIRE(a->y && a->x, "col_mean / col_mean_std: null pointer");
      ROWOP_REQUIRE(a->B > 0 && a->T > 0 && a->D > 0 && a->ldx >= a->D, "col_mean / col_mean_std: B, T, D >= 1; ldx >= D");
      ROWOP_REQUIRE(f32_out, "col_mean / col_mean_std: dtype (fp32 output)");
      return op == ITTS_ROWOP_COL_MEAN ? col_mean((float*)a->y, a->x, a->B, a->T, a->D, a->ldx, tx, s)
                                       : col_mean_std((float*)a->y, a->x, a->B, a->T, a->D, a->ldx, tx, s);
    case ITTS_ROWOP_SCALE_COLS_ADD:
      ROWOP_REQUIRE(a->y && a->x && a->w, "scale_cols_add: null pointer");
      ROWOP_REQUIRE(a->B > 0 && a->T > 0 && a->D > 0 && a->ldx >= a->D && a->ldy >= a->D && (!a->x2 || a->ld2 >= a->D),
                    "scale_cols_add: B, T, D >= 1; ldx, ldy, ld2 >= D");
      ROWOP_REQUIRE(one_type, "scale_cols_add: dtype");
      return scale_cols_add(a->y, a->ldy, a->x, a->ldx, a->w, a->x2, a->ld2, a->B, a->T, a->D, tx, s);
    case ITTS_ROWOP_ASP_POOL:
      ROWOP_REQUIRE(a->y && a->x && a->x2 && a->w && a->b, "asp_pool: null pointer");
      ROWOP_REQUIRE(a->B > 0 && a->T > 0 && a->D > 0, "asp_pool: B, T, D >= 1");
      ROWOP_REQUIRE(f32_out, "asp_pool: dtype (fp32 output)");
      return asp_pool((float*)a->y, a->x, a->x2, a->w, a->b, a->B, a->T, a->D, tx, s);
    case ITTS_ROWOP_RELPOS_PACK:
      ROWOP_REQUIRE(a->y && a->y2 && a->x && a->x2 && a->w && a->b, "relpos_pack: null pointer");
      ROWOP_REQUIRE(a->T > 0 && a->N > 0 && a->D > 0, "relpos_pack: T, N, D >= 1");
      ROWOP_REQUIRE(one_type, "relpos_pack: dtype");
      return relpos_pack(a->y, a->y2, a->x, a->x2, a->w, a->b, a->T, a->N, a->D, tx, s);
    case ITTS_ROWOP_DVAE_ARGMIN:
      ROWOP_REQUIRE(a->y && a->x && a->b, "dvae_argmin: null pointer");
      ROWOP_REQUIRE(a->rows > 0 && a->N > 0, "dvae_argmin: rows, N >= 1");
      ROWOP_REQUIRE(tx == F32, "dvae_argmin: dtype (fp32 dots)");
      return dvae_argmin((int*)a->y, (const float*)a->x, a->b, a->rows, a->N, s);
    default:  // ITTS_ROWOP_PAIR_ROWS
      ROWOP_REQUIRE(a->y && a->x, "pair_rows: null pointer");
      ROWOP_REQUIRE(a->B > 0 && a->T > 0 && a->D > 0, "pair_rows: B, T, D >= 1");
      ROWOP_REQUIRE(one_type, "pair_rows: dtype");
      return pair_rows(a->y, a->x, a->B, a->T, a->D, tx, s);
  }
#undef ROWOP_REQUIRE
}

// ---- token choice, operator level: the argument blocks are checked here, on the host, before anything touches the device ----
#define TOKEN_REQUIRE(name, cond, msg)          \
  do {                                          \
    if (!(cond)) {                              \
      set_error(name ": " msg " (" #cond ")");  \
      return E_INVALID;                         \
    }                                           \
  } while (0)

int itts_beam_step(const itts_beam_step_args* p, itts_stream stream) {
#define REQ(cond, msg) TOKEN_REQUIRE("itts_beam_step", cond, msg)
  REQ(p, "null args");
  REQ(p->mode == 0 || p->mode == 1, "mode 0 (candidates + select) or 1 (select on the caller's picks)");
  REQ(p->nb >= 2 && p->nb <= 10 && p->items >= 1, "2 <= num_beams <= 10, items >= 1");
  REQ(p->V >= 2 && p->V <= 15000, "2 <= V <= 15000");
  REQ(p->max_gen >= 1 && p->Smax >= 1, "max_gen, Smax >= 1");
  REQ(p->stop >= 0 && p->stop < p->V && p->start_tok >= 0 && p->start_tok < p->V && p->fake_id >= 0 && p->fake_id < p->V,
      "stop / start_tok / fake_id outside the vocabulary");
  REQ(p->len && p->cur_tok && p->unfinished && p->ids && p->anc && p->prefix && p->beam_scores && p->done, "null state pointer");
  REQ(p->hyp_tok && p->hyp_score && p->hyp_len && p->hyp_order && p->hyp_n && p->hyp_worst && p->hyp_counter, "null state pointer (hypotheses)");
  REQ(p->input_n >= 0 && (p->input_n == 0 || p->forced), "input_n > 0 needs forced");
  REQ(p->emb_bf16 == 0 || p->emb_bf16 == 1, "emb_bf16 is 0 (fp32 tables) or 1 (bf16 tables)");
  REQ(!p->h_next || (p->emb && p->pos && p->D >= 1 && p->pos_rows >= 1), "h_next needs emb, pos, D >= 1, pos_rows >= 1");
  if (p->mode == 0) {
    REQ(p->logits, "mode 0 needs logits");
    REQ(p->cand_sc && p->cand_tok && p->cand_n, "mode 0 needs the candidate scratch");
    REQ(p->do_sample == 0 || p->do_sample == 1, "do_sample 0 or 1");
    if (p->do_sample) {
      REQ(p->top_k >= 1 && p->top_k <= BEAM_MAX_CAND, "the narrow pair samples with 1 <= top_k <= 128");
      REQ(p->top_p > 0.f && p->temperature > 0.f, "top_p > 0, temperature > 0");
      REQ(p->uniforms, "do_sample needs uniforms");
    }
    REQ(p->penalty > 0.f, "penalty > 0");
  } else {
    REQ(p->pick_score && p->pick_tok && p->pick_beam, "mode 1 needs the picks");
  }
#undef REQ
  (void)hipGetLastError();  // drop stale errors left by other HIP users (torch)
  BeamArgs a;
  a.logits = p->logits; a.V = p->V; a.max_gen = p->max_gen; a.stop = p->stop; a.suppress_stop = p->suppress_stop; a.nb = p->nb;
  a.B = p->items; a.top_k = p->top_k; a.start_tok = p->start_tok; a.fake_id = p->fake_id; a.Smax = p->Smax; a.penalty = p->penalty;
  a.top_p = p->top_p; a.temperature = p->temperature; a.uniforms = p->uniforms; a.len = p->len; a.cur_tok = p->cur_tok;
  a.unfinished = p->unfinished; a.ids = p->ids; a.anc = (uint8_t*)p->anc; a.prefix_dev = p->prefix; a.beam_scores = p->beam_scores;
  a.hyp_tok = p->hyp_tok; a.hyp_score = p->hyp_score; a.hyp_len = p->hyp_len; a.hyp_order = p->hyp_order; a.hyp_n = p->hyp_n;
  a.hyp_worst = p->hyp_worst; a.hyp_counter = p->hyp_counter; a.done = p->done; a.h_next = p->h_next; a.emb = p->emb; a.pos = p->pos;
  a.D = p->D; a.pos_rows = p->pos_rows; a.emb_bf16 = p->emb_bf16; a.preprocessed = p->preprocessed; a.do_sample = p->do_sample;
  a.length_penalty = p->length_penalty; a.cand_sc = p->cand_sc; a.cand_tok = p->cand_tok; a.cand_n = p->cand_n; a.forced = p->forced;
  a.input_n = p->input_n;
  if (p->mode == 0) return beam_sample_step(a, (hipStream_t)stream);
  a.host_sc = p->pick_score; a.host_tok = p->pick_tok; a.host_beam = p->pick_beam;
  return beam_commit_step(a, (hipStream_t)stream);
}

int itts_typical_rows(const itts_typical_args* p, itts_stream stream) {
#define REQ(cond, msg) TOKEN_REQUIRE("itts_typical_rows", cond, msg)
  REQ(p, "null args");
  REQ(p->logits && p->out, "null logits / out");
  REQ(p->rows >= 1, "rows >= 1");
  REQ(p->V >= 2 && p->V <= 16384, "2 <= V <= 16384");
  REQ(p->mass > 0.f && p->mass < 1.f, "0 < mass < 1");
  REQ(p->min_keep >= 1 && p->penalty > 0.f, "min_keep >= 1, penalty > 0");
  REQ(p->stop >= 0 && p->stop < p->V, "stop outside the vocabulary");
  REQ(!(p->seen && p->beam_ids), "one seen source: the byte map or the beam histories");
  if (p->beam_ids) {
    REQ(p->len && p->max_gen >= 1, "beam_ids needs len and max_gen >= 1");
    REQ(p->start_tok >= 0 && p->start_tok < p->V && p->fake_id >= 0 && p->fake_id < p->V, "start_tok / fake_id outside the vocabulary");
  }
#undef REQ
  (void)hipGetLastError();
  TypicalArgs t;
  t.logits = p->logits; t.out = p->out; t.V = p->V; t.stop = p->stop; t.suppress_stop = p->suppress_stop; t.min_keep = p->min_keep;
  t.log_softmax_first = p->log_softmax_first; t.penalty = p->penalty; t.mass = p->mass; t.seen = (const uint8_t*)p->seen;
  t.beam_ids = p->beam_ids; t.len = p->len; t.max_gen = p->max_gen; t.start_tok = p->start_tok; t.fake_id = p->fake_id;
  return typical_filter(t, p->rows, (hipStream_t)stream);
}

// what both sampler entries ask of the state and the embedding tables (REQ: the caller's TOKEN_REQUIRE with its own name)
#define SAMPLER_STATE_CHECKS                                                                                                     \
  REQ(p, "null args");                                                                                                           \
  REQ(p->logits && p->seen && p->ids && p->cur_tok && p->unfinished && p->step, "null state pointer");                           \
  REQ(p->B >= 1 && p->V >= 1 && p->max_gen >= 1, "B, V, max_gen >= 1");                                                          \
  REQ(p->stop >= 0 && p->stop < p->V, "stop outside the vocabulary");                                                            \
  REQ(p->input_n >= 0 && (p->input_n == 0 || p->forced), "input_n > 0 needs forced");                                            \
  REQ(p->emb_bf16 == 0 || p->emb_bf16 == 1, "emb_bf16 is 0 (fp32 tables) or 1 (bf16 tables)");                                   \
  REQ(!p->h_next || (p->emb && p->pos && p->D >= 1 && p->pos_rows >= 1), "h_next needs emb, pos, D >= 1, pos_rows >= 1")

static SamplerArgs sampler_state_args(const itts_sampler_step_args* p) {  // everything but the sampling settings
  SamplerArgs a;
  a.logits = p->logits; a.seen = (uint8_t*)p->seen; a.ids = p->ids; a.cur_tok = p->cur_tok; a.unfinished = p->unfinished; a.step = p->step;
  a.V = p->V; a.max_gen = p->max_gen; a.stop = p->stop; a.suppress_stop = p->suppress_stop; a.h_next = p->h_next;
  a.emb = p->emb; a.pos = p->pos; a.D = p->D; a.pos_rows = p->pos_rows; a.emb_bf16 = p->emb_bf16; a.B = p->B; a.uniforms = p->uniforms;
  a.forced = p->forced; a.input_n = p->input_n; a.preprocessed = p->preprocessed; a.kept = p->kept;
  return a;
}

int itts_sampler_step(const itts_sampler_step_args* p, itts_stream stream) {
#define REQ(cond, msg) TOKEN_REQUIRE("itts_sampler_step", cond, msg)
  SAMPLER_STATE_CHECKS;
  REQ(p->penalty > 0.f, "penalty > 0");
  REQ(p->do_sample == 0 || p->do_sample == 1, "do_sample 0 or 1");
  if (p->do_sample) {
    REQ(p->uniforms, "do_sample needs uniforms");
    REQ(p->top_p > 0.f && p->temperature > 0.f, "top_p > 0, temperature > 0");
    if (p->top_k >= 1 && p->top_k <= BEAM_MAX_CAND)
      REQ(p->V <= 15360, "1 <= top_k <= 128 keeps the vocabulary in LDS: V <= 15360");
    else
      REQ(p->V <= 16384, "top_k outside 1..128 sorts the whole vocabulary: V <= 16384");
  }
#undef REQ
  (void)hipGetLastError();
  SamplerArgs a = sampler_state_args(p);
  a.penalty = p->penalty; a.do_sample = p->do_sample; a.top_k = p->top_k < 1 ? 0 : p->top_k; a.top_p = p->top_p; a.temperature = p->temperature;
  return sampler2_step(a, p->B, (hipStream_t)stream);
}

// every entry of a host row table, and the classes it holds (bit ROWCLS_*); 0 with *why set = refused.  No HIP call
static int row_table_classes(const itts_row_sampling* rows, int B, const char** why) {
  int classes = 0;
  for (int b = 0; b < B; ++b) {
    const itts_row_sampling& r = rows[b];
    if (r.mode != 0 && r.mode != 1) return *why = "mode is 0 (greedy) or 1 (sample)", 0;
    if (!(r.top_p > 0.f && r.top_p <= 1.f)) return *why = "0 < top_p <= 1", 0;
    if (!(r.temperature > 0.f)) return *why = "temperature > 0", 0;
    if (!(r.penalty > 0.f)) return *why = "penalty > 0", 0;
    classes |= 1 << row_class(r.mode, r.top_k);
  }
  return classes;
}

int itts_sampler_step_rows(const itts_sampler_step_args* p, const itts_row_sampling* rows_host, void* rows_dev_scratch, itts_stream stream) {
  static_assert(sizeof(itts_row_sampling) == sizeof(RowSampling) && sizeof(RowSampling) == 20, "the public row entry is the kernels' own");
#define REQ(cond, msg) TOKEN_REQUIRE("itts_sampler_step_rows", cond, msg)
  SAMPLER_STATE_CHECKS;
  REQ(rows_host && rows_dev_scratch && !((uintptr_t)rows_dev_scratch & 3), "null row table / device scratch (4-byte aligned)");
  const char* why = nullptr;
  const int classes = row_table_classes(rows_host, p->B, &why);
  if (!classes) {
    set_error(std::string("itts_sampler_step_rows: bad row entry: ") + why);
    return E_INVALID;
  }
  REQ(!(classes & ~(1 << ROWCLS_GREEDY)) || p->uniforms, "a sampled row needs uniforms");
  REQ(!(classes >> ROWCLS_NARROW & 1) || p->V <= 15360, "1 <= top_k <= 128 keeps the vocabulary in LDS: V <= 15360");
  REQ(!(classes >> ROWCLS_WIDE & 1) || p->V <= 16384, "top_k outside 1..128 sorts the whole vocabulary: V <= 16384");
#undef REQ
  (void)hipGetLastError();
  hipStream_t s = (hipStream_t)stream;
  std::vector<RowSampling> tab((size_t)p->B);
  for (int b = 0; b < p->B; ++b)
    tab[b] = {rows_host[b].mode, rows_host[b].top_k < 1 ? 0 : rows_host[b].top_k, rows_host[b].top_p, rows_host[b].temperature, rows_host[b].penalty};
  ITTS_HIP_CHECK(hipMemcpyAsync(rows_dev_scratch, tab.data(), tab.size() * sizeof(RowSampling), hipMemcpyHostToDevice, s));
  ITTS_HIP_CHECK(hipStreamSynchronize(s));  // tab is a host buffer of this call
  SamplerArgs a = sampler_state_args(p);
  a.rows = (const RowSampling*)rows_dev_scratch;
  return sampler_rows_step(a, p->B, classes, s);
}
#undef SAMPLER_STATE_CHECKS
#undef TOKEN_REQUIRE

int itts_engine_create(const itts_config* cfg, itts_engine** out) {
  if (!cfg || !out) {
    set_error("itts_engine_create: null argument");
    return E_INVALID;
  }
  if (cfg->dtype != F32 && cfg->dtype != BF16) {
    set_error("itts_engine_create: dtype must be ITTS_F32 or ITTS_BF16");
    return E_INVALID;
  }
  if (cfg->model_dim <= 0 || cfg->heads <= 0 || cfg->model_dim % cfg->heads != 0 || cfg->model_dim / cfg->heads != 64) {
    set_error("itts_engine_create: model_dim/heads must give head_dim 64");
    return E_INVALID;
  }
  if (cfg->bv_num_up > 8 || cfg->bv_num_res > 4 || cfg->bv_num_dil > 4) {
    set_error("itts_engine_create: vocoder topology out of range");
    return E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("itts_engine_create: no HIP device (this library has no CPU fallback)");
    return E_HIP;
  }
  itts_engine* e = new (std::nothrow) itts_engine();
  if (!e) return E_NOMEM;
  e->e.cfg = *cfg;
  e->e.adt = cfg->dtype;
  e->e.es = dtype_size(cfg->dtype);
  *out = e;
  return OK;
}

void itts_engine_destroy(itts_engine* e) { delete e; }

int itts_engine_bind_tensor(itts_engine* e, const char* name, const void* ptr, int dtype, int ndim, const int64_t* dims) {
  if (!e || !name || !ptr || ndim < 1 || ndim > 4 || !dims) {
    set_error("itts_engine_bind_tensor: bad argument");
    return E_INVALID;
  }
#ifdef ITTS_HALF_F16
  if (dtype == FP8) {  // the fp8 readers expand to bf16 pairs (v_cvt_scalef32_pk_bf16_fp8): BASELINE config 5 is a bf16-build mode
    set_error("itts_engine_bind_tensor: fp8 weight copies are not supported by the f16 build of the library");
    return E_INVALID;
  }
#endif
  Tensor t;
  t.p = ptr;
  t.dt = dtype;
  t.nd = ndim;
  for (int i = 0; i < ndim; ++i) t.d[i] = dims[i];
  e->e.tensors[name] = t;
  e->e.finalized = false;
  return OK;
}

int itts_engine_finalize(itts_engine* e) { return e ? e->e.finalize() : E_INVALID; }

#define ENG(e)                           \
  (void)hipGetLastError();               \
  if (!(e)) {                            \
    set_error("null engine");            \
    return E_INVALID;                    \
  }

int itts_conditioning(itts_engine* e, const void* mel, int F, float* cond_out, itts_stream s) {
  ENG(e);
  return e->e.conditioning(mel, F, cond_out, (hipStream_t)s);
}
int itts_conditioning_padded(itts_engine* e, const void* mel, int F, int F_total, float* cond_out, itts_stream s) {
  ENG(e);
  return e->e.conditioning(mel, F, cond_out, (hipStream_t)s, F_total);
}
int itts_ecapa(itts_engine* e, const void* mel, int B, int F, float* spk_out, itts_stream s) {
  ENG(e);
  return e->e.ecapa(mel, B, F, spk_out, (hipStream_t)s);
}
int itts_gpt_prefill(itts_engine* e, const float* cond, const int32_t* text_ids_host, int B, int L, int max_gen,
                     float repetition_penalty, int suppress_stop, itts_stream s) {
  ENG(e);
  return e->e.gpt_prefill(cond, text_ids_host, B, L, max_gen, repetition_penalty, suppress_stop, (hipStream_t)s);
}
int itts_gpt_set_sampling(itts_engine* e, int do_sample, int top_k, float top_p, float temperature, const float* uniforms_host,
                          int64_t n_uniforms) {
  ENG(e);
  return e->e.gpt_set_sampling(do_sample, top_k, top_p, temperature, uniforms_host, (long)n_uniforms);
}
int itts_gpt_set_sampling_rows(itts_engine* e, const itts_row_sampling* rows_host, int B, const float* uniforms_host, int64_t n_uniforms) {
  ENG(e);
  if (B < 0 || (B > 0 && !rows_host)) {
    set_error("itts_gpt_set_sampling_rows: B >= 0, and a row table for B > 0");
    return E_INVALID;
  }
  return e->e.gpt_set_sampling_rows((const RowSampling*)rows_host, B, uniforms_host, (long)n_uniforms);
}
int itts_gpt_set_beam_sample(itts_engine* e, int num_beams, int top_k, float top_p, float temperature, const float* uniforms_host,
                             int64_t n_uniforms) {
  ENG(e);
  return e->e.gpt_set_beam_sample(num_beams, top_k, top_p, temperature, uniforms_host, (long)n_uniforms);
}
int itts_gpt_set_beams(itts_engine* e, int num_beams, int do_sample, int top_k, float top_p, float temperature, float length_penalty,
                       const float* uniforms_host, int64_t n_uniforms) {
  ENG(e);
  return e->e.gpt_set_beams(num_beams, do_sample, top_k, top_p, temperature, length_penalty, uniforms_host, (long)n_uniforms);
}
int itts_gpt_set_beam_returns(itts_engine* e, int num_return_sequences) {
  ENG(e);
  return e->e.gpt_set_beam_returns(num_return_sequences);
}
int itts_gpt_set_typical(itts_engine* e, float mass) {
  ENG(e);
  return e->e.gpt_set_typical(mass);
}
int itts_gpt_set_input_tokens(itts_engine* e, const int32_t* ids_host, int B, int n) {
  ENG(e);
  return e->e.gpt_set_input_tokens(ids_host, B, n);
}
int itts_gpt_decode_mode(itts_engine* e) { return e ? e->e.ds.last_mode : -1; }
int itts_gpt_set_cond_per_row(itts_engine* e, int on) {
  ENG(e);
  e->e.cond_per_row = on ? 1 : 0;
  return OK;
}
int itts_gpt_set_host_sampling(itts_engine* e, int on) {
  ENG(e);
  return e->e.gpt_set_host_sampling(on);
}
int itts_gpt_commit(itts_engine* e, const int32_t* tokens_host, itts_stream s) {
  ENG(e);
  return e->e.gpt_commit(tokens_host, (hipStream_t)s);
}
int itts_gpt_beam_state(itts_engine* e, int32_t* ids_host, float* scores_host, int32_t* done_host, int* step_host, itts_stream s) {
  ENG(e);
  return e->e.gpt_beam_state(ids_host, scores_host, done_host, step_host, (hipStream_t)s);
}
int itts_gpt_commit_beams(itts_engine* e, const float* pick_score_host, const int32_t* pick_tok_host, const int32_t* pick_beam_host,
                          itts_stream s) {
  ENG(e);
  return e->e.gpt_commit_beams(pick_score_host, pick_tok_host, pick_beam_host, (hipStream_t)s);
}
int itts_gpt_beam_picks(itts_engine* e, float* score_host, int32_t* tok_host, int32_t* beam_host, int32_t* kept_host, itts_stream s) {
  ENG(e);
  return e->e.gpt_beam_picks(score_host, tok_host, beam_host, kept_host, (hipStream_t)s);
}
int itts_gpt_set_forced(itts_engine* e, const int32_t* ids_host, int B, int n) {
  ENG(e);
  return e->e.gpt_set_forced(ids_host, B, n);
}
int itts_gpt_decode(itts_engine* e, int nsteps, itts_stream s) {
  ENG(e);
  return e->e.gpt_decode(nsteps, (hipStream_t)s);
}
int itts_gpt_status(itts_engine* e, int* steps, int* n_unf, itts_stream s) {
  ENG(e);
  return e->e.gpt_status(steps, n_unf, (hipStream_t)s);
}
int itts_gpt_fetch(itts_engine* e, int32_t* codes, float* logits, itts_stream s) {
  ENG(e);
  return e->e.gpt_fetch(codes, logits, (hipStream_t)s);
}
int itts_gpt_retire_rows(itts_engine* e, int* rows_now_host, itts_stream s) {
  ENG(e);
  return e->e.gpt_retire_rows(rows_now_host, (hipStream_t)s);
}
int itts_gpt_set_retire_beams(itts_engine* e, int on) {
  ENG(e);
  return e->e.gpt_set_retire_beams(on);
}
int itts_gpt_set_admit_beams(itts_engine* e, int on) {
  ENG(e);
  return e->e.gpt_set_admit_beams(on);
}
int itts_gpt_rows(itts_engine* e) { return e ? (e->e.ds.active ? e->e.ds.B : 0) : -1; }
int itts_gpt_admit_rows(itts_engine* e, const float* cond, int cond_rows, const int32_t* text_ids_host, int n, int L,
                        const itts_row_sampling* rows_host, const float* uniforms_host, const int32_t* forced_host, int n_forced,
                        int32_t* slots_host, itts_stream s) {
  ENG(e);
  return e->e.gpt_admit_rows(cond, cond_rows, text_ids_host, n, L, (const RowSampling*)rows_host, uniforms_host, forced_host, n_forced,
                             slots_host, (hipStream_t)s);
}
int itts_gpt_row_status(itts_engine* e, int32_t* orig_host, int32_t* len_host, int32_t* unfinished_host, itts_stream s) {
  ENG(e);
  return e->e.gpt_row_status(orig_host, len_host, unfinished_host, (hipStream_t)s);
}
int itts_gpt_graph_captures(itts_engine* e) { return e ? e->e.ds.graph_captures : -1; }
int itts_gpt_rows_total(itts_engine* e) { return e ? (e->e.ds.active ? e->e.ds.B0 : 0) : -1; }
int itts_gpt_keep_row_table(itts_engine* e, int on) {
  ENG(e);
  return e->e.gpt_keep_row_table(on);
}
int itts_gpt_latent(itts_engine* e, const float* cond, const int32_t* text_ids_host, int L, const int32_t* codes_host,
                    int T, void* latent_out, itts_stream s) {
  ENG(e);
  return e->e.gpt_latent(cond, text_ids_host, L, codes_host, T, latent_out, (hipStream_t)s);
}
int itts_gpt_latent_batch(itts_engine* e, const float* cond, const int32_t* text_ids_host, const int32_t* text_lens_host,
                          const int32_t* codes_host, const int32_t* code_lens_host, int nseq, void* latent_out,
                          itts_stream s) {
  ENG(e);
  return e->e.gpt_latent_batch(cond, text_ids_host, text_lens_host, codes_host, code_lens_host, nseq, latent_out,
                               (hipStream_t)s);
}
int itts_gpt_latent_batch_cond(itts_engine* e, const float* cond, const int32_t* cond_index_host, int n_cond, const int32_t* text_ids_host,
                               const int32_t* text_lens_host, const int32_t* codes_host, const int32_t* code_lens_host, int nseq,
                               void* latent_out, itts_stream s) {
  ENG(e);
  if (!cond_index_host || n_cond < 1) {
    set_error("itts_gpt_latent_batch_cond: needs cond_index_host and n_cond >= 1");
    return E_INVALID;
  }
  return e->e.gpt_latent_batch(cond, text_ids_host, text_lens_host, codes_host, code_lens_host, nseq, latent_out, (hipStream_t)s,
                               cond_index_host, n_cond);
}
int itts_gpt_latent_packed(itts_engine* e, const float* cond, const int32_t* cond_index_host, int n_cond, const int32_t* text_ids_host,
                           const int32_t* text_lens_host, const int32_t* codes_host, const int32_t* code_lens_host, int nseq,
                           void* latent_out, itts_stream s) {
  ENG(e);
  return e->e.gpt_latent_packed(cond, text_ids_host, text_lens_host, codes_host, code_lens_host, nseq, latent_out, (hipStream_t)s,
                                cond_index_host, n_cond);
}
int itts_gpt_latent_stream_open(itts_engine* e, const float* cond, const int32_t* cond_index_host, int n_cond, const int32_t* text_ids_host,
                                const int32_t* text_lens_host, int nseq, int max_codes, itts_stream s) {
  if (!e) {
    set_error("itts_gpt_latent_stream_open: null engine");
    return E_INVALID;
  }
  (void)hipGetLastError();
  return e->e.gpt_latent_stream_open(cond, cond_index_host, n_cond, text_ids_host, text_lens_host, nseq, max_codes, (hipStream_t)s);
}
int itts_gpt_latent_stream_append(itts_engine* e, const int32_t* codes_host, const int32_t* counts_host, void* latent_out, itts_stream s) {
  if (!e) {
    set_error("itts_gpt_latent_stream_append: null engine");
    return E_INVALID;
  }
  (void)hipGetLastError();
  return e->e.gpt_latent_stream_append(codes_host, counts_host, latent_out, (hipStream_t)s);
}
int itts_gpt_latent_stream_close(itts_engine* e) {
  if (!e) {
    set_error("itts_gpt_latent_stream_close: null engine");
    return E_INVALID;
  }
  (void)hipGetLastError();
  return e->e.gpt_latent_stream_close(nullptr);
}
int itts_bigvgan(itts_engine* e, const void* latent, const float* spk, int B, int T, float* wav_out, itts_stream s) {
  ENG(e);
  return e->e.bigvgan(latent, spk, B, T, wav_out, (hipStream_t)s);
}
int itts_bigvgan_ragged(itts_engine* e, const void* latent, const float* spk, int B, int T, const int32_t* lens_host, float* wav_out,
                        itts_stream s) {
  // refused before any HIP call
  const char* why = !e ? "null engine" : (!latent || !spk || !lens_host || !wav_out) ? "null pointer" : nullptr;
  if (!why && (B < 1 || B > e->e.cfg.max_batch)) why = "B outside [1, max_batch]";
  if (!why && T < 1) why = "T < 1";
  for (int b = 0; !why && b < B; ++b)
    if (lens_host[b] < 1 || lens_host[b] > T) why = "a length outside [1, T]";
  if (why) {
    set_error(std::string("itts_bigvgan_ragged: ") + why);
    return E_INVALID;
  }
  (void)hipGetLastError();
  return e->e.bigvgan(latent, spk, B, T, wav_out, (hipStream_t)s, lens_host);
}
int itts_bigvgan_packed(itts_engine* e, const void* latent, const float* spk, const int32_t* off_host, const int32_t* lens_host, int n,
                        float* wav_out, itts_stream s) {
  if (!e) {
    set_error("itts_bigvgan_packed: null engine");
    return E_INVALID;
  }
  if (int st = itts_bigvgan_packed_check(&e->e.cfg, latent, spk, off_host, lens_host, n, wav_out)) return st;  // before any HIP call
  (void)hipGetLastError();
  return e->e.bigvgan_packed(latent, spk, off_host, lens_host, n, wav_out, (hipStream_t)s);
}
int itts_dvae_decode(itts_engine* e, const int32_t* codes_host, int B, int T, void* mel_out, itts_stream s) {
  ENG(e);
  return e->e.dvae_decode(codes_host, B, T, mel_out, (hipStream_t)s);
}

int itts_dvae_encode(itts_engine* e, const void* mel_btc, int B, int T, int32_t* codes_host, itts_stream s) {
  ENG(e);
  return e->e.dvae_encode(mel_btc, B, T, codes_host, (hipStream_t)s);
}

int itts_debug_enable(itts_engine* e, int on) {
  ENG(e);
  e->e.debug = on & 1;
  e->e.force_simple = (on & 2) != 0;
  e->e.use_graph = (on & 4) == 0;
  e->e.ds.fuse = (on & 8) != 0;  // bit 3: the fused projection + attention launch instead of two launches (A/B, parity tests)
  e->e.ds.eng_off = (on & 16) != 0;  // bit 4: the launch path instead of the persistent decode engine (A/B, parity tests)
  e->e.ds.eng_force = (on & 32) != 0;  // bit 5: the persistent decode engine whatever ITTS_ENGINE says
  return OK;
}

int itts_gpt_set_engine_fp8(itts_engine* e, int on) {
  ENG(e);
  e->e.ds.eng_fp8 = on != 0;
  return OK;
}

int itts_gpt_set_kv_fp8(itts_engine* e, int on) {
  ENG(e);
  if (on && e->e.adt != BF16) {
    set_error("itts_gpt_set_kv_fp8: the fp8 (e4m3) K/V cache needs a 16-bit engine, this one is fp32");
    return E_INVALID;
  }
  e->e.ds.kv_fp8 = on != 0;  // latched by the next itts_gpt_prefill
  return OK;
}

int itts_gpt_set_engine_kv_fp8(itts_engine* e, int on) {
  ENG(e);
  return e->e.gpt_set_engine_kv_fp8(on);
}

int64_t itts_debug_fetch(itts_engine* e, const char* name, float* out_host, int64_t max_elems) {
  if (!e || !name) return -1;
  auto it = e->e.taps.find(name);
  if (it == e->e.taps.end()) return -1;
  const int64_t n = (int64_t)it->second.size();
  if (out_host) std::memcpy(out_host, it->second.data(), (size_t)std::min(n, max_elems) * 4);
  return n;
}

}  // extern "C"

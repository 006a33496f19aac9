/* libitts_hip - C ABI of the MI355X-native IndexTTS hot path.
 *
 * Conventions: plain pointers and sizes, no torch types; every pointer is a DEVICE pointer
 * unless the parameter name ends in `_host`; the caller allocates outputs; calls are asynchronous on the
 * given HIP stream unless stated; the return value is 0 or a negative error code (ITTS_E_*) and
 * `itts_last_error()` returns the message (thread-local).  One engine per host thread (the reference's
 * web UI shares one engine between threads without a lock, webui.py:441-452: callers must serialise).
 *
 * dtype codes: 0 = f32, 1 = bf16, 5 = f16 (itts_snake_aa_fwd only).  Activations are channels-last ([B, T, C]) everywhere.
 */
#ifndef ITTS_HIP_H
#define ITTS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* itts_stream; /* hipStream_t */
typedef struct itts_engine itts_engine;

#define ITTS_F32 0
#define ITTS_BF16 1
#define ITTS_FP8 4 /* OCP e4m3fn bytes without a scale: the opt-in K/V cache type (itts_decode_attn, itts_kv_scatter, itts_gpt_set_kv_fp8) */
#define ITTS_F16 5 /* IEEE half: accepted by itts_snake_aa_fwd only (the reference op dispatches float/half/bf16) */

/* status codes */
#define ITTS_OK 0
#define ITTS_E_INVALID (-1)
#define ITTS_E_HIP (-2)
#define ITTS_E_NOMEM (-3)
#define ITTS_E_STATE (-4)
#define ITTS_E_MISSING (-5)
/* itts_gpt_status / itts_gpt_fetch: a hand-off wait inside the persistent decode engine gave up (20 ms wall clock; the engine
 * needs the 256 CUs of its GPU to itself - ONE process per GPU).  The codes of this generation are not valid;
 * the engine object has switched itself to the five-launches-per-block path, so the caller simply generates again (the Python
 * shim does, once, with a logged warning). */
#define ITTS_E_HANDOFF (-6)

const char* itts_last_error(void);
int itts_abi_version(void);
/* The 16-bit storage type behind dtype code ITTS_BF16 in THIS build of the library: 0 = bfloat16 (libitts_hip.so), 1 = IEEE
 * binary16 (libitts_hip_f16.so: the same sources with -DITTS_HALF_F16 - the reference's GPU precision, `is_fp16=True` =
 * fp16 autocast / .half(), indextts/infer.py:39,44,52).  Weights, activations and the K/V cache are stored in it; accumulation is
 * fp32 in both.  The f16 build has no fp8 weight copies (BASELINE config 5 is a bf16-build mode). */
int itts_half_is_f16(void);

/* ---- operator level -------------------------------------------------------------------------------- */

/* Fused anti-aliased SnakeBeta.  Replaces the reference's only native entry point
 *   anti_alias_activation_cuda.forward(input, up_filter, down_filter, alpha, beta) -> Tensor
 *   (indextts/BigVGAN/alias_free_activation/cuda/anti_alias_activation.cpp:19-23, fwd_cuda .cu:214-256)
 * Same contract: alpha/beta are LOG-scale fp32 [C]; filters fp32 [12]; dst has the shape/dtype of src;
 * src is not modified.  layout 0 = [B, C, T] (the reference's), 1 = [B, T, C] (engine-native). */
int itts_snake_aa_fwd(void* dst, const void* src, const float* up12, const float* down12, const float* log_alpha,
                      const float* log_beta, int B, int C, int T, int dtype, int layout, itts_stream stream);

/* Generic linear / conv1d / transposed conv1d on channels-last activations (replaces nn.Linear, nn.Conv1d,
 * nn.ConvTranspose1d calls of BigVGAN/models.py:149-161,184 and the conformer/GPT projections).
 * W is [nphase][N][taps*Cin].  See csrc/itts_common.h GemmArgs for the epilogue definition. */
typedef struct {
  const void* A; const void* W; void* C;
  int M, N, Cin, taps, lda, ldc, T, dil, pad_left, pad_mode, in_up, nphase;
  int phase_shift[8];
  const float* bias; int bias_bstride; int act;
  const float* scale; const float* shift; int act2;
  const void* R; int ldr; float alpha;
  const void* ADD; int ldadd; float beta;
  int dtype_a, dtype_w, dtype_c;
  int force_simple; /* 1 = vector-ALU kernel even when the MFMA kernel supports the shape */
} itts_gemm_args;
int itts_gemm(const itts_gemm_args* args, itts_stream stream);
/* Which kernel family itts_gemm takes for these arguments (no launch): 0 vector ALU, 1 register-staged MFMA, 2 LDS-DMA staged
 * 128-wide tiles, 3 the 256 x 256 eight-phase kernel, 4 the LDS-tiled narrow conv.  Tests and tools/bench_gemm.py use it. */
int itts_gemm_which(const itts_gemm_args* args);
/* itts_gemm on ONE kernel family named by the caller, whatever itts_gemm_which would answer: family 0 - 3 as above (family 4 runs
 * through itts_gemm / itts_act_conv).  The families' own launchers, i.e. the production code path, below the tile counts at which the
 * selector sends a shape to them - the operator tests (tests/test_gpu_gemm_family.py) run every kernel at the smallest shapes that
 * reach its paths.  variant: 0 = whatever that family's launcher picks; family 1 only: tile | depth << 4 | nbuf << 8 with tile
 * 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 128x32, depth 1 / 2 / 4 chunk pairs in flight, nbuf 1 / 2 LDS buffers (tiles 1 - 3 need
 * N >= 64).  ksplit: 1 = none; > 1, family 3 only: that many K splits into ws (16-byte aligned, ws_bytes >= ksplit * M * N * 4,
 * nphase == 1, (ksplit - 1) * ceil(nk / ksplit) < nk for nk = taps * Cin / 64 K-tiles).  Never falls back to another family:
 * whatever the family's launcher would refuse is refused here with ITTS_E_INVALID and a message before any HIP call - null args or
 * pointers, an unknown family or variant, dtype, lda / ldc, M % T, force_simple on a family other than 0, and every shape outside the
 * family's structural rule (1: Cin % 8, M >= 16; 2: Cin % 64, in_up == 1, nphase == 1, N >= 64, M >= 256; 3: Cin % 64, in_up == 1,
 * N >= 192, N % 64, taps * Cin >= 256).  itts_gemm_family_supported: 1 / 0, no launch (the workspace by its size alone). */
int itts_gemm_family(const itts_gemm_args* args, int family, int variant, int ksplit, void* ws, size_t ws_bytes, itts_stream stream);
int itts_gemm_family_supported(const itts_gemm_args* args, int family, int variant, int ksplit, size_t ws_bytes);
/* conv (itts_gemm semantics) whose input A is Activation1d(A) applied inside the kernel (conv_lds.hip ACT): the anti-aliased
 * SnakeBeta of itts_snake_aa_fwd (log_alpha / log_beta fp32 [Cin], filt12 the 12-tap filter, up = down) runs while the input tile
 * is staged, and the convolution sees exactly the 16-bit values itts_snake_aa_fwd (layout 1) would have written - the a -> conv of
 * the narrow BigVGAN stages as the engine issues it.  A is the PRE-activation tensor and is not modified.
 * Refuses (ITTS_E_INVALID, before any HIP call) whatever it cannot run FUSED - it never runs the conv without the activation:
 * null args or pointers, force_simple, a dtype that is not the 16-bit one, lda != Cin, every shape itts_gemm_which does not answer
 * 4 for (T < 256, Cin > 96 or < 16, N % 8, reflect padding, taps < 3, (taps - 1) * dil > 64, nphase / in_up != 1,
 * ITTS_NO_CONV_LDS set) and ITTS_NO_CONV_ACT set (both switches are read per call).  itts_act_conv_supported: 1 / 0, no launch. */
int itts_act_conv(const itts_gemm_args* args, const float* log_alpha, const float* log_beta, const float* filt12, itts_stream stream);
int itts_act_conv_supported(const itts_gemm_args* args);

/* ---- padded ragged batches (the vocoder over latents of unequal length) ----
 * A [B, T, C] tensor holds B signals of lens_dev[b] * mul rows each (lens_dev: device int32 [B]; mul >= 1, the up-sampling between
 * the unit of the lengths and this tensor's rows; a product outside [0, T] is clamped to it; the fused convolution
 * clamps to [1, T]).  All three refuse null pointers,
 * B < 1, T < 1, C < 1 and mul < 1 with ITTS_E_INVALID before any HIP call; the lengths are device memory and are not read on the host.
 *
 * itts_snake_aa_fwd_len: itts_snake_aa_fwd, layout 1 ([B, T, C]) only, with the signal of item b ending at row lens_dev[b] * mul - its
 * replicate padding is taken there, not at the end of the buffer.  The first lens_dev[b] * mul rows of dst have the bits of
 * itts_snake_aa_fwd on the item cut to that length, the rows behind them are written as zeros.  dtype 0 / 1 / 5 as there.
 * itts_act_conv_len: itts_act_conv with the same per-item signal length inside the fused Activation1d (args->T stays the row count of
 * the buffers): the convolution reads zeros behind an item's end - the zero "same" padding the item would see alone.  Every output row
 * is stored; rows < lens_dev[b] * mul have the bits of itts_snake_aa_fwd_len followed by itts_gemm.  The refusals of itts_act_conv.
 * itts_zero_tail_rows: rows [lens_dev[b] * mul, T) of item b of x become zeros, nothing else is written.  dtype 0 / 1; B <= 65535. */
int itts_snake_aa_fwd_len(void* dst, const void* src, const float* up12, const float* down12, const float* log_alpha,
                          const float* log_beta, int B, int C, int T, const int* lens_dev, int mul, int dtype, itts_stream stream);
int itts_act_conv_len(const itts_gemm_args* args, const float* log_alpha, const float* log_beta, const float* filt12,
                      const int* lens_dev, int mul, itts_stream stream);
int itts_zero_tail_rows(void* x, int B, int T, int C, const int* lens_dev, int mul, int dtype, itts_stream stream);
/* ---- packed sentences (the vocoder over sentences back to back in ONE item) ----
 * A [off[n] * mul, C] tensor holds n sentences back to back in time: sentence b owns rows [off_host[b] * mul, off_host[b + 1] * mul) -
 * its capacity - of which the first lens_host[b] * mul are signal (off_host: host int32 [n + 1], lens_host: host int32 [n]; mul >= 1,
 * the up-sampling between the unit of the table and this tensor's rows).  The table is read on the host and travels by value in the
 * kernels' argument block: nothing of the caller's outlives the call.  All three refuse with ITTS_E_INVALID before any HIP call:
 * null pointers, n outside [1, 128], mul < 1, off[0] < 0, a length < 1, offsets not increasing, a capacity below its length,
 * off[n] * mul >= 2^31, C < 1, an unsupported dtype.  Rows outside [off[0] * mul, off[n] * mul) are never written.
 *
 * itts_snake_aa_fwd_seg: itts_snake_aa_fwd (layout 1) per sentence - the replicate padding is taken at the sentence's own last signal
 * row; its signal rows have the bits of itts_snake_aa_fwd on the sentence cut out, the rest of its capacity is written as zeros.
 * dtype 0 / 1 / 5.
 * itts_act_conv_seg: itts_act_conv per sentence (one grid row each): rows before a sentence's first and behind its last signal row
 * enter the convolution as zeros, output rows are stored up to the capacity and never beyond.  args->M == args->T >= off[n] * mul (one
 * item that holds the pack).  Signal rows have the bits of itts_snake_aa_fwd_seg followed by itts_gemm on the whole pack wherever
 * the gaps are at least the convolution's reach.  The shape rule is itts_gemm_which_pinned_conv == 4, i.e. that of itts_act_conv
 * apart from the row count (a sentence of one row runs); also refused: force_simple, a dtype that is not the 16-bit one,
 * lda != Cin, a bias with bias_bstride != 0 (the pack is one item and its bias one row of N; per-sentence rows are
 * itts_seg_bias_mask's), ITTS_NO_CONV_LDS / ITTS_NO_CONV_ACT set.
 * itts_seg_bias_mask: the signal rows of sentence b get bias[b][0 .. C) added (fp32 [n, C], one fp32 sum rounded to the tensor's type;
 * bias NULL = they are left alone), the rest of its capacity becomes zeros.  dtype 0 / 1.  16-byte units where a row is a whole number
 * of them and x is 16-byte aligned, else one element (4 or 2 bytes) per lane.
 * itts_gemm_which_pinned_conv: the family the packed vocoder takes for a convolution (no launch): 4 where the shape apart from its
 * row count is the narrow conv's, else 3 (gemm_p8 wherever it can run the shape), 1, 0 - never 2, never by M or T. */
int itts_snake_aa_fwd_seg(void* dst, const void* src, const float* up12, const float* down12, const float* log_alpha,
                          const float* log_beta, int C, const int32_t* off_host, const int32_t* lens_host, int n, int mul, int dtype,
                          itts_stream stream);
int itts_act_conv_seg(const itts_gemm_args* args, const float* log_alpha, const float* log_beta, const float* filt12,
                      const int32_t* off_host, const int32_t* lens_host, int n, int mul, itts_stream stream);
int itts_seg_bias_mask(void* x, const float* bias, int C, const int32_t* off_host, const int32_t* lens_host, int n, int mul, int dtype,
                       itts_stream stream);
int itts_gemm_which_pinned_conv(const itts_gemm_args* args);
/* Which instantiation the bf16 decode GEMV of the launch path (1-4 rows) takes for a call (no launch): -1 = it does not take the
 * call, else nb | rpw << 4 | nch << 8 | waves << 16 (batch rows compiled in, weight rows per wave, 512-column chunks per lane, waves
 * per workgroup).  w5 = the ITTS_GEMV_W5 rows.  tests/test_gemv_selector.py uses it. */
int itts_gemv_which(int B, int N, int K, int prologue, int x_bf16, int y_bf16, int w5);
/* itts_gemm with a caller-owned fp32 workspace (16-byte aligned, ws_bytes long): few-tile, deep-K shapes (M x N in fewer than 128
 * tiles of 256 x 256, K >= 1024) split K over up to 8 workgroups per tile - raw sums into ws[split][M][N], a second launch adds
 * them in split order (deterministic) and runs the epilogue.  Other shapes run exactly as itts_gemm.  itts_gemm_ksplit returns the
 * split count the call would use (1 = none) without launching.  The engine's own GEMMs use a 64 MiB workspace of the engine. */
int itts_gemm_ws(const itts_gemm_args* args, void* ws, size_t ws_bytes, itts_stream stream);
int itts_gemm_ksplit(const itts_gemm_args* args, size_t ws_bytes);

int itts_layernorm(void* y, int dtype_y, const void* x, int dtype_x, const float* gamma, const float* beta, int rows,
                   int D, float eps, itts_stream stream);

/* attention over strided q/k/v (see csrc/itts_kernels.h AttnArgs) */
int itts_attention(void* o, const void* q, const void* k, const void* v, int B, int H, int Sq, int Sk, int dqk, int dv,
                   int ldq, int ldk, int ldv, int ldo, float scale, int causal, const int* kv_start, int dtype,
                   itts_stream stream);
/* itts_attention on ONE kernel named by the caller: kernel 0 = the dispatcher (exactly itts_attention), 1 = attention_simple
 * (csrc/attention.hip: vector ALU, fp32 or 16-bit, dqk <= 128, dv <= 64), 2 = attention_mfma (csrc/attention_mfma.hip: matrix cores,
 * 16-bit, dqk 64 or 128, dv 64, Sq >= 16, ldq / ldk / ldv % 8 == 0, q / k / v 16-byte aligned).  The named kernel runs or nothing
 * does - never the other one.  The operator tests (tests/test_gpu_attention.py) run each kernel at every shape this way.
 * itts_attention_which: 1 or 2, the kernel the dispatcher takes for the call (ITTS_ATTN_SIMPLE, read once per process, makes it 1),
 * without a launch; -1 for a call the entries refuse.  All three entries share one host-side check, made before any HIP call, that
 * answers ITTS_E_INVALID with a message that begins with the entry's name: a null q / k / v / o; B, H, Sq or Sk <= 0; B or H > 65535;
 * a dtype other than ITTS_F32 / ITTS_BF16 (the library's 16-bit type); dqk outside 1..128 or dv outside 1..64; ldq or ldk < H * dqk,
 * ldv or ldo < H * dv; a kernel other than 0, 1, 2; and for kernel 2 whatever the matrix-core kernel's rule above rejects. */
int itts_attention_kernel(void* o, const void* q, const void* k, const void* v, int B, int H, int Sq, int Sk, int dqk, int dv,
                          int ldq, int ldk, int ldv, int ldo, float scale, int causal, const int* kv_start, int dtype, int kernel,
                          itts_stream stream);
int itts_attention_which(const void* q, const void* k, const void* v, int B, int H, int Sq, int Sk, int dqk, int dv, int ldq,
                         int ldk, int ldv, int ldo, float scale, int causal, const int* kv_start, int dtype);

/* Causal self-attention over PACKED sequences (csrc/attention_varlen.hip): sequence b owns token rows [seq_off_host[b],
 * seq_off_host[b + 1]) of q, k, v and o (row r, head h, dim d at q[r * ldq + h * dqk + d], likewise k, v with dv, o with ldo); query i
 * of a sequence sees keys 0 .. i of the same sequence and nothing else.  No pad rows, and every sequence is tiled from its own key 0:
 * a sequence's output has the same bits alone, with any companions and in any order, and they are the bits of
 * itts_attention_kernel(B = 1, Sq = Sk = len, causal = 1, kv_start = NULL) of the same kernel family on that sequence's rows.
 * seq_off_host: nseq + 1 host ints, passed to the kernel by value (no upload; the array may be reused once the call returns).
 * kernel: 0 = the dispatcher, 1 = attn_varlen_simple (vector ALU, fp32 or the 16-bit type, dqk <= 128, dv <= 64), 2 =
 * attn_varlen_mfma (matrix cores: the 16-bit type, dqk = dv = 64, ldq / ldk / ldv % 8 == 0, q / k / v 16-byte aligned - and EVERY
 * length >= 1).  The named kernel runs or nothing does.  The dispatcher's pick depends on type, head dims, leading dims and
 * alignment only, never on a length (ITTS_ATTN_SIMPLE, read once per process, makes it 1).
 * itts_attention_varlen_which: 1 or 2, that pick, without a launch; -1 for a call the entry refuses.
 * Both share one host-side check, made before any HIP call, that answers ITTS_E_INVALID with a message that begins with the entry's
 * name: a null q / k / v / o / seq_off_host; nseq outside 1 .. ITTS_VARLEN_MAX_SEQ; seq_off_host[0] != 0; offsets that are not strictly
 * increasing (a length < 1); H outside 1 .. 65535; a dtype other than ITTS_F32 / ITTS_BF16 (the library's 16-bit type); dqk outside
 * 1..128 or dv outside 1..64; ldq or ldk < H * dqk, ldv or ldo < H * dv; a kernel other than 0, 1, 2; and for kernel 2 whatever the
 * matrix-core kernel's rule above rejects. */
#define ITTS_VARLEN_MAX_SEQ 128
int itts_attention_varlen(void* o, const void* q, const void* k, const void* v, const int32_t* seq_off_host, int nseq, int H, int dqk,
                          int dv, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, int kernel, itts_stream stream);
int itts_attention_varlen_which(const void* q, const void* k, const void* v, const int32_t* seq_off_host, int nseq, int H, int dqk,
                                int dv, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, int kernel);

/* Causal self-attention for APPENDED rows (csrc/attention_append.hip; the incremental packed latent pass).  Sequence b
 * brings n_new_host[b] new queries, positions pos0_host[b] .. pos0_host[b] + n_new_host[b] - 1, in rows q_off_host[b] .. of q and o (the
 * chunk's buffers: row r, head h, dim d at q[r * ldq + h * dqk + d], o likewise with dv and ldo); its keys and values are rows
 * 0 .. pos0 + n_new - 1 of its block of a K/V history, which starts at row kv_off_host[b] of k_hist / v_hist (ldk, ldv) and holds
 * kv_off_host[b + 1] - kv_off_host[b] rows - the new rows' k / v are already there (itts_kv_rows_append).  Query at position i sees keys
 * 0 .. i.  n_new_host[b] = 0 leaves sequence b alone.
 * The bit relation: a delivered row has the bits itts_attention_varlen of the same kernel number gives that row in a pass over the
 * COMPLETE sequence (query tiles aligned to the sequence's key 0, 64-key tiles from key 0, the same mask, online-softmax update, P
 * rounding and store).  Rows of a tile in front of pos0 are never stored; o rows outside the appended ranges are not touched; no key
 * row at or behind pos0 + n_new is read, whatever the history holds there.
 * q_off_host, kv_off_host: nseq + 1 host ints each (non-decreasing, [0] >= 0); pos0_host, n_new_host: nseq host ints; all four are
 * passed to the kernel by value (no upload; the arrays may be reused once the call returns).
 * kernel: 0 = the dispatcher, 1 = attn_append_simple (vector ALU, fp32 or the 16-bit type, dqk <= 128, dv <= 64), 2 = attn_append_mfma
 * (matrix cores: the 16-bit type, dqk = dv = 64, ldq / ldk / ldv % 8 == 0, q / k_hist / v_hist 16-byte aligned).  The named kernel runs or
 * nothing does.  The dispatcher's pick is itts_attention_varlen's rule: type, head dims, leading dims and alignment only, never a length
 * or a count (ITTS_ATTN_SIMPLE, read once per process, makes it 1).
 * itts_attention_append_which: 1 or 2, that pick, without a launch; -1 for a call the entry refuses.
 * Both share one host-side check, made before any HIP call, that answers ITTS_E_INVALID with a message that begins with the entry's
 * name: a null q / k_hist / v_hist / o or array; nseq outside 1 .. ITTS_VARLEN_MAX_SEQ; a negative offset, pos0 or n_new; offsets that
 * decrease; n_new past the sequence's rows of q / o; pos0 + n_new past the sequence's history block; H outside 1 .. 65535; a dtype other
 * than ITTS_F32 / ITTS_BF16 (the library's 16-bit type); dqk outside 1..128 or dv outside 1..64; ldq or ldk < H * dqk, ldv or ldo < H * dv;
 * a kernel other than 0, 1, 2; and for kernel 2 whatever the matrix-core kernel's rule above rejects. */
int itts_attention_append(void* o, const void* q, const void* k_hist, const void* v_hist, const int32_t* q_off_host,
                          const int32_t* kv_off_host, const int32_t* pos0_host, const int32_t* n_new_host, int nseq, int H, int dqk, int dv,
                          int ldq, int ldk, int ldv, int ldo, float scale, int dtype, int kernel, itts_stream stream);
int itts_attention_append_which(const void* q, const void* k_hist, const void* v_hist, const int32_t* q_off_host,
                                const int32_t* kv_off_host, const int32_t* pos0_host, const int32_t* n_new_host, int nseq, int H, int dqk,
                                int dv, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, int kernel);
/* The history write that goes in front of it (kv_rows_append_kernel, one launch): for r < n_new_host[b], columns [0, wk) of k_src row
 * q_off_host[b] + r go to k_hist row kv_off_host[b] + pos0_host[b] + r, columns [0, wv) of v_src to the same row of v_hist (ld_src is
 * the row stride of both sources - the k and v thirds of a qkv tensor).  fp32 or the 16-bit type, no conversion.  The same arrays and
 * the same host-side refusals as above (message "itts_kv_rows_append: ..."), plus widths < 1 and a leading dim below its width. */
int itts_kv_rows_append(void* k_hist, void* v_hist, const void* k_src, const void* v_src, const int32_t* q_off_host,
                        const int32_t* kv_off_host, const int32_t* pos0_host, const int32_t* n_new_host, int nseq, int ld_src, int ldk,
                        int ldv, int wk, int wv, int dtype, itts_stream stream);

/* Decode-step batched GEMV (GPT2 Conv1D on one token per row, HF GPT2Attention/GPT2MLP):
 * Y[b, n] (+)= act(prologue(X)[b, :] . W[n, :] + bias[n]); X, Y fp32; prologue 0 none, 1 LayerNorm, 2 LN o LN.
 * version 0 = auto, 1 = generic kernel, 2 = register-resident kernel (B <= 4). */
int itts_gemv(float* Y, const float* X, const void* W, const float* bias, int B, int N, int K, int act, int accumulate,
              int prologue, const float* ln_gamma, const float* ln_beta, const float* ln2_gamma, const float* ln2_beta,
              int dtype_w, int version, itts_stream stream);

/* The bf16 decode GEMV of the launch path (1-4 rows, csrc/decode_gemv.hip gemv_bf16), as the decode step calls it:
 * Y[b, n] (+)= act(prologue(X)[b, :] . W[n, :] + bias[n]), X [B, K] fp32 or bf16 (x_bf16), Y [B, N] fp32 or bf16 (y_bf16, no
 * accumulate), W bf16 [N, K] - or W8, [N, K] OCP e4m3 bytes with one fp32 scale per output row (wscale), used instead of W when
 * set.  bias may be null.  prologue 0 none (bf16 X), 1 LayerNorm without affine (eps 1e-5; fp32 X), 2 LayerNorm(ln_gamma,
 * ln_beta) then LayerNorm without affine (fp32 X), 3 X is merged from the split-attention partials attn_o
 * [B][K/64][4][64] / attn_ml [B][K/64][2][4] (X unused, K % 64 == 0).  Calls itts_gemv_which answers -1 for are refused with an
 * error and nothing is launched; ITTS_GEMV_MODE / ITTS_GEMV_W5 (read once per process) choose the kernel form as in the engine. */
int itts_gemv_bf16(void* Y, int y_bf16, const void* X, int x_bf16, const void* W, const float* bias, int B, int N, int K, int act,
                   int accumulate, int prologue, const float* ln_gamma, const float* ln_beta, const float* attn_o,
                   const float* attn_ml, const void* W8, const float* wscale, itts_stream stream);

/* The single-query attention over the K/V cache of one decode step with this step's append fused in (csrc/decode_attn.hip
 * decode_attn2), as the launch path calls it once per layer.  Per (row b, head h): pos = prefix[0] + len[b]; this step's k and v
 * are rounded to the cache type and stored at cache row pos of the row's own block; the output is softmax(q . K / 8) V over the
 * cache rows kv_start[b] <= j < pos plus that appended row.  The caller guarantees 0 <= kv_start[b] <= pos < Smax and finite cache
 * contents (rows outside the range are multiplied by a weight of zero).  dh = 64 only.
 *   kc, vc   [B][H][Smax][64], tc = 0 fp32, 1 the 16-bit type of the library, or ITTS_FP8 (whole forms only, `to` 0 or 1): OCP
 *            e4m3 bytes without a scale, 8-byte aligned; the step's k / v are clamped to [-448, 448] and rounded to nearest even
 *            (what x.clamp(-448, 448).to(torch.float8_e4m3fn) gives: no NaN byte is ever written), and the kernel computes,
 *            operation for operation, what the 16-bit form computes on a cache holding the same values
 *   qkv      [B][3 * H * 64] fp32: q, k, v of the step, heads side by side
 *   len, kv_start int32 [B]; prefix int32 [1]
 *   ctx      [B][H * 64] in `to` (0 fp32, 1 16-bit; an fp32 cache writes fp32 only); ctx_tiled = 1 (16-bit only): the MFMA-fragment
 *            tiles of a [B, H * 64] matrix instead (ceil(B / 16) row tiles, rows past B are not written)
 *   part_o   when set, the split form (16-bit cache only; an fp8 cache is refused): four workgroups per (row, head) each take every fourth group of 32 cache
 *            rows and write an un-normalised partial, part_o [B][H][4][64] fp32 and part_ml [B][H][2][4] fp32 = the four
 *            maxima, then the four sums (a split without a visible key: -inf, 0 and zeros) - what prologue 3 of
 *            itts_gemv_bf16 merges; ctx is not written and may be null
 *   anc      when set (beam ancestry): uint8 [2][B][Smax], the half anc[len[b] & 1] is read; entry [b][j] names which of the nb
 *            physical rows of the row's batch item (rows (b / nb) * nb ..) holds position j of its history, values past nb - 1
 *            are clamped; B % nb == 0, 1 <= nb <= 16.  The appended row always goes to the row's own block.
 * Forms the kernel does not have are refused with an error status and nothing is launched. */
int itts_decode_attn(void* ctx, int to, const float* qkv, void* kc, void* vc, const int* len, const int* kv_start, const int* prefix,
                     int B, int H, int dh, int Smax, int tc, int ctx_tiled, float* part_o, float* part_ml, const uint8_t* anc, int nb,
                     itts_stream stream);

/* The prefill's K/V cache write (csrc/decode.hip kv_scatter) on caller memory: the k and v thirds of qkv [B][S][3 * H * dh]
 * (type tq) go to rows 0 .. S - 1 of each [Smax][dh] block of kc / vc [B][H][Smax][dh] (type tc), rounded to the cache type
 * (ITTS_FP8: clamped to [-448, 448], then nearest even); rows S .. Smax - 1 are not touched.  (tq, tc): fp32 -> fp32, 16-bit ->
 * 16-bit, fp32 -> ITTS_FP8, 16-bit -> ITTS_FP8.  Null pointers, non-positive shapes, S > Smax and other type pairs are refused
 * with an error status and nothing is launched. */
int itts_kv_scatter(void* kc, void* vc, const void* qkv, int B, int S, int H, int dh, int Smax, int tq, int tc, itts_stream stream);

/* One sampler launch of the decode step (csrc/decode_sampler.hip) on caller memory, stateless: HF 4.36.2 sample() for B rows -
 * RepetitionPenalty (seen: [B, V] bytes, non-zero = the row has seen the id; null = none) and stop suppression (both skipped
 * when preprocessed) -> / temperature -> TopK -> TopP -> the inverse-CDF draw of uniforms[b] over the kept tokens in
 * descending-score order (lower id first on ties).  logits fp32 [B, V]; tok int32 [B] the drawn ids; kept int32 [B] the number
 * of tokens that survived the warpers.  1 <= top_k <= 128 runs the narrow kernel (V <= 15360; kept is then -1), top_k <= 0
 * (TopK off) or > 128 the whole-vocabulary kernel (V <= 16384).  scratch: B * (V + 16) bytes, 4-byte aligned, overwritten;
 * no caller array is modified.  0 < top_p <= 1, temperature > 0. */
int itts_sample_rows(int32_t* tok, int32_t* kept, const float* logits, const uint8_t* seen, int B, int V, float penalty, int stop,
                     int suppress_stop, int preprocessed, int top_k, float top_p, float temperature, const float* uniforms,
                     void* scratch, size_t scratch_bytes, itts_stream stream);

/* The whole-vocabulary beam sampler (csrc/beam.hip beam_wide_cand_kernel + beam_wide_pick_kernel) on caller memory, stateless: one
 * step of HF 4.36.2 beam_sample up to (not including) BeamSearchScorer.process for `items` batch items of num_beams beams.  Per
 * beam row: log_softmax -> RepetitionPenalty over fake_id, start_tok and the row's k ids (ids int32 [items * num_beams][ids_stride],
 * may be null when k = 0) -> stop suppression (all three skipped when preprocessed) -> / temperature -> TopK (top_k >= 1 only,
 * min_tokens_to_keep = 2, ties with the k-th score stay) -> TopP (min_tokens_to_keep = 2) -> + beam_scores[row]; then 2 * num_beams
 * draws without replacement by inverse CDF of uniforms [items][2 * num_beams] over the item's kept tokens in flat (beam-major,
 * token-ascending) order.  pick_score / pick_tok / pick_beam [items][2 * num_beams] in draw order, kept int32 [items * num_beams].
 * Always these two kernels, 1 <= top_k <= 128 included.  All pointers are device pointers; scratch: (items * num_beams * (V + 1) +
 * items) * 4 bytes, 4-byte aligned, overwritten.  V <= 16384, 2 <= num_beams <= 10, top_p > 0, temperature > 0: anything else is
 * refused with an error status before any launch. */
int itts_beam_sample_rows(float* pick_score, int32_t* pick_tok, int32_t* pick_beam, int32_t* kept, const float* logits,
                          const int32_t* ids, int ids_stride, int k, const float* beam_scores, int items, int num_beams, int V,
                          float penalty, int stop, int suppress_stop, int start_tok, int fake_id, int preprocessed, int top_k,
                          float top_p, float temperature, const float* uniforms, void* scratch, size_t scratch_bytes,
                          itts_stream stream);

/* Decode-step projections at batch > 4 (same Conv1D call sites): X bf16 [B, K], W bf16 [N, K], weights streamed once,
 * batch on MFMA; Y fp32 [B, N] (store, or += when accumulate) or bf16 when y_bf16.  K % 32 == 0, B <= 128.
 * ksplit > 1 splits K over workgroups: raw sums go to partial[ksplit][B][N] (no bias / act / Y), to be absorbed by
 * itts_ln_rows_bf16 (deterministic two-stage reduction, no atomics).
 * layout bit 0: X is MFMA-fragment tiled, bit 1: bf16 Y is written tiled - element (b, k) at
 * ((k/32) * ceil(B/16) + b/16) * 512 + ((k%32)/8 * 16 + b%16) * 8 + k%8 (csrc/itts_decode.h tile_off).
 * layout bit 2: W is the fragment-tiled copy made by itts_retile_weights (same bits out, 1.3x faster weight stream).
 * B <= 16 only - bit 3: X is the fp32 residual stream and LayerNorm (eps 1e-5, affine folded into W) runs in the
 * prologue (K <= 1280, ksplit 1); bit 4: 8 features per workgroup (narrow residual projections, ksplit 1).
 * A tiled bf16 Y needs N % 32 == 0 (the tiles are 32 columns wide).  Null X / W (Y unless ksplit > 1; partial when ksplit > 1),
 * non-positive B / N / K / ksplit and every shape itts_skinny_gemm_supported says 0 for are refused with ITTS_E_INVALID and a
 * message that begins with the entry's name, before any HIP call. */
int itts_skinny_gemm(void* Y, int y_bf16, const void* X, const void* W, const float* bias, int B, int N, int K, int act,
                     int accumulate, int ksplit, float* partial, int layout, itts_stream stream);

/* The same projection from fp8 weights (BASELINE config 5): W8 [N, K] OCP e4m3 bytes, wscale fp32 [N] one scale per output
 * row (y = wscale[n] * (x . W8[n]) + bias[n]); W8t null, or the fragment-tiled copy of W8 made by itts_retile_weights_fp8, which
 * the kernel then streams instead (W8 still has to be given).  No bf16 weights are read.  layout bits 0, 1, 3, 4 as above; bit 2
 * is refused (W8t says that the weights are tiled).  W8 and W8t 8-byte aligned. */
int itts_skinny_gemm_fp8(void* Y, int y_bf16, const void* X, const void* W8, const void* W8t, const float* wscale, const float* bias,
                         int B, int N, int K, int act, int accumulate, int ksplit, float* partial, int layout, itts_stream stream);

/* Host only, no HIP call: 1 when the two entries above take this shape (fp8 != 0: itts_skinny_gemm_fp8), 0 when they refuse it -
 * the rule the launcher itself enforces: 1 <= B <= 128, N >= 1, K a positive multiple of 32, 1 <= ksplit <= K / 32, no activation
 * with ksplit > 1, no accumulate into bf16 Y, bits 3 and 4 at B <= 16 with ksplit 1 and not together, bit 3 at K <= 1280, a tiled
 * bf16 Y at N % 32 == 0, no layout bit past 4.  Pointer alignment is checked at the launch. */
int itts_skinny_gemm_supported(int y_bf16, int B, int N, int K, int act, int accumulate, int ksplit, int layout, int fp8);

/* dst[16*ceil(N/16)*K] <- bf16 W[N, K] in MFMA-fragment tiles: element (n, k) at
 * ((n/16) * (K/32) + k/32) * 512 + ((k%32)/8 * 16 + n%16) * 8 + k%8, rows past N zero (csrc/itts_decode.h wtile_off).
 * The engine makes these copies of the GPT projections itself on the first batched generation. */
int itts_retile_weights(void* dst, const void* src, int N, int K, itts_stream stream);

/* The same order for fp8 weights, one byte per element: dst[16*ceil(N/16)*K] bytes <- W8[N, K]; both 8-byte aligned. */
int itts_retile_weights_fp8(void* dst, const void* src, int N, int K, itts_stream stream);

/* y (bf16) = LayerNorm(x fp32) [passes == 2: LayerNorm again without affine], GPT-2 ln_1 / ln_2 / ln_f o final_norm.
 * nsplit > 0: first x += partial_bias + sum_s partial[s] (the residual add of a split-K projection), written back.
 * gamma and beta come together or not at all; rows >= 1, 1 <= D <= 2048, passes 1 or 2, nsplit 0 .. 8 (partial[nsplit][rows][D]
 * with them, partial_bias may be null), tiled y at D % 32 == 0: anything else is refused with ITTS_E_INVALID before any HIP call. */
int itts_ln_rows_bf16(void* y, float* x, const float* gamma, const float* beta, int rows, int D, float eps, int passes,
                      const float* partial, int nsplit, const float* partial_bias, int y_tiled, itts_stream stream);

int itts_transpose(void* y, const void* x, int B, int R, int C, int dtype, itts_stream stream);

/* One operator-level entry to the row-wise / elementwise kernels (csrc/elementwise.hip, and the two small kernels of
 * csrc/model_vocoder.hip that feed the DVAE encoder), as the engine calls them; tests/test_gpu_elementwise.py uses it.  The struct is
 * read per op as listed; fields an op does not name are ignored.  w / b / codes aside, pointers are in dtype_x (inputs) and dtype_y
 * (outputs); ops with one type take dtype_x == dtype_y, ITTS_F32 or ITTS_BF16.  Activations are row-major, channels last.
 *   LAYERNORM      y[rows][ldy] = act(LayerNorm(x[rows][ldx], D, eps) * w + b); w, b fp32 [D], both or neither; any of the four
 *                  type pairs; act: an ITTS act code of csrc/itts_common.h (0 none, 2 SiLU)
 *   RMSNORM_UNIT   y fp32 [rows][D] = x / max(|x|, 1e-12) * sqrt(D) * w; dtype_y = ITTS_F32
 *   GLU            y[rows][D] = x[rows][0:D] * sigmoid(x[rows][D:2D])
 *   GEGLU          y[rows][ldy]: columns < D = x[rows][0:D] * gelu_erf(x[rows][D:2D]), columns D .. ldy - 1 = 0
 *   DWCONV         y[B][T][D] = depthwise conv over T, k taps, zero padding (k - 1) / 2 each side; w fp32 [D][k], b fp32 [D] or null
 *   CONV2D_SUB2    y[B][T'][N][D'] = relu(Conv2d(1, N, 3, stride 2)) of x [B][T][D]; T' = (T - 3) / 2 + 1, D' = (D - 3) / 2 + 1;
 *                  w fp32 [N][3][3], b fp32 [N]; T, D >= 3
 *   CAST_COPY      y[rows * D] = x[rows * D], any of the four type pairs
 *   COPY_ROWS      y[rows][ldy] <- x[rows][ldx], D columns
 *   ADD_STRIDED    y[rows][ldy] = x[rows][ldx] + x2[rows][ld2], D columns
 *   COL_MEAN       y fp32 [B][D] = mean over T of x[B][T][ldx]
 *   COL_MEAN_STD   y fp32 [B][2 D] = that mean | the population std, sqrt(max(var, 1e-12))
 *   SCALE_COLS_ADD y[B * T][ldy] = x[B * T][ldx] * w[B][D] (+ x2[B * T][ld2] when x2 is set)
 *   ASP_POOL       y fp32 [B][2 D]: per (b, column) the softmax over T of x [B][T][D] weights x2 [B][T][D]: weighted mean | std
 *                  (sqrt(max(var, 1e-12))), then * w[2 D] + b[2 D]
 *   RELPOS_PACK    x = qkv [T][3 N D] (q | k | v, N heads of D), x2 = p [T][N D]: y [T][N][2 D] = q + w | q + b (w, b fp32 [N D]),
 *                  y2 [T][N][2 D] = k | p
 *   DVAE_ARGMIN    y int32 [rows] = the first n that minimises b[n] - 2 x[row][n]; x fp32 [rows][N] (dtype_x = ITTS_F32), b fp32 [N]
 *   PAIR_ROWS      y[B][(T + 1) / 2][2 D] = x[B][2 t][:] | x[B][2 t + 1][:] (zero past T)
 * Null required pointers, non-positive dimensions, a row stride below the row width, an unknown op or type pair and CONV2D_SUB2
 * below 3 x 3 are refused with ITTS_E_INVALID and a message before any HIP call. */
enum {
  ITTS_ROWOP_LAYERNORM = 0, ITTS_ROWOP_RMSNORM_UNIT, ITTS_ROWOP_GLU, ITTS_ROWOP_GEGLU, ITTS_ROWOP_DWCONV, ITTS_ROWOP_CONV2D_SUB2,
  ITTS_ROWOP_CAST_COPY, ITTS_ROWOP_COPY_ROWS, ITTS_ROWOP_ADD_STRIDED, ITTS_ROWOP_COL_MEAN, ITTS_ROWOP_COL_MEAN_STD,
  ITTS_ROWOP_SCALE_COLS_ADD, ITTS_ROWOP_ASP_POOL, ITTS_ROWOP_RELPOS_PACK, ITTS_ROWOP_DVAE_ARGMIN, ITTS_ROWOP_PAIR_ROWS,
  ITTS_ROWOP_COUNT
};
typedef struct {
  void* y; void* y2;
  const void* x; const void* x2;
  const float* w; const float* b;
  int dtype_x, dtype_y;
  int rows, B, T, D, N, k;
  int ldx, ldy, ld2;
  int act; float eps;
} itts_rowop_args;
int itts_rowop(int op, const itts_rowop_args* args, itts_stream stream);

/* ---- token choice, operator level: one launch (pair) of the beam step, the typical filter and the one-beam samplers on
 * caller-owned device memory.  Every pointer is a device pointer; the blocks mirror the kernels' own argument blocks (csrc/itts_decode.h
 * BeamArgs, TypicalArgs, SamplerArgs) and the entries add nothing to them - no scratch, no reset of any state.  Each entry checks
 * its block on the host and returns ITTS_E_INVALID with a message before any HIP call.  Additions to ABI 4. */

/* One beam step for `items` batch items of nb beams (rows = items * nb).
 * mode 0: beam_cand_kernel + beam_select_kernel (the narrow pair of the device-sampled generation: do_sample 1 = beam_sample with
 *         1 <= top_k <= 128, top_p > 0, temperature > 0 and uniforms [max_gen][items][2 nb]; do_sample 0 = beam_search);
 * mode 1: beam_select_kernel on the caller's 2 nb picks per item IN DRAW ORDER (pick_score with the beam score included, pick_tok,
 *         pick_beam: [items][2 nb]), what itts_gpt_commit_beams runs.
 * State, read and advanced as a generation's: len / cur_tok / unfinished / beam_scores [rows]; ids int32 [2][rows][max_gen] and anc
 * uint8 [2][rows][Smax], ping-pong planes by the parity of len; prefix int32 [1]; the finished hypotheses hyp_tok int32
 * [items][nb + 1][max_gen], hyp_score / hyp_len / hyp_order [items][nb + 1] (order -1 = free slot), hyp_n / hyp_worst / hyp_counter /
 * done [items]; mode 0 scratch cand_sc / cand_tok [rows][128], cand_n [rows].  Optional: forced int32 [rows][max_gen] with input_n
 * (steps below input_n take the given token); h_next fp32 [rows][D] = emb[tok] + pos[min(position, pos_rows - 1)] with emb / pos
 * fp32 or, emb_bf16 = 1, bf16 tables.
 * Refused: nb outside 2..10, items < 1, V < 2 or > 15000, max_gen < 1, Smax < 1, stop / start_tok / fake_id outside the vocabulary,
 * under do_sample in mode 0 top_k outside 1..128, top_p <= 0, temperature <= 0 or no uniforms, h_next without emb, pos, D >= 1 and
 * pos_rows >= 1, emb_bf16 outside {0, 1}, input_n > 0 without forced, a null state pointer, mode 0 without logits or candidate
 * scratch, mode 1 without picks. */
typedef struct {
  const float* logits; const float* uniforms;
  int* len; int* cur_tok; int* unfinished; int* ids; void* anc; const int* prefix; float* beam_scores;
  int* hyp_tok; float* hyp_score; int* hyp_len; int* hyp_order; int* hyp_n; float* hyp_worst; int* hyp_counter; int* done;
  float* h_next; const void* emb; const void* pos;
  float* cand_sc; int* cand_tok; int* cand_n;
  const int* forced;
  const float* pick_score; const int* pick_tok; const int* pick_beam;
  int mode, items, nb, V, max_gen, Smax, stop, start_tok, fake_id, suppress_stop, preprocessed, do_sample, top_k, input_n;
  int D, pos_rows, emb_bf16;
  float penalty, top_p, temperature, length_penalty;
} itts_beam_step_args;
int itts_beam_step(const itts_beam_step_args* args, itts_stream stream);

/* typical_filter_kernel on `rows` rows: logits fp32 [rows][V] -> out fp32 [rows][V], the processed scores (log_softmax first when
 * log_softmax_first, repetition penalty over the seen set, stop suppression) with everything behind the typical mass at -inf; the
 * first min_keep ranks always stay.  The seen set is the byte map seen uint8 [rows][V] (may be null: nothing seen), or - beam_ids
 * given - fake_id, start_tok and the first len[row] ids of beam_ids int32 [2][rows][max_gen], plane len[row] & 1.
 * Refused: null logits / out, rows < 1, V < 2 or > 16384, mass outside (0, 1), min_keep < 1, penalty <= 0, stop outside the
 * vocabulary, both seen sources at once, beam_ids without len, max_gen >= 1 and start_tok / fake_id inside the vocabulary. */
typedef struct {
  const float* logits; float* out; const void* seen; const int* beam_ids; const int* len;
  int rows, V, stop, suppress_stop, min_keep, log_softmax_first, max_gen, start_tok, fake_id;
  float penalty, mass;
} itts_typical_args;
int itts_typical_rows(const itts_typical_args* args, itts_stream stream);

/* One sampler launch on a generation's state for B rows: do_sample 0 = sampler2_kernel (greedy), else sampler_sample_kernel
 * (1 <= top_k <= 128, V <= 15360) or sampler_wide_kernel (any other top_k, V <= 16384; kept int32 [B], may be null, receives the
 * kept ranks).  State: logits fp32 [B][V], seen uint8 [B][V], ids int32 [B][max_gen], cur_tok / unfinished / step int32 [B];
 * uniforms fp32 [max_gen][B] (row min(step, max_gen - 1) is read); optional forced int32 [B][max_gen] (>= 0 replaces the choice)
 * with input_n, and h_next / emb / pos / D / pos_rows / emb_bf16 as in itts_beam_step.  itts_sample_rows is the stateless form.
 * Refused: a null state pointer, B < 1, V < 1 or above the kernel's limit, max_gen < 1, stop outside the vocabulary, penalty <= 0,
 * sampling without uniforms, top_p <= 0 or temperature <= 0, h_next without its tables, emb_bf16 outside {0, 1}, input_n > 0 without
 * forced. */
typedef struct {
  const float* logits; void* seen; int* ids; int* cur_tok; int* unfinished; int* step;
  float* h_next; const void* emb; const void* pos; const float* uniforms; const int* forced; int* kept;
  int B, V, max_gen, stop, suppress_stop, preprocessed, do_sample, top_k, input_n, D, pos_rows, emb_bf16;
  float penalty, top_p, temperature;
} itts_sampler_step_args;
int itts_sampler_step(const itts_sampler_step_args* args, itts_stream stream);

/* One row of a mixed decode batch: its own token choice.  mode 0 = greedy (top_k / top_p / temperature unread), 1 = sample.
 * top_k <= 0 switches the TopK warper off.  0 < top_p <= 1, temperature > 0, penalty > 0 (the row's repetition penalty). */
typedef struct {
  int mode, top_k;
  float top_p, temperature, penalty;
} itts_row_sampling;

/* itts_sampler_step with one setting per row: rows_host is a HOST table of args->B entries, and the scalar sampling fields of
 * args (do_sample, top_k, top_p, temperature, penalty) are ignored.  rows_dev_scratch: args->B * sizeof(itts_row_sampling) bytes
 * of caller device memory, 4-byte aligned, which the call fills on the stream (the host table is the caller's again on return).
 * Every row gets the bits of itts_sampler_step with its entry as the scalar setting: a greedy row runs in sampler2_kernel, a row
 * with 1 <= top_k <= 128 in sampler_sample_kernel, any other sampled row in sampler_wide_kernel - one launch per class present,
 * each over all rows, a row's block returning at once in the kernels of the other classes.  Refused with ITTS_E_INVALID before
 * any device call: what itts_sampler_step refuses, null rows_host / rows_dev_scratch, a mode outside {0, 1}, top_p outside
 * (0, 1], temperature <= 0, penalty <= 0, a sampled row without uniforms, V > 15360 with a narrow row, V > 16384 with a wide row. */
int itts_sampler_step_rows(const itts_sampler_step_args* args, const itts_row_sampling* rows_host, void* rows_dev_scratch,
                           itts_stream stream);

/* ---- engine level ----------------------------------------------------------------------------------- */

typedef struct {
  int dtype; /* weight + activation dtype of the engine (ITTS_F32 parity path / ITTS_BF16 throughput path) */
  /* gpt (UnifiedVoice ctor, gpt/model.py:301-379) */
  int model_dim, layers, heads, max_mel_tokens, max_text_tokens, number_text_tokens, number_mel_codes;
  int start_mel_token, stop_mel_token, start_text_token, stop_text_token, cond_latents;
  /* conformer + perceiver (condition_module) */
  int cond_dim, cond_ff, cond_heads, cond_blocks, cond_idim, perc_inner, perc_layers;
  /* bigvgan (BigVGAN.__init__, BigVGAN/models.py:132-197) */
  int bv_gpt_dim, bv_init_ch, bv_num_up, bv_up_rates[8], bv_up_kernels[8];
  int bv_num_res, bv_res_kernels[4], bv_res_dils[4][4], bv_num_dil, bv_spk_dim, bv_num_mels;
  /* ECAPA-TDNN (ECAPA_TDNN.py:429-449 defaults) */
  int ec_channels[5], ec_kernels[5], ec_dils[5], ec_att, ec_scale, ec_se;
  /* DVAE decoder (vqvae/xtts_dvae.py:202-291) */
  int dv_channels, dv_tokens, dv_hidden, dv_resblocks, dv_codebook, dv_layers, dv_kernel;
  /* limits */
  int max_batch;
} itts_config;

int itts_engine_create(const itts_config* cfg, itts_engine** out);
void itts_engine_destroy(itts_engine* e);
/* Register a packed tensor that lives in caller-owned device memory (the weight arena). */
int itts_engine_bind_tensor(itts_engine* e, const char* name, const void* ptr, int dtype, int ndim, const int64_t* dims);
/* Validate that every tensor the configured model needs is bound with the right shape/dtype. */
int itts_engine_finalize(itts_engine* e);

/* G2/C1/P1  UnifiedVoice.get_conditioning (gpt/model.py:490-502): mel [1, F, idim] -> cond fp32 [latents, D] */
int itts_conditioning(itts_engine* e, const void* mel_bfc, int F, float* cond_out, itts_stream stream);
/* The same for a prompt that is the first F frames of a tensor padded to F_total frames (get_conditioning with
 * cond_mel_lengths, gpt/model.py:490-502: masked conformer + perceiver; mel_bfc holds at least F frames). */
int itts_conditioning_padded(itts_engine* e, const void* mel_bfc, int F, int F_total, float* cond_out, itts_stream stream);
/* V6  ECAPA_TDNN.forward (BigVGAN/ECAPA_TDNN.py:545-581): mel [B, F, num_mels] -> spk fp32 [B, spk_dim] */
int itts_ecapa(itts_engine* e, const void* mel_bfc, int B, int F, float* spk_out, itts_stream stream);

/* Sampling mode of the next itts_gpt_prefill / itts_gpt_decode calls: HF 4.36.2 GenerationMixin.sample as
 * indextts/infer.py:116-124 + gpt/model.py:690-703 configure it with num_beams = 1 (RepetitionPenaltyLogitsProcessor ->
 * TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax -> one draw).  The draw is the inverse CDF
 * of uniforms_host[k * B + b] (step k, row b; host array of n_uniforms >= max_gen * B floats in [0, 1)) over the kept
 * tokens in descending-score order, so a caller-side RNG fixes the sequence.  do_sample = 0 returns to greedy.
 * Any top_k: <= 0 switches the TopK warper off (HF `top_k = 0 / None`, stored as 0); 1 .. 128 runs the narrow sampler, 0 and
 * > 128 the whole-vocabulary sampler (number_mel_codes <= 16384; parallel fp32 sums: the same distribution as torch's, the
 * top-p boundary within 64 * 2^-24 of it).  0 < top_p <= 1, temperature > 0. */
int itts_gpt_set_sampling(itts_engine* e, int do_sample, int top_k, float top_p, float temperature, const float* uniforms_host,
                          int64_t n_uniforms);

/* Mixed batches (opt-in): one setting per row for the following single-beam generations.  rows_host: HOST table of B entries,
 * row b of a batch of B; uniforms_host [max_gen][B] as in itts_gpt_set_sampling, needed when any row samples.  B = 0 clears the
 * table (the scalar setting then is what itts_gpt_set_sampling last said, or greedy after a table that was not uniform).
 * itts_gpt_prefill latches the table and refuses when B is not its batch, when beams, typical filtering or host sampling are on.
 * Every row's `penalty` replaces the prefill's repetition_penalty argument.
 * A table whose rows are all equal IS the scalar setting with those values - the same code path, the persistent engine's in-launch
 * greedy sampler included, the same bits.  With any other table the step (the persistent engine's blocks and head at <= 6 rows,
 * the launch path above) is followed by one sampler launch per class present (itts_sampler_step_rows), and every row's codes and
 * logits are the bits of a generation of the same rows with that row's entry as the scalar setting and the same uniforms.
 * A sampled row with top_k outside 1..128 always runs on the device's whole-vocabulary sampler (number_mel_codes <= 16384).
 * itts_gpt_retire_rows carries the entries with their rows. */
int itts_gpt_set_sampling_rows(itts_engine* e, const itts_row_sampling* rows_host, int B, const float* uniforms_host,
                               int64_t n_uniforms);

/* Beam-sample mode of the next generations: HF 4.36.2 GenerationMixin.beam_sample + BeamSearchScorer, the generate() mode
 * the reference's DEFAULT kwargs select (infer.py:116-124: do_sample=True, num_beams=3, top_k=30, top_p=0.8,
 * length_penalty=0.0; call site gpt/model.py:698-703; cache re-ordering gpt/model.py:194-207).  Per step and batch item:
 * log_softmax -> RepetitionPenalty -> Temperature -> TopK -> TopP (min_tokens_to_keep 2) -> + beam scores -> 2 * num_beams
 * draws without replacement -> BeamSearchScorer.process, all on the device; the KV cache is not copied when beams swap
 * (per-beam ancestry rows).  itts_gpt_prefill then takes B batch items and runs B * num_beams rows (<= max_batch);
 * itts_gpt_fetch returns the finalized best hypothesis per batch item, codes [B, max_gen] padded with the stop token.
 * uniforms_host: [max_gen][B][2 * num_beams] floats in [0, 1): draw j of (step, item) is the inverse CDF of its uniform over
 * the not-yet-drawn candidates in flat (beam-major, token-ascending) order.  2 <= num_beams <= 10; num_beams <= 1 = off. */
int itts_gpt_set_beam_sample(itts_engine* e, int num_beams, int top_k, float top_p, float temperature, const float* uniforms_host,
                             int64_t n_uniforms);

/* The general beam entry point (itts_gpt_set_beam_sample = do_sample 1, length_penalty 0): do_sample = 0 selects HF
 * beam_search - deterministic, per step the 2 * num_beams best of log_softmax + repetition penalty + beam score, no warpers,
 * no uniforms - which is what `num_beams > 1, do_sample=False` means to generate(); length_penalty enters
 * BeamHypotheses' score = sum_logprobs / generated_len ** length_penalty (infer.py:121 passes 0.0).  2 <= num_beams <= 10
 * (the web UI offers num_beams 1..10, top_k 0..100).  do_sample with any top_k: <= 0 switches the TopK warper off (HF `top_k = 0 /
 * None`, stored as 0); 1 .. 128 runs the narrow pair of kernels, 0 and > 128 the whole-vocabulary pair (number_mel_codes <= 16384;
 * parallel fp32 sums: the same distribution as torch's, boundaries within 512 * 2^-24 of the mass of it). */
int itts_gpt_set_beams(itts_engine* e, int num_beams, int do_sample, int top_k, float top_p, float temperature, float length_penalty,
                       const float* uniforms_host, int64_t n_uniforms);

/* `num_return_sequences` of generate() under beams (gpt/model.py:655,698-703 forwards it; HF's BeamSearchScorer keeps
 * num_beam_hyps_to_keep = num_return_sequences hypotheses per batch item): itts_gpt_fetch then returns the n best
 * hypotheses of every batch item, best first, as codes [B * n][max_gen].  1 <= n <= num_beams (checked by
 * itts_gpt_prefill, with HF's message); stays in force until changed.  (Without beams the caller repeats the rows, as HF
 * does: indextts/gpt/model.py.)  ABI 4. */
int itts_gpt_set_beam_returns(itts_engine* e, int num_return_sequences);

/* `typical_sampling=True` of UnifiedVoice.inference_speech (gpt/model.py:690-697): the reference's TypicalLogitsWarper
 * (utils/typical_sampling.py:9-30, mass in (0, 1); min_tokens_to_keep 2 under beams, else 1) runs right after the repetition
 * penalty and before Temperature / TopK / TopP in the sampling and beam-sample modes.  mass = 0 switches it off. */
int itts_gpt_set_typical(itts_engine* e, float mass);

/* Forced tokens for the first n steps of every following generation (n = 0 clears): ids_host int32 [B, n] (B = 1 is
 * broadcast to every row; -1 = leave that step free).  This is the `input_tokens` continuation of
 * UnifiedVoice.inference_speech (gpt/model.py:672-686: given mel tokens are appended to the prompt and generation
 * continues after them) and the teacher forcing the parity tests use; the forced tokens are returned by
 * itts_gpt_fetch as steps 0..n-1 (the reference strips them with trunc_index, model.py:687,704). */
int itts_gpt_set_forced(itts_engine* e, const int32_t* ids_host, int B, int n);

/* The same, with the positions of the reference's `input_tokens` path (gpt/model.py:141-155,672-686): the given tokens are
 * part of the reference's FIRST forward, embedded with mel positions 0 .. n ([start_mel, t1 .. tn]), and the first generated
 * token is fed at position n + 2 - so given token k (0-based) is fed at position k + 1 here, not k + 2 as a generated
 * (or teacher-forced) token would be.  n = 0 clears.  Works with beams too (itts_gpt_set_beams; B = batch items, every id
 * >= 0): the given tokens go into every beam row with the beam scores, the cache ancestry and the hypotheses untouched, and
 * HF's generated_len (length penalty, is_done) counts after them, as they belong to the decoder prompt there. */
int itts_gpt_set_input_tokens(itts_engine* e, const int32_t* ids_host, int B, int n);

/* How the last captured / launched decode step ran: 1 = the persistent decode engine (ONE launch per token step: the GPT
 * blocks, the head and - greedy search - the sampler; 1 - 6 decode rows, beam rows included (cache ancestry); IndexTTS-1.5
 * dims, a whole MI355X), 0 = five launches per block. */
int itts_gpt_decode_mode(itts_engine* e);

/* Host-side token choice, for generate() modes outside the device samplers' limits (HF warpers over the whole vocabulary:
 * `top_k = 0 / None`, infer.py:116-124 forwards it verbatim and webui.py:393-402 offers 0): with on = 1, itts_gpt_prefill and
 * itts_gpt_decode(e, 1, ..) stop behind the head GEMV; the caller reads the logits (itts_gpt_fetch), applies the logits
 * processors / warpers and the draw itself, and itts_gpt_commit hands the chosen token of every row (host int32 [B]) to the
 * sampler's bookkeeping (ids, repetition bitmap, eos state, step counter, next input embedding).  One stream sync per token. */
int itts_gpt_set_host_sampling(itts_engine* e, int on);

/* Conditioning latents per batch item: with on = 1 the `cond` of the following itts_gpt_prefill calls is [B][latents, D] (one
 * prompt per row, UnifiedVoice.inference_speech with a batch of prompts: gpt/model.py:599-602,670) instead of one [latents, D]
 * block shared by every row (what infer.py passes). */
int itts_gpt_set_cond_per_row(itts_engine* e, int on);
int itts_gpt_commit(itts_engine* e, const int32_t* tokens_host, itts_stream stream);

/* The same under beams (itts_gpt_set_host_sampling(e, 1) BEFORE itts_gpt_set_beams, which then accepts any top_k and no
 * uniforms): HF beam_sample with `top_k = 0 / None` or > 128 (infer.py:116-124 forwards the kwargs verbatim; the device beam
 * sampler keeps at most 128 candidates per beam).  Per step the caller reads the logits [B * num_beams, V] (itts_gpt_fetch) and
 * itts_gpt_beam_state - ids_host int32 [B * num_beams][max_gen]: every beam's id history (the first *step_host entries are
 * valid), scores_host [B * num_beams]: the running beam scores, done_host [B]: BeamSearchScorer._done - applies log_softmax ->
 * logits processors -> warpers -> + beam scores and draws 2 * num_beams candidates per batch item, then hands them IN DRAW
 * ORDER ([B][2 * num_beams]: score with the beam score included, token, beam index within the item) to
 * itts_gpt_commit_beams, which runs BeamSearchScorer.process (hypotheses, done) and the beam re-ordering (id histories, cache
 * ancestry = _reorder_cache, gpt/model.py:194-207) on the device as the device-sampled mode does.  itts_gpt_fetch finalizes. */
int itts_gpt_beam_state(itts_engine* e, int32_t* ids_host, float* scores_host, int32_t* done_host, int* step_host, itts_stream stream);
int itts_gpt_commit_beams(itts_engine* e, const float* pick_score_host, const int32_t* pick_tok_host, const int32_t* pick_beam_host,
                          itts_stream stream);

/* After a step of a device-sampled beam generation with top_k <= 0 or > 128 (no host sampling): that step's 2 * num_beams picks
 * per batch item IN DRAW ORDER (score_host, tok_host, beam_host: [B][2 * num_beams]) and the number of tokens every beam row kept
 * behind the warpers (kept_host int32 [B * num_beams]), copied from the sampler's device buffers; any pointer may be null.  An item
 * that was already done, and a step that took a given `input_tokens` token, leave the earlier content in place. */
int itts_gpt_beam_picks(itts_engine* e, float* score_host, int32_t* tok_host, int32_t* beam_host, int32_t* kept_host, itts_stream stream);

/* G1/G3/G4 step 0: prepare_gpt_inputs (model.py:591-654) + prefill + first greedy token.
 * cond fp32 [latents, D]; text ids host int32 [B, L] (may hold start/stop padding ids, stripped per row).
 * Synchronises the stream once (uploads the row descriptors). */
int itts_gpt_prefill(itts_engine* e, const float* cond, const int32_t* text_ids_host, int B, int L, int max_gen,
                     float repetition_penalty, int suppress_stop, itts_stream stream);
/* G4/G5/G6: run up to nsteps further greedy steps (hipGraph replay of one captured step). */
int itts_gpt_decode(itts_engine* e, int nsteps, itts_stream stream);
/* Host-visible progress (synchronises): tokens generated per row so far, rows still unfinished. */
int itts_gpt_status(itts_engine* e, int* steps_done_host, int* n_unfinished_host, itts_stream stream);
/* Copy generated codes (int32 [B, max_gen], pad = stop token) and optionally the last logits fp32 [B, V]. */
int itts_gpt_fetch(itts_engine* e, int32_t* codes_host, float* logits_host, itts_stream stream);

/* Row retirement of a running batched generation (opt-in; nothing changes for a caller that never calls it).  A finished row
 * still runs every block and its cache attention each step, although its output is fixed.  itts_gpt_retire_rows synchronises and
 * compacts the decode state - K/V history, hidden state, logits, ids, forced tokens, repetition bitmap, counters, sampling
 * uniforms - to the unfinished rows; the following itts_gpt_decode steps run, and are captured, at the smaller row count, which
 * *rows_now_host receives (itts_gpt_rows answers it too; 0 without an active generation).  The caller still sees the original
 * batch: itts_gpt_status counts the live rows, itts_gpt_fetch returns all B rows in their ORIGINAL order - retired rows with their
 * codes followed by the stop token, exactly what an unretired run holds, and with the logits of their LAST STEP BEFORE THE
 * RETIREMENT (an unretired run would keep computing logits for them; nothing reads those).  It is a no-op that reports the
 * unchanged row count without an active generation, under beams (unless itts_gpt_set_retire_beams opted in), under host sampling, while the step runs on the persistent
 * decode engine or the fused qkv + attention launch, and when no row or every row has finished.  After a retirement the
 * generation stays on the launch path even at <= 6 rows (itts_gpt_decode_mode answers 0).  The next itts_gpt_prefill resets it. */
int itts_gpt_retire_rows(itts_engine* e, int* rows_now_host, itts_stream stream);
int itts_gpt_rows(itts_engine* e);

/* Operator entry of rows_move_kernel on caller memory: for o < n_outer, move i < n_moves, chunk c < n_chunks copy chunk_bytes from
 * base + o * outer_stride + src[i] * row_stride + c * chunk_stride to the same address with dst[i] in place of src[i].  At most
 * 128 moves; the source and destination row sets must not intersect (every copy of the launch is then independent).  16-byte
 * units where base, strides and chunk_bytes are multiples of 16, else 4-byte or single bytes.  n_moves = 0 launches nothing.
 * ITTS_E_INVALID before any HIP call for: a null base, negative counts, n_moves > 128, intersecting sets, chunk_bytes >
 * chunk_stride, n_chunks * chunk_stride > row_stride. */
int itts_rows_move(void* base, size_t outer_stride, int n_outer, size_t row_stride, size_t chunk_stride, int n_chunks, size_t chunk_bytes,
                   const int* src_host, const int* dst_host, int n_moves, itts_stream stream);
/* The compaction plan alone (host only): with n live rows of B, the live rows at slots >= n move into the dead slots < n, both
 * in ascending order; live rows below n keep their slot.  src_host / dst_host hold up to B entries. */
int itts_retire_plan(const int* unfinished_host, int B, int* n_live, int* src_host, int* dst_host, int* n_moves);

/* Retirement of finished beam groups (opt-in, sticky per engine object, default 0 = itts_gpt_retire_rows stays the no-op under beams
 * that it is above).  With on = 1 itts_gpt_retire_rows compacts a beam generation (num_beams > 1) to the rows of its unfinished
 * batch items: a group of num_beams rows moves as a unit and a beam keeps its index inside its group, so the cache ancestry, which
 * is relative to the group, stays valid.  A retiring item is finalised at once from its hypothesis store - it is done, so nothing
 * can change its result - and kept on the host by original item; K/V, the per-row and per-item beam state move with rows_move, the
 * live half of the two ping-pong arrays (beam ids, ancestry) with itts_rows_gather below, the draws are re-packed by original
 * item.  itts_gpt_fetch then returns [items * num_return_sequences][max_gen] codes in the ORIGINAL item order and logits [rows][V]
 * in the original row order (retired rows: the logits of their last step before the retirement); itts_gpt_rows, itts_gpt_status
 * and itts_gpt_row_status answer for the live rows.  Same bits as the unretired run while the row count stays inside one
 * projection-kernel family.  Still a no-op that reports the unchanged row count: while the step runs on the persistent engine or
 * the fused qkv + attention launch, under host sampling (host-side beam warpers), with `input_tokens`, and when no item or every
 * item is done.  The environment variable ITTS_RETIRE_BEAMS (read per call) overrides the setter in both directions.
 * Additions to ABI 4 (the version stays): itts_gpt_set_retire_beams, itts_rows_gather. */
int itts_gpt_set_retire_beams(itts_engine* e, int on);

/* Operator entry of rows_gather_kernel on caller memory, the out-of-place companion of itts_rows_move: for plane p < n_planes and
 * j < n_rows copy row_bytes from src + p * src_plane_stride + src_rows[j] * row_bytes to dst + p * dst_plane_stride + j * row_bytes.
 * 16-byte units where both bases, both strides and row_bytes are multiples of 16, else 4-byte units or single bytes.  n_rows = 0,
 * n_planes = 0 or row_bytes = 0 launches nothing.  ITTS_E_INVALID before any HIP call for: a null dst or src, a null row list with
 * n_rows > 0, negative counts, n_rows > 128, n_planes > 65536, a row index outside [0, 65536), row_bytes >= 4 GiB, a plane stride
 * >= 1 TiB, n_planes > 1 with n_rows * row_bytes > dst_plane_stride (destination planes would overlap), and any byte that the
 * launch would both read and write (the source rows and the destination blocks must not intersect). */
int itts_rows_gather(void* dst, size_t dst_plane_stride, const void* src, size_t src_plane_stride, int n_planes, size_t row_bytes,
                     const int* src_rows_host, int n_rows, itts_stream stream);

/* Row admission into a running batched generation (opt-in; nothing changes for a caller that never calls it).  A token step costs
 * almost the same at every row count, so a slot whose row has finished is better given to the next waiting request than carried
 * to the end of the slowest row.  itts_gpt_admit_rows synchronises, takes the n lowest finished slots (finished: unfinished == 0 or
 * len >= max_gen; itts_admit_plan), keeps their rows' codes and last logits on the host, prefills the n new requests in scratch
 * with the prefill's kernels, writes their K/V into the slots (itts_kv_admit), resets the slots' state (itts_rows_admit) and
 * chooses their first token - the running rows are neither stepped nor touched.  The following itts_gpt_decode steps carry the
 * new rows with len = 0; within one projection-kernel family a row's codes and logits are those of a fresh generation.
 *   cond fp32 [cond_rows][latents, D] on the device, cond_rows = 1 (shared) or n; text_ids_host int32 [n][L], L the running
 *   generation's own (a shorter text is padded with stop ids and left-padded as in the prefill);
 *   rows_host [n] or null: in a table generation (itts_gpt_set_sampling_rows, see itts_gpt_keep_row_table) each row's own
 *   settings (null: greedy with the generation's penalty) - a class that was not present re-captures the step, any other
 *   admission keeps the captured step; a scalar generation admits only rows with its own settings (null: those);
 *   uniforms_host [n][max_gen]: the draws of the sampled rows (row-major per new row);
 *   forced_host int32 [n][n_forced] or null (-1 = free): needs a generation that was started with forced tokens;
 *   slots_host [n] (optional) receives the slots.
 * The new rows become original rows B0, B0 + 1, ..: itts_gpt_fetch then returns all B0 rows (itts_gpt_rows_total) in that order,
 * a replaced row with its codes followed by the stop token and its last logits.  itts_gpt_status still counts slots;
 * itts_gpt_row_status answers per slot.  Refused with a message before anything is changed: no active generation, beams (unless
 * itts_gpt_set_admit_beams opted in, see below), typical filtering, host sampling, `input_tokens`, the fused qkv + attention launch, a step on the persistent engine (<= 6
 * rows), after a retirement, fewer finished slots than n, n > 128, a text id out of range, L not the generation's, an entry the
 * prefill would refuse, uniforms missing for a sampled row, a sampled row in a generation without room for draws.
 * Additions to ABI 4 (the version stays): itts_gpt_admit_rows, itts_gpt_row_status, itts_gpt_rows_total, itts_gpt_graph_captures,
 * itts_gpt_keep_row_table, itts_kv_admit, itts_rows_admit, itts_admit_plan. */
int itts_gpt_admit_rows(itts_engine* e, const float* cond, int cond_rows, const int32_t* text_ids_host, int n, int L,
                        const itts_row_sampling* rows_host, const float* uniforms_host, const int32_t* forced_host, int n_forced,
                        int32_t* slots_host, itts_stream stream);
/* Per slot of the active generation (host int32 [itts_gpt_rows] each, any may be null): the original row it holds, its tokens so
 * far, whether it is unfinished.  Synchronises. */
int itts_gpt_row_status(itts_engine* e, int32_t* orig_host, int32_t* len_host, int32_t* unfinished_host, itts_stream stream);
/* Rows itts_gpt_fetch returns: the prefill's batch plus every admitted row (0 without an active generation). */
int itts_gpt_rows_total(itts_engine* e);
/* Times this engine object has captured its decode step so far (a replayed step does not count): what tells an admission that
 * kept the captured step from one that re-captured. */
int itts_gpt_graph_captures(itts_engine* e);
/* on = 1: the following prefills keep a per-row table that is uniform as a table generation (one sampler launch per class, room
 * for draws) instead of the scalar path, so that it can admit rows of other settings.  itts_gpt_set_sampling_rows is unchanged. */
int itts_gpt_keep_row_table(itts_engine* e, int on);

/* Operator entry of kv_admit_kernel on caller memory: the k and v thirds of qkv [n][S][3 * H * dh] (type tq) -> positions 0 .. S - 1
 * of rows slots_host[i] of kc / vc [Bcache][H][Smax][dh] (type tc), the bytes itts_kv_scatter writes for the same rows; nothing else
 * is written.  16 bytes per lane (8 into an e4m3 cache).  ITTS_E_INVALID before any HIP call for: null pointers, n outside
 * [1, 128], S / H / dh / Smax / Bcache < 1, S > Smax, a type pair itts_kv_scatter refuses, dh no multiple of 8 (4: fp32 cache),
 * qkv not 16-byte aligned, a cache not 16-byte (e4m3: 8-byte) aligned, a slot outside [0, Bcache), a slot twice. */
int itts_kv_admit(void* kc, void* vc, const void* qkv, int n, int S, int H, int dh, int Smax, int Bcache, int tq, int tc,
                  const int* slots_host, itts_stream stream);
/* Operator entry of rows_admit_kernel on caller memory: the state of a fresh generation for n slots of B - seen [B][V] bytes
 * (1 at fake_id and start_tok), unfinished = 1, cur_tok = start_tok, len = 0, kv_start = kv_start_host[i], the ids row filled with
 * stop, the forced row (forced null: skipped; forced_src [n][max_gen] device or null: -1) and, uniforms_src [n][max_gen] given,
 * column slot of uniforms [max_gen][B].  No other slot is written. */
typedef struct {
  void *seen, *unfinished, *cur_tok, *len, *kv_start, *ids, *forced, *uniforms;
  const void *forced_src, *uniforms_src;
  const int *slots_host, *kv_start_host; /* [n] */
  int n, B, V, max_gen, fake_id, start_tok, stop;
} itts_rows_admit_args;
int itts_rows_admit(const itts_rows_admit_args* args, itts_stream stream);
/* The slot choice alone (host only): the min(n, *n_free) lowest finished slots in ascending order, *n_free = all finished slots. */
int itts_admit_plan(const int* unfinished_host, const int* len_host, int B, int max_gen, int n, int* slots_host, int* n_free);

/* Row admission under beams (opt-in, sticky per engine object, default 0 = itts_gpt_admit_rows refuses a beam generation as above).
 * With on = 1 itts_gpt_admit_rows admits whole BATCH ITEMS into a running beam generation (num_beams > 1, beam_sample or
 * beam_search on the device): n counts items, text_ids_host is [n][L], cond_rows is 1 or n (items), uniforms_host is
 * [n][max_gen][2 * num_beams] (required for beam_sample, ignored for beam_search), rows_host and forced_host must be null, and
 * slots_host [n] receives ITEM slots.  An item is finished when it is done or its rows hold max_gen tokens; the n lowest finished
 * items leave: they are finalised on the host at their own step (itts_gpt_set_beam_returns hypotheses each) and kept, with their
 * rows' last logits, by original item.  The new items are prefilled as n * num_beams rows - the rows and kernels of a fresh
 * generation of those items -, their K/V goes to rows item * num_beams + beam (itts_kv_admit), the rows' state is reset
 * (itts_rows_admit), the groups' beam state is reset (itts_beam_admit) and their first token is chosen by the beam kernels on a
 * grid of one item each; the running groups are neither stepped nor touched, and the captured step is kept.  Every beam kernel
 * takes its step, its ping-pong half and its draws from the item's own len, so the groups then run at different steps.  The new
 * items become original items items0, items0 + 1, ..: itts_gpt_fetch returns [itts_gpt_rows_total / num_beams *
 * num_return_sequences][max_gen] codes in original item order and logits [itts_gpt_rows_total][V] in original row order;
 * itts_gpt_rows_total counts rows, itts_gpt_row_status answers per row.  Within one projection-kernel family an admitted item's
 * codes and logits are those of a fresh generation of the admitted items.  itts_gpt_retire_rows (with itts_gpt_set_retire_beams)
 * still retires done groups afterwards: both ping-pong halves move, the draws are re-packed from the generation's own copy by
 * original item; an admission after a retirement stays refused.  itts_gpt_status keeps reporting the step of row 0.
 * Refused with a message before anything is changed: typical filtering, host sampling (host-side beam warpers), `input_tokens`,
 * the fused qkv + attention launch, a step on the persistent engine (<= 6 rows), after a retirement, fewer finished items than n,
 * n * num_beams > 128, a non-null rows_host or forced_host, draws missing for beam_sample, and what the single-beam form refuses
 * for its texts.  The environment variable ITTS_ADMIT_BEAMS (read per call) overrides the setter in both directions.
 * Additions to ABI 4 (the version stays): itts_gpt_set_admit_beams, itts_beam_admit. */
int itts_gpt_set_admit_beams(itts_engine* e, int on);
/* Operator entry of beam_admit_kernel on caller memory: the beam state of a fresh generation for n of `items` batch items of nb
 * beams - beam_scores [items * nb] (0; with do_sample = 0: 0 for an item's first beam and -1e9 behind it), both halves of anc
 * [2][items * nb][Smax] bytes (row item * nb + q filled with q), hyp_order [items][nb + 1] = -1, hyp_n = 0, hyp_worst = 1e9,
 * hyp_counter = 0, beam_done = 0 (each [items]) and, uniforms_src [n][max_gen][2 * nb] (device) given, the item's column of
 * uniforms [max_gen][items][2 * nb].  Nothing else is written.  ITTS_E_INVALID before any HIP call for: a null pointer (uniforms
 * and uniforms_src may be null, uniforms_src without uniforms may not), n outside [1, 128], nb outside [2, 10], n * nb > 128,
 * items * nb outside [1, 65536], max_gen outside [1, 65536], Smax outside [16, 65536] or no multiple of 16, anc not 16-byte
 * aligned, an item outside [0, items), an item twice. */
typedef struct {
  void *beam_scores, *anc, *hyp_order, *hyp_n, *hyp_worst, *hyp_counter, *beam_done, *uniforms;
  const void* uniforms_src;
  const int* items_host; /* [n] */
  int n, nb, items, Smax, max_gen, do_sample;
} itts_beam_admit_args;
int itts_beam_admit(const itts_beam_admit_args* args, itts_stream stream);

/* G8  UnifiedVoice.forward(return_latent=True) for one sentence (model.py:521-589):
 * text ids host [L], codes host [T] -> latent [T, D] in the engine dtype. */
int itts_gpt_latent(itts_engine* e, const float* cond, const int32_t* text_ids_host, int L, const int32_t* codes_host,
                    int T, void* latent_out, itts_stream stream);

/* Same for several sentences at once (concatenated ids / codes with per-sentence lengths): rows are stacked with
 * left padding and masked keys, so each sentence's latent equals the batch-1 result.  latent_out = [sum T_i, D]. */
int itts_gpt_latent_batch(itts_engine* e, const float* cond, const int32_t* text_ids_host, const int32_t* text_lens_host,
                          const int32_t* codes_host, const int32_t* code_lens_host, int nseq, void* latent_out,
                          itts_stream stream);
/* The same with one voice per sentence: cond = [n_cond][latents, D] fp32 on the device, sentence i reads block
 * cond_index_host[i] (host, [nseq], each in [0, n_cond)).  itts_gpt_latent_batch is the all-zero index. */
int itts_gpt_latent_batch_cond(itts_engine* e, const float* cond, const int32_t* cond_index_host, int n_cond,
                               const int32_t* text_ids_host, const int32_t* text_lens_host, const int32_t* codes_host,
                               const int32_t* code_lens_host, int nseq, void* latent_out, itts_stream stream);
/* The PACKED latent pass: the interface of itts_gpt_latent_batch_cond (cond_index_host may be NULL = block 0 for every sentence;
 * n_cond >= 1), 1 <= nseq <= ITTS_VARLEN_MAX_SEQ.  The tokens of all sentences lie back to back [sum S_i, D] with no pad rows, the
 * attention tiles every sentence from its own key 0 (itts_attention_varlen's dispatcher), no GEMM splits K and the GEMM kernel
 * family is picked from the projection's own dims, never from the row count: a sentence's latent has the same bits alone, with any
 * companions, in any order and in any chunking.  Writes no K/V cache.  latent_out = [sum T_i, D] in the engine dtype. */
int itts_gpt_latent_packed(itts_engine* e, const float* cond, const int32_t* cond_index_host, int n_cond,
                           const int32_t* text_ids_host, const int32_t* text_lens_host, const int32_t* codes_host,
                           const int32_t* code_lens_host, int nseq, void* latent_out, itts_stream stream);

/* The INCREMENTAL packed latent pass (opt-in): the sequences of itts_gpt_latent_packed, opened together and fed their
 * codes in pieces while they are still being decoded.  The engine keeps each sequence's K/V history ([layers][nseq][prefix + max_codes]
 * [2 D] in the engine dtype), allocated by open and freed by close - never inside an append, and no buffer of a captured decode step
 * moves.  One stream per engine.
 * itts_gpt_latent_stream_open: cond / cond_index_host / n_cond / text_ids_host / text_lens_host / nseq as itts_gpt_latent_packed (cond
 * must stay valid until close); max_codes = the most codes any sequence will be given (1 .. max_mel_tokens + 1).
 * itts_gpt_latent_stream_append: counts_host[b] more codes for sequence b (0 leaves it alone), codes_host = those codes, sequence after
 * sequence; latent_out [sum counts, D] in the engine dtype receives one latent row per code, sequence after sequence.  The identity:
 * after any sequence of appends the rows delivered so far are, bit for bit, the first rows itts_gpt_latent_packed gives for the final
 * codes (latent row j reads the start token and the codes < j, so a code's own row is computed by the append that follows it).  A
 * call with fewer than 16 rows on a 16-bit engine re-runs the last rows it already computed, so that every GEMM keeps the kernel
 * family of the packed pass.  Synchronises the stream before it returns.
 * itts_gpt_latent_stream_close: frees the history; without an open stream it does nothing.
 * Refused with ITTS_E_INVALID before any HIP call, with a message that begins with the entry's name: an append without an open stream;
 * an append past max_codes; a mel code outside [0, number_mel_codes); a negative count; a second open; null pointers; nseq outside
 * 1 .. ITTS_VARLEN_MAX_SEQ; a text length or id, a conditioning index or max_codes out of range. */
int itts_gpt_latent_stream_open(itts_engine* e, const float* cond, const int32_t* cond_index_host, int n_cond,
                                const int32_t* text_ids_host, const int32_t* text_lens_host, int nseq, int max_codes, itts_stream stream);
int itts_gpt_latent_stream_append(itts_engine* e, const int32_t* codes_host, const int32_t* counts_host, void* latent_out,
                                  itts_stream stream);
int itts_gpt_latent_stream_close(itts_engine* e);

/* V1-V5  BigVGAN.forward given the speaker embedding (BigVGAN/models.py:201-250):
 * latent [B, T, gpt_dim] (engine dtype), spk fp32 [B, spk_dim] -> wav fp32 [B, T * prod(up_rates)] */
int itts_bigvgan(itts_engine* e, const void* latent, const float* spk, int B, int T, float* wav_out, itts_stream stream);

/* The same over a padded ragged batch (opt-in): item b is a latent of lens_host[b] frames (host int32 [B], each in
 * [1, T]) at the head of its T rows, whatever the rows behind them hold (they are not read as signal; latent is not modified).
 * wav_out fp32 [B][T * prod(up_rates)]: the first lens_host[b] * prod(up_rates) samples of row b are the waveform of that latent run
 * alone (the same kernels on the same values; a K-split or tile choice that depends on the row count may reorder fp32 sums), the
 * samples behind them are zero.  Refused with ITTS_E_INVALID before any HIP call: null pointers, B outside [1, max_batch], T < 1,
 * a length outside [1, T].  lens_host is consumed before the call returns. */
int itts_bigvgan_ragged(itts_engine* e, const void* latent, const float* spk, int B, int T, const int32_t* lens_host, float* wav_out,
                        itts_stream stream);

/* The same over PACKED sentences (opt-in): latent [off_host[n], gpt_dim] (engine dtype) holds n sentences back to back,
 * sentence b the frames [off_host[b], off_host[b + 1]) of which the first lens_host[b] are signal; whatever the rest holds is not read
 * as signal (latent is not modified).  spk fp32 [n, spk_dim], one row per sentence.  wav_out fp32 [off_host[n] * prod(up_rates)]:
 * samples [off_host[b] * up, (off_host[b] + lens_host[b]) * up) are the waveform of sentence b, the rest of its capacity is zero.  The
 * matrix kernels see one item; a tap that leaves a sentence reads the zeros of a gap, which is the zero "same" padding the sentence
 * sees alone, so every capacity must be at least lens_host[b] + itts_bigvgan_packed_gap(cfg) frames.  No GEMM splits K and every
 * kernel family is picked without looking at the row count (short packs are extended by zero frames to the families' minimum rows):
 * a sentence's samples are the same bits alone, with any companions, in any order and in any chunking.
 * Refused with ITTS_E_INVALID before any HIP call (itts_bigvgan_packed_check is that judgement alone, engine-free, on host memory):
 * null engine / pointers, n outside [1, 128], off_host[0] != 0, a length < 1, offsets not increasing, a capacity below
 * len + gap ("gap too small"), more than 2^31 - 1 output samples.  off_host / lens_host are consumed before the call returns. */
int itts_bigvgan_packed(itts_engine* e, const void* latent, const float* spk, const int32_t* off_host, const int32_t* lens_host, int n,
                        float* wav_out, itts_stream stream);
int itts_bigvgan_packed_check(const itts_config* cfg, const void* latent, const float* spk, const int32_t* off_host,
                              const int32_t* lens_host, int n, const float* wav_out);
/* The zero frames a packed sentence needs behind its signal: the largest reach of any convolution of the generator (conv_pre, every
 * ups[i] at its input rate, every AMP conv (k * d - d) / 2 at its stage's rate, conv_post) in latent frames, rounded up. */
int itts_bigvgan_packed_gap(const itts_config* cfg);

/* Q1  DiscreteVAE.decode (vqvae/xtts_dvae.py:332-351): codes host int32 [B, T] -> mel [B, 4T, channels] engine dtype */
int itts_dvae_decode(itts_engine* e, const int32_t* codes_host, int B, int T, void* mel_out, itts_stream stream);

/* DiscreteVAE.get_codebook_indices (vqvae/xtts_dvae.py:325-330; Quantize.forward distance arg-min :86-92):
 * mel [B, T, channels] engine dtype -> codes host int32 [B, T'], T' = T halved (rounding up) once per stride-2 layer.
 * Needs the encoder tensors of the checkpoint (dvae.enc* / dvae.erb* / dvae.eout / dvae.codebook_sq). Synchronises. */
int itts_dvae_encode(itts_engine* e, const void* mel_btc, int B, int T, int32_t* codes_host, itts_stream stream);

/* Opt-in: let a model whose GPT projections and mel_head all carry fp8-e4m3 copies (BASELINE config 5) run its 1 - 6 row
 * decode steps on the persistent decode engine, which then streams the fp8 bytes (bf16 build only).  Sticky per engine
 * object, default 0 = the launch path, bit-identical results either way.  The environment variable ITTS_ENGINE_FP8, read
 * per call, overrides it in both directions (1: on for every engine, 0: off). */
int itts_gpt_set_engine_fp8(itts_engine* e, int on);

/* Opt-in: keep the K/V cache of the GPT decode steps as OCP e4m3 bytes without a scale instead of the engine's 16-bit type (half
 * the bytes the batched decode step streams, half the largest allocation of a generation).  Both libraries; an fp32 engine is
 * refused with an error.  Sticky per engine object, default 0 = the 16-bit cache, which behaves exactly as before.  The
 * environment variable ITTS_KV_FP8 overrides it in both directions (1 / 0; fp32 engines ignore it).  The value is latched by
 * itts_gpt_prefill for the whole generation: a change takes effect at the next prefill, which re-zeroes the cache and re-captures
 * the step.  With an fp8 cache every decode step takes the launch path's whole-form attention (itts_gpt_decode_mode answers 0:
 * no persistent engine - unless itts_gpt_set_engine_kv_fp8 below opted in -, no split form, no fused qkv + attention launch); everything else - fp8 weights, samplers, beams, forced
 * and input tokens, host sampling - is unaffected.  Accuracy and speed as measured: INTEGRATION.md, profiles/kv_fp8.txt. */
int itts_gpt_set_kv_fp8(itts_engine* e, int on);

/* Opt-in, on top of itts_gpt_set_kv_fp8: let a generation with an fp8 K/V cache run its 1 - 6 row decode steps (beam rows included)
 * on the persistent decode engine, whose attention phase then reads and appends the e4m3 rows itself (itts_gpt_decode_mode
 * answers 1).  Both libraries; together with itts_gpt_set_engine_fp8 in the bf16 build.  Sticky per engine object, default 0 = an
 * fp8 cache keeps the launch path at every row count, as before; without an fp8 cache the switch has no effect.  The environment
 * variable ITTS_ENGINE_KV_FP8, read per call, overrides it in both directions (1: on for every engine, 0: off).  The launch
 * path's whole-form attention and the engine read the same cache bytes but sum in another order: results agree to a tolerance,
 * not bit for bit (profiles/engine_kv_fp8.txt). */
int itts_gpt_set_engine_kv_fp8(itts_engine* e, int on);

/* Debug/testing: copy a named intermediate of the LAST call into host memory (fp32), returns element count. */
int64_t itts_debug_fetch(itts_engine* e, const char* name, float* out_host, int64_t max_elems);
int itts_debug_enable(itts_engine* e, int on);

#ifdef __cplusplus
}
#endif
#endif

// The host-side judgements of the append entries: attention_append / kv_rows_append (attention_append.hip) and the latent stream
// (itts_gpt_latent_stream_open / _append).  Plain C++ on host memory - no HIP call, no allocation, no engine - so that the entries
// can refuse before anything runs and so that tests/host/append_check_main.cpp can run every refusal under the host sanitizers.
#include <cstdlib>

#include "itts_kernels.h"

namespace itts {

// attention_varlen_mfma_supported's rule on the append arguments: type, head dims, leading dims, alignment - never a length or a count
bool attention_append_mfma_supported(const AppendArgs& a, int dt) {
  return dt == BF16 && a.dqk == 64 && a.dv == 64 && a.ldq % 8 == 0 && a.ldk % 8 == 0 && a.ldv % 8 == 0 &&
         !(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v) & 15);
}

// the four arrays alone (both entries): counts, ranges, the rows a sequence may touch
static const char* append_table_refusal(const AppendArgs& a) {
  if (a.nseq < 1 || a.nseq > VARLEN_MAX_SEQ) return "nseq outside 1 .. 128";
  if (a.q_off[0] < 0 || a.kv_off[0] < 0) return "q_off_host[0] and kv_off_host[0] must be >= 0";
  for (int b = 0; b < a.nseq; ++b) {
    if (a.q_off[b + 1] < a.q_off[b] || a.kv_off[b + 1] < a.kv_off[b]) return "q_off_host and kv_off_host must not decrease";
    if (a.n_new[b] < 0) return "negative n_new";
    if (a.pos0[b] < 0) return "negative pos0";
    if (a.n_new[b] > a.q_off[b + 1] - a.q_off[b]) return "n_new past the sequence's rows of q / o (q_off_host[b + 1] - q_off_host[b])";
    if ((long)a.pos0[b] + a.n_new[b] > (long)a.kv_off[b + 1] - a.kv_off[b])
      return "pos0 + n_new past the sequence's history block (kv_off_host[b + 1] - kv_off_host[b])";
  }
  return nullptr;
}

const char* attention_append_refusal(const AppendArgs& a, int dt, int kernel) {
  if (!a.q || !a.k || !a.v || !a.o) return "null pointer (q, k, v, o, q_off_host, kv_off_host, pos0_host, n_new_host)";
  if (const char* why = append_table_refusal(a)) return why;
  if (a.H < 1 || a.H > 65535) return "H is a grid dimension (1 .. 65535)";
  if (dt != F32 && dt != BF16) return "dtype must be ITTS_F32 or ITTS_BF16 (the library's 16-bit type)";
  if (a.dqk < 1 || a.dqk > 128 || a.dv < 1 || a.dv > 64) return "head dims out of range (1 <= dqk <= 128, 1 <= dv <= 64)";
  if (a.ldq < a.H * a.dqk || a.ldk < a.H * a.dqk || a.ldv < a.H * a.dv || a.ldo < a.H * a.dv)
    return "bad leading dims (ldq, ldk >= H * dqk; ldv, ldo >= H * dv)";
  if (kernel < 0 || kernel > 2) return "unknown kernel (0 dispatcher, 1 attn_append_simple, 2 attn_append_mfma)";
  if (kernel == 2 && !attention_append_mfma_supported(a, dt))
    return "attn_append_mfma needs the 16-bit type, dqk 64, dv 64, ldq / ldk / ldv % 8 == 0 and 16-byte aligned q, k, v";
  return nullptr;
}

int attention_append_which(const AppendArgs& a, int dt) {
  static const bool no_mfma = getenv("ITTS_ATTN_SIMPLE") != nullptr;  // the switch of attention(): one meaning for every dispatcher
  return !no_mfma && attention_append_mfma_supported(a, dt) ? 2 : 1;
}

const char* kv_rows_append_refusal(const AppendArgs& a, const void* ksrc, const void* vsrc, int lds, int wk, int wv, int dt) {
  if (!a.k || !a.v || !ksrc || !vsrc) return "null pointer (k_hist, v_hist, k_src, v_src, q_off_host, kv_off_host, pos0_host, n_new_host)";
  if (const char* why = append_table_refusal(a)) return why;
  if (dt != F32 && dt != BF16) return "dtype must be ITTS_F32 or ITTS_BF16 (the library's 16-bit type)";
  if (wk < 1 || wv < 1) return "widths must be >= 1";
  if (lds < wk || lds < wv || a.ldk < wk || a.ldv < wv) return "bad leading dims (ld_src >= wk, wv; ldk >= wk; ldv >= wv)";
  return nullptr;
}

const char* latent_stream_open_refusal(const LatentStreamState& st, const void* cond, const int32_t* cond_index, int n_cond,
                                       const int32_t* text_ids, const int32_t* text_lens, int nseq, int max_codes, int max_text_tokens,
                                       int max_mel_tokens, int number_text_tokens) {
  if (st.open) return "a stream is already open (close it first)";
  if (!cond || !text_ids || !text_lens) return "null pointer (cond, text_ids_host, text_lens_host)";
  if (nseq < 1 || nseq > VARLEN_MAX_SEQ) return "nseq outside 1 .. 128";
  if (n_cond < 1) return "n_cond must be >= 1";
  if (max_codes < 1 || max_codes > max_mel_tokens + 1) return "max_codes outside 1 .. max_mel_tokens + 1";
  long to = 0;
  for (int b = 0; b < nseq; ++b) {
    if (text_lens[b] < 1 || text_lens[b] > max_text_tokens) return "a text length outside 1 .. max_text_tokens";
    const int cb = cond_index ? cond_index[b] : 0;
    if (cb < 0 || cb >= n_cond) return "conditioning index outside [0, n_cond)";
    for (int i = 0; i < text_lens[b]; ++i)
      if (text_ids[to + i] < 0 || text_ids[to + i] > number_text_tokens) return "text id out of range";
    to += text_lens[b];
  }
  return nullptr;
}

const char* latent_stream_append_refusal(const LatentStreamState& st, const int32_t* codes, const int32_t* counts, const void* latent_out) {
  if (!st.open) return "no open stream (itts_gpt_latent_stream_open first)";
  if (!codes || !counts || !latent_out || !st.done) return "null pointer (codes_host, counts_host, latent_out)";
  long co = 0;
  for (int b = 0; b < st.nseq; ++b) {
    if (counts[b] < 0) return "negative count";
    if ((long)st.done[b] + counts[b] > st.max_codes) return "append past max_codes";
    for (int i = 0; i < counts[b]; ++i)
      if (codes[co + i] < 0 || codes[co + i] >= st.number_mel_codes) return "mel code out of range";
    co += counts[b];
  }
  return nullptr;
}

}  // namespace itts

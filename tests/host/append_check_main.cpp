// The host-side checks of the append entries (csrc/append_check.cpp) run stand-alone under the host sanitizers: no GPU, no Python, no
// preload.  Built and run by tests/test_append_check_host.py:
//   hipcc -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I index-tts-ipex_amd/csrc
//         tests/host/append_check_main.cpp index-tts-ipex_amd/csrc/append_check.cpp -o append_check_host
// Every case is one of the refusals of itts_attention_append / itts_kv_rows_append / itts_gpt_latent_stream_open / _append; the arrays
// are exactly as long as the entries may read them, so a read past an end is the sanitizer's to report.  Exit status 0 = every case
// answered as expected.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "itts_kernels.h"

using namespace itts;

static int failures = 0;

static void expect(const char* what, const char* got, const char* needle) {
  const bool ok = needle ? (got && strstr(got, needle)) : !got;
  if (!ok) {
    ++failures;
    printf("FAIL %s: got %s, expected %s\n", what, got ? got : "(accepted)", needle ? needle : "(accepted)");
  }
}

static AppendArgs good() {
  static float buf[64] __attribute__((aligned(16)));
  AppendArgs a;
  a.q = a.k = a.v = buf;
  a.o = buf;
  a.H = 2, a.dqk = 64, a.dv = 64, a.nseq = 3;
  a.ldq = 384, a.ldk = a.ldv = 256, a.ldo = 128;
  const int q_off[4] = {0, 17, 80, 81}, kv_off[4] = {0, 136, 199, 203}, pos0[3] = {0, 0, 0}, n_new[3] = {17, 63, 1};
  memcpy(a.q_off, q_off, sizeof q_off);
  memcpy(a.kv_off, kv_off, sizeof kv_off);
  memcpy(a.pos0, pos0, sizeof pos0);
  memcpy(a.n_new, n_new, sizeof n_new);
  return a;
}

int main() {
  // ---- attention_append_refusal ----
  // (on the heap: AppendArgs is 2 KiB and the sanitizers pad every stack object)
  auto pa = std::make_unique<AppendArgs>(good());
  AppendArgs& a = *pa;
  expect("good bf16 dispatcher", attention_append_refusal(a, BF16, 0), nullptr);
  expect("good bf16 mfma", attention_append_refusal(a, BF16, 2), nullptr);
  expect("good fp32 simple", attention_append_refusal(a, F32, 1), nullptr);
  if (!attention_append_mfma_supported(a, BF16) || attention_append_mfma_supported(a, F32)) ++failures, printf("FAIL mfma rule\n");
  a.q = nullptr;
  expect("null q", attention_append_refusal(a, BF16, 0), "null pointer");
  a = good(), a.o = nullptr;
  expect("null o", attention_append_refusal(a, BF16, 0), "null pointer");
  a = good(), a.nseq = 0;
  expect("nseq 0", attention_append_refusal(a, BF16, 0), "nseq");
  a = good(), a.nseq = 129;
  expect("nseq 129", attention_append_refusal(a, BF16, 0), "nseq");
  a = good(), a.nseq = 128;  // the arrays' last entries are read and are zeros: offsets decrease
  expect("nseq 128 over a 3-sequence table", attention_append_refusal(a, BF16, 0), "must not decrease");
  a = good(), a.n_new[1] = -1;
  expect("negative n_new", attention_append_refusal(a, BF16, 0), "negative n_new");
  a = good(), a.pos0[2] = -1;
  expect("negative pos0", attention_append_refusal(a, BF16, 0), "negative pos0");
  a = good(), a.pos0[1] = 1;
  expect("pos0 + n_new past the block", attention_append_refusal(a, BF16, 0), "history block");
  a = good(), a.pos0[0] = 0x7fffffff, a.n_new[0] = 17;
  expect("pos0 + n_new overflows int", attention_append_refusal(a, BF16, 0), "history block");
  a = good(), a.n_new[0] = 18;
  expect("n_new past the q rows", attention_append_refusal(a, BF16, 0), "rows of q");
  a = good();
  expect("kernel 2 on fp32", attention_append_refusal(a, F32, 2), "attn_append_mfma needs");
  expect("kernel 3", attention_append_refusal(a, BF16, 3), "unknown kernel");
  expect("dtype", attention_append_refusal(a, I32, 0), "dtype");
  a.ldk = 64;
  expect("ldk", attention_append_refusal(a, BF16, 0), "leading dims");
  a = good(), a.dqk = 129;
  expect("dqk", attention_append_refusal(a, F32, 1), "head dims");
  a = good(), a.q = (const char*)a.q + 2;
  expect("misaligned q for mfma", attention_append_refusal(a, BF16, 2), "attn_append_mfma needs");
  if (attention_append_which(a, BF16) != 1) ++failures, printf("FAIL misaligned q must take the vector kernel\n");
  // ---- kv_rows_append_refusal ----
  a = good();
  expect("kv good", kv_rows_append_refusal(a, a.q, a.q, 384, 128, 128, BF16), nullptr);
  expect("kv null src", kv_rows_append_refusal(a, nullptr, a.q, 384, 128, 128, BF16), "null pointer");
  expect("kv width", kv_rows_append_refusal(a, a.q, a.q, 384, 0, 128, BF16), "widths");
  expect("kv ld", kv_rows_append_refusal(a, a.q, a.q, 64, 128, 128, BF16), "leading dims");
  a.pos0[1] = 1;
  expect("kv past the block", kv_rows_append_refusal(a, a.q, a.q, 384, 128, 128, BF16), "history block");
  // ---- the latent stream ----
  const float cond = 0.f;
  const std::vector<int32_t> text = {5, 6, 7, 8, 9}, lens = {2, 3}, cidx = {1, 0};
  LatentStreamState st;
  auto open = [&](int nseq, int max_codes, const int32_t* ci = nullptr, int n_cond = 1) {
    return latent_stream_open_refusal(st, &cond, ci, n_cond, text.data(), lens.data(), nseq, max_codes, 32, 64, 40);
  };
  expect("open good", open(2, 10), nullptr);
  expect("open good with voices", open(2, 10, cidx.data(), 2), nullptr);
  expect("open voice out of range", open(2, 10, cidx.data(), 1), "conditioning index");
  expect("open nseq 0", open(0, 10), "nseq");
  expect("open nseq 129", open(129, 10), "nseq");
  expect("open max_codes 0", open(2, 0), "max_codes");
  expect("open max_codes too large", open(2, 66), "max_codes");
  expect("open null cond", latent_stream_open_refusal(st, nullptr, nullptr, 1, text.data(), lens.data(), 2, 10, 32, 64, 40), "null pointer");
  expect("open text id", latent_stream_open_refusal(st, &cond, nullptr, 1, text.data(), lens.data(), 2, 10, 32, 64, 8), "text id");
  expect("open text length", latent_stream_open_refusal(st, &cond, nullptr, 1, text.data(), lens.data(), 2, 10, 2, 64, 40), "text length");
  const std::vector<int32_t> codes = {1, 2, 3, 4}, counts = {3, 1}, none = {0, 0};
  float out = 0.f;
  expect("append without a stream", latent_stream_append_refusal(st, codes.data(), counts.data(), &out), "no open stream");
  std::vector<int> done = {0, 9};
  st.open = true, st.nseq = 2, st.max_codes = 10, st.number_mel_codes = 5, st.done = done.data();
  expect("second open", open(2, 10), "already open");
  expect("append good", latent_stream_append_refusal(st, codes.data(), counts.data(), &out), nullptr);
  expect("append nothing", latent_stream_append_refusal(st, codes.data(), none.data(), &out), nullptr);
  done[1] = 10;
  expect("append past max_codes", latent_stream_append_refusal(st, codes.data(), counts.data(), &out), "past max_codes");
  done[1] = 0, st.number_mel_codes = 4;
  expect("mel code out of range", latent_stream_append_refusal(st, codes.data(), counts.data(), &out), "mel code out of range");
  st.number_mel_codes = 5;
  const std::vector<int32_t> neg = {3, -1};
  expect("negative count", latent_stream_append_refusal(st, codes.data(), neg.data(), &out), "negative count");
  expect("append null", latent_stream_append_refusal(st, nullptr, counts.data(), &out), "null pointer");
  printf(failures ? "%d case(s) failed\n" : "append_check: every case answered as expected\n", failures);
  return failures ? 1 : 0;
}

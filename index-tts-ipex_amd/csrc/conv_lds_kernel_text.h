// The text of conv_lds_kernel (conv_lds.hip), compiled three times (no include guard):
//   ITTS_CONV_RAG 0   conv_lds_kernel       every item is a signal of g.T rows
//   ITTS_CONV_RAG 1   conv_lds_rag_kernel   (ACT only) padded ragged batch: item b is the signal of its first Tv = lens[b] * mul rows inside
//                     the g.T-row buffer.  Tv stands for T in exactly the four places that mean "signal length" - the replicate clamp
//                     of the raw-row load, the two zero-fill loops and snake_run; the item stride and the epilogue keep g.T (rows behind
//                     Tv are computed from zero-padded input and stored like any other).  lens / mul are kernel parameters of this form
//                     only: GemmArgs, a by-value argument of every GEMM kernel, does not grow.
//   ITTS_CONV_RAG 2   conv_lds_seg_kernel   (ACT only) packed sentences, one grid row (blockIdx.y) per sentence: sentence b owns rows
//                     [off[b] * mul, off[b + 1] * mul) of every operand - that capacity stands for T in the item base, the tile bound and
//                     the epilogue - and its signal is the first Tv = len[b] * mul of them.  Halo rows with t < 0 or t >= Tv are zero
//                     as in form 1 (the zero "same" padding the sentence would see alone); no output row outside the capacity is stored
//                     and a tile behind the capacity leaves before the first barrier.  The table is a by-value parameter of this form.
// One text, so the two forms cannot drift apart; a second inclusion instead of a template flag, so that the symbols, arguments and
// instructions of the plain kernels stay exactly what they were.
#if ITTS_CONV_RAG == 2
#define CONV_LDS_KERNEL conv_lds_seg_kernel
#define CONV_LDS_RAG_PARAMS , SegTable seg, int mul
#define CONV_LDS_ITEM_ROW0(b, T) ((size_t)seg.off[b] * mul)  // first row of sentence b
#elif ITTS_CONV_RAG
#define CONV_LDS_KERNEL conv_lds_rag_kernel
#define CONV_LDS_RAG_PARAMS , const int* __restrict__ lens, int mul
#define CONV_LDS_ITEM_ROW0(b, T) (size_t)b * T
#else
#define CONV_LDS_KERNEL conv_lds_kernel
#define CONV_LDS_RAG_PARAMS
#define CONV_LDS_ITEM_ROW0(b, T) (size_t)b * T
#endif

// MT x NT 16x16 tiles per wave, WAVES_M x WAVES_N waves (= 4)
template <int MT, int NT, int WAVES_M, int WAVES_N, bool ACT>
__global__ __launch_bounds__(256) void CONV_LDS_KERNEL(GemmArgs g, int tiles_per_item, int HR, int CP CONV_LDS_RAG_PARAMS) {
#if ITTS_CONV_RAG
  static_assert(ACT, "the ragged form exists for the fused activation only");
#endif
  constexpr int BM = WAVES_M * MT * 16, NP = WAVES_N * NT * 16;
  constexpr int WROWS = (NP + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // LDS: [planes][staged weights], or with ACT [planes][raw tile] with the staged weights on top of the raw tile once it is dead
  bf16_t* sA = reinterpret_cast<bf16_t*>(smem);                              // [CP / 32 planes][HR][32] (CP = channels rounded up to 32)
  bf16_t* sW = reinterpret_cast<bf16_t*>(smem + (size_t)HR * CP * 2);        // [2][NP][WROW]
  bf16_t* sX = sW;                                                           // ACT: raw rows [HR + 12][C], row j = x[clamp(tlo - 6 + j)]
  float* sC = reinterpret_cast<float*>(smem);                                // epilogue: [BM][NP + 4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
#if ITTS_CONV_RAG == 2
  const int b = blockIdx.y, t0 = blockIdx.x * BM;  // grid (tiles of the longest capacity, sentences)
  const int T = (seg.off[b + 1] - seg.off[b]) * mul, C = g.Cin, K = g.taps * C;  // T: rows of the sentence's capacity
  if (t0 >= T) return;  // (workgroup-uniform, before the first barrier)
#else
  const int b = blockIdx.x / tiles_per_item, t0 = (blockIdx.x - b * tiles_per_item) * BM;
  const int T = g.T, C = g.Cin, K = g.taps * C;
#endif
  const bf16_t* __restrict__ A = (const bf16_t*)g.A + CONV_LDS_ITEM_ROW0(b, T) * g.lda;
  const bf16_t* __restrict__ W = (const bf16_t*)g.W;

  // ---- resident input tile: rows t0 - pad_left + i, zero outside [0, T); pad columns zero ----
  if constexpr (!ACT) {
    // (row, 16-byte column) of vector v = tid + 256 * step, stepped without a division per vector
    const int vpr = CP >> 3, cv = C >> 3, nvec = HR * vpr;
    const int di = 256 / vpr, dq = 256 - di * vpr;
    int i = tid / vpr, q = tid - i * vpr;
    for (int v = tid; v < nvec; v += 256, i += di, q += dq) {
      if (q >= vpr) {
        q -= vpr;
        ++i;
      }
      const int ts = t0 - g.pad_left + i;
      u32x4 val = u32x4{0u, 0u, 0u, 0u};
      if (q < cv && ts >= 0 && ts < T) val = *reinterpret_cast<const u32x4*>(A + (size_t)ts * g.lda + q * 8);
      *reinterpret_cast<u32x4*>(sA + ((size_t)(q >> 2) * HR + i) * PROWE + (((q & 3) ^ swz4(i)) << 3)) = val;
    }
  } else {
    const int tlo = t0 - g.pad_left;  // time of plane row 0
#if ITTS_CONV_RAG == 2
    const long lv = (long)seg.len[b] * mul;
    const int Tv = lv < 1 ? 1 : (lv > T ? T : (int)lv);  // signal length of this sentence
#elif ITTS_CONV_RAG
    const long lv = (long)lens[b] * mul;
    const int Tv = lv < 1 ? 1 : (lv > T ? T : (int)lv);  // signal length of this item (device lengths are clamped to [1, T])
#else
    const int Tv = T;  // signal length = rows of the buffer
#endif
    {  // raw rows, replicate-clamped (Activation1d pads its input and its up-sampled signal by replication, resample.py:24-33)
      const int cv = C >> 3, nvec = (HR + 12) * cv;
      const int di = 256 / cv, dq = 256 - di * cv;
      int i = tid / cv, q = tid - i * cv;
      for (int v = tid; v < nvec; v += 256, i += di, q += dq) {
        if (q >= cv) {
          q -= cv;
          ++i;
        }
        int ts = tlo - 6 + i;
        ts = ts < 0 ? 0 : (ts >= Tv ? Tv - 1 : ts);
        *reinterpret_cast<u32x4*>(sX + (size_t)i * C + q * 8) = *reinterpret_cast<const u32x4*>(A + (size_t)ts * g.lda + q * 8);
      }
    }
    // the channels behind C of the last plane multiply as zero whatever they hold (cok), but must be finite: clear them
    if ((C & 31) != 0) {
      const int padv = (CP - C) >> 3, cvv = C >> 3;  // 16-byte slots per row to clear
      for (int v = tid; v < HR * padv; v += 256) {
        const int i = v / padv, q = cvv + (v - i * padv);
        *reinterpret_cast<u32x4*>(sA + ((size_t)(q >> 2) * HR + i) * PROWE + (((q & 3) ^ swz4(i)) << 3)) = u32x4{0u, 0u, 0u, 0u};
      }
    }
    __syncthreads();
    const int runs = 256 / C, c = tid % C, run = tid / C;
    if (run < runs) {
      const int per = (HR + runs - 1) / runs;
      const int i0 = run * per, i1 = min(i0 + per, HR);  // plane rows [i0, i1) = times tlo + i
      const float ea = expf(g.pre_alpha[c]);
      const float inv_b = 1.f / (expf(g.pre_beta[c]) + 1e-9f);
      float fu[12], fd[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) fu[i] = fd[i] = g.pre_filt[i];
      const int pl = c >> 5, sl = (c & 31) >> 3, el = c & 7;
      auto put = [&](int i, float y) {
        sA[((size_t)pl * HR + i) * PROWE + ((sl ^ swz4(i)) << 3) + el] = (bf16_t)y;
      };
      // rows whose time lies outside [0, Tv) are the convolution's ZERO padding (of the activated signal)
      const int ta = max(tlo + i0, 0), tb = min(tlo + i1, Tv);
      for (int i = i0; i < min(i1, -tlo); ++i) put(i, 0.f);
      for (int i = max(i0, Tv - tlo); i < i1; ++i) put(i, 0.f);
      if (ta < tb) snake_run<bf16_t, true>(sX + c, C, tlo - 6, ta, tb, Tv, ea, inv_b, fu, fd, [&](int t, float y) { put(t - tlo, y); });
    }
    __syncthreads();  // the planes are complete and the raw tile is dead: the staged weights may take its place
  }
  const int cpt = (C + 31) >> 5, nchunk = g.taps * cpt, npair = (nchunk + 1) >> 1;
  const int lr = tid >> 2, lq = tid & 3;
  const bf16_t* w_row[WROWS];
#pragma unroll
  for (int p = 0; p < WROWS; ++p) w_row[p] = W + (size_t)min(lr + 64 * p, g.N - 1) * K;
  u32x4 rw[2][WROWS];
  unsigned wok = 0;
  int nx_ch = 0, nx_tap = 0, nx_c0 = 0;  // weight chunks are requested in order: running (tap, channel) counters, no division
  auto load_w = [&]() {
    wok = 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const bool live = nx_ch < nchunk;
      const int tap = live ? nx_tap : 0, c0 = live ? nx_c0 : 0;
      const bool cok = live && lq * 8 < C - c0;
      const int cq = cok ? lq * 8 : 0;
#pragma unroll
      for (int p = 0; p < WROWS; ++p) {
        rw[c][p] = *reinterpret_cast<const u32x4*>(w_row[p] + (size_t)tap * C + c0 + cq);
        wok |= ((cok && lr + 64 * p < g.N) ? 1u : 0u) << (c * 8 + p);  // rows >= N and channels >= C multiply as zero
      }
      ++nx_ch;
      nx_c0 += 32;
      if (nx_c0 >= C) {
        nx_c0 = 0;
        ++nx_tap;
      }
    }
  };
  auto store_w = [&]() {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int p = 0; p < WROWS; ++p)
        if (lr + 64 * p < NP)
          *reinterpret_cast<u32x4*>(sW + ((size_t)c * NP + lr + 64 * p) * WROW + ((lq ^ swz4(lr + 64 * p)) << 3)) =
              ((wok >> (c * 8 + p)) & 1u) ? rw[c][p] : u32x4{0u, 0u, 0u, 0u};
  };
  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  load_w();
  store_w();
  __syncthreads();
  const int fr = lane & 15, fg = lane >> 4, fk = fg * 8;
  const int a_row0 = wm * MT * 16 + fr;  // fragment row of tile 0 before the tap shift (tiles i: + 16 i, which leaves the swizzle key alone)
  const bf16_t* w_lane = sW + (size_t)(wn * NT * 16 + fr) * WROW + ((fg ^ swz4(fr)) << 3);  // (rows + multiples of 16: same key)
  int tap = 0, c0 = 0;  // chunk consumed by the MFMAs, same running-counter scheme
  for (int pr = 0; pr < npair; ++pr) {
    load_w();  // pair pr + 1 (past the end: clamped addresses, stored as zeros and never read)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (2 * pr + c < nchunk) {  // block-uniform
        const bool cok = fk < C - c0;  // lanes past the last channel of a partial chunk read zero
        const int arow = a_row0 + tap * g.dil;
        const bf16_t* ap = sA + ((size_t)(c0 >> 5) * HR + arow) * PROWE + ((fg ^ swz4(arow)) << 3);
        half8_bits af[MT], wf[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const half8_bits v = *reinterpret_cast<const half8_bits*>(ap + (size_t)i * 16 * PROWE);
          af[i] = cok ? v : half8_bits{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) wf[j] = *reinterpret_cast<const half8_bits*>(w_lane + ((size_t)c * NP + j * 16) * WROW);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = half_mfma16(af[i], wf[j], acc[i][j]);
        c0 += 32;
        if (c0 >= C) {
          c0 = 0;
          ++tap;
        }
      }
    }
    __syncthreads();  // every wave is done with this weight pair (and, on the last pass, with the input tile)
    if (pr + 1 < npair) {
      store_w();
      __syncthreads();
    }
  }
  // ---- epilogue through LDS: fp32 tile [BM][NP + 4], then row-contiguous 16-byte traffic ----
  constexpr int CS = NP + 4;
  const int cr = (lane >> 4) * 4, cc = lane & 15;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) sC[(size_t)(wm * MT * 16 + i * 16 + cr + r) * CS + wn * NT * 16 + j * 16 + cc] = acc[i][j][r];
  __syncthreads();
  const int nv = g.N >> 3;  // 8-column vectors per row
  bf16_t* __restrict__ Cc = (bf16_t*)g.C + CONV_LDS_ITEM_ROW0(b, T) * g.ldc;
  const bf16_t* __restrict__ R = g.R ? (const bf16_t*)g.R + CONV_LDS_ITEM_ROW0(b, T) * g.ldr : nullptr;
  const bf16_t* __restrict__ ADD = g.ADD ? (const bf16_t*)g.ADD + CONV_LDS_ITEM_ROW0(b, T) * g.ldadd : nullptr;
  const float* bias = g.bias ? g.bias + (size_t)b * g.bias_bstride : nullptr;
  const bool plain = g.act == ACT_NONE && g.act2 == ACT_NONE && !g.scale && !g.shift && (!bias || ((uintptr_t)bias & 15) == 0);
  const int dm = 256 / nv, dq2 = 256 - dm * nv;
  int m = tid / nv, q = tid - m * nv;
  for (int v = tid; v < BM * nv; v += 256, m += dm, q += dq2) {
    if (q >= nv) {
      q -= nv;
      ++m;
    }
    const int t = t0 + m;
    if (t >= T) continue;
    const int n = q * 8;
    float o[8];
    const float4 s0 = *reinterpret_cast<const float4*>(sC + (size_t)m * CS + n);
    const float4 s1 = *reinterpret_cast<const float4*>(sC + (size_t)m * CS + n + 4);
    o[0] = s0.x; o[1] = s0.y; o[2] = s0.z; o[3] = s0.w; o[4] = s1.x; o[5] = s1.y; o[6] = s1.z; o[7] = s1.w;
    u32x4 rv = u32x4{0u, 0u, 0u, 0u}, av = u32x4{0u, 0u, 0u, 0u};
    if (R) rv = *reinterpret_cast<const u32x4*>(R + (size_t)t * g.ldr + n);
    if (ADD) av = *reinterpret_cast<const u32x4*>(ADD + (size_t)t * g.ldadd + n);
    const bf16_t* rb = reinterpret_cast<const bf16_t*>(&rv);
    const bf16_t* ab = reinterpret_cast<const bf16_t*>(&av);
    u32x4 ov;
    bf16_t* ob = reinterpret_cast<bf16_t*>(&ov);
    if (plain) {
      // the AMP-block form (bias, residual, alpha, beta * running sum; no activation / BN affine): straight-line code -
      // on the narrow stages this epilogue is issue-bound
      float bv[8];
      if (bias) {
        const float4 b0 = *reinterpret_cast<const float4*>(bias + n), b1 = *reinterpret_cast<const float4*>(bias + n + 4);
        bv[0] = b0.x; bv[1] = b0.y; bv[2] = b0.z; bv[3] = b0.w; bv[4] = b1.x; bv[5] = b1.y; bv[6] = b1.z; bv[7] = b1.w;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float x = o[e] + bv[e] + (float)rb[e];        // rv / av are zero vectors when R / ADD are absent
        x = fmaf(g.beta, (float)ab[e], x * g.alpha);
        ob[e] = (bf16_t)x;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float x = o[e];
        if (bias) x += bias[n + e];
        x = act_apply(g.act, x);
        x = x * (g.scale ? g.scale[n + e] : 1.f) + (g.shift ? g.shift[n + e] : 0.f);
        x = act_apply(g.act2, x);
        if (R) x += (float)rb[e];
        x *= g.alpha;
        if (ADD) x += g.beta * (float)ab[e];
        ob[e] = (bf16_t)x;
      }
    }
    *reinterpret_cast<u32x4*>(Cc + (size_t)t * g.ldc + n) = ov;
  }
}

#undef CONV_LDS_KERNEL
#undef CONV_LDS_RAG_PARAMS
#undef CONV_LDS_ITEM_ROW0

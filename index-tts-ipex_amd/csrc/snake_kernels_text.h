// The text of the two channels-last Activation1d kernels of snake.hip, compiled three times (no include guard):
//   ITTS_SNAKE_LEN 0   snake_aa_kernel, snake_aa_lds_kernel                  every item is a signal of Tn rows
//   ITTS_SNAKE_LEN 1   snake_aa_len_kernel, snake_aa_lds_len_kernel          padded ragged batch: Tn stays the row count (stride) of the
//                      buffer, the signal of item b is its first lens[b] * mul rows - the replicate clamp is taken at ITS last row -
//                      and the rows behind it are written as zeros (the zero "same" padding the next convolution reads).  A chunk /
//                      tile that lies wholly behind the signal stores zeros and reads nothing.
//   ITTS_SNAKE_LEN 2   snake_aa_seg_kernel, snake_aa_lds_seg_kernel          packed sentences (one item, back to back in time): sentence b =
//                      blockIdx.y owns rows [off[b] * mul, off[b + 1] * mul) - its CAPACITY stands where the length-aware form has the
//                      rows of the buffer - and its signal is the first len[b] * mul of them.  Base and capacity are the only differences
//                      from form 1; a chunk / tile behind the capacity leaves at once (before any barrier), so nothing is ever written
//                      into the next sentence.  The table travels by value in the argument block.
// One text, so the two forms cannot drift apart; a second inclusion instead of a template flag, so that the symbols, arguments and
// instructions of the plain kernels stay exactly what they were.
#if ITTS_SNAKE_LEN == 2
#define SNAKE_KERNEL(name) name##_seg_kernel
#define SNAKE_LEN_PARAMS , SegTable seg, int mul
#define SNAKE_ITEM_ROW0(b, Tb) ((size_t)seg.off[b] * mul)  // first row of sentence b
#elif ITTS_SNAKE_LEN
#define SNAKE_KERNEL(name) name##_len_kernel
#define SNAKE_LEN_PARAMS , const int* __restrict__ lens, int mul
#define SNAKE_ITEM_ROW0(b, Tb) (size_t)b * Tb
#else
#define SNAKE_KERNEL(name) name##_kernel
#define SNAKE_LEN_PARAMS
#define SNAKE_ITEM_ROW0(b, Tb) (size_t)b * Tb
#endif

template <typename T>
__global__ __launch_bounds__(256) void SNAKE_KERNEL(snake_aa)(T* __restrict__ y, const T* __restrict__ x,
                                                              const float* __restrict__ la, const float* __restrict__ lb,
                                                              const float* __restrict__ up12, const float* __restrict__ dn12,
                                                              int B, int Tn, int C, int nchunk SNAKE_LEN_PARAMS) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
#if ITTS_SNAKE_LEN == 2
  if (gid >= (long)nchunk * C) return;  // grid (chunks of the longest capacity x channels, sentences)
  const int c = (int)(gid % C);
  const int ch = (int)(gid / C);
  const int b = blockIdx.y;
  const int Tb = seg_rows(seg, mul, b);  // rows of the sentence's capacity
  if (ch * RUN >= Tb) return;
#else
  const long total = (long)B * nchunk * C;
  if (gid >= total) return;
  const int c = (int)(gid % C);
  const int ch = (int)((gid / C) % nchunk);
  const int b = (int)(gid / ((long)C * nchunk));
  const int Tb = Tn;  // rows of the buffer
#endif
#if ITTS_SNAKE_LEN
#if ITTS_SNAKE_LEN == 2
  Tn = seg_valid_rows(seg, mul, b, Tb);
#else
  Tn = valid_rows(lens, mul, b, Tb);
#endif
  {
    T* __restrict__ yz = y + SNAKE_ITEM_ROW0(b, Tb) * C + c;
    for (int t = max(ch * RUN, Tn); t < min(ch * RUN + RUN, Tb); ++t) stf(yz + (size_t)t * C, 0.f);
    if (ch * RUN >= Tn) return;
  }
#endif
  SnakeCtx<T> k;
  k.x = x + SNAKE_ITEM_ROW0(b, Tb) * C + c;
  k.Tn = Tn;
  k.C = C;
  k.ea = expf(la[c]);
  k.inv_b = 1.f / (expf(lb[c]) + 1e-9f);
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    k.fu[i] = up12[i];
    k.fd[i] = dn12[i];
  }
  T* __restrict__ yo = y + SNAKE_ITEM_ROW0(b, Tb) * C + c;
  const int t0 = ch * RUN;
  const int t1 = min(t0 + RUN, Tn);
  // window v[j] = V(2t - 5 + j), j = 0..11
  float v[12];
#pragma unroll
  for (int j = 0; j < 10; ++j) v[j] = k.v_at(2 * t0 - 5 + j);
  // input window xs[i] = x[clamp(t + i)], i = 0..5
  float xs[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) xs[i] = k.xin(t0 + i);
  const int mlast = 2 * Tn - 1;
  for (int t = t0; t < t1; ++t) {
    // new samples m = 2t+5 (odd, q = t+2) and m = 2t+6 (even, q = t+3): both read x[t .. t+5]
    float uo = 0.f, ue = 0.f;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      uo = fmaf(k.fu[2 * r], xs[5 - r], uo);
      ue = fmaf(k.fu[2 * r + 1], xs[5 - r], ue);
    }
    const float vprev = v[9];
    v[10] = (2 * t + 5 <= mlast) ? k.snake_precise(2.f * uo) : vprev;
    v[11] = (2 * t + 6 <= mlast) ? k.snake_precise(2.f * ue) : v[10];
    float o = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) o = fmaf(k.fd[j], v[j], o);
    stf(yo + (size_t)t * C, o);
#pragma unroll
    for (int j = 0; j < 10; ++j) v[j] = v[j + 2];
#pragma unroll
    for (int i = 0; i < 5; ++i) xs[i] = xs[i + 1];
    xs[5] = k.xin(t + 6);
  }
}


// ---- channels-last, LDS-tiled: the form used for every C % 8 == 0 ----------------------------------------------------
// One workgroup owns TT = (256 / CT) * RUN time steps x CT channels (CT = C for the narrow stages, a 64-channel slab
// otherwise).  The TT + 12 input rows arrive with 16-byte loads issued back to back (rows of a narrow stage are
// adjacent in memory, so the tile is one contiguous span), each lane then slides down its channel reading LDS, and the
// outputs leave through LDS as 16-byte row-contiguous stores.  The register-window kernel above pays one dependent
// global load per time step and 48-byte rows at C = 24; this one pays one memory latency per tile.
// FAST: v_sin_f32 (__sinf) as the reference's fast-math CUDA build does (bf16 I/O); fp32 I/O keeps sinf for parity.
template <typename T, bool FAST>
__global__ __launch_bounds__(256) void SNAKE_KERNEL(snake_aa_lds)(T* __restrict__ y, const T* __restrict__ x,
                                                                  const float* __restrict__ la, const float* __restrict__ lb,
                                                                  const float* __restrict__ up12, const float* __restrict__ dn12,
                                                                  int Tn, int C, int CT, int tiles_t, int slabs SNAKE_LEN_PARAMS) {
  constexpr int VEC = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_snake[];
  const int runs = 256 / CT, TT = runs * RUNL;
  T* sx = reinterpret_cast<T*>(smem_snake);                       // [(TT + 12)][CT]
  T* so = sx + (size_t)(TT + 12) * CT;                            // [TT][CT]
  int bid = blockIdx.x;
  const int slab = bid % slabs;
  bid /= slabs;
#if ITTS_SNAKE_LEN == 2
  const int tile = bid, b = blockIdx.y;  // grid (tiles of the longest capacity x slabs, sentences)
  const int t0 = tile * TT, c0 = slab * CT;
  const int Tb = seg_rows(seg, mul, b);  // rows of the sentence's capacity
  if (t0 >= Tb) return;                  // (workgroup-uniform, before the first barrier) a tile behind the capacity
#else
  const int tile = bid % tiles_t, b = bid / tiles_t;
  const int t0 = tile * TT, c0 = slab * CT;
  const int Tb = Tn;  // rows of the buffer
#endif
  const T* __restrict__ xb = x + SNAKE_ITEM_ROW0(b, Tb) * C + c0;
  T* __restrict__ yb = y + SNAKE_ITEM_ROW0(b, Tb) * C + c0;
  const int tid = threadIdx.x;
#if ITTS_SNAKE_LEN
#if ITTS_SNAKE_LEN == 2
  Tn = seg_valid_rows(seg, mul, b, Tb);
#else
  Tn = valid_rows(lens, mul, b, Tb);
#endif
  if (t0 >= Tn) {  // (workgroup-uniform) nothing of the signal in this tile
    const int vpr = CT / VEC, nvec = min(TT, Tb - t0) * vpr;
    for (int v = tid; v < nvec; v += 256) {
      const int i = v / vpr, q = v - i * vpr;
      *reinterpret_cast<uint4*>(yb + (size_t)(t0 + i) * C + q * VEC) = uint4{0u, 0u, 0u, 0u};
    }
    return;
  }
#endif
  {
    const int vpr = CT / VEC, nvec = (TT + 12) * vpr;
    const int di = 256 / vpr, dq = 256 - di * vpr;  // (row, vector) stepped without a division per vector
    int i = tid / vpr, q = tid - i * vpr;
    for (int v = tid; v < nvec; v += 256, i += di, q += dq) {
      if (q >= vpr) {
        q -= vpr;
        ++i;
      }
      int t = t0 - 6 + i;
      t = t < 0 ? 0 : (t >= Tn ? Tn - 1 : t);  // replicate padding resolved at load time
      *reinterpret_cast<uint4*>(sx + (size_t)i * CT + q * VEC) = *reinterpret_cast<const uint4*>(xb + (size_t)t * C + q * VEC);
    }
  }
  __syncthreads();
  const int c = tid % CT, run = tid / CT;
  if (run < runs) {
    const float ea = expf(la[c0 + c]);
    const float inv_b = 1.f / (expf(lb[c0 + c]) + 1e-9f);
    float fu[12], fd[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      fu[i] = up12[i];
      fd[i] = dn12[i];
    }
    const int ts = t0 + run * RUNL;
    const int te = min(ts + RUNL, Tn);
    // row i of the tile holds x[clamp(t0 - 6 + i)] (the replicate padding was resolved when the tile was loaded)
    if (ts < Tn) snake_run<T, FAST>(sx + c, CT, t0 - 6, ts, te, Tn, ea, inv_b, fu, fd, [&](int t, float o) { stf(so + (t - t0) * CT + c, o); });
  }
  __syncthreads();
  {
    const int vpr = CT / VEC, rows = min(TT, Tb - t0), nvec = rows * vpr;
    const int di = 256 / vpr, dq = 256 - di * vpr;
    int i = tid / vpr, q = tid - i * vpr;
    for (int v = tid; v < nvec; v += 256, i += di, q += dq) {
      if (q >= vpr) {
        q -= vpr;
        ++i;
      }
#if ITTS_SNAKE_LEN
      if (t0 + i >= Tn) {  // a row no run wrote
        *reinterpret_cast<uint4*>(yb + (size_t)(t0 + i) * C + q * VEC) = uint4{0u, 0u, 0u, 0u};
        continue;
      }
#endif
      *reinterpret_cast<uint4*>(yb + (size_t)(t0 + i) * C + q * VEC) = *reinterpret_cast<const uint4*>(so + (size_t)i * CT + q * VEC);
    }
  }
}

#undef SNAKE_KERNEL
#undef SNAKE_LEN_PARAMS
#undef SNAKE_ITEM_ROW0

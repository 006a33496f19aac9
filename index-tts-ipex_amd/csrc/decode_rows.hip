// Row retirement of a running batched decode (Engine::gpt_retire_rows, itts_rows_move): rows_move_kernel, a three-level strided row
// copy on raw bytes that compacts the K/V cache and the per-row state arrays to the unfinished rows, and retire_plan, the host
// function that says which rows go where.  No element type: both builds compile it identically.
#include <cstdint>

#include "itts_decode.h"

namespace itts {
namespace {

typedef unsigned rm_u32x4 __attribute__((ext_vector_type(4)));

// for o < n_outer, move i < n_moves, chunk c < n_chunks: chunk_bytes from base + o * outer_stride + src[i] * row_stride +
// c * chunk_stride to the same address with dst[i].  T = the copy unit (16 / 4 / 1 bytes: base, strides and chunk_bytes are
// multiples of it, rows_move picks the widest that fits).  A workgroup takes tiles of 256 threads x 4 units of one chunk and
// grid-strides over (outer, move, chunk, tile); the source and destination row sets are disjoint (rows_move_check), so every
// copy of the launch is independent: no atomics, no LDS, no hand-off between workgroups.  Loads and stores are non-temporal:
// every byte is touched once.
template <typename T>
__global__ __launch_bounds__(256) void rows_move_kernel(RowsMoveArgs a) {
  const unsigned upc = (unsigned)(a.chunk_bytes / sizeof(T));  // units per chunk
  const unsigned n_tiles = (upc + 1023u) / 1024u;
  const unsigned long long work = (unsigned long long)a.n_outer * a.n_moves * a.n_chunks * n_tiles;
  for (unsigned long long w = blockIdx.x; w < work; w += gridDim.x) {
    const unsigned t = (unsigned)(w % n_tiles);
    unsigned sgm = (unsigned)(w / n_tiles);
    const unsigned c = sgm % (unsigned)a.n_chunks;
    sgm /= (unsigned)a.n_chunks;
    const unsigned m = sgm % (unsigned)a.n_moves, o = sgm / (unsigned)a.n_moves;
    char* chunk = a.base + (size_t)o * a.outer_stride + (size_t)c * a.chunk_stride;
    const T* __restrict__ src = reinterpret_cast<const T*>(chunk + (size_t)a.src[m] * a.row_stride);
    T* __restrict__ dst = reinterpret_cast<T*>(chunk + (size_t)a.dst[m] * a.row_stride);
    const unsigned u0 = t * 1024u + threadIdx.x;
    T v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (u0 + j * 256u < upc) v[j] = __builtin_nontemporal_load(src + u0 + j * 256u);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (u0 + j * 256u < upc) __builtin_nontemporal_store(v[j], dst + u0 + j * 256u);
  }
}

}  // namespace

// everything rows_move refuses, without a HIP call (itts_rows_move checks before it touches the device)
int rows_move_check(const void* base, size_t outer_stride, int n_outer, size_t row_stride, size_t chunk_stride, int n_chunks,
                    size_t chunk_bytes, const int* src, const int* dst, int n_moves) {
  ITTS_REQUIRE(base, "rows_move: null base");
  ITTS_REQUIRE(n_outer >= 0 && n_chunks >= 0 && n_moves >= 0, "rows_move: negative count");
  ITTS_REQUIRE(n_moves <= ROWS_MOVE_MAX, "rows_move: more than 128 moves");
  ITTS_REQUIRE(n_moves == 0 || (src && dst), "rows_move: null move list");
  ITTS_REQUIRE(chunk_bytes <= chunk_stride, "rows_move: chunk_bytes > chunk_stride");
  ITTS_REQUIRE(chunk_bytes < (size_t(1) << 32), "rows_move: chunk_bytes must stay below 4 GiB");
  ITTS_REQUIRE(n_chunks == 0 || chunk_stride <= row_stride / (size_t)n_chunks, "rows_move: n_chunks * chunk_stride > row_stride");
  int hi = -1;
  for (int i = 0; i < n_moves; ++i) {
    ITTS_REQUIRE(src[i] >= 0 && src[i] < 65536 && dst[i] >= 0 && dst[i] < 65536, "rows_move: row index outside [0, 65536)");
    hi = src[i] > hi ? src[i] : hi;
    hi = dst[i] > hi ? dst[i] : hi;
  }
  // disjoint source and destination sets, no destination twice: the copies of one launch do not depend on each other
  for (int i = 0; i < n_moves; ++i)
    for (int j = 0; j < n_moves; ++j) {
      ITTS_REQUIRE(src[i] != dst[j], "rows_move: source and destination rows intersect");
      ITTS_REQUIRE(i == j || dst[i] != dst[j], "rows_move: a destination row is written twice");
    }
  ITTS_REQUIRE(n_outer <= 1 || hi < 0 || row_stride <= outer_stride / (size_t)(hi + 1), "rows_move: a moved row reaches past outer_stride");
  return OK;
}

int rows_move(void* base, size_t outer_stride, int n_outer, size_t row_stride, size_t chunk_stride, int n_chunks, size_t chunk_bytes,
              const int* src, const int* dst, int n_moves, hipStream_t s) {
  ITTS_TRY(rows_move_check(base, outer_stride, n_outer, row_stride, chunk_stride, n_chunks, chunk_bytes, src, dst, n_moves));
  if (n_moves == 0 || n_outer == 0 || n_chunks == 0 || chunk_bytes == 0) return OK;  // nothing to launch
  RowsMoveArgs a;
  a.base = (char*)base;
  a.outer_stride = outer_stride;
  a.row_stride = row_stride;
  a.chunk_stride = chunk_stride;
  a.chunk_bytes = chunk_bytes;
  a.n_outer = n_outer;
  a.n_moves = n_moves;
  a.n_chunks = n_chunks;
  for (int i = 0; i < n_moves; ++i) {
    a.src[i] = (unsigned short)src[i];
    a.dst[i] = (unsigned short)dst[i];
  }
  const size_t all = (size_t)(uintptr_t)base | outer_stride | row_stride | chunk_stride | chunk_bytes;
  const size_t unit = all % 16 == 0 ? 16 : all % 4 == 0 ? 4 : 1;
  const unsigned long long tiles = (chunk_bytes / unit + 1023) / 1024;
  const unsigned long long work = (unsigned long long)n_outer * n_moves * n_chunks * tiles;
  const dim3 grid((unsigned)(work < 2048 ? work : 2048)), blk(256);
  if (unit == 16)
    hipLaunchKernelGGL(rows_move_kernel<rm_u32x4>, grid, blk, 0, s, a);
  else if (unit == 4)
    hipLaunchKernelGGL(rows_move_kernel<unsigned>, grid, blk, 0, s, a);
  else
    hipLaunchKernelGGL(rows_move_kernel<unsigned char>, grid, blk, 0, s, a);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

// The hazard-free compaction of a batch to its n live rows: only live rows at slots >= n move, into the dead slots < n, both in
// ascending order.  Sources and destinations are disjoint sets, live rows below n keep their slot, the fewest bytes move.
int retire_plan(const int* unfinished, int B, int* n_live, int* src, int* dst, int* n_moves) {
  ITTS_REQUIRE(unfinished && n_live && src && dst && n_moves && B >= 0, "retire_plan: bad arguments");
  int n = 0;
  for (int b = 0; b < B; ++b) n += unfinished[b] != 0;
  int m = 0, hole = 0;
  for (int b = n; b < B; ++b) {
    if (!unfinished[b]) continue;
    while (unfinished[hole]) ++hole;  // as many dead slots below n as live rows at and above it
    src[m] = b;
    dst[m++] = hole++;
  }
  *n_live = n;
  *n_moves = m;
  return OK;
}

}  // namespace itts

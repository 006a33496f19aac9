// Row retirement of a running batched decode (Engine::gpt_retire_rows, itts_rows_move): rows_move_kernel, a three-level strided row
// copy on raw bytes that compacts the K/V cache and the per-row state arrays to the unfinished rows, rows_gather_kernel
// (itts_rows_gather), its out-of-place companion for the beam arrays whose second half starts at a base that depends on the row
// count, and retire_plan, the host function that says which rows go where.  No element type: both builds compile it identically.
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

// The out-of-place companion (rows_gather, itts_rows_gather): for plane p < n_planes and j < n_rows, row_bytes from src +
// p * src_plane_stride + src_rows[j] * row_bytes to dst + p * dst_plane_stride + j * row_bytes.  T as above.  A workgroup takes
// tiles of 256 threads x 4 units of one row and grid-strides over (plane, row, tile); the source and destination byte ranges of a
// launch do not intersect (rows_gather_check), so every copy is independent: no atomics, no LDS, no hand-off between workgroups.
template <typename T>
__global__ __launch_bounds__(256) void rows_gather_kernel(RowsGatherArgs a) {
  const unsigned upr = (unsigned)(a.row_bytes / sizeof(T));  // units per row
  const unsigned n_tiles = (upr + 1023u) / 1024u;
  const unsigned long long work = (unsigned long long)a.n_planes * a.n_rows * n_tiles;
  for (unsigned long long w = blockIdx.x; w < work; w += gridDim.x) {
    const unsigned t = (unsigned)(w % n_tiles);
    const unsigned pj = (unsigned)(w / n_tiles);
    const unsigned j = pj % (unsigned)a.n_rows, p = pj / (unsigned)a.n_rows;
    const T* __restrict__ src = reinterpret_cast<const T*>(a.src + (size_t)p * a.src_plane_stride + (size_t)a.src_rows[j] * a.row_bytes);
    T* __restrict__ dst = reinterpret_cast<T*>(a.dst + (size_t)p * a.dst_plane_stride + (size_t)j * a.row_bytes);
    const unsigned u0 = t * 1024u + threadIdx.x;
    T v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (u0 + i * 256u < upr) v[i] = __builtin_nontemporal_load(src + u0 + i * 256u);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (u0 + i * 256u < upr) __builtin_nontemporal_store(v[i], dst + u0 + i * 256u);
  }
}

}  // namespace

// everything rows_gather refuses, without a HIP call (itts_rows_gather checks before it touches the device)
int rows_gather_check(const void* dst, size_t dst_plane_stride, const void* src, size_t src_plane_stride, int n_planes, size_t row_bytes,
                      const int* src_rows, int n_rows) {
  ITTS_REQUIRE(dst && src, "rows_gather: null pointer");
  ITTS_REQUIRE(n_planes >= 0 && n_rows >= 0, "rows_gather: negative count");
  ITTS_REQUIRE(n_rows <= ROWS_MOVE_MAX, "rows_gather: more than 128 rows");
  ITTS_REQUIRE(n_rows == 0 || src_rows, "rows_gather: null row list");
  ITTS_REQUIRE(n_planes <= 65536, "rows_gather: more than 65536 planes");
  ITTS_REQUIRE(row_bytes < (size_t(1) << 32), "rows_gather: row_bytes must stay below 4 GiB");
  ITTS_REQUIRE(dst_plane_stride < (size_t(1) << 40) && src_plane_stride < (size_t(1) << 40), "rows_gather: plane stride must stay below 1 TiB");
  int lo = 65536, hi = -1;
  for (int j = 0; j < n_rows; ++j) {
    ITTS_REQUIRE(src_rows[j] >= 0 && src_rows[j] < 65536, "rows_gather: row index outside [0, 65536)");
    lo = src_rows[j] < lo ? src_rows[j] : lo;
    hi = src_rows[j] > hi ? src_rows[j] : hi;
  }
  if (n_planes == 0 || n_rows == 0 || row_bytes == 0) return OK;  // nothing is read or written
  const size_t block = (size_t)n_rows * row_bytes;  // what one plane of the destination holds
  ITTS_REQUIRE(n_planes == 1 || block <= dst_plane_stride, "rows_gather: n_rows * row_bytes > dst_plane_stride");
  // no byte is both read and written by the launch: the copies do not depend on each other.  Whole ranges first, then, where those
  // touch, every source row against every destination plane
  const uintptr_t d0 = (uintptr_t)dst, s0 = (uintptr_t)src;
  const uintptr_t d_end = d0 + (size_t)(n_planes - 1) * dst_plane_stride + block;
  const uintptr_t s_lo = s0 + (size_t)lo * row_bytes, s_end = s0 + (size_t)(n_planes - 1) * src_plane_stride + (size_t)(hi + 1) * row_bytes;
  if (d_end <= s_lo || s_end <= d0) return OK;
  for (int p = 0; p < n_planes; ++p)
    for (int j = 0; j < n_rows; ++j) {
      const uintptr_t r0 = s0 + (size_t)p * src_plane_stride + (size_t)src_rows[j] * row_bytes, r1 = r0 + row_bytes;
      if (r1 <= d0 || d_end <= r0) continue;
      // the destination plane(s) this row can reach: planes are dst_plane_stride apart and `block` long
      const size_t off = r1 - 1 - d0;  // of the row's last byte
      size_t q = n_planes == 1 ? 0 : off / dst_plane_stride;
      if (q > (size_t)(n_planes - 1)) q = (size_t)(n_planes - 1);
      const uintptr_t q0 = d0 + q * dst_plane_stride;  // the last plane that begins at or before the row's last byte
      ITTS_REQUIRE(!(r0 < q0 + block && q0 < r1), "rows_gather: source and destination ranges intersect");
      if (q > 0) {  // and the one before it, which the row's first bytes may still reach
        const uintptr_t e0 = q0 - dst_plane_stride;
        ITTS_REQUIRE(!(r0 < e0 + block && e0 < r1), "rows_gather: source and destination ranges intersect");
      }
    }
  return OK;
}

int rows_gather(void* dst, size_t dst_plane_stride, const void* src, size_t src_plane_stride, int n_planes, size_t row_bytes,
                const int* src_rows, int n_rows, hipStream_t s) {
  ITTS_TRY(rows_gather_check(dst, dst_plane_stride, src, src_plane_stride, n_planes, row_bytes, src_rows, n_rows));
  if (n_planes == 0 || n_rows == 0 || row_bytes == 0) return OK;  // nothing to launch
  RowsGatherArgs a;
  a.dst = (char*)dst;
  a.src = (const char*)src;
  a.dst_plane_stride = dst_plane_stride;
  a.src_plane_stride = src_plane_stride;
  a.row_bytes = row_bytes;
  a.n_planes = n_planes;
  a.n_rows = n_rows;
  for (int j = 0; j < n_rows; ++j) a.src_rows[j] = (unsigned short)src_rows[j];
  const size_t all = (size_t)(uintptr_t)dst | (size_t)(uintptr_t)src | row_bytes | dst_plane_stride | src_plane_stride;
  const size_t unit = all % 16 == 0 ? 16 : all % 4 == 0 ? 4 : 1;
  const unsigned long long tiles = (row_bytes / unit + 1023) / 1024;
  const unsigned long long work = (unsigned long long)n_planes * n_rows * tiles;
  const dim3 grid((unsigned)(work < 2048 ? work : 2048)), blk(256);
  if (unit == 16)
    hipLaunchKernelGGL(rows_gather_kernel<rm_u32x4>, grid, blk, 0, s, a);
  else if (unit == 4)
    hipLaunchKernelGGL(rows_gather_kernel<unsigned>, grid, blk, 0, s, a);
  else
    hipLaunchKernelGGL(rows_gather_kernel<unsigned char>, grid, blk, 0, s, a);
  ITTS_HIP_CHECK(hipGetLastError());
  return OK;
}

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

// Rows of uint16 pixels as 16-byte vectors of eight, and what the exact-integer passes over
// a uint16 stack share around them: quality.hip (q1), temporal_sums.hip (q2), shift_search.hip
// (s1), refine.hip (g1), refine_tiles.hip (g2).
#pragma once

#include "kcmc_internal.h"

namespace kcmc {

typedef unsigned long long u64;

// Lanes of the vector at column c0 (a multiple of 8) outside [x0, x1) read as 0.
__device__ __forceinline__ uint4 mask8(uint4 q, int c0, int x0, int x1) {
  if (c0 >= x0 && c0 + 8 <= x1) return q;
  uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + 2 * k;
    const uint32_t lo = (c >= x0 && c < x1) ? 0xffffu : 0u;
    const uint32_t hi = (c + 1 >= x0 && c + 1 < x1) ? 0xffff0000u : 0u;
    w[k] &= lo | hi;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// The 8 pixels of an image row from column c0 (a multiple of 8, >= 0).  VEC: c0 + 8 <= W.
template <bool VEC>
__device__ __forceinline__ uint4 load8(const uint16_t* __restrict__ row, int c0, int W) {
  if (VEC) return *reinterpret_cast<const uint4*>(row + c0);
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + 2 * k;
    const uint32_t lo = c < W ? (uint32_t)row[c] : 0u;
    const uint32_t hi = c + 1 < W ? (uint32_t)row[c + 1] : 0u;
    w[k] = lo | (hi << 16);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// f(j, pixel) for the vector's eight pixels j = 0 .. 7 in column order.
template <class F>
__device__ __forceinline__ void for_each_px(const uint4& q, F&& f) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f(2 * k, w[k] & 0xffffu);
    f(2 * k + 1, w[k] >> 16);
  }
}

template <class T>  // uint32_t or int32_t
__device__ __forceinline__ void unpack8(const uint4& q, T* v) {
  for_each_px(q, [&](int j, uint32_t px) { v[j] = (T)px; });
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// The workgroup's sums of K per-thread values: for thread k < K the total of v[k] (other
// threads get 0).  red: the caller's __shared__ scratch, one column per wave of the block.
template <int K, int WAVES>
__device__ __forceinline__ u64 block_sums(const u64 (&v)[K], u64 (&red)[K][WAVES]) {
  u64 t[K];
#pragma unroll
  for (int k = 0; k < K; ++k) t[k] = wave_sum(v[k]);
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < K; ++k) red[k][threadIdx.x >> 6] = t[k];
  __syncthreads();
  u64 r = 0;
  if (threadIdx.x < K)
    for (int w = 0; w < WAVES; ++w) r += red[threadIdx.x][w];
  return r;
}

// out: entries of five words in groups of `group`.  Words 1 and 3 (Sb, Sbb) of every group's
// first entry to the group's other entries, after the kernel that summed them on stream s.
int launch_copy_b(u64* out, size_t n_entries, int group, hipStream_t s);

// The checks kcmc_frame_stats_u16, kcmc_shift_search_u16 and kcmc_gradient_sums_u16 share, in
// one order; fn prefixes the messages.  The rectangle grown by `margin` on every side must
// stay inside the image (grown: the margin's name in the message, NULL for no margin).
int check_rect(const char* fn, kcmc_ctx* ctx, int n_frames, int n_sel, int H, int W, int y0, int y1, int x0, int x1,
               int margin, const char* grown);
int check_pointers(const char* fn, const void* frames, int n_frames, const void* ref, const void* out);

// log2 of the thread columns of a 256-thread workgroup that walks rows of nvec 8-pixel vectors
// (g1, g2): the largest power of two in [8, 256] that idles at most 1/8 of the thread columns
// over the row's vectors, else the one that idles fewest.
inline int thread_columns_log2(int nvec) {
  int ct_log2 = 3;
  long long best = -1;
  for (int l = 8; l >= 3; --l) {
    const long long ct = 1ll << l, used = (nvec + ct - 1) / ct * ct;
    if (used * 8 <= (long long)nvec * 9) return l;
    if (best < 0 || used < best) {
      best = used;
      ct_log2 = l;
    }
  }
  return ct_log2;
}

// Whether every row of the frames and of ref starts on a 16-byte boundary.
inline bool rows_vectorizable(int W, const void* frames, const void* ref) {
  return W % 8 == 0 && (((uintptr_t)frames | (uintptr_t)ref) & 15) == 0;
}

}  // namespace kcmc

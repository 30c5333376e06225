// Shared by the K1 matchers (match.hip, match_hamming.hip, match_f32.hip) and their
// per-frame filter (match_filter.hip): the device helpers of the knn kernels, the knn
// argument check and the tail of the kcmc_match_frames* entries.
#pragma once

#include "kcmc_internal.h"

namespace kcmc {

constexpr int kMaxFilterTpl = 8192;  // template rows the filter sorts (match_filter.hip)
constexpr int kMaxMatchFrames = 65535;

__device__ __forceinline__ uint32_t med3_u32(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

__device__ __forceinline__ uint4 load16(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);  // global_load_dwordx4 (unaligned access is allowed for global memory)
  return v;
}

// The u8 and Hamming kernels stage a frame row as np = ceil(D / 16) 16-byte loads, so row
// r reads bytes [r D, r D + 16 np) of des_q, which ends at (r + 1 + rows_after) D when
// `rows_after` rows follow r.  True when the last of those loads would run past the
// buffer: the row then takes its last piece bytewise.  For D % 16 == 0 no row does; for
// D >= 15 only the buffer's last row; for a small D the last few rows (16 np - D <= 15, so
// never a row with 15 or more rows after it -- which also keeps the product small).
__host__ __device__ constexpr bool staged_row_overruns(int D, int rows_after) {
  return rows_after < 15 && rows_after * D < 16 * ((D + 15) >> 4) - D;
}
// (the definition, every D the kernels take: the loads' end 16 np against the buffer's end
// (rows_after + 1) D, both counted from the row's first byte)
constexpr bool staged_row_overruns_is_exact() {
  for (int D = 1; D <= 64; ++D)
    for (int n = 0; n < 64; ++n)
      if (staged_row_overruns(D, n) != (16 * ((D + 15) >> 4) > (n + 1) * D)) return false;
  return true;
}
static_assert(staged_row_overruns_is_exact(), "staged_row_overruns: a row overruns iff its loads end past the buffer");
static_assert(staged_row_overruns(1, 0) && staged_row_overruns(1, 14), "D = 1: the last fifteen rows");
static_assert(!staged_row_overruns(1, 15) && !staged_row_overruns(1, 16), "D = 1: row last - 15 ends at the buffer's end");
static_assert(staged_row_overruns(7, 0) && staged_row_overruns(7, 1) && !staged_row_overruns(7, 2), "D = 7: the last two rows");
static_assert(staged_row_overruns(8, 0) && !staged_row_overruns(8, 1), "D = 8: the last row");
static_assert(staged_row_overruns(33, 0) && !staged_row_overruns(33, 1), "D = 33: the last row");
static_assert(!staged_row_overruns(64, 0), "D % 16 == 0: the loads end with the row");

// One staged row's pieces: pf[k] = bytes [16 k, 16 k + 16) of the row for the np pieces that
// hold it (the further ones repeat the last: they are masked off whole when landing).  A
// row whose last piece would overrun des_q (`tail`) reads that piece's bytes inside the
// row one by one and never issues the 16-byte load.
template <int NP>
__device__ __forceinline__ void load_row_pieces(const uint8_t* __restrict__ row, int D, bool tail, uint4 (&pf)[NP]) {
  const int np = (D + 15) >> 4;  // pieces holding the row (uniform)
  if (!tail) {
#pragma unroll
    for (int k = 0; k < NP; ++k) pf[k] = load16(row + 16 * min(k, np - 1));
    return;
  }
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if (16 * (np - 1) + c < D) w[c >> 2] |= (uint32_t)row[16 * (np - 1) + c] << (8 * (c & 3));
#pragma unroll
  for (int k = 0; k < NP; ++k)  // (a register array is never indexed at run time)
    pf[k] = k < np - 1 ? load16(row + 16 * k) : make_uint4(w[0], w[1], w[2], w[3]);
}

// mask of the bytes of word `w` (0..3) of 16-byte piece `k` that lie inside the descriptor
__device__ __forceinline__ uint32_t byte_mask(int D, int k, int w) {
  const int n = D - 16 * k - 4 * w;  // bytes of this word inside the row
  return n >= 4 ? ~0u : (n <= 0 ? 0u : (1u << (8 * n)) - 1u);
}

// The knn entries' argument check, messages tagged `tag` (match / match_hamming /
// match_f32).  own_limit() is the matcher's own size limit, checked after D.
template <typename OwnLimit>
int check_knn_args(const char* tag, int d_max, const void* des_tpl, int n_tpl, int D, const void* des_q,
                   const void* q_off, int n_frames, int max_nq, const void* o1, const void* o2, OwnLimit own_limit) {
  const std::string t(tag);
  if (n_tpl < 0 || n_frames < 0 || max_nq < 0) return fail(KCMC_EINVAL, t + ": negative size");
  if (D < 1 || D > d_max)
    return fail(KCMC_EUNSUPPORTED, t + ": descriptor length D must be in [1, " + std::to_string(d_max) + "] (got " +
                                       std::to_string(D) + ")");
  KCMC_TRY(own_limit());
  if (n_frames > kMaxMatchFrames) return fail(KCMC_EUNSUPPORTED, t + ": at most 65535 frames per call");
  if (n_frames > 0 && n_tpl > 0 && (!des_tpl || !q_off || !o1 || !o2 || (max_nq > 0 && !des_q)))
    return fail(KCMC_EINVAL, t + ": NULL pointer");
  return KCMC_OK;
}

// The tail of the kcmc_match_frames* entries after check_knn_args: the filter's pointers
// and template cap, then launch_knn() (the matcher's knn on `s`) and the filter.
template <typename LaunchKnn>
int match_frames_tail(const char* entry, LaunchKnn launch_knn, const double* kp_tpl, const double* kp_q,
                      const int32_t* q_off, int n_frames, int n_tpl, int max_nq, double ratio, double d_lo,
                      double d_hi, const int32_t* out_idx, const float* out_dist, double* out_kp_ordered,
                      uint32_t* out_keep_bits, int32_t* out_counts, hipStream_t s) {
  if (n_frames > 0 && n_tpl > 0 && (!kp_tpl || !out_kp_ordered || !out_keep_bits || !out_counts || (max_nq > 0 && !kp_q)))
    return fail(KCMC_EINVAL, std::string(entry) + ": NULL pointer");
  if (n_tpl > kMaxFilterTpl)
    return fail(KCMC_EUNSUPPORTED, std::string(entry) + ": n_tpl > " + std::to_string(kMaxFilterTpl));
  if (n_frames == 0 || n_tpl == 0) return KCMC_OK;
  KCMC_TRY(launch_knn());
  return launch_match_filter(out_idx, out_dist, kp_tpl, kp_q, q_off, n_frames, n_tpl, ratio, d_lo, d_hi,
                             out_kp_ordered, out_keep_bits, out_counts, s);
}

}  // namespace kcmc

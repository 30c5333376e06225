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

// K1b: the per-frame match filters on knn output, shared by the three matchers.
//
// Reference: VA:196-214 (best-match reorder, ratio filter, median displacement filter) in
// float64 with the reference's exact operation order (no FMA contraction; file built with
// -ffp-contract=off).
//
// match_filter_regs_kernel<T> -- T threads per frame, template i = T k + tid in register
//   k (k < 8) of thread tid.  The median of the ratio survivors comes from a bitonic sort
//   of all 8 T register slots (slot e = 8 tid + k, non-survivors +inf), so the survivors
//   need no compaction: the sorted slots 0 .. nr - 1 are their sorted displacements.
//   Strides < 8 stay within a thread, < 512 are shuffles inside a wave, and only the
//   strides >= 512 go through LDS with barriers.
//     T = 64    n_tpl <= 512: one wave per frame, four frames per workgroup, no barrier
//               and no LDS
//     T = 512   n_tpl <= 4096: one workgroup per frame, 6 of the 78 stages through LDS
//     T = 1024  n_tpl <= 8192: one workgroup per frame, 10 of the 91 stages through LDS
#include "match_common.h"

namespace kcmc {
namespace {

constexpr int kFilterWaveFrames = 4;  // T = 64: frames (waves) per 256-thread workgroup

__device__ __forceinline__ void cmpx(double& a, double& b, bool asc) {
  const double lo = fmin(a, b), hi = fmax(a, b);
  a = asc ? lo : hi;
  b = asc ? hi : lo;
}

template <int T>
__global__ __launch_bounds__(T == 64 ? 64 * kFilterWaveFrames : T) void match_filter_regs_kernel(
    const int32_t* __restrict__ idx, const float* __restrict__ dist, const double* __restrict__ kp_tpl,
    const double* __restrict__ kp_q, const int32_t* __restrict__ q_off, int n_frames, int n_tpl, double ratio,
    double d_lo, double d_hi, double* __restrict__ kp_ordered, uint32_t* __restrict__ keep_bits,
    int32_t* __restrict__ counts) {
  // only the T > 64 code refers to these (T = 64 keeps 0 bytes of LDS)
  __shared__ double sx[T > 64 ? 8 * T : 1];
  __shared__ int s_cnt[T > 64 ? T / 64 : 1];
  __shared__ double s_med[2];
  const int tid = T == 64 ? threadIdx.x & 63 : threadIdx.x;  // thread of the frame
  const int lane = tid & 63, wave = tid >> 6;
  const int f = T == 64 ? blockIdx.x * kFilterWaveFrames + (threadIdx.x >> 6) : blockIdx.x;
  if constexpr (T == 64) {
    if (f >= n_frames) return;  // the whole wave
  }
  const int q_begin = q_off[f];
  const int words = (n_tpl + 31) >> 5;
  // pass 1: reorder (VA:197-200), ratio filter (VA:202-203), displacement of survivors (VA:208)
  double dv[8];
  uint64_t okm[8];
  int nr = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int i = T * k + tid;
    bool ok = false;
    double d = INFINITY;
    if (i < n_tpl) {
      const size_t o = ((size_t)f * n_tpl + i) * 2;
      const int j0 = idx[o];
      double qx = 0.0, qy = 0.0;
      if (j0 >= 0) {
        qx = kp_q[2 * (size_t)(q_begin + j0)];
        qy = kp_q[2 * (size_t)(q_begin + j0) + 1];
      }
      kp_ordered[((size_t)f * n_tpl + i) * 2] = qx;
      kp_ordered[((size_t)f * n_tpl + i) * 2 + 1] = qy;
      ok = (double)dist[o] < ratio * (double)dist[o + 1];
      if (ok) {
        const double dx = kp_tpl[2 * i] - qx, dy = kp_tpl[2 * i + 1] - qy;
        d = sqrt(dx * dx + dy * dy);
      }
    }
    dv[k] = d;
    okm[k] = __ballot(ok);
    nr += __popcll(okm[k]);
  }
  if constexpr (T > 64) {
    if (lane == 0) s_cnt[wave] = nr;
    __syncthreads();
    nr = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) nr += s_cnt[w];
  }
  // bitonic sort (ascending) of the 8 T slots e = 8 tid + k
  double v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = dv[k];
#pragma unroll
  for (int size = 2; size <= 8 * T; size <<= 1) {
    const bool asc_t = (tid & (size >> 3)) == 0;  // (e & size) == 0 for size >= 8
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if constexpr (T > 64) {
        if (stride >= 512) {  // partner in another wave: through LDS
          const int ts = stride >> 3;
          const bool lower = (tid & ts) == 0;
#pragma unroll
          for (int k = 0; k < 8; ++k) sx[8 * tid + k] = v[k];
          __syncthreads();
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const double o = sx[8 * (tid ^ ts) + k];
            v[k] = (lower == asc_t) ? fmin(v[k], o) : fmax(v[k], o);
          }
          __syncthreads();
          continue;
        }
      }
      if (stride >= 8) {
        const int ls = stride >> 3;
        const bool lower = (tid & ls) == 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const double o = __shfl_xor(v[k], ls, 64);
          v[k] = (lower == asc_t) ? fmin(v[k], o) : fmax(v[k], o);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if ((k & stride) == 0) {
            const bool asc = size >= 8 ? asc_t : (k & size) == 0;
            cmpx(v[k], v[k | stride], asc);
          }
        }
      }
    }
  }
  // the median of the nr survivors: sorted slots (nr - 1) / 2 and nr / 2 (np.median, VA:210)
  double med = 0.0;
  if constexpr (T > 64) {
    if (nr > 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = 8 * tid + k;
        if (e == (nr >> 1)) s_med[1] = v[k];
        if ((nr & 1) == 0 && e == (nr >> 1) - 1) s_med[0] = v[k];
      }
    }
    __syncthreads();
    if (nr > 0) med = (nr & 1) ? s_med[1] : (s_med[0] + s_med[1]) / 2.0;
  } else if (nr > 0) {
    auto slot = [&](int e) -> double {
      double x = v[0];
#pragma unroll
      for (int k = 1; k < 8; ++k)
        if ((e & 7) == k) x = v[k];  // wave-uniform
      return __shfl(x, e >> 3, 64);
    };
    const double b = slot(nr >> 1);
    med = (nr & 1) ? b : (slot((nr >> 1) - 1) + b) / 2.0;
  }
  const double lo = d_lo * med, hi = d_hi * med;
  // pass 2: keep = ratio survivor and lo <= d <= hi (VA:210); bitmask + counts
  int nk = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const bool keep = nr > 0 && ((okm[k] >> lane) & 1ull) && lo <= dv[k] && dv[k] <= hi;
    const uint64_t m = __ballot(keep);
    nk += __popcll(m);
    const int w0 = (T * k + 64 * wave) >> 5;
    if (lane == 0) {
      if (w0 < words) keep_bits[(size_t)f * words + w0] = (uint32_t)m;
      if (w0 + 1 < words) keep_bits[(size_t)f * words + w0 + 1] = (uint32_t)(m >> 32);
    }
  }
  if constexpr (T > 64) {
    __syncthreads();  // s_cnt is reused
    if (lane == 0) s_cnt[wave] = nk;
    __syncthreads();
    nk = 0;
    if (tid == 0)
      for (int w = 0; w < T / 64; ++w) nk += s_cnt[w];
  }
  if (tid == 0) {
    counts[4 * (size_t)f + 0] = n_tpl;  // len(kp_query) after the reorder at VA:200
    counts[4 * (size_t)f + 1] = n_tpl;  // len(matches)
    counts[4 * (size_t)f + 2] = nr;
    counts[4 * (size_t)f + 3] = nk;
  }
}

static_assert(8 * 1024 >= kMaxFilterTpl, "the widest instantiation sorts every template slot");

template <int T>
int launch_filter(const int32_t* idx, const float* dist, const double* kp_tpl, const double* kp_q,
                  const int32_t* q_off, int n_frames, int n_tpl, double ratio, double d_lo, double d_hi,
                  double* kp_ordered, uint32_t* keep_bits, int32_t* counts, hipStream_t s) {
  const int per_wg = T == 64 ? kFilterWaveFrames : 1;  // frames per workgroup
  hipLaunchKernelGGL(match_filter_regs_kernel<T>, dim3(ceil_div(n_frames, per_wg)), dim3(T * per_wg), 0, s, idx, dist,
                     kp_tpl, kp_q, q_off, n_frames, n_tpl, ratio, d_lo, d_hi, kp_ordered, keep_bits, counts);
  return launch_check("match_filter_regs_kernel");
}

}  // namespace

int launch_match_filter(const int32_t* idx, const float* dist, const double* kp_tpl, const double* kp_q,
                        const int32_t* q_off, int n_frames, int n_tpl, double ratio, double d_lo, double d_hi,
                        double* kp_ordered, uint32_t* keep_bits, int32_t* counts, hipStream_t s) {
  auto* launch = n_tpl <= 8 * 64 ? launch_filter<64> : n_tpl <= 8 * 512 ? launch_filter<512> : launch_filter<1024>;
  return launch(idx, dist, kp_tpl, kp_q, q_off, n_frames, n_tpl, ratio, d_lo, d_hi, kp_ordered, keep_bits, counts, s);
}

}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_match_filter(kcmc_ctx* ctx, const int32_t* idx, const float* dist, const double* kp_tpl,
                                 const double* kp_q, const int32_t* q_off, int n_frames, int n_tpl, double ratio,
                                 double d_lo, double d_hi, double* out_kp_ordered, uint32_t* out_keep_bits,
                                 int32_t* out_counts, kcmc_stream_t stream) {
  if (!ctx) return fail(KCMC_EINVAL, "kcmc_match_filter: ctx is NULL");
  if (n_tpl < 0 || n_frames < 0) return fail(KCMC_EINVAL, "kcmc_match_filter: negative size");
  if (n_frames > kMaxMatchFrames) return fail(KCMC_EUNSUPPORTED, "kcmc_match_filter: at most 65535 frames per call");
  if (n_tpl > kMaxFilterTpl)
    return fail(KCMC_EUNSUPPORTED, "kcmc_match_filter: n_tpl > " + std::to_string(kMaxFilterTpl));
  if (n_frames == 0 || n_tpl == 0) return KCMC_OK;
  if (!idx || !dist || !kp_tpl || !kp_q || !q_off || !out_kp_ordered || !out_keep_bits || !out_counts)
    return fail(KCMC_EINVAL, "kcmc_match_filter: NULL pointer");
  return launch_match_filter(idx, dist, kp_tpl, kp_q, q_off, n_frames, n_tpl, ratio, d_lo, d_hi, out_kp_ordered,
                             out_keep_bits, out_counts, (hipStream_t)stream);
}

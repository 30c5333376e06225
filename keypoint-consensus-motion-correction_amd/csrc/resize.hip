// f1 (scale pyramid): the exact bilinear resize that builds level l of the detector's
// pyramid from level l - 1 (build-defined, integer, bit-identical to the
// numpy restatement in tests/test_orb_pyramid_host.py).  Per axis, source length n,
// destination length m, destination index x:
//
//   num = (2x + 1) n - m,  den = 2m,  i = floor(num / den),
//   a   = ((num - i den) 2048 + m) / den              (the 11-bit weight of tap i + 1)
//   i < 0       ->  i = 0,     a = 0
//   i >= n - 1  ->  i = n - 1, a = 0                  (the second tap clamped to n - 1)
//
//   dst(x, y) = (sum of the 4 taps x (2048 - a | a)(2048 - b | b) + 2^21) >> 22
//
// so m == n is the identity and an exact 2:1 is (sum of the 2x2 + 2) >> 2.  num reaches
// 2^33 at 65535 px: the tables are computed in 64-bit integers.
//
// One workgroup per 256 destination columns x kBandH destination rows, no LDS for the
// image: a thread owns one column (its column tap and weight are computed once) and walks
// down the band keeping the horizontally blended values h(r) = (2048 - a) s(r, i) +
// a s(r, i + 1) of the last two source rows in registers.  Consecutive destination rows
// share source rows (the second tap row of one is the first of the next, or both when
// upscaling), so inside a band every source row is loaded once; byte loads and stores of
// adjacent lanes fall into the same cache lines, and no alignment is assumed.
// 1.5 TB/s at 1080p -> 900 x 1600 against a copy's 4.5 (profiles/orb_pyramid.md).  Three
// other forms ran no faster there: all loads of 8 rows issued first (0.75 x), the band's
// source box staged in LDS with 4-byte loads (1.1 x alone, 0.93 x inside the pyramid), and
// this walk with the row values in vector registers (the same).  What they share is one
// pixel and one byte store per lane; four pixels per lane with word stores is the next
// thing to try, and needs a per-row column phase because level widths are odd.
#include "kcmc_internal.h"

namespace kcmc {
namespace {

constexpr int kCols = 256;   // threads = destination columns per workgroup
constexpr int kBandH = 32;   // destination rows per workgroup

// The tap index and weight of destination index x (see above); n, m in [1, 65535].
__device__ __forceinline__ void axis_tap(int x, int n, int m, int& i, int& a) {
  const long long num = (long long)(2 * x + 1) * n - m;
  if (num < 0) {
    i = 0;
    a = 0;
    return;
  }
  const unsigned long long den = 2ull * (unsigned)m;
  const unsigned long long q = (unsigned long long)num / den;
  if (q >= (unsigned long long)(n - 1)) {
    i = n - 1;
    a = 0;
    return;
  }
  const uint32_t rem = (uint32_t)((unsigned long long)num - q * den);  // < 2m <= 131070
  i = (int)q;
  a = (int)((rem * 2048u + (uint32_t)m) / (uint32_t)den);              // < 2^28 + 2^16
}

__global__ __launch_bounds__(kCols) void resize_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          int H, int W, int DH, int DW) {
  __shared__ int s_row[kBandH], s_wgt[kBandH];
  const int x = blockIdx.x * kCols + threadIdx.x;
  const int y0 = blockIdx.y * kBandH;
  const int rows = min(kBandH, DH - y0);
  if ((int)threadIdx.x < rows) axis_tap(y0 + (int)threadIdx.x, H, DH, s_row[threadIdx.x], s_wgt[threadIdx.x]);
  __syncthreads();
  if (x >= DW) return;  // no barriers below
  int i, a;
  axis_tap(x, W, DW, i, a);
  const int i1 = min(i + 1, W - 1);
  const uint32_t wa1 = (uint32_t)a, wa0 = 2048u - wa1;
  const uint8_t* S = src + (size_t)blockIdx.z * H * W;
  uint8_t* D = dst + (size_t)blockIdx.z * DH * DW + (size_t)y0 * DW;
  // the two most recent source rows, blended horizontally (<= 255 * 2048)
  int rA = -1, rB = -1;
  uint32_t hA = 0, hB = 0;
  for (int r = 0; r < rows; ++r) {
    // the row's tap and weight are the same in every lane: scalar registers, so that the row
    // addresses are scalar arithmetic and a lane adds only its column
    const int j0 = __builtin_amdgcn_readfirstlane(s_row[r]), j1 = min(j0 + 1, H - 1);
    const uint32_t wb1 = (uint32_t)__builtin_amdgcn_readfirstlane(s_wgt[r]), wb0 = 2048u - wb1;
    uint32_t h0, h1;
    if (j0 == rA) {
      h0 = hA;
    } else if (j0 == rB) {
      h0 = hB;
    } else {
      const uint8_t* p = S + (size_t)j0 * W;
      h0 = wa0 * p[i] + wa1 * p[i1];
    }
    if (j1 == j0) {
      h1 = h0;
    } else if (j1 == rB) {
      h1 = hB;
    } else if (j1 == rA) {
      h1 = hA;
    } else {
      const uint8_t* p = S + (size_t)j1 * W;
      h1 = wa0 * p[i] + wa1 * p[i1];
    }
    rA = j0, hA = h0, rB = j1, hB = h1;
    // <= 255 * 2048 * 2048 + 2^21 < 2^31
    (D + (size_t)r * DW)[x] = (uint8_t)((wb0 * h0 + wb1 * h1 + (1u << 21)) >> 22);
  }
}

}  // namespace

int launch_resize_u8(const uint8_t* src, int n_frames, int H, int W, uint8_t* dst, int dst_h, int dst_w,
                     hipStream_t s) {
  hipLaunchKernelGGL(resize_u8_kernel, dim3(ceil_div(dst_w, kCols), ceil_div(dst_h, kBandH), n_frames), dim3(kCols), 0,
                     s, src, dst, H, W, dst_h, dst_w);
  return launch_check("resize_u8_kernel");
}

}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_resize_u8(kcmc_ctx* ctx, const uint8_t* src, int n_frames, int H, int W, uint8_t* dst, int dst_h,
                              int dst_w, kcmc_stream_t stream) {
  if (!ctx) return fail(KCMC_EINVAL, "kcmc_resize_u8: ctx is NULL");
  if (n_frames < 0) return fail(KCMC_EINVAL, "kcmc_resize_u8: negative frame count");
  if (H < 1 || W < 1 || dst_h < 1 || dst_w < 1 || H > 65535 || W > 65535 || dst_h > 65535 || dst_w > 65535)
    return fail(KCMC_EINVAL, "kcmc_resize_u8: sizes must be in [1, 65535]");
  if (n_frames == 0) return KCMC_OK;
  if (!src || !dst) return fail(KCMC_EINVAL, "kcmc_resize_u8: NULL pointer");
  if (n_frames > 65535) return fail(KCMC_EUNSUPPORTED, "kcmc_resize_u8: at most 65535 frames per call");
  return launch_resize_u8(src, n_frames, H, W, dst, dst_h, dst_w, (hipStream_t)stream);
}

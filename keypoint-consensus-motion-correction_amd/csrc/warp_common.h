// Pure per-pixel helpers of the warps (warp.hip: warpAffine / warpPerspective; warp_field.hip:
// the piecewise-rigid field warp): OpenCV's rounding and saturation, its in-place inversion of
// the forward map, the remapBilinear blend and the range-checked direct gather.  Both files are
// compiled with -ffp-contract=off, so the arithmetic is reproduced operation by operation.
#pragma once

#include "kcmc_internal.h"

namespace kcmc {

static __device__ __forceinline__ int cv_round(double v) { return (int)__builtin_rint(v); }

static __device__ __forceinline__ uint16_t sat_u16(float v) {
  const int iv = (int)__builtin_rintf(v);
  return (uint16_t)((unsigned)iv <= 65535u ? iv : (iv > 0 ? 65535 : 0));
}

static __device__ __forceinline__ int sat_s16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// OpenCV warpAffine's in-place inversion of the forward map.
static __device__ __forceinline__ void invert_affine(const double* Min, double* M) {
  for (int k = 0; k < 6; ++k) M[k] = Min[k];
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0 ? 1. / D : 0;
  const double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11;
  M[1] *= -D;
  M[3] *= -D;
  M[4] = A22;
  const double b1 = -M[0] * M[2] - M[1] * M[5];
  const double b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1;
  M[5] = b2;
}

// Frames whose map holds a NaN (no RANSAC model) are warped to zeros, as OpenCV's
// BORDER_CONSTANT gives for coordinates that land outside the image; the pipeline warps
// them again with the gap-filled maps (VA:347-407) before handing the frames out.
static __device__ __forceinline__ bool map_has_nan(const double* M, int n) {
  bool nan = false;
  for (int k = 0; k < n; ++k) nan = nan || M[k] != M[k];
  return nan;
}

static __device__ __forceinline__ void load_map(const double* __restrict__ Mall, int f, int inverse_map, double* M) {
  if (inverse_map) {
    for (int k = 0; k < 6; ++k) M[k] = Mall[6 * (size_t)f + k];
  } else {
    invert_affine(Mall + 6 * (size_t)f, M);
  }
}

// remapBilinear<Cast<float, ushort>>'s blend in exact integer/float steps that are cheap
// on the VALU: w_k = K_k / 1024 with K_k = (32-fy|fy) * (32-fx|fx) an integer, and
// fl(v * K/1024) = fl(v*K) * 2^-10 (power-of-two scaling commutes with rounding), where
// fl(v*K) = cvt_f32_u32(v*K) because the integer product is exact and the conversion
// rounds to nearest-even like the multiply.  The left-to-right sum scales the same way.
static __device__ __forceinline__ uint16_t blend_int(uint32_t v00, uint32_t v01, uint32_t v10, uint32_t v11, int fx,
                                                     int fy) {
  const uint32_t ax = 32 - fx, ay = 32 - fy;
  const float q0 = (float)__umul24(v00, __umul24(ay, ax));
  const float q1 = (float)__umul24(v01, __umul24(ay, (uint32_t)fx));
  const float q2 = (float)__umul24(v10, __umul24((uint32_t)fy, ax));
  const float q3 = (float)__umul24(v11, __umul24((uint32_t)fy, (uint32_t)fx));
  return sat_u16((((q0 + q1) + q2) + q3) * 0.0009765625f);
}

// Direct-gather path (tiles whose source box does not fit the LDS budget): taps are
// loaded from clamped in-image addresses and zeroed when outside (branch-free, so the
// loads of a row's pixels are all in flight together).
template <int C>
static __device__ __forceinline__ void bilinear_px(const uint16_t* __restrict__ S, int H, int W, int X, int Y,
                                                   uint16_t* out) {
  const int sx = sat_s16(X >> 5), sy = sat_s16(Y >> 5);
  const int fx = X & 31, fy = Y & 31;
  const bool x0 = (unsigned)sx < (unsigned)W, x1 = (unsigned)(sx + 1) < (unsigned)W;
  const bool y0 = (unsigned)sy < (unsigned)H, y1 = (unsigned)(sy + 1) < (unsigned)H;
  const int cx0 = min(max(sx, 0), W - 1), cx1 = min(max(sx + 1, 0), W - 1);
  const int cy0 = min(max(sy, 0), H - 1), cy1 = min(max(sy + 1, 0), H - 1);
  const size_t r0 = (size_t)cy0 * W, r1 = (size_t)cy1 * W;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const uint32_t t00 = S[(r0 + cx0) * C + k], t01 = S[(r0 + cx1) * C + k];
    const uint32_t t10 = S[(r1 + cx0) * C + k], t11 = S[(r1 + cx1) * C + k];
    out[k] = blend_int((x0 && y0) ? t00 : 0u, (x1 && y0) ? t01 : 0u, (x0 && y1) ? t10 : 0u, (x1 && y1) ? t11 : 0u,
                       fx, fy);
  }
}

}  // namespace kcmc

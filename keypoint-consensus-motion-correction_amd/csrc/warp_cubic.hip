// K3c: bicubic warpAffine of uint16 grayscale frames -- kcmc_warp_affine_u16's coordinates with
// OpenCV's classic INTER_CUBIC resampling (remapBicubic<Cast<float, ushort>, float, 1>,
// BORDER_CONSTANT 0) in place of the 2 x 2 blend.
//
// Build-defined semantics (the reference never resamples cubically; include/kcmc.h and
// DESIGN.md hold the definition, tests/test_warp_cubic_host.py the numpy restatement).  For
// output pixel (x, y): X, Y in 1/1024 px exactly as warp.hip, sx = sat_short(X >> 10),
// fx = (X >> 5) & 31, likewise sy, fy.  The 1-D weights c_0..c_3 of a fraction f are the
// cubic-convolution kernel with A = -3/4 at t = f / 32; every one is an integer multiple of
// 2^-17, so the 32 x 4 integer table kCubicNum below defines them exactly.  The 2-D weight is
// w_ij = fl32(c_i(fy) c_j(fx)) (one rounding: OpenCV's BicubicTab_f entry), the taps are
// S[sy - 1 + i][sx - 1 + j] as float32 (0 outside the image), every product fl32(S w) and every
// sum a separate float32 operation (this file is compiled with -ffp-contract=off):
//   interior pixel (the 4 x 4 footprint inside the image): r_i = ((p_i0 + p_i1) + p_i2) + p_i3,
//                                                          sum = ((r_0 + r_1) + r_2) + r_3
//   any other pixel: sum = 0, then sum += p_ij for i = 0..3 and within that j = 0..3
// and the output is saturate_cast<ushort>(sum) (sat_u16).
//
// Layout, plan modes and staging: the shared tile skeleton (warp_tile.h).  The source box is
// the affine box widened to the footprint, one more column and row on the low side and two on
// the high side.  A staged tile whose box lies inside the image holds interior pixels only and
// makes the interior sum alone; a tile that touches the border makes both sums from the same
// sixteen products and selects per pixel, as the gather path does, so the paths give the same bits.
//
// LDS: a lane reads its taps with 16-bit reads.  One read instruction takes the same tap (i, j)
// of 64 neighbouring pixel pairs, so the lanes of a 32-lane group read consecutive dwords of a
// box row whatever the pitch; where a rotated row steps to the next box row the two runs can
// meet on a bank, two-way at the most.  So the pitch stays the box width rounded to 8 pixels, as
// in the other warps, and the 20 KB box keeps seven workgroups on a CU.  The 1-D weights sit in
// 512 bytes of LDS behind the box.  A lane's two pixels share twelve of their sixteen taps under
// near-identity maps (cubic_rows), and their arithmetic runs on packed fp32, one element each.
// Bound by VALU issue at about three times the bilinear warp's time (DESIGN K3c).
#include "warp_tile.h"

namespace kcmc {
namespace {

// c_j(f) 2^17 for f = 0..31: ((A(t+1) - 5A)(t+1) + 8A)(t+1) - 4A, ((A+2)t - (A+3))t^2 + 1,
// the same at 1 - t, and 1 - the three, with A = -3/4 and t = f / 32 (exact: t has 5 bits).
__constant__ int kCubicNum[32][4] = {
    {0, 131072, 0, 0},           {-2883, 130789, 3259, -93},   {-5400, 129960, 6872, -360},
    {-7569, 128615, 10809, -783}, {-9408, 126784, 15040, -1344}, {-10935, 124497, 19535, -2025},
    {-12168, 121784, 24264, -2808}, {-13125, 118675, 29197, -3675}, {-13824, 115200, 34304, -4608},
    {-14283, 111389, 39555, -5589}, {-14520, 107272, 44920, -6600}, {-14553, 102879, 50369, -7623},
    {-14400, 98240, 55872, -8640}, {-14079, 93385, 61399, -9633}, {-13608, 88344, 66920, -10584},
    {-13005, 83147, 72405, -11475}, {-12288, 77824, 77824, -12288}, {-11475, 72405, 83147, -13005},
    {-10584, 66920, 88344, -13608}, {-9633, 61399, 93385, -14079}, {-8640, 55872, 98240, -14400},
    {-7623, 50369, 102879, -14553}, {-6600, 44920, 107272, -14520}, {-5589, 39555, 111389, -14283},
    {-4608, 34304, 115200, -13824}, {-3675, 29197, 118675, -13125}, {-2808, 24264, 121784, -12168},
    {-2025, 19535, 124497, -10935}, {-1344, 15040, 126784, -9408}, {-783, 10809, 128615, -7569},
    {-360, 6872, 129960, -5400},  {-93, 3259, 130789, -2883}};

// ------------------------------------------------------------------------------- plan
// Thread t < tiles: the tile's plan.  The box: the affine box widened to the 4 x 4 footprint,
// taps sx - 1 .. sx + 2.
template <int TILE_H>
__global__ __launch_bounds__(256) void cubic_plan_kernel(const double* __restrict__ Mall, int n_frames, int H, int W,
                                                         int inverse_map, int ntx, int nty,
                                                         TilePlan* __restrict__ plan, double* __restrict__ minv) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)ntx * nty * n_frames) return;
  const PlanTile p = plan_tile<TILE_H>(t, Mall, inverse_map, H, W, ntx, nty, minv);
  const Box1024 b = affine_box(p.M, p.xb, p.yb, p.xl, p.yl);
  plan[t] = classify_box((b.x0 >> 10) - 1, (b.x1 >> 10) + 2, (b.y0 >> 10) - 1, (b.y1 >> 10) + 2, H, W, true,
                         map_has_nan(p.M, 6));
}

// ------------------------------------------------------------------------------- pixel
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The sixteen products and the sum of a lane's two pixels, on packed fp32 (one element per
// pixel; every element operation is the scalar one, separately rounded).  v[i][j]: the taps as
// float32; cy, cx: the 1-D weights of fy, fx.  BORDER: a pixel may lie outside the interior --
// both sum orders are made from the same products and `interior` selects per pixel.
template <bool BORDER>
__device__ __forceinline__ void cubic_sum2(const f32x2 (&v)[4][4], const f32x2 (&cy)[4], const f32x2 (&cx)[4],
                                           const bool (&interior)[2], uint16_t (&o)[2]) {
  f32x2 p[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) p[i][j] = v[i][j] * (cy[i] * cx[j]);
  f32x2 r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = ((p[i][0] + p[i][1]) + p[i][2]) + p[i][3];
  f32x2 sum = ((r[0] + r[1]) + r[2]) + r[3];
  if (BORDER) {
    f32x2 seq = {0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) seq = seq + p[i][j];
    sum[0] = interior[0] ? sum[0] : seq[0];
    sum[1] = interior[1] ? sum[1] : seq[1];
  }
  o[0] = sat_u16(sum[0]);
  o[1] = sat_u16(sum[1]);
}

// ------------------------------------------------------------------------------- tiles
// Output rows of one tile on one path (0: staged box inside the image, 1: zeros, 2: direct
// gather, 3: staged box that touches the border).  Wave w makes rows w, w + 4, ...; lane l the
// pixels x = xb + 2l, xb + 2l + 1.
template <int TILE_H, int MODE>
__device__ __forceinline__ void cubic_rows(const uint16_t* stile, const float (*wtab)[4], int pitch, int ax0, int sy0,
                                           const uint16_t* __restrict__ S, uint16_t* __restrict__ Dst, int H, int W,
                                           int xb, int yb, int wave, int lane, const int (&ad)[2], const int (&bd)[2],
                                           int X0v, int Y0v, bool pair_ok) {
  const int x = xb + 2 * lane;
  const bool pair_store = pair_ok && x + 2 <= W;
#pragma unroll 2
  for (int i = 0; i < TILE_H / 4; ++i) {
    const int y = yb + wave + 4 * i;  // wave-uniform
    if (y >= H) break;
    const int X0 = __builtin_amdgcn_readlane(X0v, i), Y0 = __builtin_amdgcn_readlane(Y0v, i);
    uint16_t o[2] = {0, 0};
    if (MODE != 1) {
      f32x2 v[4][4], cy[4], cx[4];
      bool interior[2];
      int bx0 = 0, by0 = 0;  // staged paths: pixel 0's box-relative tap origin
      float u4[4];           // and the column behind its footprint
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int tX = (int)((uint32_t)X0 + (uint32_t)ad[p]), tY = (int)((uint32_t)Y0 + (uint32_t)bd[p]);
        const int fx = (tX >> 5) & 31, fy = (tY >> 5) & 31;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          cy[k][p] = wtab[fy][k];
          cx[k][p] = wtab[fx][k];
        }
        int sx, sy;
        if (MODE == 2) {
          // direct gather (bilinear_px's scheme): taps from clamped in-image addresses, zeroed
          // when outside
          sx = sat_s16(tX >> 10);
          sy = sat_s16(tY >> 10);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ty = sy - 1 + r;
            const bool yok = (unsigned)ty < (unsigned)H;
            const size_t ro = (size_t)min(max(ty, 0), H - 1) * W;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int tx = sx - 1 + c;
              const uint32_t t = S[ro + min(max(tx, 0), W - 1)];
              v[r][c][p] = (float)((yok && (unsigned)tx < (unsigned)W) ? t : 0u);
            }
          }
        } else {
          // box-relative taps: the plan bounded the footprint inside the staged box (the box
          // origin is folded into X0, Y0, a multiple of 1024)
          const int bx = tX >> 10, by = tY >> 10;  // >= 1: the footprint starts one column / row before
          const uint16_t* t = stile + (int)__umul24((uint32_t)(by - 1), (uint32_t)pitch) + (bx - 1);
          if (p == 0) {
            // pixel 0 reads five columns: under the near-identity maps of motion correction
            // pixel 1's footprint is pixel 0's moved by one column, and the fifth column (inside
            // the box then; never used otherwise, stile's tail keeps the read inside the array)
            // spares it twelve of its sixteen reads
            bx0 = bx;
            by0 = by;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
              for (int c = 0; c < 4; ++c) v[r][c][0] = (float)(uint32_t)t[r * pitch + c];
              u4[r] = (float)(uint32_t)t[r * pitch + 4];
            }
          } else if (bx == bx0 + 1 && by == by0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
              for (int c = 0; c < 3; ++c) v[r][c][1] = v[r][c + 1][0];
              v[r][3][1] = u4[r];
            }
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int c = 0; c < 4; ++c) v[r][c][1] = (float)(uint32_t)t[r * pitch + c];
          }
          sx = bx + ax0;
          sy = by + sy0;
        }
        interior[p] = sx >= 1 && sx + 2 <= W - 1 && sy >= 1 && sy + 2 <= H - 1;
      }
      cubic_sum2<MODE != 0>(v, cy, cx, interior, o);
    }
    uint16_t* drow = Dst + (size_t)y * W + x;
    if (pair_store) {
      // streaming store: the aligned frame is written once and not re-read by this kernel
      __builtin_nontemporal_store((uint32_t)o[0] | ((uint32_t)o[1] << 16), reinterpret_cast<uint32_t*>(drow));
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (x + q < W) drow[q] = o[q];
    }
  }
}

// no-unaligned-access-mode: keeps adjacent 16-bit tap reads from being fused into one 4-byte
// LDS read at a 2-byte-aligned address (warp.hip).
template <int TILE_H>
__global__ __launch_bounds__(kThreads) __attribute__((target("no-unaligned-access-mode"))) void warp_cubic_u16_kernel(
    const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, const TilePlan* __restrict__ plan,
    const double* __restrict__ minv, int H, int W, int vec_ok, int pair_ok) {
  __shared__ __attribute__((aligned(16))) uint16_t stile[kLdsElems + 8];  // + the fifth column's overhang
  __shared__ float wtab[32][4];  // the 1-D weights
  const TileId t = tile_decode<TILE_H>();
  const int tid = threadIdx.x, xb = t.xb, yb = t.yb, wave = t.wave, lane = t.lane;
  const uint16_t* S = src + (size_t)t.f * H * W;
  uint16_t* Dst = dst + (size_t)t.f * H * W;
  const TilePlan tp = plan[t.tile];
  const int mode = tp.mode, ax0 = tp.ax0, sy0 = tp.sy0, pitch = tp.pitch();
  const bool vec_stage = mode == 0 && vec_ok;

  uint4 chunk[kRowPasses];
  stage_load(S, tp, H, W, vec_stage, chunk);
  if (tid < 128) wtab[tid >> 2][tid & 3] = (float)kCubicNum[tid >> 2][tid & 3] * 0x1p-17f;  // exact
  const double* M = minv + 6 * (size_t)t.f;
  int ad[2], bd[2], X0v, Y0v;
  lane_columns(M, xb, lane, W, ad, bd);
  row_origins<TILE_H>(M, t, tp, X0v, Y0v);
  stage_commit(stile, S, tp, H, W, vec_stage, chunk);
  __syncthreads();
  // one row loop per path (a path-uniform branch inside the loop drains the stores every row)
  if (mode == 0 && tp.inside())
    cubic_rows<TILE_H, 0>(stile, wtab, pitch, ax0, sy0, S, Dst, H, W, xb, yb, wave, lane, ad, bd, X0v, Y0v, pair_ok);
  else if (mode == 0)
    cubic_rows<TILE_H, 3>(stile, wtab, pitch, ax0, sy0, S, Dst, H, W, xb, yb, wave, lane, ad, bd, X0v, Y0v, pair_ok);
  else if (mode == 1)
    cubic_rows<TILE_H, 1>(stile, wtab, pitch, ax0, sy0, S, Dst, H, W, xb, yb, wave, lane, ad, bd, X0v, Y0v, pair_ok);
  else
    cubic_rows<TILE_H, 2>(stile, wtab, pitch, ax0, sy0, S, Dst, H, W, xb, yb, wave, lane, ad, bd, X0v, Y0v, pair_ok);
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_warp_affine_cubic_u16(kcmc_ctx* ctx, const uint16_t* src, uint16_t* dst, const double* M,
                                          int n_frames, int H, int W, int C, int inverse_map, kcmc_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  return run_tile_warp(
      "kcmc_warp_affine_cubic_u16", "warp_cubic_u16_kernel", ctx, src, dst, M != nullptr, n_frames, H, W, 0, s,
      [&] {
        if (C == 3 || C == 4)
          return fail(KCMC_EUNSUPPORTED, "kcmc_warp_affine_cubic_u16: grayscale only in this version (C must be 1)");
        return C != 1 ? fail(KCMC_EINVAL, "kcmc_warp_affine_cubic_u16: C must be 1") : (int)KCMC_OK;
      },
      [&](auto th, const TileLaunch& l) {
        constexpr int TILE_H = decltype(th)::value;
        hipLaunchKernelGGL((cubic_plan_kernel<TILE_H>), dim3((unsigned)((l.tiles + 255) / 256)), dim3(256), 0, s, M,
                           n_frames, H, W, inverse_map, l.ntx, l.nty, l.plan, l.minv);
        hipLaunchKernelGGL((warp_cubic_u16_kernel<TILE_H>), dim3(l.ntx, l.nty, n_frames), dim3(kThreads), 0, s, src,
                           dst, l.plan, l.minv, H, W, l.vec_ok, l.pair_ok);
      });
}

// K3f: piecewise-rigid field warp of uint16 grayscale frames -- kcmc_warp_affine_u16 with a
// smooth per-pixel residual displacement added to the fixed-point source coordinate.
//
// Build-defined semantics (the reference has no such mode; include/kcmc.h and DESIGN.md hold
// the definition, tests/test_piecewise_host.py the numpy restatement).  Per frame: the 2x3 map
// and q [gy, gx, 2] int32, the residual source displacement (x, y) at the grid's nodes in
// 1/1024 px.  For output pixel (x, y)
//   X_aff = adelta[x] + X0(y), Y_aff likewise       (WarpAffineInvoker, as warp.hip)
//   (j0, wx) = axis_weight(x, W, gx), (i0, wy) = axis_weight(y, H, gy)
//   v_j  = (q[i0][j] (1024 - wy) + q[i0+1][j] wy + 512) >> 10       vertical step, per row
//   val  = (v_j0 (1024 - wx) + v_{j0+1} wx + 512) >> 10             horizontal step, per pixel
//   X = X_aff + val_x, Y = Y_aff + val_y
// and from there warpAffine again: sx = sat_short(X >> 10), fx = (X >> 5) & 31, the float
// blend of remapBilinear, taps outside the image read 0.  Integer arithmetic throughout
// (arithmetic right shifts), int32 under the contract |q| <= 2^20.
//
// Layout, plan modes and staging: the shared tile skeleton (warp_tile.h).  Each rounded
// interpolation step lies between the values it mixes, so the source box is the affine box moved
// by the minimum and maximum of the node values whose cells touch the tile; every tile that
// touches a node outside the contract gathers.  The vertical step is made once per tile into LDS
// (tile rows x gx nodes); a pixel reads its two neighbours there and pays two multiplies per
// component.  The per-column / per-row (node, weight) pairs depend only on (W, gx) / (H, gy) and
// come from two tables the plan kernel writes.
//
// Blend: OpenCV's float blend (blend_int: the float evaluation with exact integer products)
// for every pixel; the affine warp's dark-box integer shortcut is not used here.
#include "warp_tile.h"

namespace kcmc {
namespace {

constexpr int kMaxGrid = 16;    // nodes per axis
constexpr int kMaxQ = 1 << 20;  // contract on |q|

// (k0, w) of pixel index p along an axis of length L with g nodes: the two neighbour nodes
// k0, k0 + 1 and the weight w / 1024 of the second; held constant outside the outermost node
// centres.  g == 1: (0, 0).  Packed k0 | w << 16.
__host__ __device__ inline int axis_weight(int p, int L, int g) {
  if (g == 1) return 0;
  int num = (2 * p + 1) * g - L;
  num = num < 0 ? 0 : (num > 2 * L * (g - 1) ? 2 * L * (g - 1) : num);
  int k0 = num / (2 * L);
  k0 = k0 > g - 2 ? g - 2 : k0;
  const int w = ((num - k0 * 2 * L) * 1024 + L) / (2 * L);
  return k0 | (w << 16);
}

// (a (1024 - w) + b w + 512) >> 10.  Under the contract |a|, |b| <= 2^20 and 0 <= w <= 1024 fit
// the full-rate 24-bit multiply and the sum fits int32; outside it (tiles the plan sends to the
// range-checked gather) the value is unspecified: low 24 bits, two's-complement wrap-around.
__device__ __forceinline__ int mix10(int a, int b, int w) {
  return (int)((uint32_t)__mul24(a, 1024 - w) + (uint32_t)__mul24(b, w) + 512u) >> 10;
}

// ------------------------------------------------------------------------------- plan
// Thread t < tiles: the tile's plan; thread t < W / t < H: the column / row weight tables.
template <int TILE_H>
__global__ __launch_bounds__(256) void field_plan_kernel(const double* __restrict__ Mall,
                                                         const int32_t* __restrict__ field, int n_frames, int H, int W,
                                                         int gy, int gx, int inverse_map, int ntx, int nty,
                                                         TilePlan* __restrict__ plan, double* __restrict__ minv,
                                                         int* __restrict__ coltab, int* __restrict__ rowtab) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t < W) coltab[t] = axis_weight((int)t, W, gx);
  if (t < H) rowtab[t] = axis_weight((int)t, H, gy);
  if (t >= (long long)ntx * nty * n_frames) return;
  const PlanTile p = plan_tile<TILE_H>(t, Mall, inverse_map, H, W, ntx, nty, minv);
  const Box1024 b = affine_box(p.M, p.xb, p.yb, p.xl, p.yl);
  // the nodes whose cells touch the tile: k0 is monotone along an axis
  const int j_lo = axis_weight(p.xb, W, gx) & 0xffff, j_hi = min((axis_weight(p.xl, W, gx) & 0xffff) + 1, gx - 1);
  const int i_lo = axis_weight(p.yb, H, gy) & 0xffff, i_hi = min((axis_weight(p.yl, H, gy) & 0xffff) + 1, gy - 1);
  const int32_t* Q = field + (size_t)p.f * gy * gx * 2;
  int qx0 = INT_MAX, qx1 = INT_MIN, qy0 = INT_MAX, qy1 = INT_MIN;
  for (int i = i_lo; i <= i_hi; ++i)
    for (int j = j_lo; j <= j_hi; ++j) {
      const int vx = Q[2 * (i * gx + j)], vy = Q[2 * (i * gx + j) + 1];
      qx0 = min(qx0, vx);
      qx1 = max(qx1, vx);
      qy0 = min(qy0, vy);
      qy1 = max(qy1, vy);
    }
  const bool in_contract = qx0 >= -kMaxQ && qx1 <= kMaxQ && qy0 >= -kMaxQ && qy1 <= kMaxQ;
  plan[t] = classify_box((b.x0 + qx0) >> 10, ((b.x1 + qx1) >> 10) + 1, (b.y0 + qy0) >> 10, ((b.y1 + qy1) >> 10) + 1, H,
                         W, in_contract, map_has_nan(p.M, 6));
}

// ------------------------------------------------------------------------------- tiles
// Output rows of one tile on one path.  Wave w makes rows w, w + 4, ...; lane l the pixels
// x = xb + 2l, xb + 2l + 1.
template <int TILE_H, int MODE>
__device__ __forceinline__ void field_rows(const uint16_t* stile, const int2* vtab, int gx, int pitch,
                                           const uint16_t* __restrict__ S, uint16_t* __restrict__ Dst, int H, int W,
                                           int xb, int yb, int wave, int lane, const int (&ad)[2], const int (&bd)[2],
                                           const int (&j0)[2], const int (&j1)[2], const int (&wx)[2], int X0v, int Y0v,
                                           bool pair_ok) {
  const int x = xb + 2 * lane;
  const bool pair_store = pair_ok && x + 2 <= W;
#pragma unroll
  for (int i = 0; i < TILE_H / 4; ++i) {
    const int y = yb + wave + 4 * i;  // wave-uniform
    if (y >= H) break;
    const int X0 = __builtin_amdgcn_readlane(X0v, i), Y0 = __builtin_amdgcn_readlane(Y0v, i);
    const int2* vrow = vtab + (wave + 4 * i) * gx;
    uint16_t o[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (MODE == 1) {
        o[p] = 0;
        continue;
      }
      const int2 va = vrow[j0[p]], vb = vrow[j1[p]];
      const int tX = (int)((uint32_t)X0 + (uint32_t)ad[p] + (uint32_t)mix10(va.x, vb.x, wx[p]));
      const int tY = (int)((uint32_t)Y0 + (uint32_t)bd[p] + (uint32_t)mix10(va.y, vb.y, wx[p]));
      if (MODE == 0) {  // box-relative taps: the plan bounded them inside the staged box
        const int fx = (tX >> 5) & 31, fy = (tY >> 5) & 31;
        const int li = (int)__umul24((uint32_t)(tY >> 10), (uint32_t)pitch) + (tX >> 10);
        o[p] = blend_int(stile[li], stile[li + 1], stile[li + pitch], stile[li + pitch + 1], fx, fy);
      } else {
        bilinear_px<1>(S, H, W, tX >> 5, tY >> 5, o + p);
      }
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

// no-unaligned-access-mode: keeps the two adjacent 16-bit tap reads from being fused into one
// 4-byte LDS read at a 2-byte-aligned address (warp.hip).
template <int TILE_H>
__global__ __launch_bounds__(kThreads) __attribute__((target("no-unaligned-access-mode"))) void warp_field_u16_kernel(
    const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, const int32_t* __restrict__ field,
    const TilePlan* __restrict__ plan, const double* __restrict__ minv, const int* __restrict__ coltab,
    const int* __restrict__ rowtab, int H, int W, int gy, int gx, int vec_ok, int pair_ok) {
  __shared__ __attribute__((aligned(16))) uint16_t stile[kLdsElems];
  extern __shared__ int2 vtab[];  // the vertical step: [tile row][node column gx] (x, y), TILE_H * gx entries
  const TileId t = tile_decode<TILE_H>();
  const int tid = threadIdx.x, xb = t.xb, yb = t.yb, wave = t.wave, lane = t.lane;
  const uint16_t* S = src + (size_t)t.f * H * W;
  uint16_t* Dst = dst + (size_t)t.f * H * W;
  const int32_t* Q = field + (size_t)t.f * gy * gx * 2;
  const TilePlan tp = plan[t.tile];
  const int mode = tp.mode, pitch = tp.pitch();
  const bool vec_stage = mode == 0 && vec_ok;

  uint4 chunk[kRowPasses];
  stage_load(S, tp, H, W, vec_stage, chunk);
  // the vertical step of every tile row at every node column (rows past the frame edge reuse
  // the last row's weights and are never read)
  if (mode != 1) {
    for (int e = tid; e < TILE_H * gx; e += kThreads) {
      const int r = e / gx, j = e - r * gx;
      const int rt = rowtab[min(yb + r, H - 1)];
      const int i0 = rt & 0xffff, wy = rt >> 16, i1 = min(i0 + 1, gy - 1);
      const int32_t* qa = Q + 2 * (i0 * gx + j);
      const int32_t* qb = Q + 2 * (i1 * gx + j);
      vtab[r * gx + j] = make_int2(mix10(qa[0], qb[0], wy), mix10(qa[1], qb[1], wy));
    }
  }
  const double* M = minv + 6 * (size_t)t.f;
  int ad[2], bd[2], j0[2], j1[2], wx[2], X0v, Y0v;
  lane_columns(M, xb, lane, W, ad, bd);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int ct = coltab[min(xb + 2 * lane + q, W - 1)];
    j0[q] = ct & 0xffff;
    wx[q] = ct >> 16;
    j1[q] = min(j0[q] + 1, gx - 1);
  }
  row_origins<TILE_H>(M, t, tp, X0v, Y0v);
  stage_commit(stile, S, tp, H, W, vec_stage, chunk);
  __syncthreads();
  // one row loop per path (a path-uniform branch inside the loop drains the stores every row)
  if (mode == 0)
    field_rows<TILE_H, 0>(stile, vtab, gx, pitch, S, Dst, H, W, xb, yb, wave, lane, ad, bd, j0, j1, wx, X0v, Y0v, pair_ok);
  else if (mode == 1)
    field_rows<TILE_H, 1>(stile, vtab, gx, pitch, S, Dst, H, W, xb, yb, wave, lane, ad, bd, j0, j1, wx, X0v, Y0v, pair_ok);
  else
    field_rows<TILE_H, 2>(stile, vtab, gx, pitch, S, Dst, H, W, xb, yb, wave, lane, ad, bd, j0, j1, wx, X0v, Y0v, pair_ok);
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_warp_field_u16(kcmc_ctx* ctx, const uint16_t* src, uint16_t* dst, const double* M,
                                   const int32_t* field, int n_frames, int H, int W, int gy, int gx, int inverse_map,
                                   kcmc_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const size_t tables = ((size_t)W + (size_t)H) * sizeof(int);  // behind the plan: coltab [W], rowtab [H] i32
  return run_tile_warp(
      "kcmc_warp_field_u16", "warp_field_u16_kernel", ctx, src, dst, M && field, n_frames, H, W, tables, s,
      [&] {
        if (gy < 1 || gx < 1 || gy > kMaxGrid || gx > kMaxGrid || gy > H || gx > W)
          return fail(KCMC_EINVAL, "kcmc_warp_field_u16: grid must satisfy 1 <= gy, gx <= 16, gy <= H, gx <= W");
        return (int)KCMC_OK;
      },
      [&](auto th, const TileLaunch& l) {
        constexpr int TILE_H = decltype(th)::value;
        int* coltab = static_cast<int*>(l.extra);
        int* rowtab = coltab + W;
        const long long threads = std::max<long long>(l.tiles, std::max(W, H));
        hipLaunchKernelGGL((field_plan_kernel<TILE_H>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, M,
                           field, n_frames, H, W, gy, gx, inverse_map, l.ntx, l.nty, l.plan, l.minv, coltab, rowtab);
        // dynamic LDS: the vertical step's table behind the 20 KB box (2 KB at a 4 x 4 grid, 8 KB at 16 x 16)
        hipLaunchKernelGGL((warp_field_u16_kernel<TILE_H>), dim3(l.ntx, l.nty, n_frames), dim3(kThreads),
                           (size_t)TILE_H * gx * sizeof(int2), s, src, dst, field, l.plan, l.minv, coltab, rowtab, H, W,
                           gy, gx, l.vec_ok, l.pair_ok);
      });
}

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
// Layout: the affine warp's -- 128 x 56 (or 64) output tiles, one workgroup per tile, one
// output row per wave and pass, lane l the pixels 2l, 2l + 1.  A plan kernel (one thread per
// tile) inverts the map and bounds the tile's source box: the affine part is separable and
// monotone (warp.hip source_box) and each rounded interpolation step lies between the values
// it mixes, so the box is the affine box moved by the minimum and maximum of the node values
// whose cells touch the tile.  Boxes within the staging budget are staged in LDS, boxes that
// miss the image store zeros, every other tile (and every tile that touches a node outside the
// contract) gathers from global memory with range-checked taps.  The vertical step is made
// once per tile into LDS (tile rows x gx nodes); a pixel reads its two neighbours there and
// pays two multiplies per component.  The per-column / per-row (node, weight) pairs depend only
// on (W, gx) / (H, gy) and come from two tables the plan kernel writes.
//
// Blend: OpenCV's float blend (blend_int: the float evaluation with exact integer products)
// for every pixel; the affine warp's dark-box integer shortcut is not used here.
#include <climits>

#include "kcmc_internal.h"
#include "warp_common.h"

namespace kcmc {
namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 128;      // output columns per tile (64 lanes x 2 pixels)
constexpr int kMaxPitch = 256;   // staged row length limit (32 x 16-byte chunks)
constexpr int kLdsElems = 10240; // uint16 staging budget per box (20 KB)
constexpr int kRowPasses = 9;    // staging passes of 8 rows x 32 chunks (box rows <= 72)
constexpr int kMaxGrid = 16;     // nodes per axis
constexpr int kMaxQ = 1 << 20;   // contract on |q|

// the affine warp's tile-height rule (warp.hip use_tile64)
inline bool use_tile64(int H) { return H % 64 == 0 && H % 56 != 0; }

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

struct FieldPlan {
  int mode;        // 0: staged in LDS, 1: zeros, 2: direct gather
  int ax0, sy0;    // first staged column (multiple of 8) / row
  int pitch_rows;  // pitch | rows << 16
};

// ------------------------------------------------------------------------------- plan
// Thread t < tiles: the tile's plan (and, for the frame's first tile, the inverted map);
// thread t < W / t < H: the column / row weight tables.
template <int TILE_H>
__global__ __launch_bounds__(256) void field_plan_kernel(const double* __restrict__ Mall,
                                                         const int32_t* __restrict__ field, int n_frames, int H, int W,
                                                         int gy, int gx, int inverse_map, int ntx, int nty,
                                                         FieldPlan* __restrict__ plan, double* __restrict__ minv,
                                                         int* __restrict__ coltab, int* __restrict__ rowtab) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t < W) coltab[t] = axis_weight((int)t, W, gx);
  if (t < H) rowtab[t] = axis_weight((int)t, H, gy);
  if (t >= (long long)ntx * nty * n_frames) return;
  const int f = (int)(t / (ntx * nty)), t2 = (int)(t - (long long)f * ntx * nty);
  const int xb = (t2 % ntx) * kTileW, yb = (t2 / ntx) * TILE_H;
  double M[6];
  load_map(Mall, f, inverse_map, M);
  if (t2 == 0)
    for (int k = 0; k < 6; ++k) minv[6 * (size_t)f + k] = M[k];
  // the affine box in 1/1024 px (warp.hip source_box: monotone in x and in y)
  const int xl = min(xb + kTileW, W) - 1, yl = min(yb + TILE_H, H) - 1;
  const long long a0 = cv_round(M[0] * xb * 1024), a1 = cv_round(M[0] * xl * 1024);
  const long long b0 = cv_round(M[3] * xb * 1024), b1 = cv_round(M[3] * xl * 1024);
  const long long x0 = cv_round((M[1] * yb + M[2]) * 1024) + 16, x1 = cv_round((M[1] * yl + M[2]) * 1024) + 16;
  const long long y0 = cv_round((M[4] * yb + M[5]) * 1024) + 16, y1 = cv_round((M[4] * yl + M[5]) * 1024) + 16;
  // the nodes whose cells touch the tile: k0 is monotone along an axis
  const int j_lo = axis_weight(xb, W, gx) & 0xffff, j_hi = min((axis_weight(xl, W, gx) & 0xffff) + 1, gx - 1);
  const int i_lo = axis_weight(yb, H, gy) & 0xffff, i_hi = min((axis_weight(yl, H, gy) & 0xffff) + 1, gy - 1);
  const int32_t* Q = field + (size_t)f * gy * gx * 2;
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
  const long long sx0 = (min(x0, x1) + min(a0, a1) + qx0) >> 10, sx1 = ((max(x0, x1) + max(a0, a1) + qx1) >> 10) + 1;
  const long long sy0 = (min(y0, y1) + min(b0, b1) + qy0) >> 10, sy1 = ((max(y0, y1) + max(b0, b1) + qy1) >> 10) + 1;
  const long long lim = 30000;  // keep clear of saturate_cast<short> on coordinates
  const bool small = in_contract && sx0 > -lim && sx1 < lim && sy0 > -lim && sy1 < lim;
  const long long ax0 = (sx0 >> 3) << 3;
  const long long pitch = ((sx1 - ax0 + 1) + 7) & ~7ll;
  const long long rows = sy1 - sy0 + 1;
  FieldPlan p;
  p.mode = 2;
  p.ax0 = p.sy0 = p.pitch_rows = 0;
  if (small && (sx1 < 0 || sx0 > W - 1 || sy1 < 0 || sy0 > H - 1)) {
    p.mode = 1;
  } else if (small && pitch <= kMaxPitch && rows <= 8 * kRowPasses && pitch * rows <= kLdsElems) {
    p.mode = 0;
    p.ax0 = (int)ax0;
    p.sy0 = (int)sy0;
    p.pitch_rows = (int)pitch | ((int)rows << 16);
  }
  if (map_has_nan(M, 6)) p.mode = 1;  // a NaN map (a frame RANSAC could not fit) warps to zeros
  plan[t] = p;
}

// ------------------------------------------------------------------------------- tiles
// Output rows of one tile on one path.  Wave w makes rows w, w + 4, ...; lane l the pixels
// x = xb + 2l, xb + 2l + 1.  Columns past the frame edge reuse the last valid column's
// coordinates so that their (never stored) taps stay inside the box.
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
// vec_ok: W % 8 == 0 and src 16-byte aligned (16-byte staging loads); pair_ok: W even and dst
// 4-byte aligned (one 4-byte store per lane).
template <int TILE_H>
__global__ __launch_bounds__(kThreads) __attribute__((target("no-unaligned-access-mode"))) void warp_field_u16_kernel(
    const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, const int32_t* __restrict__ field,
    const FieldPlan* __restrict__ plan, const double* __restrict__ minv, const int* __restrict__ coltab,
    const int* __restrict__ rowtab, int H, int W, int gy, int gx, int vec_ok, int pair_ok) {
  __shared__ __attribute__((aligned(16))) uint16_t stile[kLdsElems];
  extern __shared__ int2 vtab[];  // the vertical step: [tile row][node column gx] (x, y), TILE_H * gx entries
  const int ntx = gridDim.x, nty = gridDim.y;
  const int tile = xcd_remap(blockIdx.x + ntx * (blockIdx.y + nty * blockIdx.z), ntx * nty * gridDim.z);
  const int f = tile / (ntx * nty);
  const int t2 = tile - f * ntx * nty;
  const int xb = (t2 % ntx) * kTileW, yb = (t2 / ntx) * TILE_H;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const uint16_t* S = src + (size_t)f * H * W;
  uint16_t* Dst = dst + (size_t)f * H * W;
  const int32_t* Q = field + (size_t)f * gy * gx * 2;

  const FieldPlan tp = plan[tile];
  const int mode = tp.mode, ax0 = tp.ax0, sy0 = tp.sy0;
  const int pitch = tp.pitch_rows & 0xffff, rows = tp.pitch_rows >> 16;
  const bool vec_stage = mode == 0 && vec_ok;

  // staging loads first: chunk c = tid & 31 of box row tid >> 5 + 8 k; with W % 8 == 0 a
  // 16-byte chunk is entirely inside or entirely outside the image (zeros)
  uint4 chunk[kRowPasses];
  const int cpr = pitch >> 3, sc = tid & 31, sr = tid >> 5;
  if (vec_stage) {
    const int cx = ax0 + 8 * sc;
    const bool col_ok = sc < cpr && cx >= 0 && cx < W;
#pragma unroll
    for (int k = 0; k < kRowPasses; ++k) {
      const int r = sr + 8 * k, cy = sy0 + r;
      chunk[k] = make_uint4(0u, 0u, 0u, 0u);
      if (r < rows && col_ok && (unsigned)cy < (unsigned)H)
        chunk[k] = *reinterpret_cast<const uint4*>(S + (size_t)cy * W + cx);
    }
  }
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
  // the lane's two columns and, in lane i < TILE_H / 4, the origins of the wave's i-th row;
  // for a staged tile the box origin is folded into the row origins (a multiple of 1024)
  const double* M = minv + 6 * (size_t)f;
  int ad[2], bd[2], j0[2], j1[2], wx[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int x = min(xb + 2 * lane + q, W - 1);
    ad[q] = cv_round(M[0] * x * 1024);
    bd[q] = cv_round(M[3] * x * 1024);
    const int ct = coltab[x];
    j0[q] = ct & 0xffff;
    wx[q] = ct >> 16;
    j1[q] = min(j0[q] + 1, gx - 1);
  }
  const int yl = yb + wave + 4 * min(lane, TILE_H / 4 - 1);
  const int X0v = cv_round((M[1] * yl + M[2]) * 1024) + 16 - (mode == 0 ? ax0 : 0) * 1024;
  const int Y0v = cv_round((M[4] * yl + M[5]) * 1024) + 16 - (mode == 0 ? sy0 : 0) * 1024;
  if (vec_stage) {
#pragma unroll
    for (int k = 0; k < kRowPasses; ++k) {
      const int r = sr + 8 * k;
      if (r < rows && sc < cpr) *reinterpret_cast<uint4*>(&stile[r * pitch + 8 * sc]) = chunk[k];
    }
  } else if (mode == 0) {  // element-wise staging (W % 8 != 0 or an unaligned slab)
    for (int q = tid; q < rows * pitch; q += kThreads) {
      const int r = q / pitch, e = q - r * pitch;
      const int cy = sy0 + r, cx = ax0 + e;
      stile[q] = ((unsigned)cy < (unsigned)H && (unsigned)cx < (unsigned)W) ? S[(size_t)cy * W + cx] : (uint16_t)0;
    }
  }
  __syncthreads();
  // one row loop per path (a path-uniform branch inside the loop drains the stores every row)
  if (mode == 0)
    field_rows<TILE_H, 0>(stile, vtab, gx, pitch, S, Dst, H, W, xb, yb, wave, lane, ad, bd, j0, j1, wx, X0v, Y0v, pair_ok);
  else if (mode == 1)
    field_rows<TILE_H, 1>(stile, vtab, gx, pitch, S, Dst, H, W, xb, yb, wave, lane, ad, bd, j0, j1, wx, X0v, Y0v, pair_ok);
  else
    field_rows<TILE_H, 2>(stile, vtab, gx, pitch, S, Dst, H, W, xb, yb, wave, lane, ad, bd, j0, j1, wx, X0v, Y0v, pair_ok);
}

// Workspace layout: minv [F, 6] f64, plan [tiles], coltab [W] i32, rowtab [H] i32.
struct FieldWs {
  double* minv;
  FieldPlan* plan;
  int* coltab;
  int* rowtab;
  FieldWs(void* ws, int n_frames, size_t tiles, int W) {
    minv = static_cast<double*>(ws);
    plan = reinterpret_cast<FieldPlan*>(minv + 6 * (size_t)n_frames);
    coltab = reinterpret_cast<int*>(plan + tiles);
    rowtab = coltab + W;
  }
};

template <int TILE_H>
void launch_field(const uint16_t* src, uint16_t* dst, const double* M, const int32_t* field, int n_frames, int H, int W,
                  int gy, int gx, int inverse_map, void* ws, hipStream_t s) {
  const int ntx = ceil_div(W, kTileW), nty = ceil_div(H, TILE_H);
  const long long tiles = (long long)ntx * nty * n_frames;
  const FieldWs w(ws, n_frames, (size_t)tiles, W);
  const long long threads = std::max<long long>(tiles, std::max(W, H));
  hipLaunchKernelGGL((field_plan_kernel<TILE_H>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, M, field,
                     n_frames, H, W, gy, gx, inverse_map, ntx, nty, w.plan, w.minv, w.coltab, w.rowtab);
  const int vec_ok = (W & 7) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  const int pair_ok = (W & 1) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
  // dynamic LDS: the vertical step's table behind the 20 KB box (2 KB at a 4 x 4 grid, 8 KB at 16 x 16)
  hipLaunchKernelGGL((warp_field_u16_kernel<TILE_H>), dim3(ntx, nty, n_frames), dim3(kThreads),
                     (size_t)TILE_H * gx * sizeof(int2), s, src, dst, field,
                     w.plan, w.minv, w.coltab, w.rowtab, H, W, gy, gx, vec_ok, pair_ok);
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_warp_field_u16(kcmc_ctx* ctx, const uint16_t* src, uint16_t* dst, const double* M,
                                   const int32_t* field, int n_frames, int H, int W, int gy, int gx, int inverse_map,
                                   kcmc_stream_t stream) {
  if (!ctx) return fail(KCMC_EINVAL, "kcmc_warp_field_u16: ctx is NULL");
  if (n_frames < 0) return fail(KCMC_EINVAL, "kcmc_warp_field_u16: negative n_frames");
  if (H < 1 || W < 1) return fail(KCMC_EINVAL, "kcmc_warp_field_u16: H, W must be >= 1");
  if (gy < 1 || gx < 1 || gy > kMaxGrid || gx > kMaxGrid || gy > H || gx > W)
    return fail(KCMC_EINVAL, "kcmc_warp_field_u16: grid must satisfy 1 <= gy, gx <= 16, gy <= H, gx <= W");
  if (n_frames == 0) return KCMC_OK;
  if (!src || !dst || !M || !field) return fail(KCMC_EINVAL, "kcmc_warp_field_u16: NULL pointer");
  if (src == dst) return fail(KCMC_EINVAL, "kcmc_warp_field_u16: in-place warp is not supported");
  if (H > 32767 || W > 32767) return fail(KCMC_EUNSUPPORTED, "kcmc_warp_field_u16: H, W must be < 32768");
  if (n_frames > 65535) return fail(KCMC_EUNSUPPORTED, "kcmc_warp_field_u16: at most 65535 frames per call");
  const bool t64 = use_tile64(H);
  const long long tiles = (long long)ceil_div(W, kTileW) * ceil_div(H, t64 ? 64 : 56) * n_frames;
  if (tiles >= (1ll << 31)) return fail(KCMC_EUNSUPPORTED, "kcmc_warp_field_u16: too many tiles in one call");
  hipStream_t s = (hipStream_t)stream;
  void* ws = nullptr;
  const size_t wsb = (size_t)n_frames * 6 * sizeof(double) + (size_t)tiles * sizeof(FieldPlan) +
                     ((size_t)W + (size_t)H) * sizeof(int);
  KCMC_TRY(workspace_alloc(ctx, &ws, wsb, s));
  if (t64)
    launch_field<64>(src, dst, M, field, n_frames, H, W, gy, gx, inverse_map, ws, s);
  else
    launch_field<56>(src, dst, M, field, n_frames, H, W, gy, gx, inverse_map, ws, s);
  const int rc = launch_check("warp_field_u16_kernel");
  KCMC_TRY(workspace_free(ctx, ws, s, wsb));
  return rc;
}

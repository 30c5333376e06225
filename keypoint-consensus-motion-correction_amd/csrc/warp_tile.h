// The tile skeleton the four box-staging warps share (warp.hip K3 / K3p, warp_cubic.hip K3c,
// warp_field.hip K3f): everything here is described once.  The bilinear warp.hip adds its own
// configurations (tile height, budget and passes per channel count), its own classification
// (the budget depends on them), a fixed-pitch fast path (mode 3) and interleaved staging.
//
// Layout: 128 x 56 output tiles (64 rows under use_tile64), one workgroup of 256 threads per tile,
// one output row per wave and pass, lane l the pixels 2l, 2l + 1.  A plan kernel (one thread per
// tile) inverts the map and bounds the tile's source box: the affine part is separable and
// monotone (affine_box), so it is taken at the tile's corner rows / columns, and
// the kernel widens it to its footprint.  classify_box sorts the tile: a box within the staging
// budget (pitch <= 256, rows <= 72, 20 KB) is staged in LDS with zeros outside the image
// (BORDER_CONSTANT), a box that misses the image stores zeros, every other tile gathers from
// global memory with range-checked taps.  Box bound and staging loop keep every LDS and global
// access in range: a staged tile's taps are box-relative and unchecked.
//
// Tile kernel: tile_decode, the plan, stage_load (16-byte loads into registers), the kernel's
// own independent work while they fly (lane_columns, row_origins, its tables), stage_commit,
// __syncthreads, then one row loop per mode, which stays in the kernel's file with its store
// (as a shared function the store cost K3f a register: profiles/warp_tile_shared.md).
// vec_ok: W % 8 == 0 and src 16-byte aligned (16-byte staging loads, a chunk entirely inside or
// outside the image); pair_ok: W even and dst 4-byte aligned (one 4-byte store per lane).
#pragma once

#include <climits>
#include <string>
#include <type_traits>

#include "kcmc_internal.h"
#include "warp_common.h"

namespace kcmc {

constexpr int kThreads = 256;
constexpr int kTileW = 128;       // output columns per tile (64 lanes x 2 pixels)
constexpr int kMaxPitch = 256;    // staged row length limit (32 x 16-byte chunks)
constexpr int kLdsElems = 10240;  // uint16 staging budget per box (20 KB)
constexpr int kRowPasses = 9;     // staging passes of 8 rows x 32 chunks (box rows <= 72)

// the one-channel tile-height rule: frame heights that are a multiple of 64 but not of 56 (512)
// lose 9 % of their tiles to a partial last tile row at 56 rows
inline bool use_tile64(int H) { return H % 64 == 0 && H % 56 != 0; }

struct TilePlan {
  int mode;        // 0: staged in LDS, 1: zeros, 2: direct gather, 3: fixed-pitch fast path (warp.hip)
  int ax0, sy0;    // first staged column (multiple of 8) / row
  int pitch_rows;  // pitch | rows << 16 | (box inside the image) << 31
  __device__ int pitch() const { return pitch_rows & 0xffff; }
  __device__ int rows() const { return (pitch_rows >> 16) & 0x7fff; }
  __device__ bool inside() const { return pitch_rows < 0; }
};

// ------------------------------------------------------------------------------- plan
struct PlanTile {
  int f, xb, yb, xl, yl;  // frame, first and last output column / row
  double M[6];            // the inverse map
};

// Plan thread t < tiles: its tile and map; the frame's first tile also writes the inverted map.
template <int TILE_H>
__device__ __forceinline__ PlanTile plan_tile(long long t, const double* Mall, int inverse_map, int H,
                                              int W, int ntx, int nty, double* minv) {
  PlanTile p;
  p.f = (int)(t / (ntx * nty));
  const int t2 = (int)(t - (long long)p.f * ntx * nty);
  p.xb = (t2 % ntx) * kTileW, p.yb = (t2 / ntx) * TILE_H;
  p.xl = min(p.xb + kTileW, W) - 1, p.yl = min(p.yb + TILE_H, H) - 1;
  load_map(Mall, p.f, inverse_map, p.M);
  if (t2 == 0)
    for (int k = 0; k < 6; ++k) minv[6 * (size_t)p.f + k] = p.M[k];
  return p;
}

struct Box1024 {
  long long x0, x1, y0, y1;  // minimum and maximum of X and of Y over the tile, 1/1024 px
};

__device__ __forceinline__ Box1024 affine_box(const double (&M)[6], int xb, int yb, int xl, int yl) {
  const long long a0 = cv_round(M[0] * xb * 1024), a1 = cv_round(M[0] * xl * 1024);
  const long long b0 = cv_round(M[3] * xb * 1024), b1 = cv_round(M[3] * xl * 1024);
  const long long x0 = cv_round((M[1] * yb + M[2]) * 1024) + 16, x1 = cv_round((M[1] * yl + M[2]) * 1024) + 16;
  const long long y0 = cv_round((M[4] * yb + M[5]) * 1024) + 16, y1 = cv_round((M[4] * yl + M[5]) * 1024) + 16;
  return {min(x0, x1) + min(a0, a1), max(x0, x1) + max(a0, a1), min(y0, y1) + min(b0, b1), max(y0, y1) + max(b0, b1)};
}

// The plan of a tile whose taps lie in source columns sx0..sx1 and rows sy0..sy1.  extra_ok:
// the kernel's own condition for anything but the gather; has_nan: a NaN map (a frame RANSAC
// could not fit) warps to zeros.
__device__ __forceinline__ TilePlan classify_box(long long sx0, long long sx1, long long sy0, long long sy1, int H,
                                                 int W, bool extra_ok, bool has_nan) {
  const long long lim = 30000;  // keep clear of saturate_cast<short> on coordinates
  const bool small = extra_ok && sx0 > -lim && sx1 < lim && sy0 > -lim && sy1 < lim;
  const long long ax0 = (sx0 >> 3) << 3;
  const long long pitch = ((sx1 - ax0 + 1) + 7) & ~7ll;
  const long long rows = sy1 - sy0 + 1;
  TilePlan p;
  p.mode = 2;
  p.ax0 = p.sy0 = p.pitch_rows = 0;
  if (small && (sx1 < 0 || sx0 > W - 1 || sy1 < 0 || sy0 > H - 1)) {
    p.mode = 1;
  } else if (small && pitch <= kMaxPitch && rows <= 8 * kRowPasses && pitch * rows <= kLdsElems) {
    p.mode = 0;
    p.ax0 = (int)ax0;
    p.sy0 = (int)sy0;
    const bool inside = sx0 >= 0 && sx1 <= W - 1 && sy0 >= 0 && sy1 <= H - 1;
    p.pitch_rows = (int)pitch | ((int)rows << 16) | (inside ? INT_MIN : 0);
  }
  if (has_nan) p.mode = 1;
  return p;
}

// ------------------------------------------------------------------------------- tiles
struct TileId {
  int tile, f, xb, yb;  // plan index, frame, first output column / row
  int wave, lane;
};

template <int TILE_H>
__device__ __forceinline__ TileId tile_decode() {
  const int ntx = gridDim.x, nty = gridDim.y;
  TileId t;
  t.tile = xcd_remap(blockIdx.x + ntx * (blockIdx.y + nty * blockIdx.z), ntx * nty * gridDim.z);
  t.f = t.tile / (ntx * nty);
  const int t2 = t.tile - t.f * ntx * nty;
  t.xb = (t2 % ntx) * kTileW, t.yb = (t2 / ntx) * TILE_H;
  const int tid = threadIdx.x;
  t.wave = __builtin_amdgcn_readfirstlane(tid >> 6), t.lane = tid & 63;
  return t;
}

// Staging, first half: thread tid loads chunk c = tid & 31 of box rows tid >> 5 + 8 k (zeros
// where the chunk lies outside the box or the image), k < PASSES (deduced: box rows <= 8 PASSES).
template <int PASSES>
__device__ __forceinline__ void stage_load(const uint16_t* S, const TilePlan& tp, int H, int W,
                                           bool vec_stage, uint4 (&chunk)[PASSES]) {
  const int tid = threadIdx.x, cpr = tp.pitch() >> 3, sc = tid & 31, sr = tid >> 5;
  if (vec_stage) {
    const int cx = tp.ax0 + 8 * sc;
    const bool col_ok = sc < cpr && cx >= 0 && cx < W;
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
      const int r = sr + 8 * k, cy = tp.sy0 + r;
      chunk[k] = make_uint4(0u, 0u, 0u, 0u);
      if (r < tp.rows() && col_ok && (unsigned)cy < (unsigned)H)
        chunk[k] = *reinterpret_cast<const uint4*>(S + (size_t)cy * W + cx);
    }
  }
}

// Element-wise staging of a C-channel box (W % 8 != 0 or an unaligned slab).
template <int C>
__device__ __forceinline__ void stage_elements(uint16_t* stile, const uint16_t* S, const TilePlan& tp, int H, int W) {
  const int rowe = tp.pitch() * C;
  for (int q = threadIdx.x; q < tp.rows() * rowe; q += kThreads) {
    const int r = q / rowe, e = q - r * rowe;
    const int cy = tp.sy0 + r, cx = tp.ax0 + e / C, k = e % C;
    stile[q] = ((unsigned)cy < (unsigned)H && (unsigned)cx < (unsigned)W) ? S[((size_t)cy * W + cx) * C + k]
                                                                          : (uint16_t)0;
  }
}

// Second half: the chunks into LDS, or the box element by element.  stile holds the box's
// pitch * rows elements at least.
template <int PASSES>
__device__ __forceinline__ void stage_commit(uint16_t* stile, const uint16_t* S, const TilePlan& tp, int H,
                                             int W, bool vec_stage, const uint4 (&chunk)[PASSES]) {
  const int pitch = tp.pitch(), rows = tp.rows();
  const int tid = threadIdx.x, cpr = pitch >> 3, sc = tid & 31, sr = tid >> 5;
  if (vec_stage) {
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
      const int r = sr + 8 * k;
      if (r < rows && sc < cpr) *reinterpret_cast<uint4*>(&stile[r * pitch + 8 * sc]) = chunk[k];
    }
  } else if (tp.mode == 0) {
    stage_elements<1>(stile, S, tp, H, W);
  }
}

// The column deltas of the lane's two pixels.  Columns past the frame edge reuse the last valid
// column's coordinates so that their (never stored) taps stay inside the box.
__device__ __forceinline__ void lane_columns(const double* M, int xb, int lane, int W, int (&ad)[2],
                                             int (&bd)[2]) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int x = min(xb + 2 * lane + q, W - 1);
    ad[q] = cv_round(M[0] * x * 1024);
    bd[q] = cv_round(M[3] * x * 1024);
  }
}

// In lane i < TILE_H / 4: the origins of the wave's i-th row.  For a staged tile the box origin
// is folded in (a multiple of 1024), so X >> 10, Y >> 10 are box-relative.
template <int TILE_H>
__device__ __forceinline__ void row_origins(const double* M, const TileId& t, const TilePlan& tp, int& X0v,
                                            int& Y0v) {
  const int yl = t.yb + t.wave + 4 * min(t.lane, TILE_H / 4 - 1);
  X0v = cv_round((M[1] * yl + M[2]) * 1024) + 16 - (tp.mode == 0 ? tp.ax0 : 0) * 1024;
  Y0v = cv_round((M[4] * yl + M[5]) * 1024) + 16 - (tp.mode == 0 ? tp.sy0 : 0) * 1024;
}

// ------------------------------------------------------------------------------- host
// What a launch gets: the tile grid, the workspace -- minv [F, 6] f64, plan [tiles], then the
// entry's own extra bytes -- and the two alignment switches.
struct TileLaunch {
  int ntx, nty;
  long long tiles;
  double* minv;
  TilePlan* plan;
  void* extra;
  int vec_ok, pair_ok;
};

// The body of an entry `name`: the argument check (own_check() is the entry's own, made after
// H and W; maps_ok: its further pointers are not NULL), then launch(tile height constant,
// TileLaunch) between the workspace's alloc and free.
template <typename OwnCheck, typename Launch>
int run_tile_warp(const char* name, const char* kernel, kcmc_ctx* ctx, const void* src, const void* dst, bool maps_ok,
                  int n_frames, int H, int W, size_t extra_bytes, hipStream_t s, OwnCheck own_check, Launch launch) {
  const std::string t(name);
  if (!ctx) return fail(KCMC_EINVAL, t + ": ctx is NULL");
  if (n_frames < 0) return fail(KCMC_EINVAL, t + ": negative n_frames");
  if (H < 1 || W < 1) return fail(KCMC_EINVAL, t + ": H, W must be >= 1");
  KCMC_TRY(own_check());
  if (n_frames == 0) return KCMC_OK;
  if (!src || !dst || !maps_ok) return fail(KCMC_EINVAL, t + ": NULL pointer");
  if (src == dst) return fail(KCMC_EINVAL, t + ": in-place warp is not supported");
  if (H > 32767 || W > 32767) return fail(KCMC_EUNSUPPORTED, t + ": H, W must be < 32768");
  if (n_frames > 65535) return fail(KCMC_EUNSUPPORTED, t + ": at most 65535 frames per call");
  const bool t64 = use_tile64(H);
  TileLaunch l;
  l.ntx = ceil_div(W, kTileW), l.nty = ceil_div(H, t64 ? 64 : 56);
  l.tiles = (long long)l.ntx * l.nty * n_frames;
  if (l.tiles >= (1ll << 31)) return fail(KCMC_EUNSUPPORTED, t + ": too many tiles in one call");
  void* ws = nullptr;
  const size_t wsb = (size_t)n_frames * 6 * sizeof(double) + (size_t)l.tiles * sizeof(TilePlan) + extra_bytes;
  KCMC_TRY(workspace_alloc(ctx, &ws, wsb, s));
  l.minv = static_cast<double*>(ws);
  l.plan = reinterpret_cast<TilePlan*>(l.minv + 6 * (size_t)n_frames);
  l.extra = l.plan + l.tiles;
  l.vec_ok = (W & 7) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  l.pair_ok = (W & 1) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
  if (t64)
    launch(std::integral_constant<int, 64>(), l);
  else
    launch(std::integral_constant<int, 56>(), l);
  const int rc = launch_check(kernel);
  KCMC_TRY(workspace_free(ctx, ws, s, wsb));
  return rc;
}

}  // namespace kcmc

// K3: batched warpAffine of uint16 frames, OpenCV classic INTER_LINEAR semantics.
//
// Reference: VA:455-458  cv2.warpAffine(image, affine, image.shape[::-1],
// flags=cv2.INTER_LINEAR) -- no WARP_INVERSE_MAP, so OpenCV first inverts the 2x3
// map in double, then (WarpAffineInvoker) builds 1/32-pixel fixed-point source
// coordinates:  adelta[x] = cvRound(M0*x*1024), X0(y) = cvRound((M1*y + M2)*1024) + 16,
// X = (X0 + adelta[x]) >> 5, sx = X >> 5, fx = X & 31 (same for Y), and remapBilinear
// blends the four taps with float weights (1-fy/32, fy/32) x (1-fx/32, fx/32),
// ((v00*w0 + v01*w1) + v10*w2) + v11*w3 with separately rounded products, then
// cvRound to uint16 with saturation.  Taps outside the image read 0 (BORDER_CONSTANT).
// This file is compiled with -ffp-contract=off so that arithmetic is reproduced
// operation by operation.
//
// Layout: frames [F, H, W, C] u16 contiguous in HBM, processed in 128 x 56 output
// tiles on the skeleton of warp_tile.h (plan struct, tile decode, box staging, column
// deltas, row origins).  Because the fixed-point source coordinate is separable
// (X = X0[y] + adelta[x]) and monotone, the exact source bounding box of a tile follows
// from its corner values (affine_box); the box is staged into LDS with coalesced 16-byte
// loads (zero outside the image, which is exactly BORDER_CONSTANT) and every output pixel
// gathers its four taps from LDS with aligned 16-bit reads.  A wave makes one 128-pixel
// output row at a time (lane l: pixels 2l, 2l+1, one 4-byte store), so its tap reads cover
// consecutive LDS words without bank conflicts and its row-level state is wave-uniform.
// Tiles whose box exceeds the staging budget (strong zoom-out or rotation) gather from
// global memory instead; tiles whose box misses the image store zeros.
//
// Frames with W % 8 == 0 and a box that fits a fixed 144-pixel LDS pitch (the near-identity
// maps of motion correction) take a leaner form of the same path (mode 3, fast_rows): one
// plane per channel at the fixed pitch -- one channel staged by range-checked buffer loads
// at a constant row stride per thread (Fast<Cfg, 1>: the descriptor's range check is the
// zero border, one add per pass), three or four de-interleaved while they land --, scalar
// per-row origins from a per-frame table, immediate-offset taps, buffer stores, and a
// per-tile choice of blend from the staged values (exact integer blend with no range check
// when every value is < 16384; with a few bright values the integer blend and OpenCV's
// float blend only for rows with a sum near a rounding tie; the float blend on packed fp32
// for bright boxes).
//
// Two launches: warp_plan_kernel (one thread per tile) inverts the map in fp64 and
// derives each tile's source box and the frame's row-origin table, so that the tile
// kernel starts with scalar loads of its plan and issues its staging loads immediately; warp_affine_u16_kernel then makes
// one tile per workgroup, latency hidden by the other resident workgroups (a persistent
// double-buffered variant measured 25% slower).
#include "warp_tile.h"  // the tile skeleton; warp_common.h: cv_round, load_map, blend_int, bilinear_px

namespace kcmc {
namespace {

template <int TILE_H, int LDS_ELEMS, int ROW_PASSES>
struct WarpCfg {
  static constexpr int kTileH = TILE_H;          // output rows per tile (4 waves x kTileH/4)
  static constexpr int kLdsElems = LDS_ELEMS;    // uint16 staging budget per box
  static constexpr int kRowPasses = ROW_PASSES;  // staging passes of 8 rows x 32 chunks
};
using BlockCfg = WarpCfg<56, kLdsElems, kRowPasses>;  // 20 KB box, box rows <= 72 (8 workgroups per CU: all 160 KiB of LDS)
// use_tile64 frames: 64-row tiles with the same 20 KB box budget cover them exactly (the
// fast path's 71 staged rows still hold a 64-row tile rotated by up to ~2.5 deg; larger
// rotations take the general staged path or the direct gather).
using Block64Cfg = WarpCfg<64, kLdsElems, kRowPasses>;
// Multi-channel frames (RGB / RGBA, config 4): 3-4x the bytes per box pixel, so shorter
// tiles keep the interleaved box in a 32 KB LDS budget (box rows <= 32).
using ChanCfg = WarpCfg<24, 16384, 4>;

template <int C>
struct CfgFor {
  using type = std::conditional_t<C == 1, BlockCfg, ChanCfg>;
};

// The plan of a tile whose taps lie in source columns sx0..sx1 and rows sy0..sy1 (classify_box
// with this file's budgets: `budget` elements for the C-channel box under Cfg).  small: the box
// is clear of OpenCV's saturate_cast<short> on coordinates; stage_ok: it may be staged.
template <class Cfg, int C>
__device__ __forceinline__ TilePlan box_plan(long long sx0, long long sx1, long long sy0, long long sy1, int H, int W,
                                             bool small, bool stage_ok, int budget) {
  const long long ax0 = (sx0 >> 3) << 3;
  const long long pitch = ((sx1 - ax0 + 1) + 7) & ~7ll;
  const long long rows = sy1 - sy0 + 1;
  int mode = 2;
  if (small && (sx1 < 0 || sx0 > W - 1 || sy1 < 0 || sy0 > H - 1))
    mode = 1;
  else if (small && stage_ok && pitch <= kMaxPitch && rows <= 8 * Cfg::kRowPasses && pitch * rows * C <= budget)
    mode = 0;
  return TilePlan{mode, (int)ax0, (int)sy0, (int)pitch | ((int)rows << 16)};
}

// The source box of the tile's valid pixels.  adelta[x] = cvRound(M0*x*1024) and
// X0[y] = cvRound((M1*y + M2)*1024) + 16 are monotone in x and y (monotone products,
// sums and rounding), so their extremes sit at the tile's first/last valid column/row
// (affine_box) and sx = (X0[y] + adelta[x]) >> 10 spans [min, max] exactly; the second tap adds 1.
template <class Cfg, int C>
__device__ __forceinline__ TilePlan source_box(const PlanTile& p, int H, int W) {
  const Box1024 b = affine_box(p.M, p.xb, p.yb, p.xl, p.yl);
  const long long sx0 = b.x0 >> 10, sx1 = (b.x1 >> 10) + 1, sy0 = b.y0 >> 10, sy1 = (b.y1 >> 10) + 1;
  const long long lim = 30000;  // keep clear of OpenCV's saturate_cast<short> on coordinates
  const bool small = sx0 > -lim && sx1 < lim && sy0 > -lim && sy1 < lim;
  return box_plan<Cfg, C>(sx0, sx1, sy0, sy1, H, W, small, true, Cfg::kLdsElems);
}

// Generic staging of a mode-0 box, issue before the kernel's own work and land after.  One
// channel: stage_load / stage_commit (with W % 8 == 0 every 16-byte chunk is entirely inside
// or entirely outside the image; element-wise otherwise).  C channels with W % 8 == 0: 16-byte
// chunks of the interleaved rows (ax0 and W are multiples of 8 pixels, so a chunk is entirely
// inside or outside the image row and zero-filling whole chunks is exactly BORDER_CONSTANT),
// chunk q = tid + kThreads * k of the box; every load of a thread is issued before any lands
// (a load-then-store loop waits for each load in turn: the 4K RGB warp took 14.6 ms per
// 625 frames that way, 11.8 ms with the loads in flight together).
template <class Cfg, int C>
struct BoxLoads {
  static constexpr int kPasses = C == 1 ? Cfg::kRowPasses : (Cfg::kLdsElems / 8 + kThreads - 1) / kThreads;
  uint4 chunk[kPasses];
};

template <class Cfg, int C>
__device__ __forceinline__ void box_issue(const uint16_t* __restrict__ S, const TilePlan& tp, int H, int W,
                                          BoxLoads<Cfg, C>& l) {
  if (tp.mode != 0 || (W & 7) != 0) return;
  if constexpr (C == 1) {
    stage_load(S, tp, H, W, true, l.chunk);
  } else {
    const int tid = threadIdx.x, cpr = tp.pitch() * C / 8, total = tp.rows() * cpr, rowe = W * C;
#pragma unroll
    for (int k = 0; k < BoxLoads<Cfg, C>::kPasses; ++k) {
      const int q = tid + kThreads * k;
      const int r = q / cpr, cc = q - r * cpr;
      const int gy = tp.sy0 + r;
      const int e = tp.ax0 * C + 8 * cc;
      l.chunk[k] = make_uint4(0u, 0u, 0u, 0u);
      if (q < total && (unsigned)gy < (unsigned)H && e >= 0 && e < rowe)
        l.chunk[k] = *reinterpret_cast<const uint4*>(S + (size_t)gy * rowe + e);
    }
  }
}

template <class Cfg, int C>
__device__ __forceinline__ void box_land(uint16_t* stile, const uint16_t* __restrict__ S, const TilePlan& tp, int H,
                                         int W, const BoxLoads<Cfg, C>& l) {
  if (tp.mode != 0) return;
  if constexpr (C == 1) {
    stage_commit(stile, S, tp, H, W, (W & 7) == 0, l.chunk);
  } else if ((W & 7) == 0) {
    const int tid = threadIdx.x, total = tp.rows() * (tp.pitch() * C / 8);
#pragma unroll
    for (int k = 0; k < BoxLoads<Cfg, C>::kPasses; ++k) {
      const int q = tid + kThreads * k;
      if (q < total) reinterpret_cast<uint4*>(stile)[q] = l.chunk[k];
    }
  } else {
    stage_elements<C>(stile, S, tp, H, W);
  }
}

// rint(S / 1024) (round half to even) for an integer S < 2^24, as the low 16 bits of
// fl(S * 2^-10 + 1.5 * 2^23): float(S) and the scaling are exact, the fused add rounds
// once to an integer (ulp 1 at that magnitude) in round-to-nearest-even.
__device__ __forceinline__ uint16_t round_q10(uint32_t S) {
  return (uint16_t)__float_as_uint(__builtin_fmaf((float)S, 0x1p-10f, 12582912.0f));
}

// Where rint(fl(S) / 1024) -- round_q10, or the fl(S) + 1.5 * 2^33 of the fast path -- can
// differ from OpenCV's float blend, for the exact integer sum S = sum v_k K_k < 2^26.  Below
// 2^24 both are exact.  From 2^24 on, each of OpenCV's four products and three partial sums
// is below 2^26 and rounds by at most 2 (half an ulp of 4), so its float sum s3 is within
// 4 * 2 + 3 * 2 = 14 of S, and fl(S) is within 2.  Two values within 14 of S = 1024 k + r
// round to the same multiple of 1024 unless the tie 1024 k + 512 lies within 14 of S: only
// pixels with S >= 2^24 and |r - 512| <= 14 need the float formula (33 of the 1024
// residues at kTieWindow = 16).
constexpr uint32_t kTieWindow = 16;  // >= the proven 14
__device__ __forceinline__ bool near_tie(uint32_t S) {
  return (S >> 24) != 0 && ((S - (512u - kTieWindow)) & 1023u) <= 2u * kTieWindow;
}

__device__ __forceinline__ uint32_t tap(const uint16_t* stile, int i) { return stile[i]; }

// Bits 11-15 of v in one v_bfe_u32 (a shift and a mask otherwise).  The builtin, not inline
// asm: the compiler pads the wait state a VALU write of a VGPR needs after a wider-than-8-byte
// store that reads it as data, but not around inline asm -- the round-4 inline-asm form landed
// right behind the RGB path's buffer_store_dwordx3 and overwrote its first data VGPR, an
// intermittent wrong pixel pair (tools/debug/store_hazard_scan.py checks the
// built library for that pattern).
__device__ __forceinline__ uint32_t bfe_11_5(uint32_t v) { return __builtin_amdgcn_ubfe(v, 11, 5); }

// The wave's count of lanes whose chunk (its dwords OR-ed into v) holds a value >= 16384.
__device__ __forceinline__ uint32_t bright_lanes(uint32_t v) {
  return __builtin_popcountll(__builtin_amdgcn_ballot_w64((v & 0xc000c000u) != 0));
}
__device__ __forceinline__ uint32_t bright_chunks(const uint4& v) { return bright_lanes(v.x | v.y | v.z | v.w); }

// Fast staged path (mode 3; W % 8 == 0, the near-identity maps of motion correction): the
// box is staged as C channel planes at a fixed LDS pitch, so the lower tap row and the other
// planes are immediate offsets of the upper tap, and the per-row source origins come from a
// per-frame table through scalar loads.  Boxes wider than kFastPitch or taller than kRows
// take the general staged path (mode 0).
// pixels: 128-px tile + up to ~8 deg / 6 % zoom (192: fewer bank conflicts, same time)
constexpr int kFastPitch = 144;
constexpr int kFastChunks = kFastPitch / 8;  // 16-byte chunks (8-pixel groups) per staged row
template <class Cfg, int C>
struct FastPlanes {
  static constexpr int kRows = (Cfg::kLdsElems - 8) / (C * kFastPitch);  // the last 16 bytes: per-wave flags
  static constexpr int kPlane = kRows * kFastPitch;                      // elements per channel plane
  static constexpr int kFlagWord = Cfg::kLdsElems / 2 - 4;               // uint32 index of the flags
  static_assert(C * kPlane <= 2 * kFlagWord, "planes overlap the flag words");
};

// word i of plane k of an 8-pixel group: elements C (2i) + k and C (2i + 1) + k of the
// interleaved group (dwords d[e / 2], halves e % 2), as one v_perm_b32
template <int C, int K, int I>
__device__ __forceinline__ uint32_t plane_word(const uint32_t (&d)[4 * C]) {
  constexpr int e0 = C * 2 * I + K, e1 = C * (2 * I + 1) + K;
  constexpr uint32_t sel = ((e0 & 1) ? 0x0302u : 0x0100u) | ((e1 & 1) ? 0x07060000u : 0x05040000u);
  return __builtin_amdgcn_perm(d[e1 / 2], d[e0 / 2], sel);
}

template <int C, int K>
__device__ __forceinline__ uint4 plane_piece(const uint32_t (&d)[4 * C]) {
  return make_uint4(plane_word<C, K, 0>(d), plane_word<C, K, 1>(d), plane_word<C, K, 2>(d), plane_word<C, K, 3>(d));
}

// Fast-path staging for C = 3 / 4 (round 4): issue() loads, land() stores and returns the wave's
// count of bright (>= 16384) groups.  The interleaved box is de-interleaved while it lands:
// each thread loads one 8-pixel group of a box row (C 16-byte chunks, 16-byte aligned relative
// to the frame because ax0 and W are multiples of 8, absolutely only when src is: kcmc.h) and
// writes C planar 16-byte pieces (v_perm_b32 pairs), one per channel plane, at the fixed pitch.  A pixel's taps then sit at the same offset in every plane
// (immediate offsets), so the coordinate work of a pixel is shared by its C channels, and each
// lane's C output dwords (pixels 2l, 2l+1) leave in ONE 12- / 16-byte store: a wave's store
// covers 768 / 1024 contiguous bytes of the row.  The general multi-channel path (mode 0) reads
// interleaved taps with per-channel addressing and stores C separate dwords per lane at a
// 12-byte lane stride (round 3: 148 VALU, 49 SALU, 25 LDS instructions per wave row at c4).
template <class Cfg, int C>
struct Fast : FastPlanes<Cfg, C> {
  static constexpr int kPasses = (Fast::kRows * kFastChunks + kThreads - 1) / kThreads;
  struct Loads {
    uint4 g[kPasses][C];
  };

  static __device__ __forceinline__ void issue(const uint16_t* __restrict__ S, const TilePlan& tp, int H, int W,
                                               int tid, Loads& l) {
    const int gpr = tp.pitch() >> 3, rows = tp.rows();
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
      const int q = tid + kThreads * k;
      const int r = q / kFastChunks, c = q - r * kFastChunks;
      const int gy = tp.sy0 + r, gx = tp.ax0 + 8 * c;
      const bool ok = r < rows && c < gpr && (unsigned)gx < (unsigned)W && (unsigned)gy < (unsigned)H;
#pragma unroll
      for (int j = 0; j < C; ++j) l.g[k][j] = make_uint4(0u, 0u, 0u, 0u);
      if (ok) {
        const uint4* src = reinterpret_cast<const uint4*>(S + ((size_t)gy * W + gx) * C);
#pragma unroll
        for (int j = 0; j < C; ++j) l.g[k][j] = src[j];
      }
    }
  }

  static __device__ __forceinline__ uint32_t land(uint16_t* stile, const TilePlan& tp, int tid, const Loads& l) {
    const int gpr = tp.pitch() >> 3, rows = tp.rows();
    uint32_t nb = 0;
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
      const int q = tid + kThreads * k;
      const int r = q / kFastChunks, c = q - r * kFastChunks;
      uint32_t d[4 * C], any = 0;  // the group's 8 C elements, two per dword
#pragma unroll
      for (int j = 0; j < C; ++j) {
        d[4 * j] = l.g[k][j].x;
        d[4 * j + 1] = l.g[k][j].y;
        d[4 * j + 2] = l.g[k][j].z;
        d[4 * j + 3] = l.g[k][j].w;
        any |= l.g[k][j].x | l.g[k][j].y | l.g[k][j].z | l.g[k][j].w;
      }
      nb += bright_lanes(any);
      if (r < rows && c < gpr) {
        uint4* dst = reinterpret_cast<uint4*>(stile + r * kFastPitch + 8 * c);
        dst[0] = plane_piece<C, 0>(d);
        dst[Fast::kPlane / 8] = plane_piece<C, 1>(d);
        dst[2 * Fast::kPlane / 8] = plane_piece<C, 2>(d);
        if constexpr (C == 4) dst[3 * Fast::kPlane / 8] = plane_piece<C, 3>(d);
      }
    }
    return nb;
  }
};

// Fast-path staging for one channel.  Thread tid owns chunk column c = tid % kFastChunks and
// the box rows r0 + kStep k (r0 = tid / kFastChunks, kStep = 14: 252 of the 256 threads), so
// the row-major LDS slot of pass k is 16 tid + an immediate, and the source byte offset of
// pass k is the thread's first offset plus k times a wave-uniform stride: one add per pass.
// The loads are raw buffer loads through one descriptor per tile, base = the frame,
// num_records = the bytes of the frame down to the box's last row; the hardware range check
// of voffset then returns the zeros of BORDER_CONSTANT for rows above the frame (the 32-bit
// offset wraps beyond 2^31 > num_records: H, W < 2^15, |row| <= 30000), for rows below it and
// for rows below the box (not fetched), and a row never reads the neighbouring frame.  The
// column test is paid once: a thread whose chunk is outside the box's pitch or the frame's
// columns (or one of the 4 spare threads) starts at offset 2^31, out of range for every pass.
// So the load passes hold no exec-mask branch, no zero-initialised registers and no 64-bit
// address arithmetic.  kPasses whole passes cover rows 0 .. kPasses * kStep - 1 (69); a box
// with more rows (the 71st, rare) stages the rest in a tail pass behind a wave-uniform branch.
template <class Cfg>
struct Fast<Cfg, 1> : FastPlanes<Cfg, 1> {
  static constexpr int kStep = kThreads / kFastChunks;               // box rows per pass (14)
  static constexpr int kUsed = kStep * kFastChunks;                  // staging threads (252)
  static constexpr int kPasses = Fast::kRows / kStep;                // whole passes (5)
  static constexpr int kTailRows = Fast::kRows - kPasses * kStep;    // rows of the tail pass (1)
  static_assert(kTailRows < kStep && kTailRows * kFastChunks <= kThreads, "one tail pass");
  struct Loads {
    uint4 chunk[kPasses];
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff;  // byte offset of the thread's chunk in box row r0 (2^31: never in range)
    uint32_t step;  // bytes of kStep frame rows (wave-uniform)
    __device__ __forceinline__ uint4 load(int k) const {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + (uint32_t)k * step, 0, 0);
      return make_uint4(v[0], v[1], v[2], v[3]);
    }
  };

  static __device__ __forceinline__ void issue(const uint16_t* __restrict__ S, const TilePlan& tp, int H, int W,
                                               int tid, Loads& l) {
    const int r0 = tid / kFastChunks, c = tid - r0 * kFastChunks;
    const int gx = tp.ax0 + 8 * c;
    const bool col_ok = c < (tp.pitch() >> 3) && (unsigned)gx < (unsigned)W && tid < kUsed;
    // |sy0 + r0| and W fit 24 bits; the byte offset of a row above the frame wraps (see above)
    l.voff = col_ok ? 2u * (uint32_t)(__mul24(tp.sy0 + r0, W) + gx) : 0x80000000u;
    l.step = 2u * kStep * (uint32_t)W;
    l.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(S), 0, 2 * min(H, tp.sy0 + tp.rows()) * W,
                                               0x00020000);
#pragma unroll
    for (int k = 0; k < kPasses; ++k) l.chunk[k] = l.load(k);
  }

  // Lands the passes in LDS and returns the wave's count of bright (>= 16384) chunks.  Rows
  // below the box and chunks right of its pitch land as zeros (never read).
  static __device__ __forceinline__ uint32_t land(uint16_t* stile, const TilePlan& tp, int tid, const Loads& l) {
    uint4* slot = reinterpret_cast<uint4*>(stile) + tid;
    uint32_t nb = 0;
    if (tid < kUsed) {
#pragma unroll
      for (int k = 0; k < kPasses; ++k) slot[k * kUsed] = l.chunk[k];
    }
#pragma unroll
    for (int k = 0; k < kPasses; ++k) nb += bright_chunks(l.chunk[k]);
    if (kTailRows > 0 && tp.rows() > kPasses * kStep) {  // wave-uniform
      const uint4 t = l.load(kPasses);  // rows past the box are out of range: zeros
      if (tid < kTailRows * kFastChunks) slot[kPasses * kUsed] = t;
      nb += bright_chunks(t);
    }
    return nb;
  }
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// OpenCV's float evaluation of remapBilinear's blend, ((v00 w0 + v01 w1) + v10 w2) + v11 w3
// with separately rounded products and w_k = K_k / 1024 exactly (the 2^-10 scaling commutes
// with every rounding), then cvRound: packed fp32 over the lane's two pixels; returns the
// two results in the low 16 bits of each float.
__device__ __forceinline__ f32x2 blend_float2(const uint32_t (&v)[2][4], const uint32_t (&fx)[2],
                                              const uint32_t (&fy)[2]) {
  const f32x2 fxf = {(float)fx[0], (float)fx[1]}, fyf = {(float)fy[0], (float)fy[1]};
  const f32x2 axf = 32.0f - fxf, ayf = 32.0f - fyf;
  const f32x2 t0 = {(float)v[0][0], (float)v[1][0]}, t1 = {(float)v[0][1], (float)v[1][1]};
  const f32x2 t2 = {(float)v[0][2], (float)v[1][2]}, t3 = {(float)v[0][3], (float)v[1][3]};
  const f32x2 sum = ((t0 * (ayf * axf) + t1 * (ayf * fxf)) + t2 * (fyf * axf)) + t3 * (fyf * fxf);
  // cvRound(sum / 1024): one rounding of the exact sum * 2^-10 + 1.5 * 2^23
  f32x2 q;
  q[0] = __builtin_fmaf(sum[0], 0x1p-10f, 0x1.8p23f);
  q[1] = __builtin_fmaf(sum[1], 0x1p-10f, 0x1.8p23f);
  return q;
}

// Blend of a mode-3 tile, chosen once per tile from its staged box:
enum FastBlend {
  kDark = 0,    // every staged value < 16384: S = sum v_k K_k < 2^24, so the exact separable
                // integer evaluation of output_rows IS OpenCV's float result; no range check
  kMixed = 1,   // few bright values: the integer blend for every row; the rows where some
                // pixel's sum is near_tie (wave-uniform) are made again with blend_float2
  kBright = 2,  // more bright values: blend_float2 throughout
};
// VALU instructions per wave row (counted in the gfx950 code): kDark 32; kMixed 34, 44 when
// a sum is >= 2^24, and about 50 more when the row is made again; kBright 44.  So kMixed
// pays while (rows made again) < (rows with no bright sum) / 5.  With b bright chunks in a
// full 17 x 58 box: isolated hot pixels (one per chunk, <= 4 bright sums each, ~3 % of
// them near_tie) touch 1 - exp(-2 b / 58) of the rows and remake about 0.002 b of them --
// break-even near b = 35; a 32-px wide blob r rows high (b = 4 r) touches r + 1 rows and
// remakes 0.67 r -- break-even near r = 15, b = 60.  Hence a twentieth of the box (49
// chunks).  An earlier per-row choice by a test of the eight taps (41 / 53 VALU), kept
// for boxes between that and a third bright, measured slower than kBright there: bright
// taps then touch most rows (lab figures: DESIGN 4 K3).
constexpr int kBrightShare = 20;  // bright chunks * kBrightShare > box chunks -> kBright

// Output rows of a mode-3 tile over its C planes, with the per-row overheads of output_rows
// removed: row origins are scalar, the lower tap row and the other planes are immediate LDS
// offsets (the coordinate work of a pixel is shared by its channels), the store is one b32 /
// b96 / b128 buffer store per lane and row with the row offset in soffset.  The blend is
// decided once per tile and the rows to make again over every channel's sums.
// INTERIOR: the tile lies inside the frame (every row exists, every lane's pixel pair is
// stored), so the rows carry no bounds test and no store mask.
template <class Cfg, int C, int BLEND, bool INTERIOR>
__device__ __forceinline__ void fast_rows(const uint16_t* stile, const int2* __restrict__ rt, int ox, int oy,
                                          uint16_t* __restrict__ Dst, int H, int W, int xb, int yb, int wave, int lane,
                                          const int (&ad)[2], const int (&bd)[2]) {
  static_assert(C == 1 || C == 3 || C == 4, "planar fast path: gray / RGB / RGBA");
  constexpr int kPlane = Fast<Cfg, C>::kPlane;
  const uint32_t xoff = 2u * C * (uint32_t)(xb + 2 * lane);  // byte offset of the lane's pixel pair
  const bool store_ok = INTERIOR || xb + 2 * lane + 2 <= W;   // W is a multiple of 8 here
  const __amdgpu_buffer_rsrc_t dst_rsrc = __builtin_amdgcn_make_buffer_rsrc(Dst, 0, 2 * C * H * W, 0x00020000);
  int2 org[Cfg::kTileH / 4];  // all row origins up front (scalar loads; the table is padded)
#pragma unroll
  for (int i = 0; i < Cfg::kTileH / 4; ++i) org[i] = rt[i];
  // Box-relative coordinates are carried scaled by 2^6: the tap's integer column / row
  // (< 2^8 / 2^7 here) is then the high half of the word and the 1/32 fraction bits 11-15.
  // One v_perm packs (column, row) as two u16 and one v_dot2_u32_u16 with (2, 2 * pitch)
  // gives the tap's LDS byte offset (4 VALU per pixel fewer than shifts + mad).
  // Exact: |X| < 2^18 before scaling, and two's-complement wrap-around commutes with << 6.
  uint32_t ad6[2], bd6[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    ad6[p] = (uint32_t)ad[p] << 6;
    bd6[p] = (uint32_t)bd[p] << 6;
  }
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 pitch2 = {(unsigned short)2, (unsigned short)(2 * kFastPitch)};
  const char* sbytes = reinterpret_cast<const char*>(stile);
  // the lane's two pixels of a row with the scaled origin (X0, Y0): C x four taps, fractions
  auto row_taps = [&](uint32_t X0, uint32_t Y0, uint32_t(&v)[C][2][4], uint32_t(&fx)[2], uint32_t(&fy)[2]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const uint32_t tX = X0 + ad6[p], tY = Y0 + bd6[p];
      fx[p] = bfe_11_5(tX);
      fy[p] = bfe_11_5(tY);
      const uint32_t cr = __builtin_amdgcn_perm(tY, tX, 0x07060302u);  // (column, row) as u16 x 2
      const uint32_t off = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, cr), pitch2, 0u, false);
      const uint16_t* t = reinterpret_cast<const uint16_t*>(sbytes + off);
#pragma unroll
      for (int k = 0; k < C; ++k) {
        v[k][p][0] = t[k * kPlane];
        v[k][p][1] = t[k * kPlane + 1];
        v[k][p][2] = t[k * kPlane + kFastPitch];
        v[k][p][3] = t[k * kPlane + kFastPitch + 1];
      }
    }
  };
  // the lane's 2 C channel values in interleaved order, two per dword
  // (aux 2 = nontemporal: the aligned frame is written once and not re-read here)
  auto store_row = [&](const f32x2(&q)[C], int y) {
#define KCMC_Q(px, ch) __float_as_uint(q[ch][px])
    if constexpr (C == 1) {
      const uint32_t o = __builtin_amdgcn_perm(KCMC_Q(1, 0), KCMC_Q(0, 0), 0x05040100u);
      if (store_ok) __builtin_amdgcn_raw_buffer_store_b32(o, dst_rsrc, xoff, 2 * C * y * W, 2);
    } else if constexpr (C == 3) {
      typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
      const u32x3 o = {__builtin_amdgcn_perm(KCMC_Q(0, 1), KCMC_Q(0, 0), 0x05040100u),
                       __builtin_amdgcn_perm(KCMC_Q(1, 0), KCMC_Q(0, 2), 0x05040100u),
                       __builtin_amdgcn_perm(KCMC_Q(1, 2), KCMC_Q(1, 1), 0x05040100u)};
      if (store_ok) __builtin_amdgcn_raw_buffer_store_b96(o, dst_rsrc, xoff, 2 * C * y * W, 2);
    } else {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 o = {__builtin_amdgcn_perm(KCMC_Q(0, 1), KCMC_Q(0, 0), 0x05040100u),
                       __builtin_amdgcn_perm(KCMC_Q(0, 3), KCMC_Q(0, 2), 0x05040100u),
                       __builtin_amdgcn_perm(KCMC_Q(1, 1), KCMC_Q(1, 0), 0x05040100u),
                       __builtin_amdgcn_perm(KCMC_Q(1, 3), KCMC_Q(1, 2), 0x05040100u)};
      if (store_ok) __builtin_amdgcn_raw_buffer_store_b128(o, dst_rsrc, xoff, 2 * C * y * W, 2);
    }
#undef KCMC_Q
  };
  uint32_t redo = 0;  // kMixed: bit i = the wave's row i waits for the float blend (scalar)
#pragma unroll
  for (int i = 0; i < Cfg::kTileH / 4; ++i) {
    const int y = yb + wave + 4 * i;  // wave-uniform
    if (!INTERIOR && y >= H) break;
    const uint32_t X0 = (uint32_t)(org[i].x - ox) << 6, Y0 = (uint32_t)(org[i].y - oy) << 6;  // scalar
    uint32_t v[C][2][4], fx[2], fy[2];
    row_taps(X0, Y0, v, fx, fy);
    f32x2 q[C];
    if constexpr (BLEND == kBright) {
#pragma unroll
      for (int k = 0; k < C; ++k) q[k] = blend_float2(v[k], fx, fy);
    } else {
      uint32_t Sp[C][2], hi = 0;
#pragma unroll
      for (int k = 0; k < C; ++k) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const uint32_t ax = 32 - fx[p], ay = 32 - fy[p];
          uint32_t h0 = __umul24(v[k][p][0], ax) + __umul24(v[k][p][1], fx[p]);
          uint32_t h1 = __umul24(v[k][p][2], ax) + __umul24(v[k][p][3], fx[p]);
          asm volatile("" : "+v"(h0), "+v"(h1));  // keep the separable form (see output_rows)
          Sp[k][p] = __umul24(h0, ay) + __umul24(h1, fy[p]);
          hi |= Sp[k][p];
          q[k][p] = (float)Sp[k][p];
        }
        // rint(fl(S) / 1024) in the low bits: fl(S) + 1.5 * 2^33 rounds (half to even) to a
        // multiple of 1024, the float's unit in the last place there
        q[k] += 0x1.8p33f;
      }
      if constexpr (BLEND == kMixed) {
        // wave-uniform, two levels over every channel's sums: rows with no sum >= 2^24 (most)
        // pay one OR and one compare; of the others only those with a sum near a rounding tie
        // are left out here and made by the float loop below (the row loop itself stays
        // branch-lean)
        if (__builtin_amdgcn_ballot_w64((hi >> 24) != 0) != 0) {
          int tie = 0;
#pragma unroll
          for (int k = 0; k < C; ++k) tie |= (int)near_tie(Sp[k][0]) | (int)near_tie(Sp[k][1]);
          if (__builtin_amdgcn_ballot_w64(tie != 0) != 0) {
            redo |= 1u << i;
            continue;
          }
        }
      }
    }
    store_row(q, y);
  }
  if constexpr (BLEND == kMixed) {
    while (redo) {  // the rows left out above (each written once, here): OpenCV's float blend
      const int i = __builtin_ctz(redo);
      redo &= redo - 1;
      const int2 o = rt[i];
      uint32_t v[C][2][4], fx[2], fy[2];
      row_taps((uint32_t)(o.x - ox) << 6, (uint32_t)(o.y - oy) << 6, v, fx, fy);
      f32x2 q[C];
#pragma unroll
      for (int k = 0; k < C; ++k) q[k] = blend_float2(v[k], fx, fy);
      store_row(q, yb + wave + 4 * i);
    }
  }
}

// Debug instrument (tools/debug/warp_sentinel.sh builds it; never the product library): the
// whole LDS array is filled with 0xFFFF before a tile stages its box, so that a tap read
// outside the staged rows / columns returns a deterministic wrong value (65535) instead of
// whatever an earlier workgroup left in that LDS, and the bit-exact tests catch it.
#ifdef KCMC_WARP_SENTINEL
template <int ELEMS>
__device__ __forceinline__ void lds_sentinel(uint16_t* stile, int tid) {
  for (int i = tid; i < ELEMS / 2; i += kThreads) reinterpret_cast<uint32_t*>(stile)[i] = 0xffffffffu;
  __syncthreads();
}
#define KCMC_LDS_SENTINEL(stile, elems, tid) lds_sentinel<elems>(stile, tid)
#else
#define KCMC_LDS_SENTINEL(stile, elems, tid) ((void)0)
#endif

// Output rows of one tile on one path (0: LDS-staged box, 1: zeros, 2: direct gather).
// Wave w makes rows w, w + 4, ...; lane l pixels x = xb + 2l, xb + 2l + 1.  ad / bd: the
// lane's column deltas (lane_columns); X0v / Y0v: in lane i the origins of the wave's i-th
// row, box-relative for a staged tile (row_origins).
template <class Cfg, int C, int MODE>
__device__ __forceinline__ void output_rows(const uint16_t* stile, const TilePlan& tp, const uint16_t* __restrict__ S,
                                            uint16_t* __restrict__ Dst, int H, int W, const TileId& t,
                                            const int (&ad)[2], const int (&bd)[2], int X0v, int Y0v) {
  const int x = t.xb + 2 * t.lane, pitch = tp.pitch();
  const bool pair_store = C == 1 && (W & 1) == 0 && x + 2 <= W;
#pragma unroll
  for (int i = 0; i < Cfg::kTileH / 4; ++i) {
    const int y = t.yb + t.wave + 4 * i;  // wave-uniform
    if (y >= H) break;
    const int X0 = __builtin_amdgcn_readlane(X0v, i), Y0 = __builtin_amdgcn_readlane(Y0v, i);
    uint16_t o[2 * C];
    if (MODE == 0) {
      // Box-relative taps.  The blend is first evaluated exactly in integers,
      // S = ay*(v00*ax + v01*fx) + fy*(v10*ax + v11*fx) = sum v_k*K_k: while S < 2^24
      // every product and partial sum of OpenCV's float evaluation is an integer below
      // 2^24 as well, hence exact, and its result is rint(S/1024).  Of the pixels with
      // S >= 2^24 (bright: taps beyond 14 bits) only those near a rounding tie (near_tie)
      // take the float-faithful blend.
      uint32_t Sx[2 * C], hi = 0, fx[2], fy[2], li[2], v[2][C][4];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int tX = X0 + ad[p], tY = Y0 + bd[p];
        fx[p] = (tX >> 5) & 31;
        fy[p] = (tY >> 5) & 31;
        li[p] = __umul24((uint32_t)(tY >> 10), (uint32_t)pitch) + (uint32_t)(tX >> 10);
      }
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < C; ++k) {
          const int i00 = li[p] * C + k, i10 = i00 + pitch * C;
          v[p][k][0] = tap(stile, i00);
          v[p][k][1] = tap(stile, i00 + C);
          v[p][k][2] = tap(stile, i10);
          v[p][k][3] = tap(stile, i10 + C);
        }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const uint32_t ax = 32 - fx[p], ay = 32 - fy[p];
#pragma unroll
        for (int k = 0; k < C; ++k) {
          uint32_t h0 = __umul24(v[p][k][0], ax) + __umul24(v[p][k][1], fx[p]);
          uint32_t h1 = __umul24(v[p][k][2], ax) + __umul24(v[p][k][3], fx[p]);
          // keep the separable form (the compiler would otherwise expand it into the
          // four weight products, three more multiplies)
          asm volatile("" : "+v"(h0), "+v"(h1));
          const uint32_t Sv = __umul24(h0, ay) + __umul24(h1, fy[p]);
          Sx[p * C + k] = Sv;
          hi |= Sv;
          o[p * C + k] = round_q10(Sv);
        }
      }
      if (hi >> 24) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int k = 0; k < C; ++k)
            if (near_tie(Sx[p * C + k]))
              o[p * C + k] = blend_int(v[p][k][0], v[p][k][1], v[p][k][2], v[p][k][3], fx[p], fy[p]);
      }
    } else {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int X = (X0 + ad[p]) >> 5, Y = (Y0 + bd[p]) >> 5;
        if (MODE == 1) {
#pragma unroll
          for (int k = 0; k < C; ++k) o[p * C + k] = 0;
        } else {
          bilinear_px<C>(S, H, W, X, Y, o + p * C);
        }
      }
    }
    uint16_t* drow = Dst + ((size_t)y * W + x) * C;
    if (pair_store) {
      // streaming store: the aligned frame is written once and not re-read by this kernel
      __builtin_nontemporal_store((uint32_t)o[0] | ((uint32_t)o[1] << 16), reinterpret_cast<uint32_t*>(drow));
    } else if (C >= 3 && x + 2 <= W) {
      // two whole pixels: 6 (RGB) or 8 (RGBA) channels as 4-byte stores.  x is even, but drow
      // is 4-byte aligned only where (y W + x) C is even and Dst itself is: on the odd rows
      // of an RGB frame with odd W, or behind a Dst 2 bytes off the grid (as the pair store
      // above), these are unaligned global stores, which gfx950 performs (kcmc.h, K3)
#pragma unroll
      for (int k = 0; k < C; ++k)
        __builtin_nontemporal_store((uint32_t)o[2 * k] | ((uint32_t)o[2 * k + 1] << 16),
                                    reinterpret_cast<uint32_t*>(drow) + k);
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (x + q < W)
#pragma unroll
          for (int k = 0; k < C; ++k) drow[q * C + k] = o[q * C + k];
    }
  }
}

// One row loop per path (a path-uniform branch inside the loop makes the compiler drain
// the previous rows' stores with s_waitcnt vmcnt(0) every row).  A function of its own: with
// the three calls written in the kernel, the RGB / RGBA edge stores keep a dead second pixel
// (twice the 2-byte stores, two more VGPRs; profiles/warp_linear_shared.md).
template <class Cfg, int C>
__device__ __forceinline__ void output_tile(const uint16_t* stile, const TilePlan& tp, const uint16_t* __restrict__ S,
                                            uint16_t* __restrict__ Dst, int H, int W, const TileId& t,
                                            const int (&ad)[2], const int (&bd)[2], int X0v, int Y0v) {
  if (tp.mode == 0)
    output_rows<Cfg, C, 0>(stile, tp, S, Dst, H, W, t, ad, bd, X0v, Y0v);
  else if (tp.mode == 1)
    output_rows<Cfg, C, 1>(stile, tp, S, Dst, H, W, t, ad, bd, X0v, Y0v);
  else
    output_rows<Cfg, C, 2>(stile, tp, S, Dst, H, W, t, ad, bd, X0v, Y0v);
}

// (xcd_remap: kcmc_internal.h)

// ------------------------------------------------------------------------- plan
// One thread per tile (tile id = (f * nty + ty) * ntx + tx): the fp64 map inversion
// (written once per frame to minv) and the tile's source box.
// Also the frame's row-origin table for the fast path: rowtab[f][y & 3][y >> 2] =
// (X0(y), Y0(y)) = (cvRound((M1*y + M2)*1024) + 16, cvRound((M4*y + M5)*1024) + 16), so
// that a wave's rows y = yb + wave + 4i are consecutive entries; the tiles of a tile row
// share its rows.
template <int C, class Cfg>
__global__ __launch_bounds__(256) void warp_plan_kernel(const double* __restrict__ Mall, int n_frames, int H, int W,
                                                        int inverse_map, int ntx, int nty,
                                                        TilePlan* __restrict__ plan, double* __restrict__ minv,
                                                        int2* __restrict__ rowtab, int hq) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)ntx * nty * n_frames) return;
  const PlanTile p = plan_tile<Cfg::kTileH>(t, Mall, inverse_map, H, W, ntx, nty, minv);
  TilePlan b = source_box<Cfg, C>(p, H, W);
  // C == 1, 2 H W < 2^31: the frame fits the range of the fast path's buffer descriptors
  if ((W & 7) == 0 && (C > 1 || 2ll * H * W < (1ll << 31)) && b.mode == 0 && b.pitch() <= kFastPitch &&
      b.rows() <= Fast<Cfg, C>::kRows)
    b.mode = 3;
  if (map_has_nan(p.M, 6)) b.mode = 1;  // a NaN map (a frame RANSAC could not fit) warps to zeros
  plan[t] = b;
  for (int j = p.xb / kTileW; j < Cfg::kTileH && p.yb + j < H; j += ntx) {
    const int y = p.yb + j;
    rowtab[((size_t)p.f * 4 + (y & 3)) * hq + (y >> 2)] =
        make_int2(cv_round((p.M[1] * y + p.M[2]) * 1024) + 16, cv_round((p.M[4] * y + p.M[5]) * 1024) + 16);
  }
}

// ------------------------------------------------------------ one tile per workgroup
// no-unaligned-access-mode: keeps the two adjacent 16-bit tap reads from being fused
// into one 4-byte LDS read at a 2-byte-aligned address, which the LDS replays (1.75x
// slower kernel, measured in tools/warp_lab).
template <int C, class Cfg = BlockCfg>
__global__ __launch_bounds__(kThreads) __attribute__((target("no-unaligned-access-mode"))) void warp_affine_u16_kernel(
    const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, const TilePlan* __restrict__ plan,
    const double* __restrict__ minv, const int2* __restrict__ rowtab, int hq, int H, int W) {
  __shared__ __attribute__((aligned(16))) uint16_t stile[Cfg::kLdsElems];
  const TileId t = tile_decode<Cfg::kTileH>();
  const int tid = threadIdx.x;
  const uint16_t* S = src + (size_t)t.f * H * W * C;
  uint16_t* Dst = dst + (size_t)t.f * H * W * C;
  const double* M = minv + 6 * (size_t)t.f;

  const TilePlan tp = plan[t.tile];
  KCMC_LDS_SENTINEL(stile, Cfg::kLdsElems, tid);
  int ad[2], bd[2];
  if (tp.mode == 3) {
    using F = Fast<Cfg, C>;
    typename F::Loads loads;
    F::issue(S, tp, H, W, tid, loads);  // loads first
    lane_columns(M, t.xb, t.lane, W, ad, bd);
    // the box lands; its bright chunks are counted per wave into the flag words
    const uint32_t nb = F::land(stile, tp, tid, loads);
    uint32_t* flags = reinterpret_cast<uint32_t*>(stile) + F::kFlagWord;
    if (t.lane == 0) flags[t.wave] = nb;
    __syncthreads();
    const uint4 fl = *reinterpret_cast<const uint4*>(flags);
    const uint32_t bright = fl.x + fl.y + fl.z + fl.w;
    const int2* rt = rowtab + ((size_t)t.f * 4 + t.wave) * hq + (t.yb >> 2);
    const int ox = tp.ax0 * 1024, oy = tp.sy0 * 1024;
    const bool interior = t.yb + Cfg::kTileH <= H && t.xb + kTileW <= W;
#define KCMC_FAST_ROWS(blend, inside) \
  fast_rows<Cfg, C, blend, inside>(stile, rt, ox, oy, Dst, H, W, t.xb, t.yb, t.wave, t.lane, ad, bd)
    if (bright == 0) {
      if (interior)
        KCMC_FAST_ROWS(kDark, true);
      else
        KCMC_FAST_ROWS(kDark, false);
    } else if ((int)bright * kBrightShare <= tp.rows() * (tp.pitch() >> 3)) {
      if (interior)
        KCMC_FAST_ROWS(kMixed, true);
      else
        KCMC_FAST_ROWS(kMixed, false);
    } else {
      KCMC_FAST_ROWS(kBright, false);
    }
#undef KCMC_FAST_ROWS
    return;
  }
  BoxLoads<Cfg, C> loads;
  box_issue<Cfg, C>(S, tp, H, W, loads);  // loads first
  int X0v, Y0v;  // overlaps the loads
  lane_columns(M, t.xb, t.lane, W, ad, bd);
  row_origins<Cfg::kTileH>(M, t, tp, X0v, Y0v);
  box_land<Cfg, C>(stile, S, tp, H, W, loads);
  __syncthreads();
  output_tile<Cfg, C>(stile, tp, S, Dst, H, W, t, ad, bd, X0v, Y0v);
}

// ================================================================ warpPerspective
// cv2.warpPerspective(frame, H, (W, H), INTER_LINEAR), BORDER_CONSTANT 0 -- the warp of
// the homography extension (BASELINE config 5; the reference only calls warpAffine).
// OpenCV classic path: invert(M) (closed-form 3x3, core/src/lapack.cpp) unless
// WARP_INVERSE_MAP, then WarpPerspectiveInvoker (imgwarp.cpp) per block of bw0 columns:
//   X0 = M0*xo + M1*y + M2, Y0 = M3*xo + M4*y + M5, W0 = M6*xo + M7*y + M8  (xo = block's
//   first column, x1 = x - xo), W = W0 + M6*x1, W = W ? 32/W : 0,
//   X = cvRound(clamp((X0 + M0*x1)*W)), Y likewise -> 1/32-px coordinates,
// and the same remapBilinear blend as warpAffine.  The coordinates are not separable,
// so each pixel evaluates them in fp64; the tile machinery (plan, LDS-staged box,
// exact integer blend, direct gather, zeros) is the affine kernel's.

__device__ __forceinline__ void invert_perspective(const double* S, double* M) {
  double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) +
             S[2] * (S[3] * S[7] - S[4] * S[6]);
  if (d == 0.0) {
    for (int k = 0; k < 9; ++k) M[k] = 0.0;
    return;
  }
  d = 1. / d;
  M[0] = (S[4] * S[8] - S[5] * S[7]) * d;
  M[1] = (S[2] * S[7] - S[1] * S[8]) * d;
  M[2] = (S[1] * S[5] - S[2] * S[4]) * d;
  M[3] = (S[5] * S[6] - S[3] * S[8]) * d;
  M[4] = (S[0] * S[8] - S[2] * S[6]) * d;
  M[5] = (S[2] * S[3] - S[0] * S[5]) * d;
  M[6] = (S[3] * S[7] - S[4] * S[6]) * d;
  M[7] = (S[1] * S[6] - S[0] * S[7]) * d;
  M[8] = (S[0] * S[4] - S[1] * S[3]) * d;
}

// Per-tile row table of the perspective warp (round 4): WarpPerspectiveInvoker's per-(row,
// block) values X0 = M0 xo + M1 y + M2, Y0 = M3 xo + M4 y + M5, W0 = M6 xo + M7 y + M8 for
// the tile's kTileH rows and its two 64-column blocks (bw0 = 64 for every frame with
// H >= 16 and W >= 64), computed once per workgroup into the last bytes of the LDS budget
// instead of by every lane for every row (9 of a row's 39 fp64 operations per lane); the
// staged box gets the budget minus the table.
template <class Cfg>
struct PerspTab {
  static constexpr int kEntries = Cfg::kTileH * 2;                  // (row, block)
  static constexpr int kElems = kEntries * 3 * 4;                   // u16 elements of 3 doubles each
  static constexpr int kFlagWord = Cfg::kLdsElems / 2 - 4;          // the last 16 bytes: per-wave flags
  static constexpr int kBoxElems = Cfg::kLdsElems - 8 - kElems;     // the staged box's budget
  static_assert((kBoxElems * 2) % 8 == 0, "table alignment");
};

// Source box of a tile: when the projective denominator has one sign over the tile,
// the tile's image is the convex hull of its corner images; one pixel of margin on each
// side absorbs the 1/32-px rounding and the second tap.  Otherwise: direct gather.
template <class Cfg, int C>
__device__ __forceinline__ TilePlan persp_box(const double* M, int xb, int yb, int H, int W) {
  const int xl = min(xb + kTileW, W) - 1, yl = min(yb + Cfg::kTileH, H) - 1;
  const int cx[4] = {xb, xl, xb, xl}, cy[4] = {yb, yb, yl, yl};
  double mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;
  bool pos = true, neg = true, wrange = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double w = M[6] * cx[k] + M[7] * cy[k] + M[8];
    pos = pos && w > 0.0;
    neg = neg && w < 0.0;
    // the staged path's division assumes 2^-60 <= |w| <= 2^60 (w is linear over the tile:
    // its extremes are at the corners; a factor 2^4 of margin for the rounding)
    wrange = wrange && fabs(w) >= 0x1p-56 && fabs(w) <= 0x1p56;
    const double sx = (M[0] * cx[k] + M[1] * cy[k] + M[2]) / w;
    const double sy = (M[3] * cx[k] + M[4] * cy[k] + M[5]) / w;
    mnx = fmin(mnx, sx);
    mxx = fmax(mxx, sx);
    mny = fmin(mny, sy);
    mxy = fmax(mxy, sy);
  }
  const double lim = 30000.0;  // keep clear of saturate_cast<short> on coordinates
  if (!(pos || neg) || !(mnx > -lim && mxx < lim && mny > -lim && mxy < lim)) return TilePlan{2, 0, 0, 0};
  return box_plan<Cfg, C>((long long)floor(mnx) - 1, (long long)floor(mxx) + 2, (long long)floor(mny) - 1,
                          (long long)floor(mxy) + 2, H, W, true, wrange, PerspTab<Cfg>::kBoxElems);
}

template <int C, class Cfg>
__global__ __launch_bounds__(256) void persp_plan_kernel(const double* __restrict__ Mall, int n_frames, int H, int W,
                                                         int inverse_map, int ntx, int nty, TilePlan* __restrict__ plan,
                                                         double* __restrict__ minv) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)ntx * nty * n_frames) return;
  const int f = (int)(t / (ntx * nty)), t2 = (int)(t - (long long)f * ntx * nty);
  const int xb = (t2 % ntx) * kTileW, yb = (t2 / ntx) * Cfg::kTileH;
  double M[9];
  if (inverse_map) {
    for (int k = 0; k < 9; ++k) M[k] = Mall[9 * (size_t)f + k];
  } else {
    invert_perspective(Mall + 9 * (size_t)f, M);
  }
  if (t2 == 0)
    for (int k = 0; k < 9; ++k) minv[9 * (size_t)f + k] = M[k];
  TilePlan b = persp_box<Cfg, C>(M, xb, yb, H, W);
  if (map_has_nan(M, 9)) b.mode = 1;  // a NaN map (a frame RANSAC could not fit) warps to zeros
  plan[t] = b;
}

// remapBilinear's blend of four taps: exact integer evaluation, with the float-faithful
// re-blend for sums >= 2^24 near a rounding tie (near_tie; see output_rows).
__device__ __forceinline__ uint16_t blend_exact(uint32_t v00, uint32_t v01, uint32_t v10, uint32_t v11, int fx,
                                                int fy) {
  const uint32_t ax = 32 - fx, ay = 32 - fy;
  uint32_t h0 = __umul24(v00, ax) + __umul24(v01, (uint32_t)fx);
  uint32_t h1 = __umul24(v10, ax) + __umul24(v11, (uint32_t)fx);
  asm volatile("" : "+v"(h0), "+v"(h1));
  const uint32_t Sv = __umul24(h0, ay) + __umul24(h1, (uint32_t)fy);
  uint16_t r = round_q10(Sv);
  if (near_tie(Sv)) r = blend_int(v00, v01, v10, v11, fx, fy);
  return r;
}

// WarpPerspectiveInvoker's fixed-point source coordinate of an output pixel from its
// per-(block, row) values X0, Y0, W0 (xo = the first column of the pixel's bw0-wide block)
// and the column's products M0 x1, M3 x1, M6 x1 (x1 = x - xo) -- the same values OpenCV
// computes, so the result is unchanged: W = W0 + M6 x1, W = W ? 32/W : 0,
// X = cvRound(clamp((X0 + M0 x1) W)), Y likewise.  IN_RANGE: the tile's plan has bounded
// every source coordinate of the tile within +-30000 px (a staged box), so OpenCV's clamp
// to [INT_MIN, INT_MAX] is the identity and is left out.
// 32 / w correctly rounded for 2^-60 <= |w| <= 2^60: the compiler's IEEE division sequence
// without its range scaling (v_div_scale leaves both operands unscaled in that range and
// v_div_fmas is then a plain fma) and without v_div_fixup (special values only): the same
// reciprocal, two Newton steps, quotient, residual and correction, so the same bits.
__device__ __forceinline__ double div32_in_range(double w) {
  double y = __builtin_amdgcn_rcp(w);
  double e = __builtin_fma(-w, y, 1.0);
  y = __builtin_fma(y, e, y);
  e = __builtin_fma(-w, y, 1.0);
  y = __builtin_fma(y, e, y);
  const double q = 32.0 * y;
  const double r = __builtin_fma(-w, q, 32.0);
  return __builtin_fma(r, y, q);
}

// rint(x) for |x| < 2^31 as the low word of x + 1.5 * 2^52 (one round-to-nearest-even add
// to an integer-ulp binade; two's complement for negative x)
__device__ __forceinline__ int rint_small(double x) {
  return (int)(uint32_t)__double_as_longlong(x + 0x1.8p52);
}

// The staged path's coordinates relative to the box origin (cx = 1.5 * 2^52 - 32 ax0,
// cy = 1.5 * 2^52 - 32 sy0): the low word of fl(fX) + cx is rint(fX) - 32 ax0, because the
// constant is an even integer in the binade of unit ulp (the add's tie-to-even is rint's).
__device__ __forceinline__ void persp_px_box(double X0, double Y0, double W0, double m0x1, double m3x1, double m6x1,
                                             double cx, double cy, uint32_t& X, uint32_t& Y) {
  const double w = div32_in_range(W0 + m6x1);
  X = (uint32_t)__double_as_longlong((X0 + m0x1) * w + cx);
  Y = (uint32_t)__double_as_longlong((Y0 + m3x1) * w + cy);
}

template <bool IN_RANGE>
__device__ __forceinline__ void persp_px(double X0, double Y0, double W0, double m0x1, double m3x1, double m6x1,
                                         int& X, int& Y) {
  double w = W0 + m6x1;
  if (IN_RANGE) {
    // staged tiles: the plan kept |w| within [2^-60, 2^60] and every coordinate within
    // +-30000 px, so the division needs no range handling and OpenCV's clamp to
    // [INT_MIN, INT_MAX] is the identity
    w = div32_in_range(w);
    X = rint_small((X0 + m0x1) * w);
    Y = rint_small((Y0 + m3x1) * w);
    return;
  }
  w = w != 0.0 ? 32.0 / w : 0.0;
  double fX = (X0 + m0x1) * w, fY = (Y0 + m3x1) * w;
  fX = fmax((double)INT_MIN, fmin((double)INT_MAX, fX));
  fY = fmax((double)INT_MIN, fmin((double)INT_MAX, fY));
  X = (int)__builtin_rint(fX);
  Y = (int)__builtin_rint(fY);
}

// DARK (MODE 0, C == 1): every staged value is < 16384, so the exact integer blend needs no
// range check (as kDark of the affine fast path).
template <class Cfg, int C, int MODE, bool TAB, bool DARK = false>
__device__ __forceinline__ void persp_rows(const uint16_t* stile, const TilePlan& tp, const uint16_t* __restrict__ S,
                                           uint16_t* __restrict__ Dst, const double* M, int H, int W, const TileId& t,
                                           int bw0, const double* ptab) {
  const int x = t.xb + 2 * t.lane, pitch = tp.pitch();
  const bool pair_store = C == 1 && (W & 1) == 0 && x + 2 <= W;
  int xo[2], x1[2], tb[2];
  double m0x1[2], m3x1[2], m6x1[2], dxo[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int xc = min(x + q, W - 1);  // columns past the edge reuse the last column's taps
    xo[q] = xc - xc % bw0;
    x1[q] = xc - xo[q];
    tb[q] = (xo[q] - t.xb) >> 6;  // TAB (bw0 == 64): the pixel's block of the tile (0 or 1)
    // row-invariant: the column products and the block origin (round 3: hoisted out of
    // the row loop, and X0 / Y0 / W0 evaluated once per row for the lane's pixel pair)
    m0x1[q] = M[0] * x1[q];
    m3x1[q] = M[3] * x1[q];
    m6x1[q] = M[6] * x1[q];
    dxo[q] = (double)xo[q];
  }
  const bool one_block = xo[0] == xo[1];  // the pair straddles a block edge only for odd bw0
  const double mx0 = M[0] * dxo[0], mx3 = M[3] * dxo[0], mx6 = M[6] * dxo[0];
  // MODE 0, C == 1: box-relative fixed-point taps; (column, row) packed as two u16 from the
  // coordinates shifted by 11 (bits 16+: the pixel, bits 11-15: the 1/32 fraction) and the
  // LDS byte offset as one v_dot2 with (2, 2 pitch) -- as fast_rows (the generic form costs a
  // quarter-rate v_mul_lo_u32 and two more subtractions per tap)
  const double cx = 0x1.8p52 - 32.0 * tp.ax0, cy = 0x1.8p52 - 32.0 * tp.sy0;
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 pitch2 = {(unsigned short)2, (unsigned short)(2 * pitch)};
  const char* sbytes = reinterpret_cast<const char*>(stile);
#pragma unroll
  for (int i = 0; i < Cfg::kTileH / 4; ++i) {
    const int y = t.yb + t.wave + 4 * i;  // wave-uniform
    if (y >= H) break;
    uint16_t o[2 * C];
    const double dy = (double)y;
    double X0[2], Y0[2], W0[2];
    if (TAB) {  // the workgroup's table (same expressions, evaluated once per (row, block))
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const double* e = ptab + 3 * (2 * (t.wave + 4 * i) + tb[p]);
        X0[p] = e[0];
        Y0[p] = e[1];
        W0[p] = e[2];
      }
    } else {
      X0[0] = mx0 + M[1] * dy + M[2];
      Y0[0] = mx3 + M[4] * dy + M[5];
      W0[0] = mx6 + M[7] * dy + M[8];
      X0[1] = X0[0];
      Y0[1] = Y0[0];
      W0[1] = W0[0];
      if (!one_block) {
        X0[1] = M[0] * dxo[1] + M[1] * dy + M[2];
        Y0[1] = M[3] * dxo[1] + M[4] * dy + M[5];
        W0[1] = M[6] * dxo[1] + M[7] * dy + M[8];
      }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if constexpr (MODE == 0 && C == 1) {
        uint32_t X, Y;
        persp_px_box(X0[p], Y0[p], W0[p], m0x1[p], m3x1[p], m6x1[p], cx, cy, X, Y);
        const uint32_t tX = X << 11, tY = Y << 11;
        const uint32_t cr = __builtin_amdgcn_perm(tY, tX, 0x07060302u);  // (column, row) as u16 x 2
        const uint32_t off = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, cr), pitch2, 0u, false);
        const uint16_t* tp0 = reinterpret_cast<const uint16_t*>(sbytes + off);
        const uint32_t fx = X & 31, fy = Y & 31;
        const uint32_t v00 = tp0[0], v01 = tp0[1], v10 = tp0[pitch], v11 = tp0[pitch + 1];
        if constexpr (DARK) {
          const uint32_t ax = 32 - fx, ay = 32 - fy;
          uint32_t h0 = __umul24(v00, ax) + __umul24(v01, fx);
          uint32_t h1 = __umul24(v10, ax) + __umul24(v11, fx);
          asm volatile("" : "+v"(h0), "+v"(h1));  // keep the separable form (see output_rows)
          o[p] = round_q10(__umul24(h0, ay) + __umul24(h1, fy));
        } else {
          o[p] = blend_exact(v00, v01, v10, v11, (int)fx, (int)fy);
        }
        continue;
      }
      int X, Y;
      persp_px<MODE == 0>(X0[p], Y0[p], W0[p], m0x1[p], m3x1[p], m6x1[p], X, Y);
      if (MODE == 0) {
        const int fx = X & 31, fy = Y & 31;
        const int li = (int)__umul24((uint32_t)((Y >> 5) - tp.sy0), (uint32_t)pitch) + ((X >> 5) - tp.ax0);
#pragma unroll
        for (int k = 0; k < C; ++k) {
          const int i00 = li * C + k, i10 = i00 + pitch * C;
          o[p * C + k] = blend_exact(tap(stile, i00), tap(stile, i00 + C), tap(stile, i10), tap(stile, i10 + C), fx, fy);
        }
      } else if (MODE == 1) {
#pragma unroll
        for (int k = 0; k < C; ++k) o[p * C + k] = 0;
      } else {
        bilinear_px<C>(S, H, W, X, Y, o + p * C);
      }
    }
    uint16_t* drow = Dst + ((size_t)y * W + x) * C;
    if (pair_store) {
      // streaming store: the aligned frame is written once and not re-read by this kernel
      __builtin_nontemporal_store((uint32_t)o[0] | ((uint32_t)o[1] << 16), reinterpret_cast<uint32_t*>(drow));
    } else if (C >= 3 && x + 2 <= W) {
      // two whole pixels: 6 (RGB) or 8 (RGBA) channels as 4-byte stores; unaligned on the odd
      // rows of an RGB frame with odd W and behind a Dst 2 bytes off the grid (see output_rows)
#pragma unroll
      for (int k = 0; k < C; ++k)
        __builtin_nontemporal_store((uint32_t)o[2 * k] | ((uint32_t)o[2 * k + 1] << 16),
                                    reinterpret_cast<uint32_t*>(drow) + k);
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (x + q < W)
#pragma unroll
          for (int k = 0; k < C; ++k) drow[q * C + k] = o[q * C + k];
    }
  }
}

template <int C, class Cfg = BlockCfg>
__global__ __launch_bounds__(kThreads) __attribute__((target("no-unaligned-access-mode"))) void
warp_perspective_u16_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst,
                            const TilePlan* __restrict__ plan, const double* __restrict__ minv, int H, int W, int bw0) {
  __shared__ __attribute__((aligned(16))) uint16_t stile[Cfg::kLdsElems];
  const TileId t = tile_decode<Cfg::kTileH>();
  const int tid = threadIdx.x;
  const uint16_t* S = src + (size_t)t.f * H * W * C;
  uint16_t* Dst = dst + (size_t)t.f * H * W * C;

  const TilePlan tp = plan[t.tile];
  KCMC_LDS_SENTINEL(stile, Cfg::kLdsElems, tid);
  BoxLoads<Cfg, C> loads;
  box_issue<Cfg, C>(S, tp, H, W, loads);
  double M[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = minv[9 * (size_t)t.f + k];
  double* ptab = reinterpret_cast<double*>(stile + PerspTab<Cfg>::kBoxElems);
  const bool tab = bw0 == 64 && tp.mode != 1;  // uniform
  if (tab) {
    for (int e = tid; e < PerspTab<Cfg>::kEntries; e += kThreads) {
      const double dy = (double)(t.yb + (e >> 1)), dxo = (double)(t.xb + 64 * (e & 1));
      ptab[3 * e] = M[0] * dxo + M[1] * dy + M[2];
      ptab[3 * e + 1] = M[3] * dxo + M[4] * dy + M[5];
      ptab[3 * e + 2] = M[6] * dxo + M[7] * dy + M[8];
    }
  }
  const bool count = C == 1 && (W & 7) == 0;  // one channel, 16-byte staging
  uint32_t* flags = reinterpret_cast<uint32_t*>(stile) + PerspTab<Cfg>::kFlagWord;
  if (tp.mode == 0) {
    box_land<Cfg, C>(stile, S, tp, H, W, loads);
    if (count) {  // the box's bright (>= 16384) chunks, counted per wave into the flag words
      uint32_t nb = 0;
#pragma unroll
      for (int k = 0; k < BoxLoads<Cfg, C>::kPasses; ++k) nb += bright_chunks(loads.chunk[k]);
      if (t.lane == 0) flags[t.wave] = nb;
    }
  }
  __syncthreads();
  if (tp.mode == 1)
    persp_rows<Cfg, C, 1, false>(stile, tp, S, Dst, M, H, W, t, bw0, ptab);
  else if (tab) {
    if (tp.mode == 0) {
      const uint4 fl = *reinterpret_cast<const uint4*>(flags);
      if (count && fl.x + fl.y + fl.z + fl.w == 0)
        persp_rows<Cfg, C, 0, true, true>(stile, tp, S, Dst, M, H, W, t, bw0, ptab);
      else
        persp_rows<Cfg, C, 0, true>(stile, tp, S, Dst, M, H, W, t, bw0, ptab);
    } else
      persp_rows<Cfg, C, 2, true>(stile, tp, S, Dst, M, H, W, t, bw0, ptab);
  } else if (tp.mode == 0) {
    persp_rows<Cfg, C, 0, false>(stile, tp, S, Dst, M, H, W, t, bw0, ptab);
  } else {
    persp_rows<Cfg, C, 2, false>(stile, tp, S, Dst, M, H, W, t, bw0, ptab);
  }
}

// ------------------------------------------------------------------------- host
// Row-origin table entries per (frame, y & 3): padded so that a wave's scalar loads of
// its kTileH / 4 entries stay inside the frame's block.
inline int rowtab_hq(int H) { return ceil_div(H, 4) + 16; }

// WarpPerspectiveInvoker's block width: bh0 = min(16, H), bw0 = min(1024 / bh0, W)
inline int persp_bw0(int H, int W) {
  const int bh0 = H < 16 ? H : 16;
  return 1024 / bh0 < W ? 1024 / bh0 : W;
}

// Tile grid and workspace layout of both warps: minv [F, n] f64 (n = 6 doubles per affine
// map, 9 per homography), rowtab [F, 4, hq] int2 (hq = 0: no row table, the perspective
// warp), plan [tiles].
template <class Cfg>
struct LinearWs {
  int ntx, nty, hq;
  long long tiles;
  size_t tab_at, plan_at, bytes;  // byte offsets of rowtab and plan, and the whole
  LinearWs(bool perspective, int n_frames, int H, int W) {
    ntx = ceil_div(W, kTileW), nty = ceil_div(H, Cfg::kTileH);
    tiles = (long long)ntx * nty * n_frames;
    hq = perspective ? 0 : rowtab_hq(H);
    tab_at = (size_t)n_frames * (perspective ? 9 : 6) * sizeof(double);
    plan_at = tab_at + (size_t)n_frames * 4 * hq * sizeof(int2);
    bytes = plan_at + (size_t)tiles * sizeof(TilePlan);
  }
  double* minv(void* ws) const { return static_cast<double*>(ws); }
  int2* rowtab(void* ws) const { return reinterpret_cast<int2*>(static_cast<char*>(ws) + tab_at); }
  TilePlan* plan(void* ws) const { return reinterpret_cast<TilePlan*>(static_cast<char*>(ws) + plan_at); }
};

template <class Cfg>
size_t warp_workspace_bytes(int n_frames, int H, int W) {
  return LinearWs<Cfg>(false, n_frames, H, W).bytes;
}

// Plan + tile launches of either warp on `s`; ws holds LinearWs<Cfg>::bytes bytes.
template <bool PERSP, int C, class Cfg>
void launch_linear(const uint16_t* src, uint16_t* dst, const double* M, int n_frames, int H, int W, int inverse_map,
                   void* ws, hipStream_t s) {
  const LinearWs<Cfg> w(PERSP, n_frames, H, W);
  const dim3 plan_grid((unsigned)((w.tiles + 255) / 256)), tile_grid(w.ntx, w.nty, n_frames);
  if constexpr (PERSP) {
    hipLaunchKernelGGL((persp_plan_kernel<C, Cfg>), plan_grid, dim3(256), 0, s, M, n_frames, H, W, inverse_map, w.ntx,
                       w.nty, w.plan(ws), w.minv(ws));
    hipLaunchKernelGGL((warp_perspective_u16_kernel<C, Cfg>), tile_grid, dim3(kThreads), 0, s, src, dst, w.plan(ws),
                       w.minv(ws), H, W, persp_bw0(H, W));
  } else {
    hipLaunchKernelGGL((warp_plan_kernel<C, Cfg>), plan_grid, dim3(256), 0, s, M, n_frames, H, W, inverse_map, w.ntx,
                       w.nty, w.plan(ws), w.minv(ws), w.rowtab(ws), w.hq);
    hipLaunchKernelGGL((warp_affine_u16_kernel<C, Cfg>), tile_grid, dim3(kThreads), 0, s, src, dst, w.plan(ws),
                       w.minv(ws), w.rowtab(ws), w.hq, H, W);
  }
}

// The affine warp; ws holds warp_workspace_bytes<Cfg>(n_frames, H, W) bytes.
template <int C, class Cfg = typename CfgFor<C>::type>
void launch_warp(const uint16_t* src, uint16_t* dst, const double* M, int n_frames, int H, int W, int inverse_map,
                 void* ws, hipStream_t s) {
  launch_linear<false, C, Cfg>(src, dst, M, n_frames, H, W, inverse_map, ws, s);
}

// (perspective, C, use_tile64(H)) -> f(perspective, C and the configuration as types)
template <bool PERSP, int C, class Cfg>
struct LinearCfg {
  static constexpr bool kPersp = PERSP;
  static constexpr int kC = C;
  using cfg = Cfg;
};

template <bool PERSP, typename F>
int with_linear_cfg(int C, int H, F f) {
  if constexpr (!PERSP)
    if (C == 1 && use_tile64(H)) return f(LinearCfg<PERSP, 1, Block64Cfg>());
  if (C == 1) return f(LinearCfg<PERSP, 1, BlockCfg>());
  return C == 3 ? f(LinearCfg<PERSP, 3, ChanCfg>()) : f(LinearCfg<PERSP, 4, ChanCfg>());
}

template <typename F>
int with_linear_cfg(bool perspective, int C, int H, F f) {
  return perspective ? with_linear_cfg<true>(C, H, f) : with_linear_cfg<false>(C, H, f);
}

// The body of both entries.  Unlike run_tile_warp (warp_tile.h) it computes no vec_ok / pair_ok
// from the pointers: the tile kernels vectorise by W alone and src / dst need only 2-byte
// alignment, the unaligned 16- and 4-byte accesses being the device's business (kcmc.h;
// pinned on and off the grids by the warp_affine / warp_perspective sweeps of tests/sweep_cases.py).
int run_linear_warp(const char* name, const char* kernel_name, bool perspective, kcmc_ctx* ctx, const uint16_t* src,
                    uint16_t* dst, const double* M, int n_frames, int H, int W, int C, int inverse_map,
                    kcmc_stream_t stream) {
  const std::string w(name);
  if (!ctx) return fail(KCMC_EINVAL, w + ": ctx is NULL");
  if (n_frames < 0 || H < 0 || W < 0) return fail(KCMC_EINVAL, w + ": negative size");
  if (H > 32767 || W > 32767) return fail(KCMC_EUNSUPPORTED, w + ": H, W must be < 32768");
  if (n_frames > 65535) return fail(KCMC_EUNSUPPORTED, w + ": at most 65535 frames per call");
  if (C != 1 && C != 3 && C != 4) return fail(KCMC_EUNSUPPORTED, w + ": C must be 1, 3 or 4");
  if ((long long)ceil_div(W, kTileW) * ceil_div(H, ChanCfg::kTileH) * n_frames >= (1ll << 31))
    return fail(KCMC_EUNSUPPORTED, w + ": too many tiles in one call");
  if (n_frames == 0 || H == 0 || W == 0) return KCMC_OK;
  if (!src || !dst || !M) return fail(KCMC_EINVAL, w + ": NULL pointer");
  if (src == dst) return fail(KCMC_EINVAL, w + ": in-place warp is not supported");
  hipStream_t s = (hipStream_t)stream;
  return with_linear_cfg(perspective, C, H, [&](auto k) -> int {
    using K = decltype(k);
    void* ws = nullptr;
    const size_t wsb = LinearWs<typename K::cfg>(K::kPersp, n_frames, H, W).bytes;
    KCMC_TRY(workspace_alloc(ctx, &ws, wsb, s));
    launch_linear<K::kPersp, K::kC, typename K::cfg>(src, dst, M, n_frames, H, W, inverse_map, ws, s);
    const int rc = launch_check(kernel_name);
    KCMC_TRY(workspace_free(ctx, ws, s, wsb));
    return rc;
  });
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_warp_perspective_u16(kcmc_ctx* ctx, const uint16_t* src, uint16_t* dst, const double* M,
                                         int n_frames, int H, int W, int C, int inverse_map, kcmc_stream_t stream) {
  return run_linear_warp("kcmc_warp_perspective_u16", "warp_perspective_u16_kernel", true, ctx, src, dst, M, n_frames,
                         H, W, C, inverse_map, stream);
}

extern "C" int kcmc_warp_affine_u16(kcmc_ctx* ctx, const uint16_t* src, uint16_t* dst, const double* M,
                                    int n_frames, int H, int W, int C, int inverse_map, kcmc_stream_t stream) {
  return run_linear_warp("kcmc_warp_affine_u16", "warp_affine_u16_kernel", false, ctx, src, dst, M, n_frames, H, W, C,
                         inverse_map, stream);
}

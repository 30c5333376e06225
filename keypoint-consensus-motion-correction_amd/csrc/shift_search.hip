// s1: exact shift search -- the correlation moments of selected uint16 frames against a
// reference image at EVERY integer shift (dy, dx) in [-R, R]^2, for the intensity fallback of
// frames that RANSAC gave no model (kcmc_amd.fallback).  Build-defined: the reference has
// no such mode.  The layout and meaning of the five sums are those of kcmc_frame_stats_u16
// (quality.hip), so quality.pearson finishes them unchanged.
//
//   out[s][dy + R][dx + R] = (Sa, Sb, Saa, Sbb, Sab) over y in [y0, y1), x in [x0, x1),
//                            a = frame[frame_idx[s]][y + dy][x + dx], b = ref[y][x]
//
// A sliding-window correlation.  A workgroup walks tiles of 32 x 64 rectangle pixels of one
// frame; per tile it stages the reference tile (zero outside the rectangle) and the frame
// tile with a halo of R pixels in LDS, and its threads own the (2R + 1)^2 shifts (one to
// three each): every frame pixel is fetched from memory once per tile that needs it and
// reused from LDS by every shift.
//   Sab   one u16 x u16 + 64-bit multiply-add per pixel and shift (the only (2R + 1)^2 part).
//   Sa, Saa  window sums: per staged frame row and dx the sum over the tile's columns
//         (rows x (2R + 1) partial sums in LDS, 32-bit for a: 64 * 65535 < 2^32, 64-bit for
//         a^2), then per shift the sum of its 32 rows -- 1/32 of the work of the products.
//   Sb, Sbb  do not depend on the shift: summed while the reference tile is staged, left in
//         shift entry 0 and copied to the other entries by a second small kernel.
// Every accumulator that outlives a tile is 64-bit (H * W < 2^31 pixels of at most
// 65535^2 < 2^32 each stay below 2^63), the sums leave the workgroup as 64-bit integer
// atomics, so the result is exact and independent of the order in which workgroups finish.
// A workgroup takes several tiles so that the atomics stay a small fraction of the work.
//
// Tiles are anchored at column x0 & ~7, so that with frame rows on 16-byte boundaries (W % 8
// == 0, 16-byte aligned frames and ref) both tiles are staged with 16-byte loads and LDS
// stores; everything else -- odd widths, a slab view that starts mid-allocation -- stages
// element by element into the same LDS image.  No load leaves the image: vectors and
// elements outside [0, H) x [0, W) are staged as zeros (the contract keeps every pixel a
// valid shift reads inside the image; the zeros only meet reference zeros).
#include "u16_rows.h"

namespace kcmc {
namespace {

constexpr int kTH = 32;            // tile rows
constexpr int kTW = 64;            // tile columns (a multiple of 8)
constexpr int kMaxThreads = 512;
constexpr int kMaxR = 16;
constexpr int kMaxPasses = 3;      // ceil(33^2 / 512)
constexpr int kTargetWGs = 1536;   // 256 CUs x 6 resident workgroups of 5 waves

__device__ __forceinline__ int lds_col0(int R) { return (8 - (R & 7)) & 7; }  // R + lds_col0 is a multiple of 8

__device__ __forceinline__ void add_b(u64& sb, u64& sbb, uint32_t b) {
  sb += b;
  sbb += (u64)b * b;
}

// grid (n_sel, workgroups per frame), block: a multiple of 64 threads, NP * block >= S^2.
// AW: the staged frame tile's row length in pixels, a multiple of 8, >= lds_col0 + kTW + 2R.
// Dynamic LDS: A [kTH + 2R][AW] u16 | B [kTH][kTW] u16 | rsaa [kTH + 2R][S] u64 | rsa (same) u32.
template <bool VEC, int NP>
__global__ __launch_bounds__(kMaxThreads) void shift_search_kernel(
    const uint16_t* __restrict__ frames, int n_frames, int H, int W, const int32_t* __restrict__ frame_idx,
    const uint16_t* __restrict__ ref, int y0, int y1, int x0, int x1, int R, int AW, int tiles_x, int tiles,
    u64* __restrict__ out) {
  extern __shared__ uint4 smem[];
  const int s = blockIdx.x;
  const int f = frame_idx ? frame_idx[s] : s;
  if (f < 0 || f >= n_frames) return;  // uniform over the workgroup: the row stays zero
  const int S = 2 * R + 1, S2 = S * S, AH = kTH + 2 * R, ax0 = lds_col0(R);
  uint16_t* A = reinterpret_cast<uint16_t*>(smem);
  uint16_t* B = A + AH * AW;
  u64* rsaa = reinterpret_cast<u64*>(B + kTH * kTW);
  uint32_t* rsa = reinterpret_cast<uint32_t*>(rsaa + AH * S);
  const uint16_t* fr = frames + (size_t)f * H * W;
  const int tid = threadIdx.x, nt = blockDim.x;

  int dyi[NP], dxi[NP], aoff[NP];
  bool act[NP];
  u64 sab[NP], sa[NP], saa[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int sh = tid + p * nt;
    act[p] = sh < S2;
    const int shc = act[p] ? sh : 0;  // idle slots follow shift 0 and are dropped at the end
    dyi[p] = shc / S;
    dxi[p] = shc - dyi[p] * S;
    aoff[p] = dyi[p] * AW + dxi[p] + ax0;
    sab[p] = sa[p] = saa[p] = 0;
  }
  u64 sb = 0, sbb = 0;
  const int xg = x0 & ~7;

  for (int t = blockIdx.y; t < tiles; t += gridDim.y) {
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int ty0 = y0 + ty * kTH, tx0 = xg + tx * kTW;  // tx0 is a multiple of 8
    const int cb = tx0 - R - ax0;                         // image column of LDS column 0, a multiple of 8
    const int th = min(kTH, y1 - ty0);                    // the tile's rectangle rows [0, th)
    const int xa = max(0, x0 - tx0), xb = min(kTW, x1 - tx0);  // ... and columns [xa, xb)

    // ---- stage the frame tile with its halo and the reference tile
    if (VEC) {
      const int nvec = AW / 8;
      for (int i = tid; i < AH * nvec; i += nt) {
        const int r = i / nvec, v = i - r * nvec;
        const int gy = ty0 - R + r, gx = cb + 8 * v;
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (gy >= 0 && gy < H && gx >= 0 && gx + 8 <= W)
          q = *reinterpret_cast<const uint4*>(fr + (size_t)gy * W + gx);
        reinterpret_cast<uint4*>(A)[i] = q;
      }
      for (int i = tid; i < kTH * (kTW / 8); i += nt) {
        const int r = i / (kTW / 8), v = i - r * (kTW / 8);
        const int gy = ty0 + r, gx = tx0 + 8 * v;
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (gy < y1 && gx < x1 && gx + 8 > x0) {  // inside the image: gx < W, gx and W multiples of 8
          q = mask8(*reinterpret_cast<const uint4*>(ref + (size_t)gy * W + gx), gx, x0, x1);
          for_each_px(q, [&](int, uint32_t b) { add_b(sb, sbb, b); });
        }
        reinterpret_cast<uint4*>(B)[i] = q;
      }
    } else {
      for (int i = tid; i < AH * AW; i += nt) {
        const int r = i / AW, c = i - r * AW;
        const int gy = ty0 - R + r, gx = cb + c;
        uint16_t v = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = fr[(size_t)gy * W + gx];
        A[i] = v;
      }
      for (int i = tid; i < kTH * kTW; i += nt) {
        const int r = i / kTW, c = i - r * kTW;
        const int gy = ty0 + r, gx = tx0 + c;
        uint16_t v = 0;
        if (gy < y1 && gx >= x0 && gx < x1) {
          v = ref[(size_t)gy * W + gx];
          add_b(sb, sbb, v);
        }
        B[i] = v;
      }
    }
    __syncthreads();

    // ---- Sab: every thread its shifts over the tile (b = 0 outside the rectangle)
    for (int y = 0; y < th; ++y) {
      const uint32_t* brow = reinterpret_cast<const uint32_t*>(B + y * kTW);
      const uint16_t* arow = A + y * AW;
#pragma unroll 4
      for (int x2 = xa / 2; x2 < (xb + 1) / 2; ++x2) {
        const uint32_t bb = brow[x2];
        const uint32_t b0 = bb & 0xffffu, b1 = bb >> 16;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const uint16_t* a = arow + aoff[p] + 2 * x2;
          sab[p] += (u64)(uint32_t)a[0] * b0;
          sab[p] += (u64)(uint32_t)a[1] * b1;
        }
      }
    }
    // ---- per staged row and dx: the sums of a and a^2 over the tile's columns
    for (int i = tid; i < (th + 2 * R) * S; i += nt) {
      const int yy = i / S, d = i - yy * S;
      const uint16_t* a = A + yy * AW + ax0 + d;
      uint32_t ua = 0;
      u64 uaa = 0;
      for (int x = xa; x < xb; ++x) {
        const uint32_t v = a[x];
        ua += v;
        uaa += (u64)v * v;
      }
      rsa[i] = ua;
      rsaa[i] = uaa;
    }
    __syncthreads();
    // ---- Sa, Saa: per shift the sum of its rows.  (The next tile's staging leaves rsa / rsaa
    // alone, and its barrier comes before they are written again.)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int base = dyi[p] * S + dxi[p];
      for (int y = 0; y < th; ++y) {
        sa[p] += rsa[base + y * S];
        saa[p] += rsaa[base + y * S];
      }
    }
  }

  u64* o = out + (size_t)s * S2 * 5;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if (!act[p]) continue;
    u64* e = o + (size_t)(tid + p * nt) * 5;
    if (sa[p]) atomicAdd(e + 0, sa[p]);
    if (saa[p]) atomicAdd(e + 2, saa[p]);
    if (sab[p]) atomicAdd(e + 4, sab[p]);
  }
  sb = wave_sum(sb);
  sbb = wave_sum(sbb);
  if ((tid & 63) == 0) {
    if (sb) atomicAdd(o + 1, sb);
    if (sbb) atomicAdd(o + 3, sbb);
  }
}

template <bool VEC>
void launch(int passes, dim3 grid, dim3 block, size_t lds, hipStream_t s, const uint16_t* frames, int n_frames, int H,
            int W, const int32_t* frame_idx, const uint16_t* ref, int y0, int y1, int x0, int x1, int R, int AW,
            int tiles_x, int tiles, u64* out) {
  if (passes == 1)
    hipLaunchKernelGGL((shift_search_kernel<VEC, 1>), grid, block, lds, s, frames, n_frames, H, W, frame_idx, ref, y0,
                       y1, x0, x1, R, AW, tiles_x, tiles, out);
  else if (passes == 2)
    hipLaunchKernelGGL((shift_search_kernel<VEC, 2>), grid, block, lds, s, frames, n_frames, H, W, frame_idx, ref, y0,
                       y1, x0, x1, R, AW, tiles_x, tiles, out);
  else
    hipLaunchKernelGGL((shift_search_kernel<VEC, 3>), grid, block, lds, s, frames, n_frames, H, W, frame_idx, ref, y0,
                       y1, x0, x1, R, AW, tiles_x, tiles, out);
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_shift_search_u16(kcmc_ctx* ctx, const uint16_t* frames, int n_frames, int H, int W,
                                     const int32_t* frame_idx, int n_sel, const uint16_t* ref, int y0, int y1, int x0,
                                     int x1, int R, long long* out, kcmc_stream_t stream) {
  KCMC_TRY(check_rect("kcmc_shift_search_u16", ctx, n_frames, n_sel, H, W, y0, y1, x0, x1, R, "R"));
  if (R < 1 || R > kMaxR) return fail(KCMC_EINVAL, "kcmc_shift_search_u16: R must be in [1, 16]");
  if (n_sel == 0) return KCMC_OK;
  KCMC_TRY(check_pointers("kcmc_shift_search_u16", frames, n_frames, ref, out));
  hipStream_t s = (hipStream_t)stream;
  const int S = 2 * R + 1, S2 = S * S;
  const size_t n_entries = (size_t)n_sel * S2;
  KCMC_TRY(hip_check(hipMemsetAsync(out, 0, n_entries * 5 * sizeof(long long), s), "hipMemsetAsync"));
  if (n_frames == 0) return KCMC_OK;  // every index is out of range

  const bool vec = rows_vectorizable(W, frames, ref);
  const int ax0 = (8 - (R & 7)) & 7;
  const int AW = (ax0 + kTW + 2 * R + 7) / 8 * 8, AH = kTH + 2 * R;
  const int tiles_x = (x1 - (x0 & ~7) + kTW - 1) / kTW, tiles_y = (y1 - y0 + kTH - 1) / kTH;
  const long long tiles = (long long)tiles_x * tiles_y;  // < 2^31 / 2048
  const int passes = (S2 + kMaxThreads - 1) / kMaxThreads;  // <= kMaxPasses
  const int threads = ((S2 + passes - 1) / passes + 63) / 64 * 64;
  const size_t lds = (size_t)AH * AW * 2 + (size_t)kTH * kTW * 2 + (size_t)AH * S * 12;  // <= 41728 bytes
  // workgroups per frame: fill the device when the frames are few, several tiles each when many
  long long by = (kTargetWGs + n_sel - 1) / n_sel;
  by = std::max<long long>(1, std::min<long long>(by, tiles));
  auto* o = reinterpret_cast<u64*>(out);
  const dim3 grid((unsigned)n_sel, (unsigned)by), block((unsigned)threads);
  if (vec)
    launch<true>(passes, grid, block, lds, s, frames, n_frames, H, W, frame_idx, ref, y0, y1, x0, x1, R, AW, tiles_x,
                 (int)tiles, o);
  else
    launch<false>(passes, grid, block, lds, s, frames, n_frames, H, W, frame_idx, ref, y0, y1, x0, x1, R, AW, tiles_x,
                  (int)tiles, o);
  KCMC_TRY(launch_check("shift_search_kernel"));
  return launch_copy_b(o, n_entries, S2, s);  // Sb, Sbb of every frame's shift entry 0 to its other entries
}

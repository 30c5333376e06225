// g1: gradient sums -- the right-hand side of one linearised least-squares (Gauss-Newton)
// step of every frame against a reference image, for the intensity refinement of the
// frames' maps (kcmc_amd.refine).  Build-defined: the reference has no such mode.
//
//   out[s][k] = (Sa, Saa, Sab, Sagx, Sagy, Sxagy, Syagx) over the rows of band k of the
//               rectangle [y0, y1) x [x0, x1):
//     a  = frame[frame_idx[s]][y][x],  b = ref[y][x]
//     gx = ref[y][x + 1] - ref[y][x - 1],  gy = ref[y + 1][x] - ref[y - 1][x]
//     Sxagy = sum (x - cx) a gy,  Syagx = sum (y - cy) a gx,  cx = (x0 + x1) / 2, cy = (y0 + y1) / 2
//
// One workgroup owns one (frame, band) and leaves its seven sums with plain stores: no
// atomics, no memset, nothing depends on the order in which workgroups finish.
//
// The rectangle's columns are covered by the 8-pixel vectors of the image grid (x0 / 8 ..
// ceil(x1 / 8)).  The workgroup's 256 threads are CT thread columns x RG row groups (CT a
// power of two chosen by the launcher so that few thread columns idle): a thread owns one
// vector column per chunk of CT vectors and walks the contiguous rows of its row group, so
//   * the frame is read once, one 16-byte load per thread and row, the next row's load
//     issued before the current row is summed;
//   * ref rows y - 1, y, y + 1 roll through registers (one new 16-byte load per row, L2);
//     ref[y][c0 - 1] and ref[y][c0 + 8] come from the neighbouring lanes, and from memory at
//     the ends of a wave's row segment;
//   * the rectangle mask zeroes a only -- never b, whose pixels beside the rectangle the
//     gradient at its edge needs (the contract keeps them inside the image);
//   * y' is constant along a row and x' along a thread's column, so neither costs a
//     multiply per pixel: a * gy is summed per column (eight accumulators, multiplied by x'
//     once per chunk), and with R_i the thread's sum of a * gx in its i-th row, S_i = R_0 + ..
//     + R_i and Q = S_0 + .. + S_(n-1):  sum i R_i = n S_(n-1) - Q  -- two additions per row.
//   Four 32 x 32 + 64-bit multiply-adds per pixel remain (a^2, a b, a gx, a gy).
//
// Exact: every sum is a 64-bit integer in two's complement; the contract bounds the
// magnitude of every band sum below 2^63 (kcmc.h), and intermediate values are kept in
// unsigned arithmetic, where wrapping is harmless.
//
// VEC needs frame rows on 16-byte boundaries (W % 8 == 0, 16-byte aligned frames and ref);
// everything else -- odd widths, a slab view that starts mid-allocation -- gathers the same
// 8-pixel vectors element by element, every element checked against W.
#include "u16_rows.h"

namespace kcmc {
namespace {

constexpr int kThreads = 256;

typedef long long i64;

// grid (n_sel * n_bands), block 256 = (1 << ct_log2) thread columns x row groups.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void gradient_sums_kernel(
    const uint16_t* __restrict__ frames, int n_frames, int H, int W, const int32_t* __restrict__ frame_idx,
    const uint16_t* __restrict__ ref, int y0, int y1, int x0, int x1, int band_rows, int n_bands, int ct_log2,
    u64* __restrict__ out) {
  __shared__ u64 red[7][kThreads / 64];
  const unsigned blk = blockIdx.x;
  const int s = (int)(blk / (unsigned)n_bands), band = (int)(blk - (unsigned)s * (unsigned)n_bands);
  u64* o = out + (size_t)blk * 7;
  const int tid = threadIdx.x;
  const int f = frame_idx ? frame_idx[s] : s;
  if (f < 0 || f >= n_frames) {  // uniform over the workgroup: a zero row, the frames are never read
    if (tid < 7) o[tid] = 0;
    return;
  }
  const int CT = 1 << ct_log2, RG = kThreads >> ct_log2;
  const int tx = tid & (CT - 1), ty = tid >> ct_log2;
  const int ya = y0 + band * band_rows;        // < y1
  const int nb = min(band_rows, y1 - ya);      // the band's rows
  const int RB = (nb + RG - 1) / RG;           // rows per row group (uniform trip count)
  const int r0 = ya + ty * RB;                 // this thread's rows [r0, r0 + nr)
  const int nr = max(0, min(RB, ya + nb - r0));
  const int cx = (x0 + x1) >> 1, cy = (y0 + y1) >> 1;
  const int xg = x0 & ~7;
  const int nvec = ((x1 + 7) >> 3) - (x0 >> 3);
  const int em = min(CT, 64) - 1;              // a wave's row segment: min(CT, 64) neighbouring lanes
  const uint16_t* fr = frames + (size_t)f * H * W;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  u64 sa = 0, saa = 0, sab = 0, sagx = 0, sagy = 0, sxagy = 0, syagx = 0;
  for (int vb = 0; vb < nvec; vb += CT) {
    const int v = vb + tx;
    const bool vok = v < nvec;
    const int c0 = xg + 8 * v;
    const bool left_edge = (tx & em) == 0;
    const bool right_edge = (tx & em) == em || v == nvec - 1;  // the next lane holds no vector of this row
    i64 cagy[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // per column: sum over the rows of a * gy
    u64 S = 0, Q = 0;
    uint4 bm = zero, b0 = zero, a_cur = zero;  // ref rows y - 1 and y, frame row y
    if (vok && nr > 0) {
      bm = load8<VEC>(ref + (size_t)(r0 - 1) * W, c0, W);
      b0 = load8<VEC>(ref + (size_t)r0 * W, c0, W);
      a_cur = load8<VEC>(fr + (size_t)r0 * W, c0, W);
    }
    for (int i = 0; i < RB; ++i) {  // every thread makes every trip: the lanes exchange ref pixels
      const int y = r0 + i;
      const bool ok = vok && i < nr;
      uint4 bp = zero, a_nxt = zero;
      if (ok) bp = load8<VEC>(ref + (size_t)(y + 1) * W, c0, W);  // y + 1 <= y1 <= H - 1
      if (vok && i + 1 < nr) a_nxt = load8<VEC>(fr + (size_t)(y + 1) * W, c0, W);
      uint32_t lw = (uint32_t)__shfl_up((int)b0.w, 1, 64) >> 16;        // ref[y][c0 - 1]
      uint32_t rw = (uint32_t)__shfl_down((int)b0.x, 1, 64) & 0xffffu;  // ref[y][c0 + 8]
      if (left_edge) lw = (ok && c0 > 0) ? (uint32_t)ref[(size_t)y * W + c0 - 1] : 0u;
      if (right_edge) rw = (ok && c0 + 8 < W) ? (uint32_t)ref[(size_t)y * W + c0 + 8] : 0u;

      int32_t a[8], up[8], dn[8], b[10];
      unpack8(mask8(a_cur, c0, x0, x1), a);  // a_cur is zero where this thread has no row
      unpack8(bm, up);
      unpack8(bp, dn);
      unpack8(b0, b + 1);
      b[0] = (int32_t)lw;
      b[9] = (int32_t)rw;
      uint32_t a8 = 0;
      i64 rag = 0;  // this row's a * gx: |rag| < 8 * 2^32
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a8 += (uint32_t)a[j];
        saa += (u64)(uint32_t)a[j] * (uint32_t)a[j];
        sab += (u64)(uint32_t)a[j] * (uint32_t)b[j + 1];
        rag += (i64)a[j] * (b[j + 2] - b[j]);
        cagy[j] += (i64)a[j] * (dn[j] - up[j]);
      }
      sa += a8;
      S += (u64)rag;
      Q += S;
      bm = b0;
      b0 = bp;
      a_cur = a_nxt;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sagy += (u64)cagy[j];
      sxagy += (u64)(i64)(c0 + j - cx) * (u64)cagy[j];
    }
    sagx += S;
    syagx += (u64)(i64)(r0 - cy) * S + ((u64)RB * S - Q);  // sum over the rows of (r0 + i - cy) R_i
  }

  const u64 v[7] = {sa, saa, sab, sagx, sagy, sxagy, syagx};
  const u64 r = block_sums(v, red);
  if (tid < 7) o[tid] = r;
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

// The bound band_rows * (x1 - x0) * max(x1 - x0, y1 - y0) < 2^32: a band holds at most
// band_rows * (x1 - x0) pixels; a <= 65535 and |gx|, |gy| <= 65535, so |a g| < 2^32, as are a^2
// and a b; |x - cx| <= (x1 - x0) / 2 and |y - cy| <= (y1 - y0) / 2.  The largest magnitude a band
// sum can reach is therefore below band_rows * (x1 - x0) * (max / 2) * 2^32 < 2^63.
extern "C" int kcmc_gradient_sums_u16(kcmc_ctx* ctx, const uint16_t* frames, int n_frames, int H, int W,
                                      const int32_t* frame_idx, int n_sel, const uint16_t* ref, int y0, int y1, int x0,
                                      int x1, int band_rows, long long* out, kcmc_stream_t stream) {
  KCMC_TRY(check_rect("kcmc_gradient_sums_u16", ctx, n_frames, n_sel, H, W, y0, y1, x0, x1, 1, "1"));
  if (band_rows < 1) return fail(KCMC_EINVAL, "kcmc_gradient_sums_u16: band_rows must be >= 1");
  const unsigned long long w = (unsigned long long)(x1 - x0), h = (unsigned long long)(y1 - y0);
  if ((unsigned long long)band_rows > 0xffffffffull / (w * std::max(w, h)))
    return fail(KCMC_EINVAL, "kcmc_gradient_sums_u16: band_rows * (x1 - x0) * max(x1 - x0, y1 - y0) must be < 2^32");
  if (n_sel == 0) return KCMC_OK;
  KCMC_TRY(check_pointers("kcmc_gradient_sums_u16", frames, n_frames, ref, out));
  hipStream_t s = (hipStream_t)stream;
  const long long n_bands = ((long long)h + band_rows - 1) / band_rows;
  const long long blocks = n_bands * n_sel;
  if (blocks > 0x7fffffffll) return fail(KCMC_EUNSUPPORTED, "kcmc_gradient_sums_u16: n_sel * n_bands too large");

  const bool vec = rows_vectorizable(W, frames, ref);
  const int ct_log2 = thread_columns_log2((x1 + 7) / 8 - x0 / 8);
  auto* o = reinterpret_cast<unsigned long long*>(out);
  const dim3 grid((unsigned)blocks), block(kThreads);
  if (vec)
    hipLaunchKernelGGL(gradient_sums_kernel<true>, grid, block, 0, s, frames, n_frames, H, W, frame_idx, ref, y0, y1,
                       x0, x1, band_rows, (int)n_bands, ct_log2, o);
  else
    hipLaunchKernelGGL(gradient_sums_kernel<false>, grid, block, 0, s, frames, n_frames, H, W, frame_idx, ref, y0, y1,
                       x0, x1, band_rows, (int)n_bands, ct_log2, o);
  return launch_check("gradient_sums_kernel");
}

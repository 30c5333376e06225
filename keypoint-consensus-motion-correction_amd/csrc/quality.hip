// q1: registration quality metrics -- two streaming reductions of a uint16 stack
// [F, H, W] next to the normalisation front end (normalize.hip).  Every sum is an exact
// integer, so the results do not depend on the order in which workgroups finish.
//
//   kcmc_stack_sum_u16    out[p] = sum over the selected frames f of frames[f][p]  (i64):
//                         the numerator of the mean image.
//   kcmc_frame_stats_u16  out[f] = (Sa, Sb, Saa, Sbb, Sab) over a rectangle, a = frame f,
//                         b = a reference image: what Pearson's r of the frame with the
//                         mean image needs (finished on the host in exact integers).
//
// Both read the stack once with 16-byte loads, several in flight per thread, keep their
// partial sums in registers across the loop and leave one 64-bit integer atomic per
// workgroup and destination.
//
// Stack sum: a thread owns 8 neighbouring pixels (one 16-byte load per frame) and walks a
// chunk of at most 65536 frames, so its eight accumulators stay 32-bit
// (65536 * 65535 < 2^32); the frames are cut into chunks across blockIdx.y, which keeps
// enough workgroups in flight for small images (512 x 512: 128 pixel blocks).  The
// accumulators cross LDS once so that every atomic wave instruction covers 512 contiguous
// bytes of the output instead of one 8-byte word per 64 bytes.
//
// Frame stats: the rectangle's rows are covered by the 16-byte vectors of the image grid
// (x0 / 8 .. ceil(x1 / 8) per row); the lanes of the first and last vector of a row that
// fall outside [x0, x1) are zeroed in a (and in b where Sb and Sbb are summed), which removes
// them from all five sums.
// Products are u16 x u16, so each is one 32 x 32 + 64-bit multiply-add.  Sb and Sbb do not
// depend on the frame: frame 0's workgroups compute them and a small second kernel copies
// them to the other frames.
//
// The vector kernels need frame rows that start on 16-byte boundaries (a 16-byte aligned
// base, and n_px resp. W a multiple of 8); everything else -- odd sizes, a slab view that
// starts mid-allocation -- takes the element-wise kernels of the same layout.
#include "u16_rows.h"

namespace kcmc {
namespace {

constexpr int kThreads = 256;
constexpr int kMinChunk = 32;       // frames per chunk at least: <= 1 atomic byte per 8 bytes read
constexpr int kMaxChunk = 65536;    // 32-bit accumulators
constexpr int kTargetBlocks = 2048; // 256 CUs x 8 resident workgroups

__device__ __forceinline__ void add8(uint32_t* acc, const uint4& q) {
  for_each_px(q, [&](int j, uint32_t px) { acc[j] += px; });
}

// n_px % 8 == 0, frames 16-byte aligned.  grid (ceil(n_px / 2048), chunks).
template <bool SEL>
__global__ __launch_bounds__(kThreads) void stack_sum_vec_kernel(const uint16_t* __restrict__ frames, int n_frames,
                                                                 size_t n_px, int chunk,
                                                                 const uint8_t* __restrict__ sel,
                                                                 unsigned long long* __restrict__ out) {
  __shared__ uint32_t s[8 * kThreads];
  const int tid = threadIdx.x;
  const size_t nv = n_px / 8;
  const size_t v = blockIdx.x * (size_t)kThreads + tid;
  const int f0 = blockIdx.y * chunk;
  const int f1 = min(f0 + chunk, n_frames);
  uint32_t acc[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (v < nv) {
    const uint4* p = reinterpret_cast<const uint4*>(frames) + (size_t)f0 * nv + v;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    int f = f0;
    for (; f + 4 <= f1; f += 4, p += 4 * nv) {  // four 16-byte loads in flight per thread
      uint4 q0 = zero, q1 = zero, q2 = zero, q3 = zero;  // the selection is uniform over the workgroup
      if (!SEL || sel[f]) q0 = p[0];
      if (!SEL || sel[f + 1]) q1 = p[nv];
      if (!SEL || sel[f + 2]) q2 = p[2 * nv];
      if (!SEL || sel[f + 3]) q3 = p[3 * nv];
      add8(acc, q0);
      add8(acc, q1);
      add8(acc, q2);
      add8(acc, q3);
    }
    for (; f < f1; ++f, p += nv)
      if (!SEL || sel[f]) add8(acc, *p);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) s[8 * tid + k] = acc[k];
  __syncthreads();
  const size_t base = blockIdx.x * (size_t)(8 * kThreads);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const size_t px = base + j * kThreads + tid;
    const uint32_t a = s[j * kThreads + tid];
    if (px < n_px && a) atomicAdd(&out[px], (unsigned long long)a);
  }
}

// Any n_px and alignment: one pixel per thread.  grid (ceil(n_px / 256), chunks).
template <bool SEL>
__global__ __launch_bounds__(kThreads) void stack_sum_elem_kernel(const uint16_t* __restrict__ frames, int n_frames,
                                                                  size_t n_px, int chunk,
                                                                  const uint8_t* __restrict__ sel,
                                                                  unsigned long long* __restrict__ out) {
  const size_t px = blockIdx.x * (size_t)kThreads + threadIdx.x;
  if (px >= n_px) return;
  const int f0 = blockIdx.y * chunk;
  const int f1 = min(f0 + chunk, n_frames);
  const uint16_t* p = frames + (size_t)f0 * n_px + px;
  uint32_t acc = 0u;
  int f = f0;
  for (; f + 4 <= f1; f += 4, p += 4 * n_px) {
    uint32_t q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = (!SEL || sel[f + k]) ? (uint32_t)p[k * n_px] : 0u;
    acc += (q[0] + q[1]) + (q[2] + q[3]);
  }
  for (; f < f1; ++f, p += n_px)
    if (!SEL || sel[f]) acc += *p;
  if (acc) atomicAdd(&out[px], (unsigned long long)acc);
}

// ---------------------------------------------------------------------- frame stats
struct Sums {
  unsigned long long a = 0, b = 0, aa = 0, bb = 0, ab = 0;
};

template <bool WITH_B>
__device__ __forceinline__ void acc_px(Sums& s, uint32_t a, uint32_t b) {
  s.a += a;
  s.aa += (unsigned long long)a * a;
  s.ab += (unsigned long long)a * b;
  if (WITH_B) {
    s.b += b;
    s.bb += (unsigned long long)b * b;
  }
}

template <bool WITH_B>
__device__ __forceinline__ void acc_vec(Sums& s, const uint4& a, const uint4& b) {
  uint32_t pb[8];
  unpack8(b, pb);
  for_each_px(a, [&](int j, uint32_t pa) { acc_px<WITH_B>(s, pa, pb[j]); });
}

// VEC: W % 8 == 0, frames and ref 16-byte aligned.  The items of a frame are the vectors
// (VEC) or pixels of the rectangle, row by row; the workgroups of blockIdx.y share them.
template <bool VEC, bool WITH_B>
__device__ __forceinline__ void frame_sums(Sums& s, const uint16_t* __restrict__ fr, const uint16_t* __restrict__ ref,
                                           int W, int y0, int y1, int x0, int x1) {
  const uint32_t c_lo = VEC ? (uint32_t)(x0 / 8) : (uint32_t)x0;
  const uint32_t per_row = (VEC ? (uint32_t)((x1 + 7) / 8) : (uint32_t)x1) - c_lo;
  const uint32_t items = (uint32_t)(y1 - y0) * per_row;  // < 2^31: H * W < 2^31
  const uint32_t stride = gridDim.y * (uint32_t)kThreads;
  uint32_t i = blockIdx.y * (uint32_t)kThreads + threadIdx.x;
  if (VEC) {
    const uint4* fa = reinterpret_cast<const uint4*>(fr);
    const uint4* fb = reinterpret_cast<const uint4*>(ref);
    const uint32_t wv = (uint32_t)W / 8;
    auto at = [&](uint32_t it, uint32_t& col) {
      const uint32_t r = it / per_row;
      col = c_lo + (it - r * per_row);
      return ((uint32_t)y0 + r) * wv + col;
    };
    for (; i < items && items - i > stride; i += 2 * stride) {  // two vector pairs in flight per thread
      uint32_t c0, c1;
      const uint32_t o0 = at(i, c0), o1 = at(i + stride, c1);
      const uint4 a0 = fa[o0], a1 = fa[o1], b0 = fb[o0], b1 = fb[o1];
      acc_vec<WITH_B>(s, mask8(a0, 8 * c0, x0, x1), WITH_B ? mask8(b0, 8 * c0, x0, x1) : b0);
      acc_vec<WITH_B>(s, mask8(a1, 8 * c1, x0, x1), WITH_B ? mask8(b1, 8 * c1, x0, x1) : b1);
    }
    if (i < items) {
      uint32_t c0;
      const uint32_t o0 = at(i, c0);
      acc_vec<WITH_B>(s, mask8(fa[o0], 8 * c0, x0, x1), WITH_B ? mask8(fb[o0], 8 * c0, x0, x1) : fb[o0]);
    }
  } else {
    for (; i < items; i += stride) {
      const uint32_t r = i / per_row;
      const size_t o = (size_t)((uint32_t)y0 + r) * W + c_lo + (i - r * per_row);
      acc_px<WITH_B>(s, fr[o], ref[o]);
    }
  }
}

// grid (n_frames, workgroups per frame).  out [n_frames, 5] zeroed before the launch.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void frame_stats_kernel(const uint16_t* __restrict__ frames, int H, int W,
                                                               const uint16_t* __restrict__ ref, int y0, int y1,
                                                               int x0, int x1, unsigned long long* __restrict__ out) {
  __shared__ u64 red[5][kThreads / 64];
  const size_t f = blockIdx.x;
  const uint16_t* fr = frames + f * (size_t)H * W;
  Sums s;
  if (f == 0)
    frame_sums<VEC, true>(s, fr, ref, W, y0, y1, x0, x1);
  else
    frame_sums<VEC, false>(s, fr, ref, W, y0, y1, x0, x1);
  const u64 v[5] = {s.a, s.b, s.aa, s.bb, s.ab};
  const u64 t = block_sums(v, red);
  const int k = threadIdx.x;
  if (k < 5 && (f == 0 || (k != 1 && k != 3)) && t) atomicAdd(&out[f * 5 + k], t);
}

// launch_copy_b (u16_rows.h): here the group is all frames, in shift_search.hip the shifts of one frame.
__global__ __launch_bounds__(kThreads) void copy_b_kernel(u64* __restrict__ out, size_t n_entries, int group) {
  const size_t i = blockIdx.x * (size_t)kThreads + threadIdx.x;
  if (i >= n_entries) return;
  const size_t first = i / group * group;
  if (i == first) return;
  out[i * 5 + 1] = out[first * 5 + 1];
  out[i * 5 + 3] = out[first * 5 + 3];
}

}  // namespace

int launch_copy_b(u64* out, size_t n_entries, int group, hipStream_t s) {
  hipLaunchKernelGGL(copy_b_kernel, dim3((unsigned)((n_entries + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, out,
                     n_entries, group);
  return launch_check("copy_b_kernel");
}

int check_rect(const char* fn, kcmc_ctx* ctx, int n_frames, int n_sel, int H, int W, int y0, int y1, int x0, int x1,
               int margin, const char* grown) {
  const std::string p = std::string(fn) + ": ";
  if (!ctx) return fail(KCMC_EINVAL, p + "ctx is NULL");
  if (n_frames < 0 || n_sel < 0 || H <= 0 || W <= 0) return fail(KCMC_EINVAL, p + "bad shape");
  if ((long long)H * W >= (1ll << 31)) return fail(KCMC_EINVAL, p + "H * W must be < 2^31");
  if (y0 >= y1 || x0 >= x1) return fail(KCMC_EINVAL, p + "empty rectangle");
  const long long m = margin;
  if (y0 < m || x0 < m || y1 + m > H || x1 + m > W)
    return fail(KCMC_EINVAL, p + (grown ? "the rectangle grown by " + std::string(grown) + " leaves the image"
                                        : std::string("rectangle outside the image")));
  return KCMC_OK;
}

int check_pointers(const char* fn, const void* frames, int n_frames, const void* ref, const void* out) {
  const std::string p = std::string(fn) + ": ";
  if (!ref || !out || (n_frames > 0 && !frames)) return fail(KCMC_EINVAL, p + "NULL pointer");
  if (((uintptr_t)out & 7) != 0) return fail(KCMC_EINVAL, p + "out must be 8-byte aligned");
  return KCMC_OK;
}

}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_stack_sum_u16(kcmc_ctx* ctx, const uint16_t* frames, int n_frames, unsigned long long n_px,
                                  const uint8_t* sel, long long* out_sum, kcmc_stream_t stream) {
  if (!ctx) return fail(KCMC_EINVAL, "kcmc_stack_sum_u16: ctx is NULL");
  if (n_frames < 0) return fail(KCMC_EINVAL, "kcmc_stack_sum_u16: n_frames must be >= 0");
  if (n_px == 0) return fail(KCMC_EINVAL, "kcmc_stack_sum_u16: n_px must be > 0");
  if (!out_sum || (n_frames > 0 && !frames)) return fail(KCMC_EINVAL, "kcmc_stack_sum_u16: NULL pointer");
  if (((uintptr_t)out_sum & 7) != 0) return fail(KCMC_EINVAL, "kcmc_stack_sum_u16: out_sum must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  KCMC_TRY(hip_check(hipMemsetAsync(out_sum, 0, (size_t)n_px * sizeof(long long), s), "hipMemsetAsync"));
  if (n_frames == 0) return KCMC_OK;
  const bool vec = n_px % 8 == 0 && ((uintptr_t)frames & 15) == 0;
  const unsigned long long per_block = vec ? 8ull * kThreads : (unsigned long long)kThreads;
  const unsigned long long bx = (n_px + per_block - 1) / per_block;
  if (bx > 0x7fffffffull) return fail(KCMC_EUNSUPPORTED, "kcmc_stack_sum_u16: n_px too large");
  // enough chunks to fill the device, none shorter than kMinChunk or longer than kMaxChunk
  const long long want = (long long)((kTargetBlocks + bx - 1) / bx);
  long long chunk = ((long long)n_frames + want - 1) / want;
  chunk = std::min<long long>(std::max<long long>(chunk, kMinChunk), kMaxChunk);
  const unsigned by = (unsigned)(((long long)n_frames + chunk - 1) / chunk);  // <= 2^31 / 2^16
  auto* out = reinterpret_cast<unsigned long long*>(out_sum);
  const dim3 grid((unsigned)bx, by), block(kThreads);
  if (vec) {
    if (sel)
      hipLaunchKernelGGL(stack_sum_vec_kernel<true>, grid, block, 0, s, frames, n_frames, (size_t)n_px, (int)chunk, sel,
                         out);
    else
      hipLaunchKernelGGL(stack_sum_vec_kernel<false>, grid, block, 0, s, frames, n_frames, (size_t)n_px, (int)chunk,
                         sel, out);
  } else {
    if (sel)
      hipLaunchKernelGGL(stack_sum_elem_kernel<true>, grid, block, 0, s, frames, n_frames, (size_t)n_px, (int)chunk,
                         sel, out);
    else
      hipLaunchKernelGGL(stack_sum_elem_kernel<false>, grid, block, 0, s, frames, n_frames, (size_t)n_px, (int)chunk,
                         sel, out);
  }
  return launch_check("stack_sum_u16_kernel");
}

extern "C" int kcmc_frame_stats_u16(kcmc_ctx* ctx, const uint16_t* frames, int n_frames, int H, int W,
                                    const uint16_t* ref, int y0, int y1, int x0, int x1, long long* out,
                                    kcmc_stream_t stream) {
  KCMC_TRY(check_rect("kcmc_frame_stats_u16", ctx, n_frames, n_frames, H, W, y0, y1, x0, x1, 0, nullptr));
  if (n_frames == 0) return KCMC_OK;
  KCMC_TRY(check_pointers("kcmc_frame_stats_u16", frames, n_frames, ref, out));
  hipStream_t s = (hipStream_t)stream;
  KCMC_TRY(hip_check(hipMemsetAsync(out, 0, (size_t)n_frames * 5 * sizeof(long long), s), "hipMemsetAsync"));
  const bool vec = rows_vectorizable(W, frames, ref);
  const long long per_row = vec ? (x1 + 7) / 8 - x0 / 8 : x1 - x0;
  const long long items = (long long)(y1 - y0) * per_row;
  // workgroups per frame: fill the device when the frames are few, at least 4 items per thread
  long long by = (2 * kTargetBlocks + n_frames - 1) / n_frames;
  by = std::min<long long>(by, (items + 4 * kThreads - 1) / (4 * kThreads));
  by = std::min<long long>(std::max<long long>(by, 1), 4096);
  auto* o = reinterpret_cast<unsigned long long*>(out);
  const dim3 grid((unsigned)n_frames, (unsigned)by), block(kThreads);
  if (vec)
    hipLaunchKernelGGL(frame_stats_kernel<true>, grid, block, 0, s, frames, H, W, ref, y0, y1, x0, x1, o);
  else
    hipLaunchKernelGGL(frame_stats_kernel<false>, grid, block, 0, s, frames, H, W, ref, y0, y1, x0, x1, o);
  KCMC_TRY(launch_check("frame_stats_u16_kernel"));
  return n_frames > 1 ? launch_copy_b(o, (size_t)n_frames, n_frames, s) : KCMC_OK;
}

// q2: summary images of an aligned stack -- one streaming reduction of a uint16 stack
// [F, H, W] per pixel over time, beside q1 (quality.hip).  Build-defined: the reference has
// no such pass.  Every sum is an exact integer, so the result does not depend on the order
// in which workgroups finish.
//
//   kcmc_temporal_sums_u16   for every pixel p of a rectangle, over the selected frames f:
//     plane 0  sum a_f            plane 2  sum a_f * right_f        (y, x + 1)
//     plane 1  sum a_f^2          plane 3  sum a_f * down_f         (y + 1, x)
//     max      max a_f            plane 4  sum a_f * down-right_f   (y + 1, x + 1)   neighbours = 8
//                                 plane 5  sum a_f * down-left_f    (y + 1, x - 1)   neighbours = 8
//   what the max projection, the temporal standard deviation and the local correlation image
//   need (finished on the host in exact integers, kcmc_amd.summary).  A pair whose partner
//   lies outside the rectangle sums to 0.
//
// Layout: q1's stack sum with a two-dimensional tile.  A workgroup owns kRG rows x 8 * kCT
// columns of the image grid of 8-pixel vectors (x0 / 8 .. ceil(x1 / 8)) and a chunk of at
// most 65536 frames (sum a stays 32-bit: 65536 * 65535 < 2^32; the products are u16 x u16,
// one 32 x 32 + 64-bit multiply-add each).  A thread owns one vector -- eight neighbouring
// pixels of a row -- in every frame of the chunk and keeps all its sums in registers.  Per
// frame it loads its own vector, the vector below it and the three pixels beside them
// (right, down-right, down-left); everything outside the rectangle is masked to 0, which
// removes it from every sum.  The vector below is the own vector of the thread kCT lanes
// further on and the three pixels are in the neighbouring threads' vectors, so apart from
// the tile's bottom row and its side columns every second read is of a line the workgroup
// has just loaded (cache, not HBM); neighbouring tiles get neighbouring ids on one XCD
// (xcd_remap), so that the halo lines meet in one L2.  The next frame's loads are in flight
// while a frame is summed.
//
// The chunks of one tile meet in the output: one 64-bit atomicAdd per plane and pixel,
// crossed through LDS so that a wave instruction covers 512 contiguous bytes, and one
// compare-and-swap maximum per pixel on the aligned 32-bit word that holds it (gfx950 has
// no 16-bit integer atomics); zeros are skipped, so nothing outside the rectangle is touched.
//
// VEC needs frame rows on 16-byte boundaries (W % 8 == 0, 16-byte aligned frames);
// everything else -- odd widths, a slab view that starts mid-allocation -- gathers the same
// vectors element by element, every element checked against W.
#include "u16_rows.h"

namespace kcmc {
namespace {

constexpr int kThreads = 256;
constexpr int kCtLog2 = 4;                                // 16 thread columns x 16 rows: 128 x 16 px
constexpr int kCT = 1 << kCtLog2, kRG = kThreads / kCT;
constexpr int kTileW = 8 * kCT;
constexpr int kMinChunk = 32;       // as q1: few atomic bytes per byte read
constexpr int kMaxChunk = 65536;    // 32-bit sum a
constexpr int kTargetBlocks = 2048; // 256 CUs x 8 resident workgroups

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  const us2 m = __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b));
  return __builtin_bit_cast(uint32_t, m);
}

// *word = per-half max(*word, v): a half of v that is 0 leaves its half of the word alone.
__device__ __forceinline__ void atomic_pk_max_u16(uint32_t* word, uint32_t v) {
  uint32_t old = __atomic_load_n(word, __ATOMIC_RELAXED);
  for (;;) {
    const uint32_t want = pk_max_u16(old, v);
    if (want == old) return;
    const uint32_t seen = atomicCAS(word, old, want);
    if (seen == old) return;
    old = seen;
  }
}

// What a thread reads of one frame: its vector, the one below, and the pixels right of its
// vector, right of the one below and left of the one below.
struct Taps {
  uint4 a = make_uint4(0u, 0u, 0u, 0u), b = make_uint4(0u, 0u, 0u, 0u);
  uint32_t ar = 0u, br = 0u, bl = 0u;
};

// Which of them exist for this thread (inside the rectangle), constant over the frames.
struct Have {
  bool a, b, r, br, bl;
};

template <bool VEC>
__device__ __forceinline__ Taps load_taps(const uint16_t* __restrict__ row, int c0, int W, const Have& h) {
  Taps t;  // row: the thread's image row in this frame
  if (h.a) t.a = load8<VEC>(row, c0, W);
  if (h.b) t.b = load8<VEC>(row + W, c0, W);
  if (h.r) t.ar = row[c0 + 8];
  if (h.br) t.br = row[W + c0 + 8];
  if (h.bl) t.bl = row[W + c0 - 1];
  return t;
}

template <int NB>
struct Acc {
  static constexpr int kPairs = NB / 2;
  uint32_t s0[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  u64 s1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  u64 pair[kPairs][8] = {};
  uint32_t mx[4] = {0u, 0u, 0u, 0u};  // two pixels per word, as loaded

  // m: the rectangle's column mask of this thread's vector.
  __device__ __forceinline__ void add(const Taps& t, const uint4& m) {
    const uint4 a = make_uint4(t.a.x & m.x, t.a.y & m.y, t.a.z & m.z, t.a.w & m.w);
    const uint4 b = make_uint4(t.b.x & m.x, t.b.y & m.y, t.b.z & m.z, t.b.w & m.w);
    uint32_t A[9], B[10];  // A[j] = a[j], A[8] right of it; B[j + 1] = below a[j]
    unpack8(a, A);
    unpack8(b, B + 1);
    A[8] = t.ar;
    B[0] = t.bl;
    B[9] = t.br;
    mx[0] = pk_max_u16(mx[0], a.x);
    mx[1] = pk_max_u16(mx[1], a.y);
    mx[2] = pk_max_u16(mx[2], a.z);
    mx[3] = pk_max_u16(mx[3], a.w);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s0[j] += A[j];
      s1[j] += (u64)A[j] * A[j];
      pair[0][j] += (u64)A[j] * A[j + 1];
      pair[1][j] += (u64)A[j] * B[j + 1];
      if (NB == 8) {
        pair[2][j] += (u64)A[j] * B[j + 2];
        pair[3][j] += (u64)A[j] * B[j];
      }
    }
  }
};

// grid (tiles * chunks), block 256 = kCT thread columns x kRG rows.  out_sums [2 + NB / 2, H, W]
// and out_max [H, W] zeroed before the launch.
template <bool VEC, bool SEL, int NB>
__global__ __launch_bounds__(kThreads) void temporal_sums_kernel(
    const uint16_t* __restrict__ frames, int n_frames, int H, int W, const uint8_t* __restrict__ sel, int y0, int y1,
    int x0, int x1, int tiles_x, int n_tiles, int chunk, u64* __restrict__ out_sums, uint16_t* __restrict__ out_max) {
  __shared__ u64 s[8 * kThreads];
  const int tid = threadIdx.x;
  const int id = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int tile = id % n_tiles, tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
  const int f0 = (id / n_tiles) * chunk;
  const int f1 = min(f0 + chunk, n_frames);
  const int tx = tid & (kCT - 1), ty = tid >> kCtLog2;
  const int xg = x0 & ~7;
  const int ya = y0 + tile_y * kRG, xa = xg + tile_x * kTileW;  // the tile's first row and column
  const int y = ya + ty, c0 = xa + 8 * tx;
  Have h;
  h.a = y < y1 && c0 < x1;
  h.b = h.a && y + 1 < y1;
  h.r = h.a && c0 + 8 < x1;
  h.br = h.b && c0 + 8 < x1;
  h.bl = h.b && c0 - 1 >= x0;
  const uint4 m = mask8(make_uint4(~0u, ~0u, ~0u, ~0u), c0, x0, x1);
  const size_t n_px = (size_t)H * W;
  const size_t o = h.a ? (size_t)y * W : 0;  // the thread's row in a frame

  Acc<NB> acc;
  // The frames roll through registers: frame f + 1's loads are issued before frame f is summed,
  // and its selection flag one trip before its loads, so that no trip waits for a load it has
  // only just issued.  (The selection is uniform over the workgroup; an unselected frame is
  // neither loaded nor summed.)
  auto selected = [&](int g) { return g < f1 && (!SEL || sel[g]); };
  auto fetch = [&](int g, bool on) {
    Taps t;
    if (on) t = load_taps<VEC>(frames + (size_t)g * n_px + o, c0, W, h);
    return t;
  };
  bool cur = selected(f0), on = selected(f0 + 1);
  Taps t = fetch(f0, cur);
  for (int f = f0; f < f1; ++f) {
    const bool on_next = selected(f + 2);
    const Taps n = fetch(f + 1, on);
    if (!SEL || cur) acc.add(t, m);
    t = n;
    cur = on;
    on = on_next;
  }

  // The planes cross LDS one by one: s is the tile row by row, thread tid's pixels at 8 * tid.
  constexpr int K = 2 + NB / 2;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      s[8 * tid + j] = k == 0 ? (u64)acc.s0[j] : k == 1 ? acc.s1[j] : acc.pair[k < 2 ? 0 : k - 2][j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int p = j * kThreads + tid;
      const int yy = ya + p / kTileW, xx = xa + p % kTileW;
      const u64 v = s[p];
      if (v) atomicAdd(&out_sums[(size_t)k * n_px + (size_t)yy * W + xx], v);  // v != 0: inside the rectangle
    }
    __syncthreads();
  }
  if (h.a) {
    uint32_t* words = reinterpret_cast<uint32_t*>(out_max);  // 4-byte aligned (checked by the entry)
    for_each_px(make_uint4(acc.mx[0], acc.mx[1], acc.mx[2], acc.mx[3]), [&](int j, uint32_t px) {
      const size_t i = o + (size_t)(c0 + j);
      if (px) atomic_pk_max_u16(words + (i >> 1), px << (16 * (int)(i & 1)));
    });
  }
}

template <bool VEC, bool SEL>
void launch_nb(int nb, dim3 grid, hipStream_t s, const uint16_t* frames, int n_frames, int H, int W, const uint8_t* sel,
               int y0, int y1, int x0, int x1, int tiles_x, int n_tiles, int chunk, u64* out_sums, uint16_t* out_max) {
  if (nb == 8)
    hipLaunchKernelGGL((temporal_sums_kernel<VEC, SEL, 8>), grid, dim3(kThreads), 0, s, frames, n_frames, H, W, sel, y0,
                       y1, x0, x1, tiles_x, n_tiles, chunk, out_sums, out_max);
  else
    hipLaunchKernelGGL((temporal_sums_kernel<VEC, SEL, 4>), grid, dim3(kThreads), 0, s, frames, n_frames, H, W, sel, y0,
                       y1, x0, x1, tiles_x, n_tiles, chunk, out_sums, out_max);
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_temporal_sums_u16(kcmc_ctx* ctx, const uint16_t* frames, int n_frames, int H, int W,
                                      const uint8_t* sel, int y0, int y1, int x0, int x1, int neighbours,
                                      long long* out_sums, uint16_t* out_max, kcmc_stream_t stream) {
  const char* fn = "kcmc_temporal_sums_u16";
  KCMC_TRY(check_rect(fn, ctx, n_frames, n_frames, H, W, y0, y1, x0, x1, 0, nullptr));
  KCMC_TRY(check_pointers(fn, frames, n_frames, out_max, out_sums));
  if (((uintptr_t)out_max & 3) != 0) return fail(KCMC_EINVAL, std::string(fn) + ": out_max must be 4-byte aligned");
  if (neighbours != 4 && neighbours != 8) return fail(KCMC_EINVAL, std::string(fn) + ": neighbours must be 4 or 8");
  hipStream_t s = (hipStream_t)stream;
  const size_t n_px = (size_t)H * W;
  const int K = 2 + neighbours / 2;
  KCMC_TRY(hip_check(hipMemsetAsync(out_sums, 0, (size_t)K * n_px * sizeof(long long), s), "hipMemsetAsync"));
  KCMC_TRY(hip_check(hipMemsetAsync(out_max, 0, n_px * sizeof(uint16_t), s), "hipMemsetAsync"));
  if (n_frames == 0) return KCMC_OK;

  const int nvec = (x1 + 7) / 8 - x0 / 8;
  const int tiles_x = ceil_div(nvec, kCT);
  const long long n_tiles = (long long)tiles_x * ceil_div(y1 - y0, kRG);  // < 2^31 / 2048 + H + W
  // enough chunks to fill the device, none shorter than kMinChunk or longer than kMaxChunk
  const long long want = (kTargetBlocks + n_tiles - 1) / n_tiles;
  long long chunk = ((long long)n_frames + want - 1) / want;
  chunk = std::min<long long>(std::max<long long>(chunk, kMinChunk), kMaxChunk);
  const long long blocks = n_tiles * (((long long)n_frames + chunk - 1) / chunk);
  if (blocks > 0x7fffffffll) return fail(KCMC_EUNSUPPORTED, std::string(fn) + ": too many tiles and frame chunks");
  auto* o = reinterpret_cast<unsigned long long*>(out_sums);
  const dim3 grid((unsigned)blocks);
  const bool vec = rows_vectorizable(W, frames, frames);
#define KCMC_Q2_LAUNCH(VEC, SEL)                                                                                 \
  launch_nb<VEC, SEL>(neighbours, grid, s, frames, n_frames, H, W, sel, y0, y1, x0, x1, tiles_x, (int)n_tiles, \
                      (int)chunk, o, out_max)
  if (vec) {
    if (sel)
      KCMC_Q2_LAUNCH(true, true);
    else
      KCMC_Q2_LAUNCH(true, false);
  } else {
    if (sel)
      KCMC_Q2_LAUNCH(false, true);
    else
      KCMC_Q2_LAUNCH(false, false);
  }
#undef KCMC_Q2_LAUNCH
  return launch_check("temporal_sums_kernel");
}

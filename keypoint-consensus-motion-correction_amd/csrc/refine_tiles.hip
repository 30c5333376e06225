// g2: gradient sums per tile -- the right-hand sides of one linearised least-squares step of
// every frame against a reference image on every patch of a tiling, from one read of the
// stack, for the non-rigid intensity refinement (kcmc_amd.refine_field).  Build-defined: the
// reference has no such mode.
//
//   out[s][i][j] = (Sa, Saa, Sab, Sagx, Sagy) over the rows [row_edges[i], row_edges[i + 1]) and
//                  the columns [col_edges[j], col_edges[j + 1]):
//     a  = frame[frame_idx[s]][y][x],  b = ref[y][x]
//     gx = ref[y][x + 1] - ref[y][x - 1],  gy = ref[y + 1][x] - ref[y - 1][x]
//
// One workgroup owns one (frame, tile row) and leaves its tx * 5 sums with plain stores: no
// global atomics, no memset, nothing depends on the order in which workgroups finish.
//
// The covered columns [col_edges[0], col_edges[tx]) are walked as in g1 (refine.hip): the
// 8-pixel vectors of the image grid, 256 threads = CT thread columns x RG row groups, a thread
// owns one vector column per chunk of CT vectors and walks the rows of its row group, so
//   * the frame is read once, one 16-byte load per thread and row, issued two rows before
//     the row is summed (the 40 accumulators leave room for three waves per SIMD only, so
//     the loads have to be further ahead than g1's);
//   * ref rows y - 1, y, y + 1 roll through registers, row y + 2 on its way; ref[y][c0 - 1] and
//     ref[y][c0 + 8] come from the neighbouring lanes, and from memory at the ends of a wave's
//     row segment;
//   * the mask of the covered columns zeroes a only, never b.
// Tile edges are arbitrary, so a vector may straddle any number of tile columns.  A thread
// therefore keeps its five sums PER PIXEL COLUMN (40 accumulators; the same four products per
// pixel as g1, whose coordinate moments are gone) and sorts the columns into tiles only once
// per chunk, after its last row: consecutive columns of one tile are added in registers and
// each run goes to the workgroup's tx * 5 totals in LDS with 64-bit integer atomic adds --
// integer addition is associative, so their order cannot change a bit.  Neighbouring lanes
// mostly add to the same tile, and an LDS atomic serialises the lanes that share an address,
// so the totals are kept in 16 copies (lane % 16 picks one) that are added at the end.
//
// Exact: every sum is a 64-bit integer in two's complement.  A tile has fewer than 2^31
// pixels (H * W < 2^31) and every product is below 2^32 in magnitude, so no tile sum reaches
// 2^63; intermediate values are kept in unsigned arithmetic, where wrapping is harmless.
//
// VEC needs frame rows on 16-byte boundaries (W % 8 == 0, 16-byte aligned frames and ref);
// everything else gathers the same 8-pixel vectors element by element.
#include "u16_rows.h"

namespace kcmc {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxTiles = 32;  // per axis
constexpr int kCopies = 16;    // of the workgroup's totals in LDS, one per lane residue

typedef long long i64;

struct TileEdges {  // by value in the kernel's arguments: no upload, no sync
  int32_t row[kMaxTiles + 1];
  int32_t col[kMaxTiles + 1];
};

// grid (n_sel * ty), block 256 = (1 << ct_log2) thread columns x row groups.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void tile_gradient_sums_kernel(
    const uint16_t* __restrict__ frames, int n_frames, int H, int W, const int32_t* __restrict__ frame_idx,
    const uint16_t* __restrict__ ref, const TileEdges e, int ty, int tx, int ct_log2, u64* __restrict__ out) {
  // + 1: copy c starts 2 c banks on, so lanes adding to one entry of different copies do not collide
  __shared__ u64 tot[kCopies][kMaxTiles * 5 + 1];
  __shared__ int32_t ce[kMaxTiles + 1];
  const unsigned blk = blockIdx.x;
  const int s = (int)(blk / (unsigned)ty), ti = (int)(blk - (unsigned)s * (unsigned)ty);
  u64* o = out + (size_t)blk * tx * 5;
  const int tid = threadIdx.x;
  const int f = frame_idx ? frame_idx[s] : s;
  const int ya = e.row[ti], yb = e.row[ti + 1];  // the tile row's rows [ya, yb)
  const int x0 = e.col[0], x1 = e.col[tx];       // the covered columns
  // uniform over the workgroup: zero rows for an index outside the stack (never read through)
  // and for a tile row without pixels
  if (f < 0 || f >= n_frames || ya >= yb || x0 >= x1) {
    if (tid < tx * 5) o[tid] = 0;
    return;
  }
  for (int k = tid; k < kCopies * (kMaxTiles * 5 + 1); k += kThreads) (&tot[0][0])[k] = 0;
  if (tid <= tx) ce[tid] = e.col[tid];
  __syncthreads();

  const int CT = 1 << ct_log2, RG = kThreads >> ct_log2;
  const int tc = tid & (CT - 1), tr = tid >> ct_log2;
  const int nb = yb - ya;
  const int RB = (nb + RG - 1) / RG;  // rows per row group (uniform trip count)
  const int r0 = ya + tr * RB;        // this thread's rows [r0, r0 + nr)
  const int nr = max(0, min(RB, yb - r0));
  const int xg = x0 & ~7;
  const int nvec = ((x1 + 7) >> 3) - (x0 >> 3);
  const int em = min(CT, 64) - 1;  // a wave's row segment: min(CT, 64) neighbouring lanes
  const uint16_t* fr = frames + (size_t)f * H * W;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  for (int vb = 0; vb < nvec; vb += CT) {
    const int v = vb + tc;
    const bool vok = v < nvec;
    const int c0 = xg + 8 * v;
    const bool left_edge = (tc & em) == 0;
    const bool right_edge = (tc & em) == em || v == nvec - 1;  // the next lane holds no vector of this row
    u64 ca[8], caa[8], cab[8], cagx[8], cagy[8];  // per pixel column, over this thread's rows
#pragma unroll
    for (int j = 0; j < 8; ++j) ca[j] = caa[j] = cab[j] = cagx[j] = cagy[j] = 0;
    // in flight: frame rows y, y + 1 and (loaded below) y + 2; ref rows y - 1, y, y + 1 and y + 2
    uint4 bm = zero, b0 = zero, bp = zero, a_cur = zero, a_nxt = zero;
    if (vok && nr > 0) {
      bm = load8<VEC>(ref + (size_t)(r0 - 1) * W, c0, W);  // r0 - 1 >= row_edges[0] - 1 >= 0
      b0 = load8<VEC>(ref + (size_t)r0 * W, c0, W);
      bp = load8<VEC>(ref + (size_t)(r0 + 1) * W, c0, W);  // r0 + 1 <= row_edges[ty] <= H - 1
      a_cur = load8<VEC>(fr + (size_t)r0 * W, c0, W);
      if (nr > 1) a_nxt = load8<VEC>(fr + (size_t)(r0 + 1) * W, c0, W);
    }
    for (int i = 0; i < RB; ++i) {  // every thread makes every trip: the lanes exchange ref pixels
      const int y = r0 + i;
      const bool ok = vok && i < nr;
      uint4 bq = zero, a_far = zero;
      if (vok && i + 1 < nr) bq = load8<VEC>(ref + (size_t)(y + 2) * W, c0, W);  // y + 2 <= r0 + nr <= H - 1
      if (vok && i + 2 < nr) a_far = load8<VEC>(fr + (size_t)(y + 2) * W, c0, W);
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
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ca[j] += (uint32_t)a[j];
        caa[j] += (u64)(uint32_t)a[j] * (uint32_t)a[j];
        cab[j] += (u64)(uint32_t)a[j] * (uint32_t)b[j + 1];
        cagx[j] += (u64)((i64)a[j] * (b[j + 2] - b[j]));
        cagy[j] += (u64)((i64)a[j] * (dn[j] - up[j]));
      }
      bm = b0;
      b0 = bp;
      bp = bq;
      a_cur = a_nxt;
      a_nxt = a_far;
    }
    if (!vok || nr <= 0) continue;
    // the columns into their tiles: t walks the tile columns left to right with the pixel
    // columns; a run of columns in one tile is added here and goes to LDS once
    int t = 0;
    u64 run[5] = {0, 0, 0, 0, 0};
    bool any = false;
    auto flush = [&]() {
      if (any) {
#pragma unroll
        for (int k = 0; k < 5; ++k) atomicAdd(&tot[tid & (kCopies - 1)][t * 5 + k], run[k]);
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) run[k] = 0;
      any = false;
    };
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      if (c >= x0 && c < x1) {  // so ce[t + 1] > c for some t < tx: the walk stops inside the table
        if (ce[t + 1] <= c) {
          flush();
          while (ce[t + 1] <= c) ++t;
        }
        run[0] += ca[j];
        run[1] += caa[j];
        run[2] += cab[j];
        run[3] += cagx[j];
        run[4] += cagy[j];
        any = true;
      }
    }
    flush();
  }
  __syncthreads();
  if (tid < tx * 5) {
    u64 r = 0;
    for (int c = 0; c < kCopies; ++c) r += tot[c][tid];
    o[tid] = r;
  }
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_tile_gradient_sums_u16(kcmc_ctx* ctx, const uint16_t* frames, int n_frames, int H, int W,
                                           const int32_t* frame_idx, int n_sel, const uint16_t* ref,
                                           const int32_t* row_edges, int ty, const int32_t* col_edges, int tx,
                                           long long* out, kcmc_stream_t stream) {
  const std::string p = "kcmc_tile_gradient_sums_u16: ";
  if (!ctx) return fail(KCMC_EINVAL, p + "ctx is NULL");
  if (n_frames < 0 || n_sel < 0 || H <= 0 || W <= 0) return fail(KCMC_EINVAL, p + "bad shape");
  if ((long long)H * W >= (1ll << 31)) return fail(KCMC_EINVAL, p + "H * W must be < 2^31");
  if (ty < 1 || ty > kMaxTiles || tx < 1 || tx > kMaxTiles)
    return fail(KCMC_EINVAL, p + "ty and tx must be in [1, 32]");
  if (!row_edges || !col_edges) return fail(KCMC_EINVAL, p + "NULL edges");
  TileEdges e{};
  for (int i = 0; i <= ty; ++i) e.row[i] = row_edges[i];
  for (int j = 0; j <= tx; ++j) e.col[j] = col_edges[j];
  for (int i = 0; i < ty; ++i)
    if (e.row[i] > e.row[i + 1]) return fail(KCMC_EINVAL, p + "row_edges must be non-decreasing");
  for (int j = 0; j < tx; ++j)
    if (e.col[j] > e.col[j + 1]) return fail(KCMC_EINVAL, p + "col_edges must be non-decreasing");
  if (e.row[0] < 1 || e.row[ty] > H - 1 || e.col[0] < 1 || e.col[tx] > W - 1)
    return fail(KCMC_EINVAL, p + "the tiling grown by 1 leaves the image");
  if (n_sel == 0) return KCMC_OK;
  KCMC_TRY(check_pointers("kcmc_tile_gradient_sums_u16", frames, n_frames, ref, out));
  const long long blocks = (long long)n_sel * ty;
  if (blocks > 0x7fffffffll) return fail(KCMC_EUNSUPPORTED, p + "n_sel * ty too large");

  const bool vec = rows_vectorizable(W, frames, ref);
  const int ct_log2 = thread_columns_log2((e.col[tx] + 7) / 8 - e.col[0] / 8);
  auto* o = reinterpret_cast<unsigned long long*>(out);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(kThreads);
  if (vec)
    hipLaunchKernelGGL(tile_gradient_sums_kernel<true>, grid, block, 0, s, frames, n_frames, H, W, frame_idx, ref, e,
                       ty, tx, ct_log2, o);
  else
    hipLaunchKernelGGL(tile_gradient_sums_kernel<false>, grid, block, 0, s, frames, n_frames, H, W, frame_idx, ref, e,
                       ty, tx, ct_log2, o);
  return launch_check("tile_gradient_sums_kernel");
}

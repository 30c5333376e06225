// b1: bidirectional-scan phase correction -- the constant horizontal offset of the odd rows of a
// uint16 stack against its even rows (a two-photon microscope that acquires odd rows on the
// return sweep with a line clock that is slightly off).  Build-defined: the reference has no
// such mode.  The semantics are in include/kcmc.h; kcmc_amd.bidi finishes the sums.
//
//   kcmc_bidi_phase_sums_u16  out[s][d + R] = (Sa, Sb, Saa, Sbb, Sab) over every vertically adjacent
//                             row pair and the columns x in [R, W - R), a = odd row at x + d,
//                             b = even row at x: the moments of kcmc_frame_stats_u16.
//   kcmc_shift_rows_u16       the rows of one parity moved by d columns, the edge replicated.
//
// Phase sums.  Every pair has exactly one odd row, so the work is organised by odd row y: its
// pairs are (y - 1, y) and, when y + 1 < H, (y, y + 1).  A workgroup owns whole odd rows and walks
// each in tiles of kTW columns; per tile it stages the odd row with a halo of 16 pixels (zeros
// outside the image) and bs = b_up + b_dn (17 bits, zero outside [R, W - R)) in LDS.
//   Sab   sum of a(x + d) bs(x): one 32 x 32 + 64-bit multiply-add per d and column for both pairs of
//         the row.  Thread (d, c) owns shift d and every CH-th column from c, CH = 256 / (2R + 1).
//   Sb, Sbb  do not depend on d: summed while bs is staged, left in entry d = -R and copied to
//         the other entries by launch_copy_b.
//   Sa, Saa  the sum over [R + d, W - R + d) is the whole row's minus the columns left and right
//         of that window, all of which lie in the first and the last 2R columns: the row totals
//         are summed while the row is staged, 4R threads sum one edge column each, and entry d
//         subtracts its prefix of the left and its suffix of the right columns at the end.  An
//         odd row counts once per pair (m = 1 or 2).
// Every sum is a 64-bit integer (H * W < 2^31 samples of less than 2^32 each), the workgroup's
// partial sums are non-negative and leave as 64-bit integer atomics into the zeroed output, so
// the result is exact and independent of the order in which workgroups finish.
//
// Row shift.  A workgroup owns whole rows: it loads a batch of rows into LDS -- all loads before
// the barrier, so a row is read completely before any of it is written and src == dst is safe --
// and writes each from the LDS image displaced by d.  With rows on 16-byte boundaries the row
// sits in LDS between 16 replicated edge pixels on each side and the output vector at column x is
// the five aligned 32-bit words around LDS column x + d, realigned by 16 bits when d is odd:
// 16-byte global loads and stores only, no clamp.  Everything else (odd widths, a view that
// starts mid-allocation, rows too long for the padded LDS image) moves element by element and
// clamps the LDS index.  In place only the rows of the parity are visited.
#include "u16_rows.h"

namespace kcmc {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxR = 16;

// ------------------------------------------------------------------------------ phase sums
constexpr int kTW = 1024;         // tile columns (a multiple of 8)
constexpr int kHalo = 16;         // staged on both sides of a tile: >= kMaxR, a multiple of 8
constexpr int kSumWGs = 2048;     // 256 CUs x 8 resident workgroups

// grid (n_sel, workgroups per frame); out zeroed before the launch.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void bidi_sums_kernel(const uint16_t* __restrict__ frames, int n_frames, int H,
                                                             int W, const int32_t* __restrict__ frame_idx, int R,
                                                             u64* __restrict__ out) {
  __shared__ uint4 a_s[(kTW + 2 * kHalo) / 8];
  __shared__ uint32_t bs_s[kTW];
  __shared__ u64 red[4][kThreads / 64];
  __shared__ u64 tot[4];
  __shared__ u64 edge[2][4 * kMaxR];
  __shared__ u64 part[kThreads];
  const int s = blockIdx.x;
  const int f = frame_idx ? frame_idx[s] : s;
  if (f < 0 || f >= n_frames) return;  // uniform over the workgroup: the row stays zero
  uint16_t* A = reinterpret_cast<uint16_t*>(a_s);
  const uint16_t* fr = frames + (size_t)f * H * W;
  const int tid = threadIdx.x;
  const int S = 2 * R + 1, CH = kThreads / S;
  const int d = tid / CH, c = tid - d * CH;  // d >= S: idle in the products
  const int x_lo = R, x_hi = W - R;          // the columns of b
  // thread j < 4R sums image column j (j < 2R) or W - 4R + j (the last 2R columns)
  const int ecol = tid < 2 * R ? tid : W - 4 * R + tid;
  u64 sab = 0, ta = 0, taa = 0, sb = 0, sbb = 0, ea = 0, eaa = 0;

  for (int y = 1 + 2 * (int)blockIdx.y; y < H; y += 2 * (int)gridDim.y) {
    const bool dn = y + 1 < H;
    const u64 m = dn ? 2 : 1;
    const uint16_t* arow = fr + (size_t)y * W;
    const uint16_t* urow = arow - W;
    const uint16_t* drow = arow + W;  // read only when dn
    if (tid < 4 * R) {
      const u64 v = arow[ecol];
      ea += m * v;
      eaa += m * v * v;
    }
    u64 ra = 0, raa = 0;  // this thread's part of the row's totals
    for (int tx0 = 0; tx0 < W; tx0 += kTW) {
      if (VEC) {
        for (int i = tid; i < (kTW + 2 * kHalo) / 8; i += kThreads) {
          const int gx = tx0 - kHalo + 8 * i;
          uint4 q = make_uint4(0u, 0u, 0u, 0u);
          if (gx >= 0 && gx < W) {  // W and gx are multiples of 8
            q = *reinterpret_cast<const uint4*>(arow + gx);
            if (gx >= tx0 && gx < tx0 + kTW)
              for_each_px(q, [&](int, uint32_t px) {
                ra += px;
                raa += (u64)px * px;
              });
          }
          a_s[i] = q;
        }
        for (int i = tid; i < kTW / 8; i += kThreads) {
          const int gx = tx0 + 8 * i;
          uint32_t bu[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, bd[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
          if (gx < W && gx + 8 > x_lo && gx < x_hi) {
            unpack8(mask8(*reinterpret_cast<const uint4*>(urow + gx), gx, x_lo, x_hi), bu);
            if (dn) unpack8(mask8(*reinterpret_cast<const uint4*>(drow + gx), gx, x_lo, x_hi), bd);
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            bs_s[8 * i + j] = bu[j] + bd[j];
            sb += bu[j] + bd[j];
            sbb += (u64)bu[j] * bu[j] + (u64)bd[j] * bd[j];
          }
        }
      } else {
        for (int i = tid; i < kTW + 2 * kHalo; i += kThreads) {
          const int gx = tx0 - kHalo + i;
          uint32_t v = 0;
          if (gx >= 0 && gx < W) {
            v = arow[gx];
            if (gx >= tx0 && gx < tx0 + kTW) {
              ra += v;
              raa += (u64)v * v;
            }
          }
          A[i] = (uint16_t)v;
        }
        for (int i = tid; i < kTW; i += kThreads) {
          const int gx = tx0 + i;
          uint32_t bu = 0, bd = 0;
          if (gx >= x_lo && gx < x_hi) {
            bu = urow[gx];
            if (dn) bd = drow[gx];
          }
          bs_s[i] = bu + bd;
          sb += bu + bd;
          sbb += (u64)bu * bu + (u64)bd * bd;
        }
      }
      __syncthreads();
      if (d < S) {
        const int xa = max(0, x_lo - tx0), xb = min(kTW, x_hi - tx0);  // the tile's columns of b
        const uint16_t* a = A + kHalo - R + d;                         // a[x] = odd row at tx0 + x + (d - R)
        for (int x = xa + c; x < xb; x += CH) sab += (u64)(uint32_t)a[x] * bs_s[x];
      }
      __syncthreads();  // before the next tile is staged
    }
    ta += m * ra;
    taa += m * raa;
  }

  const u64 v[4] = {ta, taa, sb, sbb};
  const u64 t = block_sums(v, red);
  if (tid < 4) tot[tid] = t;
  if (tid < 4 * R) {
    edge[0][tid] = ea;
    edge[1][tid] = eaa;
  }
  part[tid] = sab;
  __syncthreads();
  if (tid >= S) return;
  // entry tid: shift tid - R, window [tid, W - 2R + tid): without the left columns [0, tid) and the
  // right columns [W - 2R + tid, W), the latter edge[2R + tid .. 4R)
  u64 sa = tot[0], saa = tot[1], p = 0;
  for (int j = 0; j < tid; ++j) {
    sa -= edge[0][j];
    saa -= edge[1][j];
  }
  for (int j = 2 * R + tid; j < 4 * R; ++j) {
    sa -= edge[0][j];
    saa -= edge[1][j];
  }
  for (int j = 0; j < CH; ++j) p += part[tid * CH + j];
  u64* e = out + ((size_t)s * S + tid) * 5;
  if (sa) atomicAdd(e + 0, sa);
  if (saa) atomicAdd(e + 2, saa);
  if (p) atomicAdd(e + 4, p);
  if (tid == 0) {
    if (tot[2]) atomicAdd(e + 1, tot[2]);
    if (tot[3]) atomicAdd(e + 3, tot[3]);
  }
}

// ------------------------------------------------------------------------------- row shift
constexpr int kPad = 16;               // replicated edge pixels on each side of a row in LDS: >= |d|
constexpr int kBatchBytes = 16384;     // LDS of a batch of rows (a longer row is a batch of its own)
constexpr int kMaxBatchRows = 8;
constexpr int kMaxLds = 65536;
constexpr int kShiftWGs = 16384;

// LDS elements per row.  VEC: the row between its pads, one spare word for the realigning read,
// rounded to whole 16-byte vectors.
inline int row_stride(bool vec, int W) { return vec ? (W + 2 * kPad + 2 + 7) / 8 * 8 : W; }

// Job j names a row: out of place every row of the stack in order (only_parity = 0), in place the
// rows of the parity (H2 of them per frame).  Returns the row's offset in elements and whether it
// is shifted.  j is uniform over the workgroup, so this is scalar work.
__device__ __forceinline__ size_t job_row(long long j, int H, int W, int parity, int H2, bool only_parity,
                                          bool& shifted) {
  if (only_parity) {
    const long long f = j / H2;
    const int y = parity + 2 * (int)(j - f * H2);
    shifted = true;
    return ((size_t)f * H + y) * W;
  }
  shifted = ((int)(j % H) & 1) == parity;
  return (size_t)j * W;
}

// grid: workgroups that stride over the batches of `rpb` rows; dynamic LDS rpb * RS u16.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void shift_rows_kernel(const uint16_t* src, uint16_t* dst, long long jobs,
                                                              int H, int W, int parity, int H2, int only_parity,
                                                              int d, int rpb, int RS) {
  extern __shared__ uint4 smem[];
  uint16_t* L = reinterpret_cast<uint16_t*>(smem);
  const int tid = threadIdx.x;
  const long long batches = (jobs + rpb - 1) / rpb;
  for (long long b = blockIdx.x; b < batches; b += gridDim.x) {
    const long long j0 = b * rpb;
    const int nr = (int)min((long long)rpb, jobs - j0);
    for (int r = 0; r < nr; ++r) {  // every load of the batch before the barrier
      bool sh;
      const uint16_t* row = src + job_row(j0 + r, H, W, parity, H2, only_parity, sh);
      uint16_t* l = L + r * RS;
      if (VEC) {
        for (int x = 8 * tid; x < W; x += 8 * kThreads)
          *reinterpret_cast<uint4*>(l + kPad + x) = *reinterpret_cast<const uint4*>(row + x);
        // the pads, the right one with the spare word: LDS columns [0, kPad) and [kPad + W, RS)
        if (tid < kPad) l[tid] = row[0];
        for (int k = kPad + W + tid; k < RS; k += kThreads) l[k] = row[W - 1];
      } else {
        for (int x = tid; x < W; x += kThreads) l[x] = row[x];
      }
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      bool sh;
      uint16_t* row = dst + job_row(j0 + r, H, W, parity, H2, only_parity, sh);
      const uint16_t* l = L + r * RS;
      const int dd = sh ? d : 0;
      if (VEC) {
        for (int x = 8 * tid; x < W; x += 8 * kThreads) {
          const int e = kPad + x + dd;  // >= 0: |d| <= kPad
          const uint32_t* w = reinterpret_cast<const uint32_t*>(l) + (e >> 1);
          uint4 q;
          if (e & 1) {  // uniform: the parity of d
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            q = make_uint4((w0 >> 16) | (w1 << 16), (w1 >> 16) | (w2 << 16), (w2 >> 16) | (w3 << 16),
                           (w3 >> 16) | (w4 << 16));
          } else {
            q = make_uint4(w[0], w[1], w[2], w[3]);
          }
          *reinterpret_cast<uint4*>(row + x) = q;
        }
      } else {
        for (int x = tid; x < W; x += kThreads) row[x] = l[min(max(x + dd, 0), W - 1)];
      }
    }
    __syncthreads();  // before the next batch overwrites the LDS image
  }
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_bidi_phase_sums_u16(kcmc_ctx* ctx, const uint16_t* frames, int n_frames, int H, int W,
                                        const int32_t* frame_idx, int n_sel, int R, uint64_t* out,
                                        kcmc_stream_t stream) {
  const char* fn = "kcmc_bidi_phase_sums_u16";
  KCMC_TRY(check_rect(fn, ctx, n_frames, n_sel, H, W, 0, H, 0, W, 0, nullptr));
  if (R < 0 || R > kMaxR) return fail(KCMC_EINVAL, std::string(fn) + ": R must be in [0, 16]");
  if (H < 2) return fail(KCMC_EINVAL, std::string(fn) + ": H must be >= 2 (a row pair)");
  if (W < 2 * R + 1) return fail(KCMC_EINVAL, std::string(fn) + ": W must be >= 2 R + 1");
  if (n_sel == 0) return KCMC_OK;
  KCMC_TRY(check_pointers(fn, frames, n_frames, out, out));
  hipStream_t s = (hipStream_t)stream;
  const int S = 2 * R + 1;
  const size_t n_entries = (size_t)n_sel * S;
  KCMC_TRY(hip_check(hipMemsetAsync(out, 0, n_entries * 5 * sizeof(uint64_t), s), "hipMemsetAsync"));
  if (n_frames == 0) return KCMC_OK;  // every index is out of range
  // workgroups per frame: fill the device when the frames are few, whole odd rows each
  long long by = (kSumWGs + n_sel - 1) / n_sel;
  by = std::max<long long>(1, std::min<long long>(by, H / 2));
  auto* o = reinterpret_cast<u64*>(out);
  const dim3 grid((unsigned)n_sel, (unsigned)by), block(kThreads);
  if (rows_vectorizable(W, frames, frames))
    hipLaunchKernelGGL(bidi_sums_kernel<true>, grid, block, 0, s, frames, n_frames, H, W, frame_idx, R, o);
  else
    hipLaunchKernelGGL(bidi_sums_kernel<false>, grid, block, 0, s, frames, n_frames, H, W, frame_idx, R, o);
  KCMC_TRY(launch_check("bidi_sums_kernel"));
  return S > 1 ? launch_copy_b(o, n_entries, S, s) : KCMC_OK;  // Sb, Sbb of entry -R to the other entries
}

extern "C" int kcmc_shift_rows_u16(kcmc_ctx* ctx, const uint16_t* src, uint16_t* dst, int n_frames, int H, int W,
                                   int parity, int d, kcmc_stream_t stream) {
  const std::string p = "kcmc_shift_rows_u16: ";
  if (!ctx) return fail(KCMC_EINVAL, p + "ctx is NULL");
  if (n_frames < 0 || H <= 0 || W <= 0) return fail(KCMC_EINVAL, p + "bad shape");
  if (H >= 32768 || W >= 32768) return fail(KCMC_EINVAL, p + "H and W must be < 32768");
  if (parity != 0 && parity != 1) return fail(KCMC_EINVAL, p + "parity must be 0 or 1");
  if (d < -kMaxR || d > kMaxR) return fail(KCMC_EINVAL, p + "d must be in [-16, 16]");
  if (n_frames == 0) return KCMC_OK;
  if (!src || !dst) return fail(KCMC_EINVAL, p + "NULL pointer");
  const size_t n = (size_t)n_frames * H * W;
  const bool in_place = src == dst;
  if (!in_place && (uintptr_t)src < (uintptr_t)(dst + n) && (uintptr_t)dst < (uintptr_t)(src + n))
    return fail(KCMC_EINVAL, p + "src and dst overlap (only src == dst, in place, is allowed)");
  const int H2 = (H - parity + 1) / 2;  // rows of the parity per frame
  if (in_place && (d == 0 || H2 == 0)) return KCMC_OK;  // nothing moves
  hipStream_t s = (hipStream_t)stream;
  const long long jobs = (long long)n_frames * (in_place ? H2 : H);
  bool vec = W % 8 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  if (vec && row_stride(true, W) * 2 > kMaxLds) vec = false;  // the padded row does not fit in LDS
  const int RS = row_stride(vec, W);
  const int rpb = std::max(1, std::min(kMaxBatchRows, kBatchBytes / (RS * 2)));
  const size_t lds = (size_t)rpb * RS * 2;  // <= 65536: W < 32768
  const long long batches = (jobs + rpb - 1) / rpb;
  const dim3 grid((unsigned)std::min<long long>(batches, kShiftWGs)), block(kThreads);
  if (vec)
    hipLaunchKernelGGL(shift_rows_kernel<true>, grid, block, lds, s, src, dst, jobs, H, W, parity, H2,
                       (int)in_place, d, rpb, RS);
  else
    hipLaunchKernelGGL(shift_rows_kernel<false>, grid, block, lds, s, src, dst, jobs, H, W, parity, H2,
                       (int)in_place, d, rpb, RS);
  return launch_check("shift_rows_kernel");
}

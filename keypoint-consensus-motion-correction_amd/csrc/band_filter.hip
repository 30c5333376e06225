// p1: the box band-pass prefilter in front of keypoint detection -- for every pixel of a uint16
// stack the rounded mean over a (2s + 1)^2 box minus the rounded mean over a (2r + 1)^2 box, both
// clipped to the image, floored at 0.  Build-defined: the reference has no such mode.  The
// semantics are in include/kcmc.h; kcmc_amd.prefilter is the host side.
//
//   kcmc_box_bandpass_u16   dst = max(m_s - m_r, 0), m_rho = (S_rho + n_rho / 2) / n_rho
//
// One read of the stack, one write of the copy, nothing in between in HBM.  A workgroup of 256
// threads owns a strip of TW = 256 - 2R output columns (R = max(s, r)) and walks down a chunk of
// rows; thread t owns the staged column x0 - R + t, so the strip's halo of R columns on each side
// is staged with it (zero outside the image: the clipped window's sum is the sum over the staged
// one).  Per image row that enters (each exactly once per chunk, R rows before the first and
// after the last output row):
//   1. the thread loads its pixel (the next row's is already in flight),
//   2. the workgroup forms the row's exclusive prefix sums E[0 .. 256] modulo 2^32 -- a shuffle scan
//      per wave, the wave totals through LDS -- into one row of an LDS ring of 2R + 1 rows.  A box
//      sum of the row is E[t + rho + 1] - E[t - rho]: exact, because the true value is below 2^32.
//   3. every output column slides its two vertical sums: V_r gains the box sum of the entering
//      row y + r and, after the output, loses that of row y - r; V_s likewise with rows y + s and
//      y - s, which are still in the ring (s <= R).
//   4. the two rounded means and the store.
// Division: n = ny nx takes at most 65 x 65 values, ny is uniform over the workgroup and nx is fixed
// per thread.  q = trunc(float(S + n / 2) * rcp(float(n))) is within 1 of the quotient (the three
// roundings are below 2^-21 relative, the quotient is below 2^16), and one signed remainder
// S + n / 2 - q n corrects it: exact for every S <= 65535 n.
//
// Every access is one element wide, so any 2-byte aligned src / dst and any W take the same path:
// a wave reads and writes 128 contiguous bytes per instruction.  The ring is static LDS in two
// depths (R <= 12: 25 rows, 25.7 KB; R <= 32: 65 rows, 66.8 KB) so that small radii keep their
// occupancy.  Row stride 257 words: consecutive lanes read consecutive banks.
#include "kcmc_internal.h"

namespace kcmc {
namespace {

// The strip width kThreads - 2R and the cut into row chunks reach Python and the tests through
// kcmc_box_bandpass_plan only: nothing outside this file restates these constants.
constexpr int kThreads = 256;
constexpr int kRow = kThreads + 1;   // E[0 .. 256] of one staged row
constexpr int kMaxSmooth = 4;
constexpr int kMaxBackground = 32;
constexpr int kSmallR = 12;          // the shallow ring's largest R
constexpr int kMinChunkRows = 32;    // a frame is cut into row chunks only down to this height
constexpr int kWantWGs = 2048;       // 256 CUs x 8: below this many strips the frames are cut into chunks
constexpr long long kMaxGrid = 1ll << 20;

// (S + n / 2) / n for S <= 65535 n, n <= 65 * 65; inv = rcp(float(n)) to 1 ulp.
__device__ __forceinline__ uint32_t rounded_mean(uint32_t S, uint32_t n, float inv) {
  const uint32_t a = S + (n >> 1);                  // < 2^29
  uint32_t q = (uint32_t)((float)a * inv);          // the quotient or one beside it
  const int32_t rem = (int32_t)(a - q * n);         // in [-n, 2n)
  if (rem < 0) q -= 1;
  else if (rem >= (int32_t)n) q += 1;
  return q;
}

__device__ __forceinline__ int next_slot(int k, int D) { return k + 1 == D ? 0 : k + 1; }

// grid: workgroups that stride over the jobs (frame, strip, chunk); KD: rows of the ring, >= 2R + 1.
template <int KD>
__global__ __launch_bounds__(kThreads) void box_bandpass_kernel(const uint16_t* __restrict__ src,
                                                                uint16_t* __restrict__ dst, long long jobs, int H,
                                                                int W, int s, int r, int strips, int chunks, int CH) {
  __shared__ uint32_t ring[KD * kRow];
  __shared__ uint32_t wtot[kThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int R = max(s, r), D = 2 * R + 1, TW = kThreads - 2 * R;
  const bool owns = t >= R && t < R + TW;  // an output column of the strip (when inside the image)

  for (long long job = blockIdx.x; job < jobs; job += gridDim.x) {
    const long long fs = job / chunks;
    const int c = (int)(job - fs * chunks);
    const long long f = fs / strips;
    const int strip = (int)(fs - f * strips);
    const int ya = c * CH, yb = min(H, ya + CH);  // the chunk's output rows
    if (ya >= H) continue;  // uniform.  The host's cut makes no empty chunk; one would load nothing
    const int gx = strip * TW - R + t;            // this thread's image column
    const bool col_in = gx >= 0 && gx < W;
    const bool writes = owns && gx < W;
    const size_t frame = (size_t)f * H * W;
    const uint16_t* col = src + frame + (col_in ? gx : 0);
    const uint32_t nxs = (uint32_t)(min(W - 1, gx + s) - max(0, gx - s) + 1);
    const uint32_t nxr = (uint32_t)(min(W - 1, gx + r) - max(0, gx - r) + 1);

    const int y_first = max(0, ya - R), y_last = min(H, yb + R) - 1;  // the rows that enter
    const int s_first = max(0, ya - s);                               // the first row of V_s
    uint32_t vs = 0, vr = 0;
    uint32_t nxt = col_in ? (uint32_t)col[(size_t)y_first * W] : 0u;
    // ring slots of the rows yy, yy - R + s, yy - R - s and yy - 2R relative to row y_first
    int k_in = 0, k_sa = (s - R + D) % D, k_ss = D - R - s, k_rs = 1;

    for (int yy = y_first; yy < yb + R; ++yy) {
      if (yy < H) {  // uniform: row yy enters
        const uint32_t v = nxt;
        if (yy < y_last) nxt = col_in ? (uint32_t)col[(size_t)(yy + 1) * W] : 0u;
        uint32_t p = v;  // inclusive scan over the wave, then over the waves
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t o = __shfl_up(p, d, 64);
          if (lane >= d) p += o;
        }
        if (lane == 63) wtot[wave] = p;
        __syncthreads();
        for (int w = 0; w < wave; ++w) p += wtot[w];
        uint32_t* E = ring + k_in * kRow;
        E[t + 1] = p;
        if (t == 0) E[0] = 0;
        __syncthreads();
      }
      const int y = yy - R;  // the output row whose windows are complete now
      if (writes) {
        const int q = y + s;  // enters V_s
        if (q >= s_first && q < H) {
          const uint32_t* E = ring + k_sa * kRow;
          vs += E[t + s + 1] - E[t - s];
        }
        if (r > 0 && yy < H) {  // row y + r = yy enters V_r
          const uint32_t* E = ring + k_in * kRow;
          vr += E[t + r + 1] - E[t - r];
        }
        if (y >= ya) {
          const uint32_t nys = (uint32_t)(min(H - 1, y + s) - max(0, y - s) + 1);
          const uint32_t ns = nys * nxs;
          const uint32_t a = rounded_mean(vs, ns, __builtin_amdgcn_rcpf((float)ns));
          uint32_t b = 0;
          if (r > 0) {
            const uint32_t nyr = (uint32_t)(min(H - 1, y + r) - max(0, y - r) + 1);
            const uint32_t nr = nyr * nxr;
            b = rounded_mean(vr, nr, __builtin_amdgcn_rcpf((float)nr));
          }
          dst[frame + (size_t)y * W + gx] = (uint16_t)(a > b ? a - b : 0u);
          if (y - s >= 0) {  // leaves V_s
            const uint32_t* E = ring + k_ss * kRow;
            vs -= E[t + s + 1] - E[t - s];
          }
          if (r > 0 && y - r >= 0) {  // leaves V_r
            const uint32_t* E = ring + k_rs * kRow;
            vr -= E[t + r + 1] - E[t - r];
          }
        }
      }
      k_in = next_slot(k_in, D);
      k_sa = next_slot(k_sa, D);
      k_ss = next_slot(k_ss, D);
      k_rs = next_slot(k_rs, D);
    }
    __syncthreads();  // before the next job overwrites the ring
  }
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

namespace {

// How kcmc_box_bandpass_u16 cuts a stack into jobs; kcmc_box_bandpass_plan reports it.
struct Plan {
  int TW, strips, chunks, CH;
};

// The checks of the shape and the radii that the two entry points share; fn prefixes the messages.
int check_shape(const std::string& p, int n_frames, int H, int W, int s, int r) {
  if (n_frames < 0) return fail(KCMC_EINVAL, p + "n_frames must be >= 0");
  if (H < 1 || W < 1) return fail(KCMC_EINVAL, p + "H and W must be >= 1");
  if (s < 0 || s > kMaxSmooth) return fail(KCMC_EINVAL, p + "smooth_radius must be in [0, 4]");
  if (r < 0 || r > kMaxBackground) return fail(KCMC_EINVAL, p + "background_radius must be 0 or in [1, 32]");
  if (s == 0 && r == 0) return fail(KCMC_EINVAL, p + "smooth_radius and background_radius are both 0 (no filter)");
  if (r > 0 && r <= s) return fail(KCMC_EINVAL, p + "background_radius must be 0 or exceed smooth_radius");
  return KCMC_OK;
}

// Whole frames per workgroup when there are enough strips to fill the device, else row chunks of
// at least kMinChunkRows rows.  The chunk count is taken again from the chunk height, so that
// no chunk is empty: (chunks - 1) CH < H <= chunks CH.
Plan make_plan(int n_frames, int H, int W, int s, int r) {
  Plan pl;
  pl.TW = kThreads - 2 * std::max(s, r);
  pl.strips = (W + pl.TW - 1) / pl.TW;
  const long long columns = std::max<long long>(1, (long long)n_frames * pl.strips);
  const long long want = (kWantWGs + columns - 1) / columns;
  const int cut = (int)std::max<long long>(1, std::min<long long>(want, H / kMinChunkRows));
  pl.CH = (H + cut - 1) / cut;
  pl.chunks = (H + pl.CH - 1) / pl.CH;
  return pl;
}

}  // namespace

extern "C" int kcmc_box_bandpass_plan(int n_frames, int H, int W, int smooth_radius, int background_radius,
                                      int* plan_host) {
  const std::string p = "kcmc_box_bandpass_plan: ";
  KCMC_TRY(check_shape(p, n_frames, H, W, smooth_radius, background_radius));
  if (!plan_host) return fail(KCMC_EINVAL, p + "NULL pointer");
  const Plan pl = make_plan(n_frames, H, W, smooth_radius, background_radius);
  plan_host[0] = pl.TW;
  plan_host[1] = pl.strips;
  plan_host[2] = pl.chunks;
  plan_host[3] = pl.CH;
  return KCMC_OK;
}

extern "C" int kcmc_box_bandpass_u16(kcmc_ctx* ctx, const uint16_t* src, uint16_t* dst, int n_frames, int H, int W,
                                     int smooth_radius, int background_radius, kcmc_stream_t stream) {
  const std::string p = "kcmc_box_bandpass_u16: ";
  const int s = smooth_radius, r = background_radius;
  if (!ctx) return fail(KCMC_EINVAL, p + "ctx is NULL");
  KCMC_TRY(check_shape(p, n_frames, H, W, s, r));
  if (n_frames == 0) return KCMC_OK;  // an empty call: the pointers are not looked at
  if (!src || !dst) return fail(KCMC_EINVAL, p + "NULL pointer");
  const size_t n = (size_t)n_frames * H * W;
  if ((uintptr_t)src < (uintptr_t)(dst + n) && (uintptr_t)dst < (uintptr_t)(src + n))
    return fail(KCMC_EINVAL, p + "src and dst overlap (a neighbourhood filter cannot run in place)");
  const Plan pl = make_plan(n_frames, H, W, s, r);
  const long long jobs = (long long)n_frames * pl.strips * pl.chunks;
  const dim3 grid((unsigned)std::min(jobs, kMaxGrid)), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (std::max(s, r) <= kSmallR)
    hipLaunchKernelGGL(box_bandpass_kernel<2 * kSmallR + 1>, grid, block, 0, st, src, dst, jobs, H, W, s, r,
                       pl.strips, pl.chunks, pl.CH);
  else
    hipLaunchKernelGGL(box_bandpass_kernel<2 * kMaxBackground + 1>, grid, block, 0, st, src, dst, jobs, H, W, s, r,
                       pl.strips, pl.chunks, pl.CH);
  return launch_check("box_bandpass_kernel");
}

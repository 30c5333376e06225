// K2: batched rigid RANSAC with scikit-image 0.18.3 semantics, and K2s: the same kernel
// for SimilarityTransform (SCALE = true: rotation, translation and one scale).
//
// Reference: VA:288-323 (_compute_euclidean_affine) ->
//   skimage.measure.ransac((kp_query, kp_template), EuclideanTransform, min_samples=2,
//   residual_threshold=2, max_trials=1000, random_state=42)   (fit.py:621-881)
//
// One workgroup (4 waves) per frame.  The frame's N point pairs are staged in LDS
// (structure of arrays, read as broadcasts); each thread scores whole hypotheses:
//   model      closed-form 2-point rigid Umeyama (the rotation maximising tr(R^T A),
//              A = sum dst_d src_d^T; identical to skimage's SVD branch up to
//              rounding; A == 0 -> NaN model, never selected)
//   residual   r_k = sqrt(dx^2 + dy^2), x' = fma(y, -s, x*c) + tx (the order OpenBLAS
//              dgemm uses for skimage's [x y 1] @ M^T), inlier iff r_k < threshold
//   score      S = sum r_k^2 in numpy's pairwise-summation order (8 accumulators,
//              blocks of 128), so that hypotheses tie-break exactly like np.sum
// Selection: max inliers, then min S, then earliest trial (skimage's strict
// comparisons); skimage's early exit (best S <= 0) is emulated sequentially in the
// rare frames where some S == 0.  The hypothesis (sample pair) of trial t is the
// t-th RandomState(seed).choice(N, 2, replace=False), precomputed on the host per N
// (kcmc_ransac_prepare) -- it depends on N only because every frame reseeds.
// Refit: rigid Umeyama over the best inlier set (wave 0 alone for N <= 128, workgroup
// reductions above; the same sums in the same order either way).
//
// K2s (kcmc_ransac_similarity): ransac(..., SimilarityTransform, min_samples=2, ...), i.e.
// _umeyama(estimate_scale=True).  With a = a00 + a11, b = a10 - a01 of the un-normalised
// covariance sums and v = sum |src_d|^2: a^2 + b^2 = (s1 +- s2)^2 (the sign of det A), so
// skimage's scale = (S @ d) / var is hypot(a, b) / v and the entries of scale * R are a / v
// and b / v (no root).  Same hypothesis tables, residual, scoring phases, selection and
// replay as the rigid model; only the 2-point fit, the refit (one more sum, v over the
// inliers) and the caller's summary differ.
#include <cfloat>
#include <cmath>

#include "kcmc_internal.h"
#include "ransac_common.h"

namespace kcmc {
namespace {

using namespace ransac_common;

struct Model {
  double c, s, tx, ty;
  bool ok;
};

// Closed-form rigid fit of two correspondences (skimage _umeyama, estimate_scale=False);
// SCALE: the similarity fit (estimate_scale=True), c and s hold the entries of scale * R.
// Every two-term sum commutes, so swapping the two points gives the same model to the bit.
template <bool SCALE>
__device__ __forceinline__ Model fit2(double sx0, double sy0, double sx1, double sy1, double dx0, double dy0,
                                      double dx1, double dy1) {
  Model m;
  const double ms0 = (sx0 + sx1) / 2.0, ms1 = (sy0 + sy1) / 2.0;
  const double md0 = (dx0 + dx1) / 2.0, md1 = (dy0 + dy1) / 2.0;
  const double a0 = sx0 - ms0, a1 = sy0 - ms1, b0 = sx1 - ms0, b1 = sy1 - ms1;
  const double p0 = dx0 - md0, p1 = dy0 - md1, q0 = dx1 - md0, q1 = dy1 - md1;
  const double a00 = p0 * a0 + q0 * b0;
  const double a01 = p0 * a1 + q0 * b1;
  const double a10 = p1 * a0 + q1 * b0;
  const double a11 = p1 * a1 + q1 * b1;
  const double a = a00 + a11, b = a10 - a01;
  m.ok = !(a == 0.0 && b == 0.0);
  if (SCALE) {
    const double v = (a0 * a0 + b0 * b0) + (a1 * a1 + b1 * b1);
    m.c = a / v;
    m.s = b / v;
  } else {
    const double hn = sqrt(a * a + b * b);
    m.c = a / hn;
    m.s = b / hn;
  }
  m.tx = md0 - (m.c * ms0 - m.s * ms1);
  m.ty = md1 - (m.s * ms0 + m.c * ms1);
  return m;
}

// The squared residual distance of point (x, y) -> (u, v) under m.  Every phase that compares q
// with tq or sums it calls this, so their q is resid2's to the bit.
__device__ __forceinline__ double q_of(const Model& m, double x, double y, double u, double v) {
  const double xp = fma(y, -m.s, x * m.c) + m.tx;
  const double yp = fma(y, m.c, x * m.s) + m.ty;
  const double ex = xp - u, ey = yp - v;
  return ex * ex + ey * ey;
}

__device__ __forceinline__ double resid2(const Model& m, const Pts& P, int k, double thresh, int& cnt) {
  const double r = sqrt_resid(q_of(m, P.sx[k], P.sy[k], P.dx[k], P.dy[k]));
  cnt += (r < thresh) ? 1 : 0;
  return r * r;
}

// Phase A of the scoring (see the kernel) in fp64: the inlier count through the squared
// distance (r < thresh <=> q < tq, tq = the smallest double whose correctly rounded root
// is >= thresh) and an fp32 estimate of S = sum r_k^2: sum_k (float)q_k in sequence.
// r_k^2 = q_k (1 + d), |d| <= 3 2^-53, numpy's pairwise sum adds <= N 2^-53 and the fp32 sum
// of N conversions <= (N + 1) 2^-24, so for S32 >= 1e-30 (no fp32 underflow matters)
// |S - S32| <= (N + 2) 2^-23 S32, used with a 2x margin.
__device__ __forceinline__ float score_fast(const Model& m, const Pts& P, int N, double tq, int& cnt) {
  float S = 0.f;
  for (int k = 0; k < N; ++k) {
    const double q = q_of(m, P.sx[k], P.sy[k], P.dx[k], P.dy[k]);
    cnt += (q < tq) ? 1 : 0;
    S += (float)q;
  }
  return S;
}

// Staging: the points (gather(k, c): point k as (x, y, u, v)) to sx .. dy, the frame's boxes
// to mg and the centred fp32 copies to pk32; ends behind a barrier.
template <bool LARGE, class Gather>
__device__ __forceinline__ void stage_points(Gather gather, int N, double* sx, double* sy, double* dx, double* dy,
                                             float4* pk32, double* red, Mag& mg) {
  const int tid = threadIdx.x, lane = tid & 63;
  if constexpr (LARGE) {
    for (int k = tid; k < N; k += kThreads) {
      double c[4];
      gather(k, c);
      sx[k] = c[0];
      sy[k] = c[1];
      dx[k] = c[2];
      dy[k] = c[3];
    }
    __syncthreads();
    frame_mag(sx, sy, dx, dy, N, red, mg);
    for (int k = tid; k < N; k += kThreads) pk32[k] = centred32(sx[k], sy[k], dx[k], dy[k], mg);
  } else if (tid < 64) {
    // N <= 128: wave 0 stages every point (k = lane, lane + 64), takes the frame's boxes by
    // wave reductions (min / max: the same bounds in any order) and writes the fp32 copies,
    // behind one barrier (the workgroup form takes five)
    double c[2][4], lo[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, hi[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k < N) {
        gather(k, c[h]);
        mag_add(c[h], lo, hi, bad);
      }
    }
    wave_bounds(lo, hi, bad);
    const Mag m = mag_of(lo, hi);
    if (lane == 0) mg = m;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k < N) {
        sx[k] = c[h][0];
        sy[k] = c[h][1];
        dx[k] = c[h][2];
        dy[k] = c[h][3];
        pk32[k] = centred32(c[h][0], c[h][1], c[h][2], c[h][3], m);
      }
    }
  }
  __syncthreads();
}

// The refit's sums (skimage fit.py:871-875 -> _umeyama over d[best_inliers]): the inliers' number,
// means of (x, y) and (u, v), un-normalised covariance and, SCALE, variance sum of (x, y).
struct Umeyama {
  double n_in, ms0, ms1, md0, md1, a00 = 0, a01 = 0, a10 = 0, a11 = 0, vs = 0;
};

template <bool LARGE, bool SCALE>
__device__ __forceinline__ Umeyama umeyama_sums(const Pts& P, const uint8_t* inl, int N, double* red) {
  Umeyama u;
  const int tid = threadIdx.x, lane = tid & 63;
  if constexpr (!LARGE) {
    // N <= 128: wave 0 alone (the caller's), with no barrier.  Lane l holds points l and l + 64,
    // the points threads l and l + 64 hold in the workgroup form below; each half goes through
    // the same butterfly as there, and the halves are added as block_sum adds its four wave
    // sums (0 + wave 0 + wave 1 + 0 + 0), so every sum is the same to the bit.
    const int k1 = lane + 64;
    const bool i0 = lane < N && inl[lane], i1 = k1 < N && inl[k1];
    auto half_sums = [&](double lo, double hi) {
      for (int o = 32; o > 0; o >>= 1) {
        lo += __shfl_xor(lo, o);
        hi += __shfl_xor(hi, o);
      }
      return (((0.0 + lo) + hi) + 0.0) + 0.0;
    };
    u.n_in = half_sums(i0 ? 1.0 : 0.0, i1 ? 1.0 : 0.0);
    u.ms0 = half_sums(i0 ? 0.0 + P.sx[lane] : 0.0, i1 ? 0.0 + P.sx[k1] : 0.0) / u.n_in;
    u.ms1 = half_sums(i0 ? 0.0 + P.sy[lane] : 0.0, i1 ? 0.0 + P.sy[k1] : 0.0) / u.n_in;
    u.md0 = half_sums(i0 ? 0.0 + P.dx[lane] : 0.0, i1 ? 0.0 + P.dx[k1] : 0.0) / u.n_in;
    u.md1 = half_sums(i0 ? 0.0 + P.dy[lane] : 0.0, i1 ? 0.0 + P.dy[k1] : 0.0) / u.n_in;
    double b[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, bv[2] = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = h ? k1 : lane;
      if (h ? i1 : i0) {
        const double u0 = P.sx[k] - u.ms0, u1 = P.sy[k] - u.ms1;
        const double v0 = P.dx[k] - u.md0, v1 = P.dy[k] - u.md1;
        b[h][0] = 0.0 + v0 * u0;
        b[h][1] = 0.0 + v0 * u1;
        b[h][2] = 0.0 + v1 * u0;
        b[h][3] = 0.0 + v1 * u1;
        if (SCALE) bv[h] = 0.0 + (u0 * u0 + u1 * u1);
      }
    }
    u.a00 = half_sums(b[0][0], b[1][0]);
    u.a01 = half_sums(b[0][1], b[1][1]);
    u.a10 = half_sums(b[0][2], b[1][2]);
    u.a11 = half_sums(b[0][3], b[1][3]);
    if (SCALE) u.vs = half_sums(bv[0], bv[1]);
  } else {
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0, cntd = 0;
    for (int k = tid; k < N; k += kThreads)
      if (inl[k]) {
        s0 += P.sx[k];
        s1 += P.sy[k];
        s2 += P.dx[k];
        s3 += P.dy[k];
        cntd += 1.0;
      }
    u.n_in = block_sum(cntd, red);
    u.ms0 = block_sum(s0, red) / u.n_in;
    u.ms1 = block_sum(s1, red) / u.n_in;
    u.md0 = block_sum(s2, red) / u.n_in;
    u.md1 = block_sum(s3, red) / u.n_in;
    for (int k = tid; k < N; k += kThreads)
      if (inl[k]) {
        const double u0 = P.sx[k] - u.ms0, u1 = P.sy[k] - u.ms1;
        const double v0 = P.dx[k] - u.md0, v1 = P.dy[k] - u.md1;
        u.a00 += v0 * u0;
        u.a01 += v0 * u1;
        u.a10 += v1 * u0;
        u.a11 += v1 * u1;
        if (SCALE) u.vs += u0 * u0 + u1 * u1;
      }
    u.a00 = block_sum(u.a00, red);
    u.a01 = block_sum(u.a01, red);
    u.a10 = block_sum(u.a10, red);
    u.a11 = block_sum(u.a11, red);
    if (SCALE) u.vs = block_sum(u.vs, red);
  }
  return u;
}

// One frame: begin, stage, phase A, A2, B or exact, select, mask, refit.  The LDS is
// RigidSmallLds / RigidLargeLds (ransac_common.h).  For N > 128 the numpy pairwise order
// comes from the per-frame split Plan; invalid trials (NaN S, or 0 inliers with S = inf)
// never win.  LARGE = false handles frames with N <= 128 (one pairwise leaf, fully in
// registers) and the NaN frames; LARGE = true handles 128 < N <= kMaxN through the split plan.
template <bool LARGE, bool SCALE>
__device__ __forceinline__ void ransac_rigid_frame(
    int f, const double* __restrict__ src, const double* __restrict__ dst, const int32_t* __restrict__ pt_idx,
    const int32_t* __restrict__ pt_off, int src_stride, const uint32_t* __restrict__ hyp,
    const int32_t* __restrict__ hyp_off, int hyp_off_len,
    int T, double thresh, double tq, double rate, int n_skip, double* __restrict__ out_params,
    uint8_t* __restrict__ out_inl, int32_t* __restrict__ out_nin, int32_t* __restrict__ out_best) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ double red[kThreads / 64 * 8];
  __shared__ Scratch sc;
  __shared__ int s_any_zero;
  __shared__ Plan s_plan;
  __shared__ Mag mg;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int p0, N, hoff;
  if (!frame_begin<LARGE, 6>(f, pt_off, n_skip, 3, hyp_off, hyp_off_len, out_params, out_inl, out_nin, out_best, p0, N,
                             hoff))
    return;
  const uint32_t* H = hyp + hoff;

  const RigidLds<LARGE> lds((size_t)N, (size_t)T);
  double *sx = lds_at<double>(smem, lds.sx), *sy = lds_at<double>(smem, lds.sy);
  double *dxs = lds_at<double>(smem, lds.dx), *dys = lds_at<double>(smem, lds.dy);
  float4* pk32 = lds_at<float4>(smem, lds.pk32);
  double* wvals = lds_at<double>(smem, lds.wvals);
  double* tS = lds_at<double>(smem, lds.tS);  // tS, tC: the exact path's records
  int* tC = lds_at<int>(smem, lds.tC);
  uint8_t* inl = lds_at<uint8_t>(smem, lds.inl);
  double* stk = nullptr;  // the combine stacks, LARGE only
  if constexpr (LARGE) stk = lds_at<double>(smem, lds.stk);
  const Records<LARGE> rec(smem, lds);  // phase A's records
  if (LARGE && tid == 0) {
    s_plan.n = 0;
    plan_gen<kPwDepth>(s_plan, 0, N);
  }

  auto gather = [&](int k, double (&c)[4]) {
    gather_point(src, dst, pt_idx, src_stride, f, p0 + k, c[0], c[1], c[2], c[3]);
  };
  if (tid == 0) s_any_zero = 0;
  stage_points<LARGE>(gather, N, sx, sy, dxs, dys, pk32, red, mg);

  const Pts P{sx, sy, dxs, dys};
  auto fit_of = [&](int t) {  // trial t's model from its sample pair
    const uint32_t pr = H[t];
    const int i = (int)(pr & 0xffffu), j = (int)(pr >> 16);
    return fit2<SCALE>(sx[i], sy[i], sx[j], sy[j], dxs[i], dys[i], dxs[j], dys[j]);
  };

  // ---- phase A: every trial's inlier count and a bracket of its S, in rec.  In fp32
  // (ransac_common.h score32: certain inliers, outliers and the undecided points between
  // them; a trial whose map or frame is too large for the fp32 bound runs the fp64 form,
  // score_fast).  A trial whose undecided points could lift it to the best certain count
  // is scored again in fp64 (phase A2), so the best count is exact.  Then only trials at
  // that count whose bracket reaches the smallest upper bound need the exact S (phase B,
  // one whole wave per candidate).  Frames the brackets cannot decide -- no trial with
  // inliers, a bracket outside [1e-30, 1e30] (so also every S == 0, skimage's early exit),
  // or a NaN tq -- score every trial exactly (the original single-phase loop).
  const bool fast = tq == tq;  // NaN: exact scoring only (threshold outside the fast range)
  int mcount = -1, flag = fast ? 0 : 1;
  if (fast) {
    int mlo = -1;
    bool deferred = false;  // trials the fp32 bound cannot take: the fp64 loop below
    for (int t = tid; t < T; t += kThreads) {
      const Model m = fit_of(t);
      int v = -1;
      double slo = NAN, shi = NAN;
      Lin32 L;
      if (m.ok && lin32_make(m.c, -m.s, m.tx, m.s, m.c, m.ty, mg, tq, L)) {
        int clo = 0, chi = 0;
        const float S32 = score32(pk32, N, L, clo, chi);
        s32_bracket(S32, N, L.be, slo, shi);
        rec.outward(slo, shi);
        v = pack_cnt(clo, chi - clo);
        if (!(slo >= 1e-30 && shi <= 1e30)) flag = 1;
      } else if (m.ok) {
        v = INT_MIN;
        deferred = true;
      }
      rec.put(t, v, slo, shi);
      mlo = max(mlo, cnt_of(v));
    }
    if (deferred) {
      for (int t = tid; t < T; t += kThreads) {
        if (!rec.deferred(t)) continue;
        const Model m = fit_of(t);
        int cnt = 0;
        const float S32 = score_fast(m, P, N, tq, cnt);
        double slo, shi;
        s64_bracket(S32, N, slo, shi);
        rec.outward(slo, shi);
        if (!(slo >= 1e-30 && shi <= 1e30)) flag = 1;
        rec.put(t, cnt, slo, shi);
        mlo = max(mlo, cnt);
      }
    }
    block_max_flag(mlo, flag, sc.cnt);
    __syncthreads();  // sc.cnt is reused
    // phase A2: the exact count of every trial the undecided points could lift to mlo, each
    // by a whole wave (the points over the lanes, fp64 as score_fast computes them)
    for_each_wave_trial(
        T, [&](int t) { return !flag && rec.und(t) > 0 && rec.cnt(t) + rec.und(t) >= mlo; },
        [&](int tc) {
          const Model m = fit_of(tc);
          int c = 0;
          double sq = 0.0;
          for (int k = lane; k < N; k += 64) {
            const double q = q_of(m, P.sx[k], P.sy[k], P.dx[k], P.dy[k]);
            c += (q < tq) ? 1 : 0;
            sq += q;
          }
          c = wave_sum_i(c);
          double slo, shi;
          sd_bracket(wave_sum(sq), N, slo, shi);
          rec.outward(slo, shi);
          if (!(slo >= 1e-30 && shi <= 1e30)) flag = 1;
          if (lane == 0) rec.put(tc, c, slo, shi);
        });
    __syncthreads();  // the A2 results of the other waves' lanes
    for (int t = tid; t < T; t += kThreads) mcount = max(mcount, rec.cnt(t));
  }
  block_max_flag(mcount, flag, sc.cnt);
  const bool exact = flag != 0 || mcount <= 0;

  Best best;
  bool any_zero = false;
  if (exact) {
    exact_trials(
        T,
        [&](int t, int& cnt) {
          const Model m = fit_of(t);
          if (!m.ok) return (double)NAN;
          return thread_pairwise<LARGE>([&](int k) { return resid2(m, P, k, thresh, cnt); }, N, s_plan, stk, tid);
        },
        tS, tC, best, any_zero);
  } else {
    double lm = INFINITY;
    for (int t = tid; t < T; t += kThreads)
      if (rec.cnt(t) == mcount) lm = fmin(lm, rec.hi(t));
    const double minhi = block_min(lm, sc.min);
    double* vals = wvals + wave * (LARGE ? 128 : N);
    double* wstk = stk + wave * kMaxStack;  // LARGE: the wave's combine stack (uniform values)
    // phase B: this wave's candidate trials, each scored by the whole wave
    for_each_wave_trial(
        T, [&](int t) { return rec.cnt(t) == mcount && rec.lo(t) <= minhi; },
        [&](int tc) {
          const Model m = fit_of(tc);
          const double S = wave_pairwise<LARGE>(
              [&](int k) {
                int c = 0;
                return resid2(m, P, k, thresh, c);
              },
              N, s_plan, vals, wstk, lane);
          if (!isnan(S)) best.take(mcount, S, tc);  // wave-uniform
        });
  }
  int best_t, best_c;
  select_best(best, any_zero, T, tS, tC, sc, s_any_zero, best_t, best_c);

  // inlier mask of the best hypothesis (same arithmetic as the scoring loop)
  Model bm{0, 0, 0, 0, false};
  if (best_t >= 0) bm = fit_of(best_t);
  for (int k = tid; k < N; k += kThreads) {
    int c = 0;
    if (bm.ok) resid2(bm, P, k, thresh, c);
    inl[k] = (uint8_t)c;
    out_inl[p0 + k] = (uint8_t)c;
  }
  __syncthreads();
  // refit on the inliers: wave 0 alone for N <= 128
  if (!LARGE && wave != 0) return;
  const Umeyama u = umeyama_sums<LARGE, SCALE>(P, inl, N, red);
  if (tid == 0) {
    double* o = out_params + 6 * (size_t)f;
    const double a = u.a00 + u.a11, b = u.a10 - u.a01;
    if (u.n_in > 0.0 && !(a == 0.0 && b == 0.0)) {
      const double hn = SCALE ? u.vs : sqrt(a * a + b * b);
      const double c = a / hn, s = b / hn;
      o[0] = c;
      o[1] = -s;
      o[2] = (u.md0 - (c * u.ms0 - s * u.ms1)) * rate;
      o[3] = s;
      o[4] = c;
      o[5] = (u.md1 - (s * u.ms0 + c * u.ms1)) * rate;
    } else {
      for (int k = 0; k < 6; ++k) o[k] = NAN;
    }
    out_nin[f] = (int32_t)u.n_in;
    out_best[f] = best_t;
  }
}

// One workgroup per frame.  The N <= 128 kernels are bounded at 5 waves per SIMD (96 VGPRs
// allocated; 90 / 94 used, no scratch): a retiring warp tile leaves 120 VGPRs per SIMD free,
// and under the bound of 4 the compiler spends 126 / 124.
template <bool LARGE, bool SCALE>
__global__ __launch_bounds__(kThreads, LARGE ? 4 : 5) void ransac_rigid_kernel(
    const double* __restrict__ src, const double* __restrict__ dst, const int32_t* __restrict__ pt_idx,
    const int32_t* __restrict__ pt_off, int src_stride, const uint32_t* __restrict__ hyp,
    const int32_t* __restrict__ hyp_off, int hyp_off_len,
    int T, double thresh, double tq, double rate, int n_skip, double* __restrict__ out_params,
    uint8_t* __restrict__ out_inl, int32_t* __restrict__ out_nin, int32_t* __restrict__ out_best) {
  ransac_rigid_frame<LARGE, SCALE>(blockIdx.x, src, dst, pt_idx, pt_off, src_stride, hyp, hyp_off, hyp_off_len, T, thresh,
                                   tq, rate, n_skip, out_params, out_inl, out_nin, out_best);
}

// The slot one retiring warp tile frees on a CU (warp.hip: 8 workgroups of 20,480 B): an
// N <= 128 workgroup at the default 1000 trials fits it with its static LDS (the reduction
// scratch, the bounding boxes and the selection flag, 224 B as compiled).  More trials keep
// working; they only do not fit the slot.
static_assert(RigidSmallLds(128, 1000).bytes() + sizeof(Scratch) + sizeof(Mag) + 16 <= 20480,
              "the N <= 128 rigid RANSAC workgroup must fit one warp tile's LDS");

}  // namespace
}  // namespace kcmc

using namespace kcmc;

template <bool SCALE>
static int ransac_rigid_impl(kcmc_ctx* ctx, const double* src, const double* dst, const int32_t* pt_idx,
                             const int32_t* pt_off, int src_frame_stride, int n_frames, int max_n, int trials,
                             double thresh, double rate, int n_skip, double* out_params, uint8_t* out_inliers,
                             int32_t* out_n_inliers, int32_t* out_best_trial, kcmc_stream_t stream) {
  const char* const who = SCALE ? "kcmc_ransac_similarity: " : "kcmc_ransac_rigid: ";  // failures only
  const int rc = check_ransac_args(who, ctx, src, dst, pt_idx, pt_off, src_frame_stride, n_frames, max_n, trials,
                                   out_params, out_inliers, out_n_inliers, out_best_trial);
  if (rc != KCMC_OK || n_frames == 0) return rc;
  if (!ctx->hyp || ctx->hyp_trials != trials)
    return fail(KCMC_EINVAL, std::string(who) + "hypothesis tables not prepared for trials=" +
                                 std::to_string(trials) + " (call kcmc_ransac_prepare)");
  return launch_small_large<RigidSmallLds, RigidLargeLds>(
      who, ransac_rigid_kernel<false, SCALE>, ransac_rigid_kernel<true, SCALE>, n_frames, max_n, 3, trials,
      (hipStream_t)stream, src, dst, pt_idx, pt_off, src_frame_stride, ctx->hyp, ctx->hyp_off, ctx->hyp_off_len, trials,
      thresh, inlier_bound(thresh), rate, n_skip, out_params, out_inliers, out_n_inliers, out_best_trial);
}

extern "C" int kcmc_ransac_rigid(kcmc_ctx* ctx, const double* src, const double* dst, const int32_t* pt_idx,
                                 const int32_t* pt_off, int src_frame_stride, int n_frames, int max_n, int trials,
                                 double thresh, double rate, int n_skip, double* out_params, uint8_t* out_inliers,
                                 int32_t* out_n_inliers, int32_t* out_best_trial, kcmc_stream_t stream) {
  return ransac_rigid_impl<false>(ctx, src, dst, pt_idx, pt_off, src_frame_stride, n_frames, max_n, trials, thresh, rate,
                                  n_skip, out_params, out_inliers, out_n_inliers, out_best_trial, stream);
}

extern "C" int kcmc_ransac_similarity(kcmc_ctx* ctx, const double* src, const double* dst, const int32_t* pt_idx,
                                      const int32_t* pt_off, int src_frame_stride, int n_frames, int max_n, int trials,
                                      double thresh, double rate, int n_skip, double* out_params, uint8_t* out_inliers,
                                      int32_t* out_n_inliers, int32_t* out_best_trial, kcmc_stream_t stream) {
  return ransac_rigid_impl<true>(ctx, src, dst, pt_idx, pt_off, src_frame_stride, n_frames, max_n, trials, thresh, rate,
                                 n_skip, out_params, out_inliers, out_n_inliers, out_best_trial, stream);
}

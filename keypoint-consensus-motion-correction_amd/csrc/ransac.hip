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

struct Pts {
  const double* sx;
  const double* sy;
  const double* dx;
  const double* dy;
};

__device__ __forceinline__ double resid2(const Model& m, const Pts& P, int k, double thresh, int& cnt) {
  const double x = P.sx[k], y = P.sy[k];
  const double xp = fma(y, -m.s, x * m.c) + m.tx;
  const double yp = fma(y, m.c, x * m.s) + m.ty;
  const double ex = xp - P.dx[k], ey = yp - P.dy[k];
  const double r = sqrt_resid(ex * ex + ey * ey);
  cnt += (r < thresh) ? 1 : 0;
  return r * r;
}

// Phase A of the scoring (see the kernel): the inlier count through the squared
// distance (r < thresh <=> q < tq, tq = the smallest double whose correctly rounded root
// is >= thresh; the q of every point is computed exactly as resid2 computes it) and an
// fp32 estimate of S = sum r_k^2: sum_k (float)q_k in sequence.  r_k^2 = q_k (1 + d),
// |d| <= 3 2^-53, numpy's pairwise sum adds <= N 2^-53 and the fp32 sum of N
// conversions <= (N + 1) 2^-24, so for S32 >= 1e-30 (no fp32 underflow matters)
// |S - S32| <= (N + 2) 2^-23 S32, used with a 2x margin.
__device__ __forceinline__ float score_fast(const Model& m, const Pts& P, int N, double tq, int& cnt) {
  float S = 0.f;
  for (int k = 0; k < N; ++k) {
    const double x = P.sx[k], y = P.sy[k];
    const double xp = fma(y, -m.s, x * m.c) + m.tx;
    const double yp = fma(y, m.c, x * m.s) + m.ty;
    const double ex = xp - P.dx[k], ey = yp - P.dy[k];
    const double q = ex * ex + ey * ey;
    cnt += (q < tq) ? 1 : 0;
    S += (float)q;
  }
  return S;
}

// For N > 128 the numpy pairwise order comes from the per-frame split Plan
// (ransac_common.h); invalid trials (NaN S, or 0 inliers with S = inf) never win.
// LARGE = false handles frames with N <= 128 (one pairwise leaf, fully in registers)
// and the NaN frames; LARGE = true handles 128 < N <= kMaxN through the split plan.
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

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int p0, N, hoff;
  if (!frame_begin<LARGE, 6>(f, pt_off, n_skip, 3, hyp_off, hyp_off_len, out_params, out_inl, out_nin, out_best, p0, N,
                             hoff))
    return;
  const uint32_t* H = hyp + hoff;

  // LDS, LARGE: sx, sy, dx, dy [N] f64 | the points as (x, y, u, v) [N] f32x4 | trial S (low
  //      bound) [T] f64 | trial S high bound [T] f64 | stack [kMaxStack][256] f64 | per-wave
  //      leaf values [4][128] f64 | trial count [T] i32 | inlier flags [N] u8
  // N <= 128 (ransac_common.h rigid_small_lds; at N = 128, T = 1000 the workgroup takes 18,336
  // B of dynamic LDS, inside the 20 KiB a retiring warp tile frees): sx, sy, dx, dy [N] f64 |
  //      a region that holds the f32x4 points in phase A and the per-wave leaf values [4][N]
  //      f64 in phase B (phase A is the only reader of the fp32 points, phase B the only
  //      writer of the leaf values, barriers between) | a trial's bracket as two floats
  //      rounded outward [T] f32 x 2 | certain count, undecided count [T] u8 x 2 | inlier
  //      flags [N] u8.  The exact path's records (S [T] f64, count [T] i32) lie over the
  //      region and the compact records: it starts behind a barrier after the last read of both.
  // Outward rounding keeps every bracket a bound on numpy's S: lo' <= lo <= S <= hi <= hi'.
  // The trial with the smallest S at the best count, S*, has lo'* <= S* <= S_t <= hi'_t for
  // every trial t at that count, so it -- and every trial that ties it -- stays a phase-B
  // candidate (lo' <= min hi'); phase B scores each candidate exactly and selects on the exact
  // values, so wider brackets add candidates and change no output.  The brackets' validity
  // tests (1e-30 .. 1e30, which also send every S == 0 to the exact path) see the rounded values.
  double* sx = smem;
  double* sy = sx + N;
  double* dxs = sy + N;
  double* dys = dxs + N;
  float4* pk32 = reinterpret_cast<float4*>(dys + N);  // 16-byte aligned: 4 N doubles before it
  double* tS = reinterpret_cast<double*>(pk32 + (LARGE ? N : 0));
  double* tSh = tS + T;  // LARGE only
  double* stk = tSh + T;
  double* wvals = LARGE ? stk + kMaxStack * kThreads : tS;
  int* tC = reinterpret_cast<int*>(LARGE ? wvals + kThreads / 64 * 128 : tS + T);
  float* fLo = reinterpret_cast<float*>(tS + 4 * N);  // N <= 128 only, and the three below
  float* fHi = fLo + T;
  uint8_t* bC = reinterpret_cast<uint8_t*>(fHi + T);
  uint8_t* bU = bC + T;
  uint8_t* inl = LARGE ? reinterpret_cast<uint8_t*>(tC + T)
                       : reinterpret_cast<uint8_t*>(tS) + max(32 * N + 10 * T, 12 * T);
  // a trial's phase-A record: v = pack_cnt(certain, undecided), -1 (no model) or INT_MIN
  // (deferred to the fp64 phase A), and the bracket of its S
  auto rec_put = [&](int t, int v, double slo, double shi) {
    if constexpr (LARGE) {
      tC[t] = v;
      tS[t] = slo;
      tSh[t] = shi;
    } else {
      bC[t] = v == INT_MIN ? kDeferred : v < 0 ? kNoModel : (uint8_t)(v & 0xffff);
      bU[t] = (uint8_t)und_of(v);
      fLo[t] = (float)slo;  // exact: outward() rounded both
      fHi[t] = (float)shi;
    }
  };
  auto outward = [&](double& slo, double& shi) {
    if constexpr (!LARGE) {
      slo = (double)f32_below(slo);
      shi = (double)f32_above(shi);
    }
  };
  auto rec_cnt = [&](int t) {
    if constexpr (LARGE) return cnt_of(tC[t]);
    else return cnt_of8(bC[t]);
  };
  auto rec_und = [&](int t) {
    if constexpr (LARGE) return und_of(tC[t]);
    else return bC[t] >= kDeferred ? 0 : (int)bU[t];
  };
  auto rec_deferred = [&](int t) {
    if constexpr (LARGE) return tC[t] == INT_MIN;
    else return bC[t] == kDeferred;
  };
  auto rec_lo = [&](int t) {
    if constexpr (LARGE) return tS[t];
    else return (double)fLo[t];
  };
  auto rec_hi = [&](int t) {
    if constexpr (LARGE) return tSh[t];
    else return (double)fHi[t];
  };
  if (LARGE && tid == 0) {
    s_plan.n = 0;
    plan_gen<kPwDepth>(s_plan, 0, N);
  }

  auto gather = [&](int k, double (&c)[4]) {
    gather_point(src, dst, pt_idx, src_stride, f, p0 + k, c[0], c[1], c[2], c[3]);
  };
  if (tid == 0) s_any_zero = 0;
  __shared__ Mag mg;
  if (!LARGE) {
    // N <= 128: wave 0 stages every point (k = lane, lane + 64), takes the frame's boxes by
    // wave reductions (min / max: the same bounds in any order) and writes the fp32 copies,
    // behind one barrier (the workgroup form takes five)
    if (wave == 0) {
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
          dxs[k] = c[h][2];
          dys[k] = c[h][3];
          pk32[k] = centred32(c[h][0], c[h][1], c[h][2], c[h][3], m);
        }
      }
    }
    __syncthreads();
  } else {
    for (int k = tid; k < N; k += kThreads) {
      double c[4];
      gather(k, c);
      sx[k] = c[0];
      sy[k] = c[1];
      dxs[k] = c[2];
      dys[k] = c[3];
    }
    __syncthreads();
    frame_mag(sx, sy, dxs, dys, N, red, mg);
    for (int k = tid; k < N; k += kThreads) pk32[k] = centred32(sx[k], sy[k], dxs[k], dys[k], mg);
    __syncthreads();
  }

  const Pts P{sx, sy, dxs, dys};
  auto fit_of = [&](int t) {  // trial t's model from its sample pair
    const uint32_t pr = H[t];
    const int i = (int)(pr & 0xffffu), j = (int)(pr >> 16);
    return fit2<SCALE>(sx[i], sy[i], sx[j], sy[j], dxs[i], dys[i], dxs[j], dys[j]);
  };

  // ---- phase A: every trial's inlier count and a bracket [tS, tSh] of its S.  In fp32
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
        outward(slo, shi);
        v = pack_cnt(clo, chi - clo);
        if (!(slo >= 1e-30 && shi <= 1e30)) flag = 1;
      } else if (m.ok) {
        v = INT_MIN;
        deferred = true;
      }
      rec_put(t, v, slo, shi);
      mlo = max(mlo, cnt_of(v));
    }
    if (deferred) {
      for (int t = tid; t < T; t += kThreads) {
        if (!rec_deferred(t)) continue;
        const Model m = fit_of(t);
        int cnt = 0;
        const float S32 = score_fast(m, P, N, tq, cnt);
        double slo, shi;
        s64_bracket(S32, N, slo, shi);
        outward(slo, shi);
        if (!(slo >= 1e-30 && shi <= 1e30)) flag = 1;
        rec_put(t, cnt, slo, shi);
        mlo = max(mlo, cnt);
      }
    }
    block_max_flag(mlo, flag, sc.cnt);
    __syncthreads();  // sc.cnt is reused
    // phase A2: the exact count of every trial the undecided points could lift to mlo, each
    // by a whole wave (the points over the lanes, fp64 as score_fast computes them)
    for_each_wave_trial(
        T, [&](int t) { return !flag && rec_und(t) > 0 && rec_cnt(t) + rec_und(t) >= mlo; },
        [&](int tc) {
          const Model m = fit_of(tc);
          int c = 0;
          double sq = 0.0;
          for (int k = lane; k < N; k += 64) {
            const double x = sx[k], y = sy[k];
            const double xp = fma(y, -m.s, x * m.c) + m.tx;
            const double yp = fma(y, m.c, x * m.s) + m.ty;
            const double ex = xp - dxs[k], ey = yp - dys[k];
            const double q = ex * ex + ey * ey;
            c += (q < tq) ? 1 : 0;
            sq += q;
          }
          c = wave_sum_i(c);
          double slo, shi;
          sd_bracket(wave_sum(sq), N, slo, shi);
          outward(slo, shi);
          if (!(slo >= 1e-30 && shi <= 1e30)) flag = 1;
          if (lane == 0) rec_put(tc, c, slo, shi);
        });
    __syncthreads();  // the A2 results of the other waves' lanes
    for (int t = tid; t < T; t += kThreads) mcount = max(mcount, rec_cnt(t));
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
      if (rec_cnt(t) == mcount) lm = fmin(lm, rec_hi(t));
    const double minhi = block_min(lm, sc.min);
    double* vals = wvals + wave * (LARGE ? 128 : N);
    double* wstk = stk + wave * kMaxStack;  // LARGE: the wave's combine stack (uniform values)
    // phase B: this wave's candidate trials, each scored by the whole wave
    for_each_wave_trial(
        T, [&](int t) { return rec_cnt(t) == mcount && rec_lo(t) <= minhi; },
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
  // refit on the inliers (skimage fit.py:871-875 -> _umeyama over d[best_inliers])
  double n_in, ms0, ms1, md0, md1, a00 = 0, a01 = 0, a10 = 0, a11 = 0, vs = 0;
  if (!LARGE) {
    // N <= 128: wave 0 alone, with no barrier.  Lane l holds points l and l + 64, the
    // points threads l and l + 64 hold in the workgroup form below; each half goes through
    // the same butterfly as there, and the halves are added as block_sum adds its four wave
    // sums (0 + wave 0 + wave 1 + 0 + 0), so every sum is the same to the bit.
    if (wave != 0) return;
    const int k1 = lane + 64;
    const bool i0 = lane < N && inl[lane], i1 = k1 < N && inl[k1];
    auto half_sums = [&](double lo, double hi) {
      for (int o = 32; o > 0; o >>= 1) {
        lo += __shfl_xor(lo, o);
        hi += __shfl_xor(hi, o);
      }
      return (((0.0 + lo) + hi) + 0.0) + 0.0;
    };
    n_in = half_sums(i0 ? 1.0 : 0.0, i1 ? 1.0 : 0.0);
    ms0 = half_sums(i0 ? 0.0 + sx[lane] : 0.0, i1 ? 0.0 + sx[k1] : 0.0) / n_in;
    ms1 = half_sums(i0 ? 0.0 + sy[lane] : 0.0, i1 ? 0.0 + sy[k1] : 0.0) / n_in;
    md0 = half_sums(i0 ? 0.0 + dxs[lane] : 0.0, i1 ? 0.0 + dxs[k1] : 0.0) / n_in;
    md1 = half_sums(i0 ? 0.0 + dys[lane] : 0.0, i1 ? 0.0 + dys[k1] : 0.0) / n_in;
    double b[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, bv[2] = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = h ? k1 : lane;
      if (h ? i1 : i0) {
        const double u0 = sx[k] - ms0, u1 = sy[k] - ms1;
        const double v0 = dxs[k] - md0, v1 = dys[k] - md1;
        b[h][0] = 0.0 + v0 * u0;
        b[h][1] = 0.0 + v0 * u1;
        b[h][2] = 0.0 + v1 * u0;
        b[h][3] = 0.0 + v1 * u1;
        if (SCALE) bv[h] = 0.0 + (u0 * u0 + u1 * u1);
      }
    }
    a00 = half_sums(b[0][0], b[1][0]);
    a01 = half_sums(b[0][1], b[1][1]);
    a10 = half_sums(b[0][2], b[1][2]);
    a11 = half_sums(b[0][3], b[1][3]);
    if (SCALE) vs = half_sums(bv[0], bv[1]);
  } else {
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0, cntd = 0;
    for (int k = tid; k < N; k += kThreads)
      if (inl[k]) {
        s0 += sx[k];
        s1 += sy[k];
        s2 += dxs[k];
        s3 += dys[k];
        cntd += 1.0;
      }
    n_in = block_sum(cntd, red);
    ms0 = block_sum(s0, red) / n_in;
    ms1 = block_sum(s1, red) / n_in;
    md0 = block_sum(s2, red) / n_in;
    md1 = block_sum(s3, red) / n_in;
    for (int k = tid; k < N; k += kThreads)
      if (inl[k]) {
        const double u0 = sx[k] - ms0, u1 = sy[k] - ms1;
        const double v0 = dxs[k] - md0, v1 = dys[k] - md1;
        a00 += v0 * u0;
        a01 += v0 * u1;
        a10 += v1 * u0;
        a11 += v1 * u1;
        if (SCALE) vs += u0 * u0 + u1 * u1;
      }
    a00 = block_sum(a00, red);
    a01 = block_sum(a01, red);
    a10 = block_sum(a10, red);
    a11 = block_sum(a11, red);
    if (SCALE) vs = block_sum(vs, red);
  }
  if (tid == 0) {
    double* o = out_params + 6 * (size_t)f;
    const double a = a00 + a11, b = a10 - a01;
    if (n_in > 0.0 && !(a == 0.0 && b == 0.0)) {
      const double hn = SCALE ? vs : sqrt(a * a + b * b);
      const double c = a / hn, s = b / hn;
      o[0] = c;
      o[1] = -s;
      o[2] = (md0 - (c * ms0 - s * ms1)) * rate;
      o[3] = s;
      o[4] = c;
      o[5] = (md1 - (s * ms0 + c * ms1)) * rate;
    } else {
      for (int k = 0; k < 6; ++k) o[k] = NAN;
    }
    out_nin[f] = (int32_t)n_in;
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
static_assert(rigid_small_lds(128, 1000) + sizeof(Scratch) + sizeof(Mag) + 16 <= 20480,
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
  const int need = max_n < 3 ? 3 : max_n;
  if (!ctx->hyp || ctx->hyp_trials != trials)
    return fail(KCMC_EINVAL, std::string(who) + "hypothesis tables not prepared for trials=" +
                                 std::to_string(trials) + " (call kcmc_ransac_prepare)");
  const int n_small = need < 128 ? need : 128;
  const size_t wvals = (size_t)kThreads / 64 * 128 * sizeof(double);
  // N <= 128: the compact layout; large: per point 4 f64 + one f32x4, per trial 2 f64 + one i32
  const size_t lds_small = rigid_small_lds((size_t)n_small, (size_t)trials);
  const size_t lds_large = (size_t)need * (4 * sizeof(double) + 16) + (size_t)trials * (2 * sizeof(double) + sizeof(int)) +
                           (size_t)kMaxStack * kThreads * sizeof(double) + wvals + (size_t)need + 16;
  return launch_small_large(who, ransac_rigid_kernel<false, SCALE>, ransac_rigid_kernel<true, SCALE>, n_frames, max_n,
                            lds_small, lds_large, (hipStream_t)stream, src, dst, pt_idx, pt_off, src_frame_stride,
                            ctx->hyp, ctx->hyp_off, ctx->hyp_off_len, trials, thresh, inlier_bound(thresh), rate, n_skip,
                            out_params, out_inliers, out_n_inliers, out_best_trial);
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

// Model-independent pieces of the batched RANSAC kernels (ransac.hip: rigid,
// ransac_model.hip: affine / projective): launch shape, numpy's pairwise-summation
// split plan, skimage's selection order, workgroup / wave sums, the control skeleton of a
// scoring workgroup and the launchers' argument checks and small / large launch pair.
#pragma once

#include <climits>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "kcmc_internal.h"

namespace kcmc {
namespace ransac_common {

constexpr int kThreads = 256;
constexpr int kMaxN = 4096;  // numpy's pairwise split tree has depth <= 6 for n <= 4096
constexpr int kPwDepth = 6;

// For n > 128 numpy's pairwise_sum recurses: pairwise(a, n) = pairwise(a, n2) +
// pairwise(a + n2, n - n2) with n2 = n/2 rounded down to a multiple of 8.  The split
// tree depends on N only, so one thread writes it once per frame as a post-order plan:
// leaves in order, each with the number of "pop b, pop a, push a+b" combines that
// follow it.  Every thread then evaluates its hypotheses with one copy of the leaf
// loop and a per-thread stack in LDS.
constexpr int kMaxLeaves = 128;
constexpr int kMaxStack = kPwDepth + 2;

struct Plan {
  int16_t start[kMaxLeaves];
  int16_t len[kMaxLeaves];
  int8_t pops[kMaxLeaves];
  int n;
};

template <int DEPTH>
__device__ __forceinline__ void plan_gen(Plan& p, int s, int n) {
  if (DEPTH == 0 || n <= 128) {
    p.start[p.n] = (int16_t)s;
    p.len[p.n] = (int16_t)n;
    p.pops[p.n] = 0;
    ++p.n;
    return;
  }
  if constexpr (DEPTH > 0) {
    int n2 = n / 2;
    n2 -= n2 % 8;
    plan_gen<DEPTH - 1>(p, s, n2);
    plan_gen<DEPTH - 1>(p, s + n2, n - n2);
    ++p.pops[p.n - 1];
  }
}

// ---------------------------------------------------------------- the workgroups' dynamic LDS
// One description per workgroup kind, built from (n points, T trials): the byte offset of every
// region.  The kernel takes its pointers from it with the frame's own N (lds_at), the launcher
// its size with the launch's largest n; bytes() does not decrease in n.  Every kind starts with
// the staged points sx, sy, dx, dy [n] f64 (Pts: (x, y) of the frame, (dx, dy) of the template).
constexpr size_t kStackBytes = kMaxStack * kThreads * sizeof(double);   // thread_pairwise's stacks
constexpr size_t kLeafBytes = kThreads / 64 * 128 * sizeof(double);     // wave_leaf's rows, [4][128] f64

struct Pts {
  const double *sx, *sy, *dx, *dy;
};

template <class T>
__device__ __forceinline__ T* lds_at(double* smem, size_t off) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(smem) + off);
}

// Rigid / similarity, N <= 128: exactly 64 n + max(10 T, 12 T - 32 n) + n + 16 bytes (18,336 at
// (128, 1000): with the static LDS inside the 20 KiB slot a retiring warp tile leaves, DESIGN
// 4, K2).  Two overlays, each side used behind a barrier after the last access of the other:
//   pk32 = wvals: phase A is the only reader of the centred fp32 points ([n] float4), phase B
//     the only writer of the per-wave leaf values ([4][n] f64);
//   tS, tC: the exact path's records (S [T] f64, count [T] i32) lie over that region and the
//     compact 10-byte records (a trial's bracket as two floats rounded outward lo, hi [T] f32,
//     its certain and undecided counts cnt, und [T] u8, see Records).
struct RigidSmallLds {
  size_t sx, sy, dx, dy, pk32, wvals, lo, hi, cnt, und, tS, tC, inl, end;
  __host__ __device__ constexpr RigidSmallLds(size_t n, size_t T)
      : sx(0), sy(8 * n), dx(16 * n), dy(24 * n), pk32(32 * n), wvals(pk32), lo(wvals + 32 * n), hi(lo + 4 * T),
        cnt(hi + 4 * T), und(cnt + T), tS(pk32), tC(tS + 8 * T),
        inl(und + T > tC + 4 * T ? und + T : tC + 4 * T), end(inl + n) {}  // inl: the inlier flags [n] u8
  __host__ __device__ constexpr size_t bytes() const { return end + 16; }  // the slot argument's figure
};
constexpr size_t rigid_small_lds(size_t n, size_t T) { return RigidSmallLds(n, T).bytes(); }

// Rigid / similarity, 128 < N <= kMaxN: the fp32 points [n] float4 | a trial's bracket lo, hi
// [T] f64 | the threads' combine stacks | the waves' leaf values | a trial's counts cnt [T] i32
// (pack_cnt) | the inlier flags [n] u8.  The exact path's tS and tC are lo and cnt.
struct RigidLargeLds {
  size_t sx, sy, dx, dy, pk32, lo, hi, stk, wvals, cnt, tS, tC, inl, end;
  __host__ __device__ constexpr RigidLargeLds(size_t n, size_t T)
      : sx(0), sy(8 * n), dx(16 * n), dy(24 * n), pk32(32 * n), lo(pk32 + 16 * n), hi(lo + 8 * T), stk(hi + 8 * T),
        wvals(stk + kStackBytes), cnt(wvals + kLeafBytes), tS(lo), tC(cnt), inl(cnt + 4 * T), end(inl + n) {}
  __host__ __device__ constexpr size_t bytes() const { return end; }
};
template <bool LARGE>
using RigidLds = std::conditional_t<LARGE, RigidLargeLds, RigidSmallLds>;

// Affine / projective, N <= 128 (LARGE = false) and 128 < N <= kMaxN: the points again as (x, y,
// dx, dy) for phase A, pk [n] of 32 B (ransac_model.hip PackedPt; N <= 128 only) | trial S [T]
// f64 | the threads' combine stacks (LARGE only: N <= 128 is one pairwise leaf) | the waves'
// leaf values | trial count [T] i32 | the winner's inlier mask [n] u8 (the fused refit's).
template <bool LARGE>
struct ModelLds {
  size_t sx, sy, dx, dy, pk, tS, stk, wvals, tC, inl, end;
  __host__ __device__ constexpr ModelLds(size_t n, size_t T)
      : sx(0), sy(8 * n), dx(16 * n), dy(24 * n), pk(32 * n), tS(pk + (LARGE ? 0 : 32 * n)), stk(tS + 8 * T),
        wvals(stk + (LARGE ? kStackBytes : 0)), tC(wvals + kLeafBytes), inl(tC + 4 * T), end(inl + n) {}
  __host__ __device__ constexpr size_t bytes() const { return end; }
};

// sqrt of a squared residual distance, the hot op of every scoring loop: the same
// rsq + Goldschmidt/Newton sequence (and so the same correctly rounded result) that
// the compiler emits for sqrt(double), without its denormal-range scaling and its
// zero/infinity selects (~7 of ~32 VALU per residual).  Identical to sqrt(d) for
// d == 0, d >= 2^-767 (|residual| >= 2^-383) and NaN; d = +inf (coordinates beyond
// 1e154) gives NaN instead of inf.  rsq of max(d, 2^-1000) keeps d == 0 finite:
// g = 0 * 2^500 = 0 and every correction term stays 0.
__device__ __forceinline__ double sqrt_resid(double d) {
  const double y = __builtin_amdgcn_rsq(fmax(d, 0x1p-1000));
  double g = d * y;
  double h = y * 0.5;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  double e = fma(-g, g, d);
  g = fma(e, h, g);
  e = fma(-g, g, d);
  return fma(e, h, g);
}

// skimage's selection order (fit.py:851-861): (count desc, S asc, trial asc).
__device__ __forceinline__ bool better(int c, double S, int t, int bc, double bS, int bt) {
  if (c != bc) return c > bc;
  if (S != bS) return S < bS;
  return t < bt;
}

// tq = the smallest double whose correctly rounded square root is >= thresh, so that
// sqrt(q) < thresh <=> q < tq for every q (the root is monotone; NaN compares false
// either way): the scoring kernels' phase A counts inliers without the root.
// sqrt_resid is the correctly rounded root for q >= 2^-767, so thresholds whose tq falls
// below that (or non-finite / non-positive ones) return NaN: exact scoring only.
inline double inlier_bound(double thresh) {
  if (!(thresh > 0x1p-380 && thresh < 0x1p500)) return NAN;
  double q = thresh * thresh;
  while (std::sqrt(q) < thresh) q = std::nextafter(q, INFINITY);
  for (double p = std::nextafter(q, 0.0); std::sqrt(p) >= thresh; p = std::nextafter(q, 0.0)) q = p;
  return q;
}

// Phase B of the scoring kernels: numpy's pairwise leaf (8 strided accumulators for
// n >= 8, sequential below; n <= 128) over r2(start + k), evaluated by one whole wave:
// the lanes write the values to the wave's LDS row `vals`, lanes j < 8 run accumulator
// j's sequential sum, and every lane finishes the same combine and remainder
// (wave-uniform result, bit-identical to a one-thread pw_leaf).
template <class R2>
__device__ __forceinline__ double wave_leaf(R2 r2, int start, int n, double* vals, int lane) {
  for (int k = lane; k < n; k += 64) vals[k] = r2(start + k);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  double res = 0.0;
  if (n < 8) {
    for (int i = 0; i < n; ++i) res += vals[i];
  } else {
    const int j = lane & 7;
    const int nfull = n - (n % 8);
    double r = vals[j];
    for (int i = j + 8; i < nfull; i += 8) r += vals[i];
    double rj[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) rj[q] = __shfl(r, q);
    res = ((rj[0] + rj[1]) + (rj[2] + rj[3])) + ((rj[4] + rj[5]) + (rj[6] + rj[7]));
    for (int i = nfull; i < n; ++i) res += vals[i];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();  // vals is rewritten by the next leaf
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return res;
}

// The exact S of one trial by one wave: a single leaf for N <= 128, else numpy's split
// plan with the combine stack in the wave's LDS slots `wstk` (uniform values).
template <bool LARGE, class R2>
__device__ __forceinline__ double wave_pairwise(R2 r2, int N, const Plan& plan, double* vals, double* wstk, int lane) {
  if (!LARGE) return wave_leaf(r2, 0, N, vals, lane);
  int sp = 0;
  for (int l = 0; l < plan.n; ++l) {
    wstk[sp++] = wave_leaf(r2, plan.start[l], plan.len[l], vals, lane);
    for (int c = plan.pops[l]; c > 0; --c) {
      const double b = wstk[--sp];
      const double a = wstk[sp - 1];
      wstk[sp - 1] = a + b;
    }
  }
  return wstk[0];
}

// Phase A's error bound (the kernels' comment): |S - S32| <= eps S32 for S32 in
// [1e-30, 1e30], with a 2x margin.
__device__ __forceinline__ double s32_eps(int N) { return (double)(N + 2) * 0x1p-22; }
// The same for an fp64 sum Sd of the q (the model scorers' phase A): numpy's S is within
// (N + 3) 2^-53 S of the exact sum of the q, Sd in any order within (N - 1) 2^-53 (2x margin); the
// range excludes every S == 0 (skimage's early exit) and the under / overflowing sums.
__device__ __forceinline__ double sd_eps(int N) { return (double)(2 * N + 8) * 0x1p-52; }
__device__ __forceinline__ bool sd_certain(double Sd) { return Sd >= 1e-290 && Sd <= 1e290; }

// ---------------------------------------------------------------- phase A in fp32
// The rigid scorer decides phase A in fp32 (round 6; fp64 VALU was 65 % of the scorers'
// instructions): a trial's map (X, Y) = a x + b y + t is rounded to fp32 and
// every point's residual e = (X - u, Y - v) and q = ex^2 + ey^2 are computed in fp32 from
// fp32 copies of the points centred on the frame's bounding boxes (x' = x - c_x, ...; the
// map's translation becomes t' = a c_x + b c_y + t - c_u, in fp64).  With
// M' = |a_x| h_x + |b_x| h_y + |t'_x| + h_u (h = the boxes' half extents, likewise for Y)
// and F = the same with the uncentred maxima, every |e32 - e| <= be = 7.01 2^-24 M' +
// 2^-49 F (the roundings of the inputs, of the map and of the three fp32 operations, plus
// the fp64 ones of the centring and of the reference's own e), so near q = tq
//   |q32 - q| <= B = 2 be sqrt(8 tq) + 2 be^2 + 8.5 2^-24 tq    (used with a 1.25 margin),
// and whenever B <= tq / 4: q32 < tq - B is an inlier, q32 > tq + B an outlier, for certain
// (far from tq the bound is relatively smaller still); points in between are counted as
// undecided, and a trial whose count the undecided points could lift to the best certain
// count is counted again in fp64 by a whole wave (phase A2).  S = sum r^2 is bracketed by
//   |S - S32| <= 2 be sqrt(2 N S') + 2 N be^2 + ((N + 2.1) 2^-24 + (N + 3) 2^-53) S'
// (Cauchy-Schwarz over the points; S' bounds the sum of the q32 from the fp32 sum S32).
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct Mag {  // the frame's bounding boxes: centres, half extents, max magnitudes
  double cx, cy, cu, cv;  // (x, y): frame points; (u, v): template points
  double hx, hy, hu, hv;
  double X, Y, U, V;
};

struct Lin32 {
  f32x2 a, b, t;  // (X - u, Y - v) = a x' + b y' + t - u' in centred coordinates
  float lo, hi;   // certain inlier: q32 < lo; certain outlier: q32 > hi
  double be;
};

__device__ __forceinline__ bool lin32_make(double ax, double bx, double tx, double ay, double by, double ty,
                                           const Mag& mg, double tq, Lin32& L) {
  const double tpx = ax * mg.cx + bx * mg.cy + tx - mg.cu;
  const double tpy = ay * mg.cx + by * mg.cy + ty - mg.cv;
  const double Mx = fabs(ax) * mg.hx + fabs(bx) * mg.hy + fabs(tpx) + mg.hu;
  const double My = fabs(ay) * mg.hx + fabs(by) * mg.hy + fabs(tpy) + mg.hv;
  const double Fx = fabs(ax) * mg.X + fabs(bx) * mg.Y + fabs(tx) + mg.U;
  const double Fy = fabs(ay) * mg.X + fabs(by) * mg.Y + fabs(ty) + mg.V;
  const double be = 7.01 * 0x1p-24 * fmax(Mx, My) + 0x1p-49 * fmax(Fx, Fy);
  const double B = 1.25 * (2.0 * be * sqrt(8.0 * tq) + 2.0 * be * be + 8.5 * 0x1p-24 * tq);
  if (!(B <= 0.25 * tq) || !(tq < 1e30)) return false;  // NaN / huge maps and coordinates: fp64
  L.a = f32x2{(float)ax, (float)ay};
  L.b = f32x2{(float)bx, (float)by};
  L.t = f32x2{(float)tpx, (float)tpy};
  float lo = (float)(tq - B), hi = (float)(tq + B);
  // directed to the safe side (both positive: tq - B >= 3 tq / 4 > 0): one ulp down / up
  if ((double)lo > tq - B) lo = __int_as_float(__float_as_int(lo) - 1);
  if ((double)hi < tq + B) hi = __int_as_float(__float_as_int(hi) + 1);
  L.lo = lo;
  L.hi = hi;
  L.be = be;
  return true;
}

// The centred fp32 copy of point (x, y) -> (u, v).
__device__ __forceinline__ float4 centred32(double x, double y, double u, double v, const Mag& mg) {
  return make_float4((float)(x - mg.cx), (float)(y - mg.cy), (float)(u - mg.cu), (float)(v - mg.cv));
}

// Phase A of one trial in fp32 over the centred points (x', y', u', v') as float4 in LDS:
// returns S32, adds the certain inliers to clo and the certain-or-undecided ones to chi.
// Two points per iteration, so the reads of a pair are in flight together.
__device__ __forceinline__ float score32(const float4* __restrict__ pk, int N, const Lin32& L, int& clo, int& chi) {
  float S = 0.f;
  auto one = [&](const float4 p) {
    f32x2 e = L.t - f32x2{p.z, p.w};
    e = __builtin_elementwise_fma(L.b, f32x2{p.y, p.y}, e);
    e = __builtin_elementwise_fma(L.a, f32x2{p.x, p.x}, e);
    const float q = __builtin_fmaf(e.x, e.x, e.y * e.y);
    S += q;
    clo += q < L.lo ? 1 : 0;
    chi += q <= L.hi ? 1 : 0;
  };
  int k = 0;
  for (; k + 2 <= N; k += 2) {
    const float4 a = pk[k], b = pk[k + 1];
    one(a);
    one(b);
  }
  if (k < N) one(pk[k]);
  return S;
}

// [lo, hi] around numpy's S of a trial scored by score32 (the bound above, 1e-9 margins).
__device__ __forceinline__ void s32_bracket(float S32, int N, double be, double& lo, double& hi) {
  const double S = (double)S32;
  const double Sp = S * (1.0 + 1.01 * N * 0x1p-24);
  const double E = 2.0 * be * sqrt(2.02 * N * Sp) + 2.0 * N * be * be + ((N + 2.1) * 0x1p-24 + (N + 3) * 0x1p-53) * Sp;
  lo = (S - E) * (1.0 - 1e-9);
  hi = (S + E) * (1.0 + 1e-9);
}

// The fp64 phase A's bracket (s32_eps) in the same form.
__device__ __forceinline__ void s64_bracket(float S32, int N, double& lo, double& hi) {
  const double eps = s32_eps(N);
  lo = (double)S32 * (1.0 - eps);
  hi = (double)S32 * (1.0 + eps);
}

// The bracket of a wave's fp64 sum Sd of the q (phase A2; sd_eps holds for any summation order).
__device__ __forceinline__ void sd_bracket(double Sd, int N, double& lo, double& hi) {
  const double eps = sd_eps(N);
  lo = Sd * (1.0 - eps);
  hi = Sd * (1.0 + eps);
}

// ---------------------------------------------------------------- the rigid scorer's compact records
// The N <= 128 rigid kernels keep a trial's bracket as two floats rounded outward (the low
// bound toward -inf, the high bound toward +inf, as lin32_make directs its bounds) and its two
// counts as bytes (Records<false> in RigidSmallLds).  f32_below(d) is the largest float <= d,
// f32_above(d) the smallest float >= d, for every finite d (beyond the float range: -inf /
// -FLT_MAX and FLT_MAX / +inf); NaN stays NaN.  Plain C++ on bit patterns: the host computes
// the same values.
__host__ __device__ inline float f32_step(float f, bool up) {  // the next float above / below a finite f
  int32_t i = __builtin_bit_cast(int32_t, f);
  if (f == 0.f) return __builtin_bit_cast(float, up ? 0x00000001 : (int32_t)0x80000001);
  i += ((f > 0.f) == up) ? 1 : -1;
  return __builtin_bit_cast(float, i);
}
__host__ __device__ inline float f32_below(double d) {
  const float f = (float)d;
  return (double)f > d ? f32_step(f, false) : f;
}
__host__ __device__ inline float f32_above(double d) {
  const float f = (float)d;
  return (double)f < d ? f32_step(f, true) : f;
}

// A trial's counts as bytes (counts <= 128): kNoModel for a trial without a model, kDeferred
// for one the fp32 bound cannot take (scored by the fp64 phase A); both read as count -1.
constexpr uint8_t kNoModel = 255, kDeferred = 254;
__host__ __device__ inline int cnt_of8(uint8_t c) { return c >= kDeferred ? -1 : (int)c; }

// Phase A's per-trial record in the tC array: the certain inlier count and the undecided
// points (cnt | und << 16, counts <= kMaxN < 2^16), -1 for a trial without a model.
__device__ __forceinline__ int pack_cnt(int cnt, int und) { return cnt | (und << 16); }
__device__ __forceinline__ int cnt_of(int v) { return v < 0 ? v : (v & 0xffff); }
__device__ __forceinline__ int und_of(int v) { return v < 0 ? 0 : (v >> 16); }

// The rigid kernels' phase-A records, 20 B per trial (LARGE) or the compact 10 B.  put(t, v, slo,
// shi): v = pack_cnt(certain, undecided), -1 (no model) or INT_MIN (deferred to the fp64 phase
// A), and the bracket of S, which outward() has rounded to what the format keeps.  Outward
// rounding keeps every bracket a bound on numpy's S: lo' <= lo <= S <= hi <= hi'.  The trial with
// the smallest S at the best count, S*, has lo'* <= S* <= S_t <= hi'_t for every trial t at that
// count, so it -- and every trial that ties it -- stays a phase-B candidate (lo' <= min hi');
// phase B scores each candidate exactly and selects on the exact values, so wider brackets add
// candidates and change no output.  The brackets' validity tests (1e-30 .. 1e30, which also send
// every S == 0 to the exact path) see the rounded values.
template <bool LARGE>
struct Records {
  using Bound = std::conditional_t<LARGE, double, float>;
  using Count = std::conditional_t<LARGE, int, uint8_t>;
  Bound *blo, *bhi;
  Count* c;
  uint8_t* u = nullptr;  // the undecided counts, !LARGE only
  __device__ Records(double* smem, const RigidLds<LARGE>& L)
      : blo(lds_at<Bound>(smem, L.lo)), bhi(lds_at<Bound>(smem, L.hi)), c(lds_at<Count>(smem, L.cnt)) {
    if constexpr (!LARGE) u = lds_at<uint8_t>(smem, L.und);
  }
  __device__ static void outward(double& slo, double& shi) {
    if constexpr (!LARGE) {
      slo = (double)f32_below(slo);
      shi = (double)f32_above(shi);
    }
  }
  __device__ void put(int t, int v, double slo, double shi) const {
    if constexpr (LARGE) {
      c[t] = v;
    } else {
      c[t] = v == INT_MIN ? kDeferred : v < 0 ? kNoModel : (uint8_t)(v & 0xffff);
      u[t] = (uint8_t)und_of(v);
    }
    blo[t] = (Bound)slo;  // exact: outward() rounded both
    bhi[t] = (Bound)shi;
  }
  __device__ int cnt(int t) const { return LARGE ? cnt_of(c[t]) : cnt_of8((uint8_t)c[t]); }
  __device__ int und(int t) const { return LARGE ? und_of(c[t]) : c[t] >= kDeferred ? 0 : (int)u[t]; }
  __device__ bool deferred(int t) const { return c[t] == (LARGE ? INT_MIN : (int)kDeferred); }
  __device__ double lo(int t) const { return (double)blo[t]; }
  __device__ double hi(int t) const { return (double)bhi[t]; }
};

__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The boxes' centres, half extents and magnitudes from their bounds (lo, hi) per coordinate.
__device__ __forceinline__ Mag mag_of(const double (&L)[4], const double (&Hh)[4]) {
  double c[4], h[4], m[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool fin = fabs(L[i]) < INFINITY && fabs(Hh[i]) < INFINITY;
    c[i] = fin ? 0.5 * L[i] + 0.5 * Hh[i] : 0.0;
    h[i] = fin ? fmax(Hh[i] - c[i], c[i] - L[i]) * (1.0 + 0x1p-50) : INFINITY;  // >= every |x - c|
    m[i] = fmax(fabs(L[i]), fabs(Hh[i]));
  }
  Mag out;
  out.cx = c[0]; out.cy = c[1]; out.cu = c[2]; out.cv = c[3];
  out.hx = h[0]; out.hy = h[1]; out.hu = h[2]; out.hv = h[3];
  out.X = m[0]; out.Y = m[1]; out.U = m[2]; out.V = m[3];
  return out;
}

// One point's contribution to the bounds (a NaN or infinite coordinate makes them infinite).
__device__ __forceinline__ void mag_add(const double (&c)[4], double (&lo)[4], double (&hi)[4], bool& bad) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bad |= !(fabs(c[i]) < INFINITY);
    lo[i] = fmin(lo[i], c[i]);
    hi[i] = fmax(hi[i], c[i]);
  }
}

// The wave's bounds in every lane (min / max: exact in any order; a lane that saw a NaN or
// infinite coordinate contributes infinite bounds).
__device__ __forceinline__ void wave_bounds(double (&lo)[4], double (&hi)[4], bool bad) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (bad) {
      lo[i] = -INFINITY;
      hi[i] = INFINITY;
    }
    for (int o = 32; o > 0; o >>= 1) {
      lo[i] = fmin(lo[i], __shfl_xor(lo[i], o));
      hi[i] = fmax(hi[i], __shfl_xor(hi[i], o));
    }
  }
}

// The frame's bounding boxes for lin32_make: workgroup min / max over the staged points.
// A NaN or infinite coordinate makes the half extents infinite (every trial then runs the
// fp64 phase A).
// The result goes to the shared `out` (read per trial, not held in registers).
__device__ inline void frame_mag(const double* sx, const double* sy, const double* dx, const double* dy, int N,
                                 double* red, Mag& out) {
  double lo[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, hi[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  bool bad = false;
  for (int k = threadIdx.x; k < N; k += kThreads) {
    const double c[4] = {sx[k], sy[k], dx[k], dy[k]};
    mag_add(c, lo, hi, bad);
  }
  wave_bounds(lo, hi, bad);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red[8 * wave + i] = lo[i];
      red[8 * wave + 4 + i] = hi[i];
    }
  __syncthreads();
  double L[4], Hh[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    L[i] = red[i];
    Hh[i] = red[4 + i];
    for (int w = 1; w < kThreads / 64; ++w) {
      L[i] = fmin(L[i], red[8 * w + i]);
      Hh[i] = fmax(Hh[i], red[8 * w + 4 + i]);
    }
  }
  if (threadIdx.x == 0) out = mag_of(L, Hh);
  __syncthreads();  // out is visible, red is free
}

__device__ inline double block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kThreads / 64; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---------------------------------------------------------------- the scoring skeleton
// What a scoring workgroup does around its model's fit, residual and phase-A scorer, the same
// for every model: which frames it owns, the point gather, the workgroup reductions, numpy's
// pairwise sum by one thread, the walk over a wave's candidate trials and skimage's selection.
// A model's own part comes in as a functor; nothing here knows which model calls it.

// The workgroup's small static scratch for the reductions below.  (The selection's flag
// s_any_zero stays a variable of its own: the compiler packs it into the padding behind the
// Plan, inside this struct it would cost the large kernels 16 bytes.)
struct Scratch {
  double min[kThreads / 64];
  double bestS[kThreads / 64];
  int cnt[kThreads / 64];
  int best[kThreads / 64 * 2];  // (count, trial) per wave; then the selection's (best_t, best_c)
};

// Frame f's points [p0, p0 + N) and the start of N's hypothesis table.  A frame RANSAC does not
// run on (fewer than n_skip or min_n points, more than kMaxN, or no table for N) gets NaN
// parameters (NPARAM per frame), an empty mask and best_trial -1 from the small launch.
// false: this launch has nothing more to do for the frame.
template <bool LARGE, int NPARAM>
__device__ __forceinline__ bool frame_begin(int f, const int32_t* __restrict__ pt_off, int n_skip, int min_n,
                                            const int32_t* __restrict__ hyp_off, int hyp_off_len,
                                            double* __restrict__ out_params, uint8_t* __restrict__ out_inl,
                                            int32_t* __restrict__ out_nin, int32_t* __restrict__ out_best, int& p0,
                                            int& N, int& hoff) {
  const int tid = threadIdx.x;
  p0 = pt_off[f];
  N = pt_off[f + 1] - p0;
  const bool skip_frame = N < n_skip || N < min_n || N > kMaxN;
  hoff = (!skip_frame && N < hyp_off_len) ? hyp_off[N] : -1;
  const bool nan_frame = skip_frame || hoff < 0;
  if (LARGE != (!nan_frame && N > 128)) return false;  // the other launch owns this frame
  if (nan_frame) {
    if (tid < NPARAM) out_params[NPARAM * (size_t)f + tid] = NAN;
    for (int k = tid; k < N; k += kThreads) out_inl[p0 + k] = 0;
    if (tid == 0) {
      out_nin[f] = skip_frame ? 0 : -1;  // -1: no hypothesis table was prepared for N
      out_best[f] = -1;
    }
    return false;
  }
  return true;
}

// Point p of frame f: (x, y) from src, (u, v) from dst, through the index list pt_idx
// (src[f * src_stride + q], dst[q] with q = pt_idx[p]) or contiguous (both at p).
__device__ __forceinline__ void gather_point(const double* __restrict__ src, const double* __restrict__ dst,
                                             const int32_t* __restrict__ pt_idx, int src_stride, int f, int p,
                                             double& x, double& y, double& u, double& v) {
  size_t si, di;
  if (pt_idx) {
    const int q = pt_idx[p];
    si = (size_t)f * src_stride + q;
    di = (size_t)q;
  } else {
    si = di = (size_t)p;
  }
  x = src[2 * si];
  y = src[2 * si + 1];
  u = dst[2 * di];
  v = dst[2 * di + 1];
}

// Workgroup maximum of a count (>= -1) and OR of a 0 / 1 flag, in every thread.  One barrier;
// a caller that uses s_cnt again puts a barrier after it.
__device__ __forceinline__ void block_max_flag(int& m, int& flag, int* s_cnt) {
  for (int o = 32; o > 0; o >>= 1) {
    m = max(m, __shfl_xor(m, o));
    flag |= __shfl_xor(flag, o);
  }
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = (m + 1) | (flag << 30);  // counts <= kMaxN
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    const int v = s_cnt[w];
    flag |= v >> 30;
    m = max(m, (v & 0x3fffffff) - 1);
  }
}

// Workgroup minimum in every thread (one barrier).
__device__ __forceinline__ double block_min(double v, double* s_min) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3]));
}

// numpy pairwise_sum over r2(start + k), k < n, for n <= 128 by one thread:
// n < 8 sequential, else 8 strided accumulators + sequential remainder.
template <class R2>
__device__ __forceinline__ double pw_leaf(R2 r2, int start, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += r2(start + i);
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = r2(start + j);
  int i = 8;
  const int nfull = n - (n % 8);
  for (; i < nfull; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += r2(start + i + j);
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += r2(start + i);
  return res;
}

// The exact S of one trial by one thread, wave_pairwise's counterpart: a single leaf for
// N <= 128 (fully in registers), else numpy's split plan with the thread's combine stack in
// LDS (stk[level * kThreads + tid]).
template <bool LARGE, class R2>
__device__ __forceinline__ double thread_pairwise(R2 r2, int N, const Plan& plan, double* stk, int tid) {
  if (!LARGE) return pw_leaf(r2, 0, N);
  int sp = 0;
  for (int l = 0; l < plan.n; ++l) {
    stk[sp++ * kThreads + tid] = pw_leaf(r2, plan.start[l], plan.len[l]);
    for (int c = plan.pops[l]; c > 0; --c) {
      const double b = stk[--sp * kThreads + tid];
      const double a = stk[(sp - 1) * kThreads + tid];
      stk[(sp - 1) * kThreads + tid] = a + b;
    }
  }
  return stk[tid];
}

// A thread's running best of skimage's selection order.
struct Best {
  int c = -1;
  double S = INFINITY;
  int t = INT_MAX;
  __device__ __forceinline__ void take(int oc, double oS, int ot) {
    if (better(oc, oS, ot, c, S, t)) {
      c = oc;
      S = oS;
      t = ot;
    }
  }
};

// Exact scoring of every trial, each by one thread (the frames phase A cannot decide):
// score(t, cnt) returns numpy's S of trial t and adds its inliers to cnt, NaN for a trial
// without a model.  Skipped trials (estimate() False) and NaN scores without inliers never win;
// with 0 inliers a trial wins only with S < inf (skimage's strict comparisons against (0, inf)).
// any_zero asks select_best for the sequential replay: some S <= 0, or a NaN S with inliers.
template <class Score>
__device__ __forceinline__ void exact_trials(int T, Score score, double* tS, int* tC, Best& best, bool& any_zero) {
  for (int t = threadIdx.x; t < T; t += kThreads) {
    int cnt = 0;
    const double S = score(t, cnt);
    tS[t] = S;
    tC[t] = cnt;
    if (!isnan(S) && (cnt > 0 || S < INFINITY)) {
      if (S <= 0.0) any_zero = true;
      best.take(cnt, S, t);
    } else if (cnt > 0) {
      // a model with inliers and S = NaN (a NaN coordinate elsewhere in the frame): skimage's
      // comparisons take it on its count alone and nothing at that count replaces it, which is
      // no order a reduction can follow: select_best replays the sequence
      any_zero = true;
    }
  }
}

// This wave's candidate trials (t = t0 + lane, pred(t) in its lane), one after the other with
// the whole wave in body(t): t is wave-uniform there.
template <class Pred, class Body>
__device__ __forceinline__ void for_each_wave_trial(int T, Pred pred, Body body) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t0 = wave * 64; t0 < T; t0 += kThreads) {
    const int t = t0 + lane;
    uint64_t todo = __ballot(t < T && pred(t));
    while (todo) {
      const int tc = t0 + __builtin_ctzll(todo);
      todo &= todo - 1;
      body(tc);
    }
  }
}

// The selection's tail: workgroup argmax of (count, -S, -t) over every thread's best, and,
// when an exactly scored trial had S <= 0 (or a NaN S with inliers), skimage's loop over the trials' records
// tS / tC (s_any_zero: zero before the barrier that precedes the scoring).  best_t = -1 and
// best_c = 0: no trial can be selected.
__device__ __forceinline__ void select_best(Best b, bool any_zero, int T, const double* tS, const int* tC, Scratch& sc,
                                            int& s_any_zero, int& best_t, int& best_c) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  for (int o = 32; o > 0; o >>= 1) b.take(__shfl_xor(b.c, o), __shfl_xor(b.S, o), __shfl_xor(b.t, o));
  if (lane == 0) {
    sc.best[2 * wave] = b.c;
    sc.best[2 * wave + 1] = b.t;
    sc.bestS[wave] = b.S;
  }
  if (any_zero) atomicOr(&s_any_zero, 1);
  __syncthreads();
  if (tid == 0) {
    Best fin;
    for (int w = 0; w < kThreads / 64; ++w) fin.take(sc.best[2 * w], sc.bestS[w], sc.best[2 * w + 1]);
    if (s_any_zero) {
      // skimage stops as soon as the running best has S <= 0 (fit.py:862-869):
      // replay the trial sequence to find where it stopped.
      int c0 = 0, t0 = -1;
      double S0 = INFINITY;
      for (int t = 0; t < T; ++t) {
        const double S = tS[t];
        const int c = tC[t];
        // skimage's own comparisons: a trial without a model (S = NaN, no inliers) never
        // passes them, one with inliers and S = NaN passes on its count
        if (c > c0 || (c == c0 && S < S0)) {
          c0 = c;
          S0 = S;
          t0 = t;
          if (S0 <= 0.0) break;
        }
      }
      fin.t = t0 < 0 ? INT_MAX : t0;
      fin.c = c0;
    }
    // only this thread has read sc.best since the barrier
    sc.best[0] = (fin.t == INT_MAX) ? -1 : fin.t;
    sc.best[1] = (fin.t == INT_MAX) ? 0 : fin.c;
  }
  __syncthreads();
  best_t = sc.best[0];
  best_c = sc.best[1];
}

// ---------------------------------------------------------------- host side of the launchers
// The argument checks every RANSAC entry point makes (who = "kcmc_ransac_...: ", the entry
// that was called).  KCMC_OK with n_frames == 0: nothing to launch.
inline int check_ransac_args(const char* who, const kcmc_ctx* ctx, const double* src, const double* dst,
                             const int32_t* pt_idx, const int32_t* pt_off, int src_frame_stride, int n_frames,
                             int max_n, int trials, const double* out_params, const uint8_t* out_inliers,
                             const int32_t* out_n_inliers, const int32_t* out_best_trial) {
  if (!ctx) return fail(KCMC_EINVAL, std::string(who) + "ctx is NULL");
  if (n_frames < 0 || max_n < 0 || trials < 1) return fail(KCMC_EINVAL, std::string(who) + "bad sizes");
  if (n_frames == 0) return KCMC_OK;
  if (!pt_off || !out_params || !out_n_inliers || !out_best_trial || (max_n > 0 && (!src || !dst || !out_inliers)))
    return fail(KCMC_EINVAL, std::string(who) + "NULL pointer");
  if (max_n > kMaxN) return fail(KCMC_EUNSUPPORTED, std::string(who) + "max_n > 4096 points per frame");
  if (pt_idx && src_frame_stride <= 0) return fail(KCMC_EINVAL, std::string(who) + "src_frame_stride must be > 0");
  return KCMC_OK;
}

// One workgroup per frame: the small kernel (frames with N <= 128 and the NaN frames) and, when
// a frame can have more points, the large one (narrower grids measured slower beside the warp,
// DESIGN 6d).  Each launch's dynamic LDS is its layout's (SmallLds, LargeLds) at the launch's
// largest frame: max_n, at least the model's min_n, and at most 128 for the small kernel.
template <class SmallLds, class LargeLds, class... P, class... A>
inline int launch_small_large(const char* who, void (*small)(P...), void (*large)(P...), int n_frames, int max_n,
                              int min_n, int trials, hipStream_t s, A... args) {
  const size_t need = max_n < min_n ? min_n : max_n;
  const size_t lds_small = SmallLds(need < 128 ? need : 128, (size_t)trials).bytes();
  const size_t lds_large = LargeLds(need, (size_t)trials).bytes();
  if ((max_n > 128 ? lds_large : lds_small) > 150 * 1024)
    return fail(KCMC_EUNSUPPORTED, std::string(who) + "max_n/trials exceed the LDS budget");
  hipLaunchKernelGGL(small, dim3((unsigned)n_frames), dim3(kThreads), lds_small, s, args...);
  KCMC_TRY(launch_check((std::string(who) + "small scoring kernel").c_str()));
  if (max_n > 128) {
    hipLaunchKernelGGL(large, dim3((unsigned)n_frames), dim3(kThreads), lds_large, s, args...);
    KCMC_TRY(launch_check((std::string(who) + "large scoring kernel").c_str()));
  }
  return KCMC_OK;
}

}  // namespace ransac_common
}  // namespace kcmc

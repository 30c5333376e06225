/*
 * kcmc CPU oracle -- TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C restatement of the third-party numerics that the reference's
 * per-frame alignment hot path calls (reference: /root/reference/VideoAligner.py,
 * cited below as VA:<line>).  Only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may load this library, and only as the checker /
 * the timed CPU baseline -- never as the product path.  The product path is the
 * HIP library under keypoint-consensus-motion-correction_amd/csrc.
 *
 * Parity pinning:
 *   - kcmc_oracle_ransac_rigid: pinned against the reference's own
 *     _compute_euclidean_affine (VA:288-323, scikit-image 0.18.3 ransac) run in
 *     the authoring container -> tests/golden/ransac_golden.npz.
 *   - kcmc_oracle_ransac_similarity: scikit-image is absent from this image, so no
 *     golden exists; pinned against the operation-for-operation numpy restatement of
 *     ransac + SimilarityTransform (SVD Umeyama) in tests/test_similarity_host.py.
 *   - kcmc_oracle_knn2_l2u8 and kcmc_oracle_warp_affine_u16: OpenCV is absent
 *     everywhere in this image, so these restate OpenCV 4.x's classic algorithms
 *     (core/src/batch_distance.cpp batchDistL2_8u32f + K-insertion;
 *     imgproc/src/imgwarp.cpp warpAffine/WarpAffineInvoker/remapBilinear) and
 *     are pinned by hand-computed known-answer tests (tests/test_oracle.py).
 *     "Parity vs real OpenCV: unpinned" -- see DESIGN.md.
 *
 * Build: gcc -O3 -march=x86-64-v3 -ffp-contract=off -fPIC -shared (oracle/Makefile).
 * -ffp-contract=off matters: every product/sum below is rounded separately unless
 * fma() is written explicitly, mirroring the reference platform.
 */
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------------- */
/* K1 oracle: cv2.BFMatcher(crossCheck=False).knnMatch(query, train, k=2)     */
/* (VA:194-195).  OpenCV default normType = NORM_L2; for CV_8U descriptors     */
/* batchDistance uses dtype CV_32F and dist = sqrtf((float)sum (a-b)^2).       */
/* The K=2 insertion compares float bit patterns as ints (positive floats) and */
/* inserts row j iff d < best[K-1], shifting while best[k] > d: ties keep the  */
/* lower train index first.                                                    */
/* ------------------------------------------------------------------------- */
int kcmc_oracle_knn2_l2u8(const uint8_t* query, int n_query, const uint8_t* train,
                          int n_train, int D, int32_t* out_idx, float* out_dist) {
  if (n_query < 0 || n_train < 0 || D <= 0) return -1;
  for (int i = 0; i < n_query; ++i) {
    const uint8_t* a = query + (size_t)i * D;
    float bd[2] = {FLT_MAX, FLT_MAX};
    int32_t bi[2] = {-1, -1};
    for (int j = 0; j < n_train; ++j) {
      const uint8_t* b = train + (size_t)j * D;
      int ssd = 0;
      for (int k = 0; k < D; ++k) {
        int t = (int)a[k] - (int)b[k];
        ssd += t * t;
      }
      float d = sqrtf((float)ssd);
      int32_t di, b1;
      memcpy(&di, &d, 4);
      memcpy(&b1, &bd[1], 4);
      if (di < b1) {
        int k = 0;
        int32_t b0;
        memcpy(&b0, &bd[0], 4);
        if (b0 > di) {
          bd[1] = bd[0];
          bi[1] = bi[0];
          k = 0;
        } else {
          k = 1;
        }
        bd[k] = d;
        bi[k] = j;
      }
    }
    out_idx[2 * i] = bi[0];
    out_idx[2 * i + 1] = bi[1];
    out_dist[2 * i] = bd[0];
    out_dist[2 * i + 1] = bd[1];
  }
  return 0;
}

/* ------------------------------------------------------------------------- */
/* K1 opt-in extension oracle: BFMatcher(NORM_HAMMING).knnMatch(k=2) on binary  */
/* descriptors (ORB / BRIEF / AKAZE-MLDB bytes).  NOT the reference's matcher:  */
/* VA:194 constructs cv2.BFMatcher with its default NORM_L2.  OpenCV's          */
/* normHamming counts the differing bits (an integer), batchDistance keeps the  */
/* K best by the same insertion as NORM_L2 (strict >, so the lower train index  */
/* wins ties), and DMatch.distance holds the count as a float.                   */
/* ------------------------------------------------------------------------- */
int kcmc_oracle_knn2_hamming(const uint8_t* query, int n_query, const uint8_t* train, int n_train, int D,
                             int32_t* out_idx, float* out_dist) {
  if (n_query < 0 || n_train < 0 || D <= 0) return -1;
  for (int i = 0; i < n_query; ++i) {
    const uint8_t* a = query + (size_t)i * D;
    int bd[2] = {INT_MAX, INT_MAX};
    int32_t bi[2] = {-1, -1};
    for (int j = 0; j < n_train; ++j) {
      const uint8_t* b = train + (size_t)j * D;
      int d = 0;
      for (int k = 0; k < D; ++k) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
      if (d < bd[1]) {
        if (d < bd[0]) {
          bd[1] = bd[0];
          bi[1] = bi[0];
          bd[0] = d;
          bi[0] = j;
        } else {
          bd[1] = d;
          bi[1] = j;
        }
      }
    }
    for (int k = 0; k < 2; ++k) {
      out_idx[2 * i + k] = bi[k];
      out_dist[2 * i + k] = bi[k] < 0 ? FLT_MAX : (float)bd[k];
    }
  }
  return 0;
}

/* ------------------------------------------------------------------------- */
/* K1 extension oracle: BFMatcher(NORM_L2).knnMatch(k=2) on float32            */
/* descriptors (BASELINE config 5, SIFT-style; the reference's detectors only  */
/* emit uint8 descriptors).  OpenCV's batchDistL2_32f sums (a-b)^2 in float    */
/* with a build-dependent SIMD accumulation order, so the build defines the    */
/* distance as the (near-)exact one: S = sum_k ((double)a_k - (double)b_k)^2   */
/* accumulated sequentially in double, dist = sqrtf((float)S); top-2 by        */
/* (dist, train index) like OpenCV's K-insertion.  Parity vs OpenCV: unpinned. */
/* ------------------------------------------------------------------------- */
float kcmc_oracle_l2f32_dist(const float* a, const float* b, int D) {
  double S = 0.0;
  for (int k = 0; k < D; ++k) {
    double t = (double)a[k] - (double)b[k];
    S += t * t;
  }
  return sqrtf((float)S);
}

int kcmc_oracle_knn2_l2f32(const float* query, int n_query, const float* train, int n_train, int D,
                           int32_t* out_idx, float* out_dist) {
  if (n_query < 0 || n_train < 0 || D <= 0) return -1;
  for (int i = 0; i < n_query; ++i) {
    float bd[2] = {FLT_MAX, FLT_MAX};
    int32_t bi[2] = {-1, -1};
    for (int j = 0; j < n_train; ++j) {
      float d = kcmc_oracle_l2f32_dist(query + (size_t)i * D, train + (size_t)j * D, D);
      if (d < bd[1]) {
        if (d < bd[0]) {
          bd[1] = bd[0];
          bi[1] = bi[0];
          bd[0] = d;
          bi[0] = j;
        } else {
          bd[1] = d;
          bi[1] = j;
        }
      }
    }
    out_idx[2 * i] = bi[0];
    out_idx[2 * i + 1] = bi[1];
    out_dist[2 * i] = bd[0];
    out_dist[2 * i + 1] = bd[1];
  }
  return 0;
}

/* ------------------------------------------------------------------------- */
/* K3 oracle: cv2.warpAffine(img, M, (W, H), flags=INTER_LINEAR) on uint16     */
/* (VA:455-458), BORDER_CONSTANT with value 0, classic fixed-point path.       */
/* ------------------------------------------------------------------------- */
static int cv_round(double v) { return (int)lrint(v); }     /* round-half-even */
static int cv_roundf(float v) { return (int)lrintf(v); }
static int16_t sat_short(int v) {
  return (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
}
static uint16_t sat_ushort_f(float v) {
  int iv = cv_roundf(v);
  return (uint16_t)((unsigned)iv <= 65535u ? iv : (iv > 0 ? 65535 : 0));
}

/* OpenCV's in-place inversion of a forward 2x3 map (warpAffine without
 * WARP_INVERSE_MAP). */
void kcmc_oracle_invert_affine(const double* Min, double* M) {
  memcpy(M, Min, 6 * sizeof(double));
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0 ? 1. / D : 0;
  double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11;
  M[1] *= -D;
  M[3] *= -D;
  M[4] = A22;
  double b1 = -M[0] * M[2] - M[1] * M[5];
  double b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1;
  M[5] = b2;
}

/* src [H,W,C] u16, dst [dH,dW,C] u16, M6 = forward 2x3 map (row-major). */
int kcmc_oracle_warp_affine_u16(const uint16_t* src, int H, int W, int C,
                                const double* M6, int inverse_map, uint16_t* dst,
                                int dH, int dW) {
  if (H <= 0 || W <= 0 || C <= 0 || dH < 0 || dW < 0) return -1;
  const int AB_BITS = 10, AB_SCALE = 1 << AB_BITS, INTER_BITS = 5;
  const int INTER_TAB_SIZE = 1 << INTER_BITS;
  const int round_delta = AB_SCALE / INTER_TAB_SIZE / 2;
  double M[6];
  if (inverse_map)
    memcpy(M, M6, sizeof(M));
  else
    kcmc_oracle_invert_affine(M6, M);
  int* adelta = (int*)malloc(sizeof(int) * (size_t)(dW > 0 ? dW : 1));
  int* bdelta = (int*)malloc(sizeof(int) * (size_t)(dW > 0 ? dW : 1));
  if (!adelta || !bdelta) {
    free(adelta);
    free(bdelta);
    return -2;
  }
  for (int x = 0; x < dW; ++x) {
    adelta[x] = cv_round(M[0] * x * AB_SCALE);
    bdelta[x] = cv_round(M[3] * x * AB_SCALE);
  }
  /* float bilinear weights, exactly as initInterTab1D/initInterTab2D build them */
  float tab1[2 * 32];
  for (int i = 0; i < INTER_TAB_SIZE; ++i) {
    float x = i * (1.f / INTER_TAB_SIZE);
    tab1[2 * i] = 1.f - x;
    tab1[2 * i + 1] = x;
  }
  const size_t sstep = (size_t)W * C;
  for (int y = 0; y < dH; ++y) {
    int X0 = cv_round((M[1] * y + M[2]) * AB_SCALE) + round_delta;
    int Y0 = cv_round((M[4] * y + M[5]) * AB_SCALE) + round_delta;
    for (int x = 0; x < dW; ++x) {
      int X = (X0 + adelta[x]) >> (AB_BITS - INTER_BITS);
      int Y = (Y0 + bdelta[x]) >> (AB_BITS - INTER_BITS);
      int sx = sat_short(X >> INTER_BITS), sy = sat_short(Y >> INTER_BITS);
      int fx = X & (INTER_TAB_SIZE - 1), fy = Y & (INTER_TAB_SIZE - 1);
      float w[4];
      w[0] = tab1[2 * fy] * tab1[2 * fx];
      w[1] = tab1[2 * fy] * tab1[2 * fx + 1];
      w[2] = tab1[2 * fy + 1] * tab1[2 * fx];
      w[3] = tab1[2 * fy + 1] * tab1[2 * fx + 1];
      uint16_t* D = dst + ((size_t)y * dW + x) * C;
      int inl = (unsigned)sx < (unsigned)(W - 1) && (unsigned)sy < (unsigned)(H - 1);
      if (inl) {
        const uint16_t* S = src + (size_t)sy * sstep + (size_t)sx * C;
        for (int k = 0; k < C; ++k) {
          float v = (float)S[k] * w[0] + (float)S[k + C] * w[1] + (float)S[sstep + k] * w[2] +
                    (float)S[sstep + k + C] * w[3];
          D[k] = sat_ushort_f(v);
        }
      } else if (sx >= W || sx + 1 < 0 || sy >= H || sy + 1 < 0) {
        for (int k = 0; k < C; ++k) D[k] = 0;
      } else {
        int sx0 = (sx >= 0 && sx < W) ? sx : -1, sx1 = (sx + 1 >= 0 && sx + 1 < W) ? sx + 1 : -1;
        int sy0 = (sy >= 0 && sy < H) ? sy : -1, sy1 = (sy + 1 >= 0 && sy + 1 < H) ? sy + 1 : -1;
        for (int k = 0; k < C; ++k) {
          float v0 = (sx0 >= 0 && sy0 >= 0) ? src[(size_t)sy0 * sstep + (size_t)sx0 * C + k] : 0;
          float v1 = (sx1 >= 0 && sy0 >= 0) ? src[(size_t)sy0 * sstep + (size_t)sx1 * C + k] : 0;
          float v2 = (sx0 >= 0 && sy1 >= 0) ? src[(size_t)sy1 * sstep + (size_t)sx0 * C + k] : 0;
          float v3 = (sx1 >= 0 && sy1 >= 0) ? src[(size_t)sy1 * sstep + (size_t)sx1 * C + k] : 0;
          float v = v0 * w[0] + v1 * w[1] + v2 * w[2] + v3 * w[3];
          D[k] = sat_ushort_f(v);
        }
      }
    }
  }
  free(adelta);
  free(bdelta);
  return 0;
}

/* ------------------------------------------------------------------------- */
/* K3 extension oracle: cv2.warpPerspective(img, M, (W, H), INTER_LINEAR) on   */
/* uint16, BORDER_CONSTANT 0 (BASELINE config 5, homography model; the        */
/* reference itself only calls warpAffine, VA:458).  Classic OpenCV 4.x path: */
/* imgwarp.cpp WarpPerspectiveInvoker (per 1024-pixel block of bw0 x bh0      */
/* pixels, double coordinates relative to the block's first column, 1/32-px   */
/* rounding) + remapBilinear's float-weight blend (same as warpAffine).       */
/* ------------------------------------------------------------------------- */

/* cv::invert(M, M) of a 3x3 double matrix with the default DECOMP_LU: OpenCV's
 * closed-form n == 3 branch (core/src/lapack.cpp): det3, then the adjugate times 1/d;
 * a singular matrix gives all zeros.  Returns 1 if invertible. */
int kcmc_oracle_invert_perspective(const double* S, double* M) {
#define SD(r, c) S[3 * (r) + (c)]
  double d = SD(0, 0) * (SD(1, 1) * SD(2, 2) - SD(1, 2) * SD(2, 1)) -
             SD(0, 1) * (SD(1, 0) * SD(2, 2) - SD(1, 2) * SD(2, 0)) +
             SD(0, 2) * (SD(1, 0) * SD(2, 1) - SD(1, 1) * SD(2, 0));
  double t[9];
  if (d == 0) {
    for (int k = 0; k < 9; ++k) M[k] = 0;
    return 0;
  }
  d = 1. / d;
  t[0] = (SD(1, 1) * SD(2, 2) - SD(1, 2) * SD(2, 1)) * d;
  t[1] = (SD(0, 2) * SD(2, 1) - SD(0, 1) * SD(2, 2)) * d;
  t[2] = (SD(0, 1) * SD(1, 2) - SD(0, 2) * SD(1, 1)) * d;
  t[3] = (SD(1, 2) * SD(2, 0) - SD(1, 0) * SD(2, 2)) * d;
  t[4] = (SD(0, 0) * SD(2, 2) - SD(0, 2) * SD(2, 0)) * d;
  t[5] = (SD(0, 2) * SD(1, 0) - SD(0, 0) * SD(1, 2)) * d;
  t[6] = (SD(1, 0) * SD(2, 1) - SD(1, 1) * SD(2, 0)) * d;
  t[7] = (SD(0, 1) * SD(2, 0) - SD(0, 0) * SD(2, 1)) * d;
  t[8] = (SD(0, 0) * SD(1, 1) - SD(0, 1) * SD(1, 0)) * d;
#undef SD
  memcpy(M, t, sizeof(t));
  return 1;
}

/* remapBilinear<Cast<float,ushort>> for one output pixel at fixed-point source
 * coordinate (X, Y) in 1/32 px: taps outside [0,W)x[0,H) read 0. */
static void bilinear_u16(const uint16_t* src, int H, int W, int C, int X, int Y, const float* tab1, uint16_t* D) {
  const size_t sstep = (size_t)W * C;
  int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
  int fx = X & 31, fy = Y & 31;
  float w[4] = {tab1[2 * fy] * tab1[2 * fx], tab1[2 * fy] * tab1[2 * fx + 1], tab1[2 * fy + 1] * tab1[2 * fx],
                tab1[2 * fy + 1] * tab1[2 * fx + 1]};
  for (int k = 0; k < C; ++k) {
    int xs[2] = {sx, sx + 1}, ys[2] = {sy, sy + 1};
    float v[4];
    for (int q = 0; q < 4; ++q) {
      int xx = xs[q & 1], yy = ys[q >> 1];
      v[q] = ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H) ? src[(size_t)yy * sstep + (size_t)xx * C + k]
                                                                        : 0.f;
    }
    D[k] = sat_ushort_f(v[0] * w[0] + v[1] * w[1] + v[2] * w[2] + v[3] * w[3]);
  }
}

int kcmc_oracle_warp_perspective_u16(const uint16_t* src, int H, int W, int C, const double* M9, int inverse_map,
                                     uint16_t* dst, int dH, int dW) {
  if (H <= 0 || W <= 0 || C <= 0 || dH < 0 || dW < 0) return -1;
  if (dH == 0 || dW == 0) return 0;
  double M[9];
  if (inverse_map)
    memcpy(M, M9, sizeof(M));
  else
    kcmc_oracle_invert_perspective(M9, M);
  float tab1[2 * 32];
  for (int i = 0; i < 32; ++i) {
    float x = i * (1.f / 32);
    tab1[2 * i] = 1.f - x;
    tab1[2 * i + 1] = x;
  }
  /* WarpPerspectiveInvoker block shape: BLOCK_SZ = 32 */
  int bh0 = 16 < dH ? 16 : dH;
  int bw0 = 1024 / bh0 < dW ? 1024 / bh0 : dW;
  for (int y = 0; y < dH; ++y) {
    for (int xb = 0; xb < dW; xb += bw0) {
      int bw = bw0 < dW - xb ? bw0 : dW - xb;
      double X0 = M[0] * xb + M[1] * y + M[2];
      double Y0 = M[3] * xb + M[4] * y + M[5];
      double W0 = M[6] * xb + M[7] * y + M[8];
      for (int x1 = 0; x1 < bw; ++x1) {
        double Wd = W0 + M[6] * x1;
        Wd = Wd != 0 ? 32 / Wd : 0;
        double fX = fmax((double)INT32_MIN, fmin((double)INT32_MAX, (X0 + M[0] * x1) * Wd));
        double fY = fmax((double)INT32_MIN, fmin((double)INT32_MAX, (Y0 + M[3] * x1) * Wd));
        int X = cv_round(fX), Y = cv_round(fY);
        bilinear_u16(src, H, W, C, X, Y, tab1, dst + ((size_t)y * dW + xb + x1) * C);
      }
    }
  }
  return 0;
}

/* ------------------------------------------------------------------------- */
/* K2 oracle: skimage 0.18.3 ransac(EuclideanTransform, min_samples=2, ...)   */
/* as called at VA:309-316, in closed form.                                    */
/* ------------------------------------------------------------------------- */

/* numpy's pairwise summation of a contiguous float64 vector (np.sum, used for
 * sum(r**2) at skimage fit.py:847): n<8 sequential, n<=128 eight strided
 * accumulators, else split at n/2 rounded down to a multiple of 8. */
double kcmc_oracle_pairwise_sum(const double* a, int n) {
  if (n < 8) {
    double res = 0.;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  } else if (n <= 128) {
    double r[8];
    int i;
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    for (i = 8; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  } else {
    int n2 = n / 2;
    n2 -= n2 % 8;
    return kcmc_oracle_pairwise_sum(a, n2) + kcmc_oracle_pairwise_sum(a + n2, n - n2);
  }
}

/* Rigid least-squares fit (skimage _umeyama without scaling, _geometric.py:72-144)
 * in closed form: R = rotation maximising tr(R^T A), A = sum dst_d src_d^T.
 * Means are sequential axis-0 sums divided by n (numpy mean).  Returns 0 and the
 * 2x3 [R|t] when A != 0, else 1 (skimage: rank(A) == 0 -> NaN model). */
static int rigid_fit(const double* src, const double* dst, const int* sel, int n, double* P) {
  double ms0 = 0, ms1 = 0, md0 = 0, md1 = 0;
  for (int k = 0; k < n; ++k) {
    int q = sel ? sel[k] : k;
    ms0 += src[2 * q];
    ms1 += src[2 * q + 1];
    md0 += dst[2 * q];
    md1 += dst[2 * q + 1];
  }
  ms0 /= n;
  ms1 /= n;
  md0 /= n;
  md1 /= n;
  double a00 = 0, a01 = 0, a10 = 0, a11 = 0;
  for (int k = 0; k < n; ++k) {
    int q = sel ? sel[k] : k;
    double s0 = src[2 * q] - ms0, s1 = src[2 * q + 1] - ms1;
    double d0 = dst[2 * q] - md0, d1 = dst[2 * q + 1] - md1;
    a00 += d0 * s0;
    a01 += d0 * s1;
    a10 += d1 * s0;
    a11 += d1 * s1;
  }
  double a = a00 + a11, b = a10 - a01;
  if (a == 0 && b == 0) return 1;
  double h = sqrt(a * a + b * b);
  double c = a / h, s = b / h;
  P[0] = c;
  P[1] = -s;
  P[3] = s;
  P[4] = c;
  P[2] = md0 - (c * ms0 - s * ms1);
  P[5] = md1 - (s * ms0 + c * ms1);
  return 0;
}

/* Similarity least-squares fit (skimage _umeyama with estimate_scale=True) in closed
 * form.  With a = a00 + a11, b = a10 - a01 as in rigid_fit, a^2 + b^2 = (s1 +- s2)^2 of
 * A's singular values (the sign of det A), so skimage's scale * R has the entries
 * a / v and b / v with v = sum |src_d|^2 and no root is taken.  v is summed per column
 * in point order and the two column sums are added last: numpy's
 * src_demean.var(axis=0).sum(), and for two points the kernel's
 * (a0 a0 + b0 b0) + (a1 a1 + b1 b1); a per-point sum rounds differently and breaks the
 * bit-exact selection.  Returns 1 (no model) when a == 0 && b == 0, which covers v == 0.
 * Not restated: a pure reflection with a == b == 0 exactly, where skimage's rank-2 branch
 * returns a scale-0 map and this form returns no model. */
static int similarity_fit(const double* src, const double* dst, const int* sel, int n, double* P) {
  double ms0 = 0, ms1 = 0, md0 = 0, md1 = 0;
  for (int k = 0; k < n; ++k) {
    int q = sel ? sel[k] : k;
    ms0 += src[2 * q];
    ms1 += src[2 * q + 1];
    md0 += dst[2 * q];
    md1 += dst[2 * q + 1];
  }
  ms0 /= n;
  ms1 /= n;
  md0 /= n;
  md1 /= n;
  double a00 = 0, a01 = 0, a10 = 0, a11 = 0, v0 = 0, v1 = 0;
  for (int k = 0; k < n; ++k) {
    int q = sel ? sel[k] : k;
    double s0 = src[2 * q] - ms0, s1 = src[2 * q + 1] - ms1;
    double d0 = dst[2 * q] - md0, d1 = dst[2 * q + 1] - md1;
    a00 += d0 * s0;
    a01 += d0 * s1;
    a10 += d1 * s0;
    a11 += d1 * s1;
    v0 += s0 * s0;
    v1 += s1 * s1;
  }
  double a = a00 + a11, b = a10 - a01;
  if (a == 0 && b == 0) return 1;
  double v = v0 + v1;
  double c = a / v, s = b / v;
  P[0] = c;
  P[1] = -s;
  P[3] = s;
  P[4] = c;
  P[2] = md0 - (c * ms0 - s * ms1);
  P[5] = md1 - (s * ms0 + c * ms1);
  return 0;
}

typedef int (*fit_fn)(const double*, const double*, const int*, int, double*);

/* The loop of skimage ransac(min_samples=2) around a two-point model's fit: shared by the
 * rigid and the similarity oracle, which differ in the fit alone. */
static int ransac_two_point(fit_fn fit, const double* src, const double* dst, int N, const int32_t* hyp,
                            int T, double thresh, double* out_params, uint8_t* out_inliers,
                            int32_t* out_best_trial, int32_t* out_n_inliers) {
  double* r2 = (double*)malloc(sizeof(double) * (size_t)(N > 0 ? N : 1));
  uint8_t* cur = (uint8_t*)malloc((size_t)(N > 0 ? N : 1));
  int* sel = (int*)malloc(sizeof(int) * (size_t)(N > 0 ? N : 1));
  if (!r2 || !cur || !sel) {
    free(r2);
    free(cur);
    free(sel);
    return -2;
  }
  int best_n = 0, best_t = -1;
  double best_S = INFINITY;
  memset(out_inliers, 0, (size_t)N);
  for (int t = 0; t < T; ++t) {
    int pair[2] = {hyp[2 * t], hyp[2 * t + 1]};
    double P[6];
    if (fit(src, dst, pair, 2, P)) continue; /* NaN model: count 0, S NaN */
    int cnt = 0;
    for (int k = 0; k < N; ++k) {
      double x = src[2 * k], y = src[2 * k + 1];
      double xp = fma(y, P[1], x * P[0]) + P[2];
      double yp = fma(y, P[4], x * P[3]) + P[5];
      double dx = xp - dst[2 * k], dy = yp - dst[2 * k + 1];
      double r = sqrt(dx * dx + dy * dy);
      cur[k] = r < thresh;
      cnt += cur[k];
      r2[k] = r * r;
    }
    double S = kcmc_oracle_pairwise_sum(r2, N);
    if (cnt > best_n || (cnt == best_n && S < best_S)) {
      best_n = cnt;
      best_S = S;
      best_t = t;
      memcpy(out_inliers, cur, (size_t)N);
      if (best_S <= 0) break; /* stop_residuals_sum = 0 (fit.py:862-869) */
    }
  }
  int rc = 1;
  if (best_n > 0) {
    int m = 0;
    for (int k = 0; k < N; ++k)
      if (out_inliers[k]) sel[m++] = k;
    rc = fit(src, dst, sel, m, out_params);
  }
  if (rc) {
    for (int k = 0; k < 6; ++k) out_params[k] = NAN;
    if (best_n == 0) memset(out_inliers, 0, (size_t)N);
  }
  *out_best_trial = best_t;
  *out_n_inliers = best_n;
  free(r2);
  free(cur);
  free(sel);
  return rc;
}

/* src = frame keypoints, dst = template keypoints (VA:310).  hyp = [T,2] sample
 * indices (trial t uses hyp[t]; numpy RandomState(seed).choice(N, 2, False)).
 * out_params [2,3] (NaN when no model), out_inliers [N] (0/1).
 * Returns 0 when a model was fitted, 1 when skimage would return None. */
int kcmc_oracle_ransac_rigid(const double* src, const double* dst, int N, const int32_t* hyp,
                             int T, double thresh, double* out_params, uint8_t* out_inliers,
                             int32_t* out_best_trial, int32_t* out_n_inliers) {
  return ransac_two_point(rigid_fit, src, dst, N, hyp, T, thresh, out_params, out_inliers, out_best_trial,
                          out_n_inliers);
}

/* K2s oracle: skimage 0.18.3 ransac(SimilarityTransform, min_samples=2, ...), the build's
 * similarity model (an extension: the reference only uses EuclideanTransform, VA:311).
 * Same arguments, return codes and loop as kcmc_oracle_ransac_rigid. */
int kcmc_oracle_ransac_similarity(const double* src, const double* dst, int N, const int32_t* hyp,
                                  int T, double thresh, double* out_params, uint8_t* out_inliers,
                                  int32_t* out_best_trial, int32_t* out_n_inliers) {
  return ransac_two_point(similarity_fit, src, dst, N, hyp, T, thresh, out_params, out_inliers, out_best_trial,
                          out_n_inliers);
}

/* ------------------------------------------------------------------------- */
/* K2 extension oracle: skimage 0.18.3 ransac with AffineTransform            */
/* (min_samples = 3) or ProjectiveTransform (min_samples = 4), the build's     */
/* configs 3-5 (the reference itself only uses EuclideanTransform, VA:311).   */
/* The hypothesis loop is restated in closed form; the final total-least-      */
/* squares refit on the inliers is done in oracle.py with numpy's SVD, as      */
/* skimage does it (_geometric.py:596-703).                                    */
/* ------------------------------------------------------------------------- */

/* skimage _center_and_normalize_points (_geometric.py:18-69) on the k points
 * sel[0..k): centroid = sequential axis-0 mean, rms = sqrt(pairwise_sum of the 2k
 * squared deviations (row-major) / k).  Returns 0 on success, 1 when rms == 0
 * (skimage: ZeroDivisionError -> estimate returns False). */
static int center_normalize(const double* p, const int32_t* sel, int k, double* cx, double* cy, double* nf) {
  double sx = 0, sy = 0;
  for (int i = 0; i < k; ++i) {
    sx += p[2 * sel[i]];
    sy += p[2 * sel[i] + 1];
  }
  *cx = sx / k;
  *cy = sy / k;
  double dev[8];
  for (int i = 0; i < k; ++i) {
    double ex = p[2 * sel[i]] - *cx, ey = p[2 * sel[i] + 1] - *cy;
    dev[2 * i] = ex * ex;
    dev[2 * i + 1] = ey * ey;
  }
  double rms = sqrt(kcmc_oracle_pairwise_sum(dev, 2 * k) / k);
  if (rms == 0) return 1;
  *nf = sqrt(2.0) / rms;
  return 0;
}

/* Affine model through 3 correspondences: the exact solution skimage's TLS finds
 * for a non-degenerate triple, L = [v1 v2][u1 u2]^-1 with u_k = s_k - s_0,
 * v_k = d_k - d_0, t = c_d - L c_s.  Degenerate (skimage's estimate returns False):
 * a point set with rms 0, det == 0, or |V[-1,-1]| = 1/sqrt(1 + |h|^2) <= 1e-8 with h
 * the model in normalised coordinates (np.isclose(V[-1,-1], 0)).  H: 3x3 row-major. */
static int affine_fit3(const double* src, const double* dst, const int32_t* sel, double* H) {
  double csx, csy, nfs, cdx, cdy, nfd;
  if (center_normalize(src, sel, 3, &csx, &csy, &nfs) || center_normalize(dst, sel, 3, &cdx, &cdy, &nfd)) return 1;
  const double *s0 = src + 2 * sel[0], *s1 = src + 2 * sel[1], *s2 = src + 2 * sel[2];
  const double *d0 = dst + 2 * sel[0], *d1 = dst + 2 * sel[1], *d2 = dst + 2 * sel[2];
  double u1x = s1[0] - s0[0], u1y = s1[1] - s0[1], u2x = s2[0] - s0[0], u2y = s2[1] - s0[1];
  double v1x = d1[0] - d0[0], v1y = d1[1] - d0[1], v2x = d2[0] - d0[0], v2y = d2[1] - d0[1];
  double det = u1x * u2y - u2x * u1y;
  if (det == 0) return 1;
  double l00 = (v1x * u2y - v2x * u1y) / det;
  double l01 = (v2x * u1x - v1x * u2x) / det;
  double l10 = (v1y * u2y - v2y * u1y) / det;
  double l11 = (v2y * u1x - v1y * u2x) / det;
  double g = nfd / nfs;
  double hn2 = g * g * (((l00 * l00 + l01 * l01) + l10 * l10) + l11 * l11);
  if (1.0 / sqrt(1.0 + hn2) <= 1e-8) return 1;
  H[0] = l00;
  H[1] = l01;
  H[2] = cdx - (l00 * csx + l01 * csy);
  H[3] = l10;
  H[4] = l11;
  H[5] = cdy - (l10 * csx + l11 * csy);
  H[6] = 0;
  H[7] = 0;
  H[8] = 1;
  return 0;
}

/* Projective model through 4 correspondences as skimage normalises it: Hartley
 * normalisation of both sets, the 8x8 DLT system with h22 = 1 in normalised
 * coordinates (rows: the four x-equations, then the four y-equations, like skimage's
 * A), Gaussian elimination with partial pivoting, H = inv(N_dst) Hn N_src.
 * Degenerate: rms 0, a zero pivot, or 1/sqrt(1 + |h|^2) <= 1e-8. */
static int projective_fit4(const double* src, const double* dst, const int32_t* sel, double* H) {
  double csx, csy, nfs, cdx, cdy, nfd;
  if (center_normalize(src, sel, 4, &csx, &csy, &nfs) || center_normalize(dst, sel, 4, &cdx, &cdy, &nfd)) return 1;
  double M[8][9];
  for (int i = 0; i < 4; ++i) {
    double xs = (src[2 * sel[i]] - csx) * nfs, ys = (src[2 * sel[i] + 1] - csy) * nfs;
    double xd = (dst[2 * sel[i]] - cdx) * nfd, yd = (dst[2 * sel[i] + 1] - cdy) * nfd;
    double rx[9] = {xs, ys, 1, 0, 0, 0, -(xd * xs), -(xd * ys), xd};
    double ry[9] = {0, 0, 0, xs, ys, 1, -(yd * xs), -(yd * ys), yd};
    memcpy(M[i], rx, sizeof(rx));
    memcpy(M[4 + i], ry, sizeof(ry));
  }
  for (int c = 0; c < 8; ++c) {
    int piv = c;
    for (int r = c + 1; r < 8; ++r)
      if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
    if (M[piv][c] == 0) return 1;
    if (piv != c)
      for (int k = c; k < 9; ++k) {
        double t = M[c][k];
        M[c][k] = M[piv][k];
        M[piv][k] = t;
      }
    for (int r = c + 1; r < 8; ++r) {
      double f = M[r][c] / M[c][c];
      for (int k = c; k < 9; ++k) M[r][k] -= f * M[c][k];
    }
  }
  double h[8];
  for (int c = 7; c >= 0; --c) {
    double v = M[c][8];
    for (int k = c + 1; k < 8; ++k) v -= M[c][k] * h[k];
    h[c] = v / M[c][c];
  }
  double hn2 = 0;
  for (int k = 0; k < 8; ++k) hn2 += h[k] * h[k];
  if (1.0 / sqrt(1.0 + hn2) <= 1e-8) return 1;
  /* H = inv(Nd) Hn Ns with inv(Nd) = [[1/nfd, 0, cdx], [0, 1/nfd, cdy], [0, 0, 1]] */
  double T[9];
  for (int r = 0; r < 3; ++r) {
    double a = h[3 * r], b = h[3 * r + 1], c = (r == 2) ? 1.0 : h[3 * r + 2];
    T[3 * r] = a * nfs;
    T[3 * r + 1] = b * nfs;
    T[3 * r + 2] = c - (a * nfs * csx + b * nfs * csy);
  }
  double id = 1.0 / nfd;
  for (int k = 0; k < 3; ++k) {
    H[k] = T[k] * id + cdx * T[6 + k];
    H[3 + k] = T[3 + k] * id + cdy * T[6 + k];
    H[6 + k] = T[6 + k];
  }
  return 0;
}

/* ProjectiveTransform._apply_mat + residuals (_geometric.py:183-202, 548-562):
 * [x y 1] @ H^T in the dgemm operation order used for the rigid model, w == 0 -> eps,
 * divide, r = sqrt(dx^2 + dy^2).  An affine H has an exact [0 0 1] last row, so
 * w == 1 and the division is exact (skipped). */
static double model_residual(int model, const double* H, double x, double y, double xd, double yd) {
  double X = fma(y, H[1], x * H[0]) + H[2];
  double Y = fma(y, H[4], x * H[3]) + H[5];
  if (model == 2) {
    double w = fma(y, H[7], x * H[6]) + H[8];
    if (w == 0) w = DBL_EPSILON;
    X = X / w;
    Y = Y / w;
  }
  double ex = X - xd, ey = Y - yd;
  return sqrt(ex * ex + ey * ey);
}

/* model 1 = affine (hyp [T,3]), 2 = projective (hyp [T,4]).  out_model [9] = the
 * winning hypothesis' 3x3 model (NaN if none), out_inliers [N], best trial and its
 * inlier count as skimage's loop leaves them.  Returns 0 if skimage refits (a best
 * hypothesis with >= 1 inlier), 1 if its model is None, -1/-2 on bad input. */
int kcmc_oracle_ransac_model(int model, const double* src, const double* dst, int N, const int32_t* hyp, int T,
                             double thresh, double* out_model, uint8_t* out_inliers, int32_t* out_best_trial,
                             int32_t* out_n_inliers) {
  if (model != 1 && model != 2) return -1;
  const int ms = model == 1 ? 3 : 4;
  double* r2 = (double*)malloc(sizeof(double) * (size_t)(N > 0 ? N : 1));
  uint8_t* cur = (uint8_t*)malloc((size_t)(N > 0 ? N : 1));
  if (!r2 || !cur) {
    free(r2);
    free(cur);
    return -2;
  }
  int best_n = 0, best_t = -1;
  double best_S = INFINITY;
  for (int k = 0; k < 9; ++k) out_model[k] = NAN;
  memset(out_inliers, 0, (size_t)N);
  for (int t = 0; t < T; ++t) {
    const int32_t* sel = hyp + (size_t)t * ms;
    double Hm[9];
    int bad = model == 1 ? affine_fit3(src, dst, sel, Hm) : projective_fit4(src, dst, sel, Hm);
    if (bad) continue; /* estimate() returned False: the trial is skipped (fit.py:835-838) */
    int cnt = 0;
    for (int k = 0; k < N; ++k) {
      double r = model_residual(model, Hm, src[2 * k], src[2 * k + 1], dst[2 * k], dst[2 * k + 1]);
      cur[k] = r < thresh;
      cnt += cur[k];
      r2[k] = r * r;
    }
    double S = kcmc_oracle_pairwise_sum(r2, N);
    if (cnt > best_n || (cnt == best_n && S < best_S)) {
      best_n = cnt;
      best_S = S;
      best_t = t;
      memcpy(out_inliers, cur, (size_t)N);
      memcpy(out_model, Hm, sizeof(Hm));
      if (best_S <= 0) break; /* stop_residuals_sum = 0 (fit.py:862-869) */
    }
  }
  if (best_n == 0) {
    memset(out_inliers, 0, (size_t)N);
    for (int k = 0; k < 9; ++k) out_model[k] = NAN;
  }
  *out_best_trial = best_t;
  *out_n_inliers = best_n;
  free(r2);
  free(cur);
  return best_n > 0 ? 0 : 1;
}

/* ------------------------------------------------------------------------- */
/* f1 oracle: the build's ORB-style detector (DESIGN.md "f1").  The reference  */
/* detects with OpenCV AKAZE/BRISK (VA:114-116, VA:190-192) and BASELINE        */
/* config 2 names ORB keypoints; OpenCV is absent from this image, so the       */
/* detector is build-defined (parity vs OpenCV unpinned) and exact in integers: */
/*   FAST-9 score (largest t for which 9 contiguous circle pixels are all        */
/*   brighter / darker than the centre by more than t), 3x3 non-maximum        */
/*   suppression (ties: the first in raster order wins), Harris response from   */
/*   integer Sobel sums over 7x7 (R = (ab - c^2) - k (a+b)^2 in double), the     */
/*   n_features largest R (ties: candidate order), intensity-centroid           */
/*   orientation binned to 32 bins with exact cross-product tests, and steered  */
/*   BRIEF (256 pairs, a rotated table per bin) on a 5x5 binomial smoothing.    */
/*   Candidate order = 64x16 tiles in row-major order, raster order inside a    */
/*   tile; the kept keypoints keep that order.                                  */
/* ------------------------------------------------------------------------- */
static const int kFastCircle[16][2] = {{0, 3},  {1, 3},   {2, 2},   {3, 1},  {3, 0},  {3, -1}, {2, -2}, {1, -3},
                                       {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};

int kcmc_oracle_fast_score(const uint8_t* img, int W, int x, int y) {
  const int v = img[(size_t)y * W + x];
  int d[16];
  for (int j = 0; j < 16; ++j) d[j] = (int)img[(size_t)(y + kFastCircle[j][1]) * W + x + kFastCircle[j][0]] - v;
  int best = -1000;
  for (int k = 0; k < 16; ++k) {
    int mb = 1000, md = 1000;
    for (int m = 0; m < 9; ++m) {
      int e = d[(k + m) & 15];
      if (e < mb) mb = e;
      if (-e < md) md = -e;
    }
    if (mb > best) best = mb;
    if (md > best) best = md;
  }
  return best;
}

double kcmc_oracle_harris(const uint8_t* img, int W, int x, int y, double k) {
  long long a = 0, b = 0, c = 0;
  for (int dy = -3; dy <= 3; ++dy)
    for (int dx = -3; dx <= 3; ++dx) {
      const uint8_t* p = img + (size_t)(y + dy) * W + (x + dx);
      int ix = ((int)p[-W + 1] + 2 * (int)p[1] + (int)p[W + 1]) - ((int)p[-W - 1] + 2 * (int)p[-1] + (int)p[W - 1]);
      int iy = ((int)p[W - 1] + 2 * (int)p[W] + (int)p[W + 1]) - ((int)p[-W - 1] + 2 * (int)p[-W] + (int)p[-W + 1]);
      a += (long long)ix * ix;
      b += (long long)iy * iy;
      c += (long long)ix * iy;
    }
  double s = (double)(a + b);
  return (double)(a * b - c * c) - k * (s * s);
}

static uint64_t order_key(double r) {
  uint64_t u;
  memcpy(&u, &r, 8);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}

/* 5x5 binomial smoothing (weights 1 4 6 4 1 per axis, /256 rounded) at (x, y). */
static int smooth5(const uint8_t* img, int W, int x, int y) {
  static const int w[5] = {1, 4, 6, 4, 1};
  int s = 0;
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j) s += w[i] * w[j] * (int)img[(size_t)(y + i - 2) * W + (x + j - 2)];
  return (s + 128) >> 8;
}

int kcmc_oracle_orientation_bin(const uint8_t* img, int W, int x, int y, const double* cs /* [32][2] */) {
  int m10 = 0, m01 = 0;
  for (int dy = -15; dy <= 15; ++dy)
    for (int dx = -15; dx <= 15; ++dx) {
      if (dx * dx + dy * dy > 225) continue;
      int v = img[(size_t)(y + dy) * W + (x + dx)];
      m10 += dx * v;
      m01 += dy * v;
    }
  if (m10 == 0 && m01 == 0) return 0;
  const double a = 0.19634954084936207; /* 2 pi / 32 */
  int k = (int)floor(atan2((double)m01, (double)m10) / a);
  k &= 31;
  double ck = (double)m01 * cs[2 * k] - (double)m10 * cs[2 * k + 1];
  int k1 = (k + 1) & 31;
  double ck1 = (double)m01 * cs[2 * k1] - (double)m10 * cs[2 * k1 + 1];
  if (ck < 0)
    k = (k + 31) & 31;
  else if (ck1 >= 0)
    k = k1;
  return k;
}

/* One frame.  pattern [32 bins][512 points][2] int8 (x, y) = the rotated BRIEF pairs
 * (point 2i and 2i+1 form pair i), cs [32][2] = cos / sin of the bin edges.
 * out_kp [n_features][2] f64 (x, y), out_des [n_features][32] u8.  Returns the count. */
int kcmc_oracle_orb_detect(const uint8_t* img, int H, int W, int threshold, int n_features, double harris_k,
                           int edge, const int8_t* pattern, const double* cs, double* out_kp, uint8_t* out_des) {
  if (H <= 0 || W <= 0) return 0;
  int* score = (int*)calloc((size_t)H * W, sizeof(int));
  size_t cap = (size_t)H * W / 4 + 16, nc = 0;
  uint64_t* key = (uint64_t*)malloc(cap * sizeof(uint64_t));
  int* pos = (int*)malloc(cap * 2 * sizeof(int));
  if (!score || !key || !pos) {
    free(score);
    free(key);
    free(pos);
    return -1;
  }
  for (int y = 3; y < H - 3; ++y)
    for (int x = 3; x < W - 3; ++x) {
      int s = kcmc_oracle_fast_score(img, W, x, y);
      score[(size_t)y * W + x] = s > threshold ? s : 0;
    }
  const int TW = 64, TH = 16;
  for (int ty = 0; ty < H; ty += TH)
    for (int tx = 0; tx < W; tx += TW)
      for (int y = ty; y < ty + TH && y < H; ++y)
        for (int x = tx; x < tx + TW && x < W; ++x) {
          if (y < edge || y >= H - edge || x < edge || x >= W - edge) continue;
          int s = score[(size_t)y * W + x];
          if (s == 0) continue;
          int keep = 1;
          for (int dy = -1; dy <= 1 && keep; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              if (!dx && !dy) continue;
              int q = score[(size_t)(y + dy) * W + (x + dx)];
              int later = dy > 0 || (dy == 0 && dx > 0);
              if (!(s > q || (s == q && later))) {
                keep = 0;
                break;
              }
            }
          if (!keep) continue;
          key[nc] = order_key(kcmc_oracle_harris(img, W, x, y, harris_k));
          pos[2 * nc] = x;
          pos[2 * nc + 1] = y;
          ++nc;
        }
  /* the n_features largest keys; ties in candidate order */
  uint64_t T = 0;
  size_t n_gt = 0;
  if ((size_t)n_features < nc) {
    /* T = the n_features-th largest key */
    uint64_t lo = 0, hi = ~0ull;
    while (lo < hi) { /* largest T with count(key >= T) >= n_features */
      uint64_t mid = lo + (hi - lo) / 2 + 1;
      size_t c = 0;
      for (size_t i = 0; i < nc; ++i) c += key[i] >= mid;
      if (c >= (size_t)n_features)
        lo = mid;
      else
        hi = mid - 1;
    }
    T = lo;
    for (size_t i = 0; i < nc; ++i) n_gt += key[i] > T;
  }
  uint8_t* sm = (uint8_t*)calloc((size_t)H * W, 1);
  int n_out = 0;
  size_t ties = 0;
  for (size_t i = 0; i < nc && sm; ++i) {
    int take;
    if ((size_t)n_features >= nc)
      take = 1;
    else if (key[i] > T)
      take = 1;
    else if (key[i] == T && ties < (size_t)n_features - n_gt) {
      take = 1;
      ++ties;
    } else
      take = 0;
    if (!take) continue;
    int x = pos[2 * i], y = pos[2 * i + 1];
    int bin = kcmc_oracle_orientation_bin(img, W, x, y, cs);
    const int8_t* pt = pattern + (size_t)bin * 512 * 2;
    uint8_t* d = out_des + (size_t)n_out * 32;
    for (int b = 0; b < 32; ++b) {
      int val = 0;
      for (int j = 0; j < 8; ++j) {
        int pi = 8 * b + j;
        int p = smooth5(img, W, x + pt[4 * pi], y + pt[4 * pi + 1]);
        int q = smooth5(img, W, x + pt[4 * pi + 2], y + pt[4 * pi + 3]);
        val |= (p < q) << j;
      }
      d[b] = (uint8_t)val;
    }
    out_kp[2 * n_out] = x;
    out_kp[2 * n_out + 1] = y;
    ++n_out;
  }
  free(sm);
  free(score);
  free(key);
  free(pos);
  return n_out;
}

/* ----------------------------------------------------------------- f4: pyrDown
 * cv2.pyrDown(src, dstsize) for one uint8 frame (VA:501-503; OpenCV 4.x
 * imgproc/src/pyramids.cpp pyrDown_ with FixPtCast<uchar, 8>, BORDER_REFLECT_101):
 * the ring buffer holds the horizontal 1-4-6-4-1 sums of the reflected source rows
 * 2y-2 .. 2y+2 (tabL / tabR reflect the border columns), the vertical pass applies the
 * same weights and rounds with (sum + 128) >> 8.  Returns -1 when OpenCV's assertion
 * |2 dw - W| <= 2 && |2 dh - H| <= 2 fails. */
static int reflect101(int p, int len) {
  if (len == 1) return 0;
  while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

int kcmc_oracle_pyr_down_u8(const uint8_t* src, int H, int W, uint8_t* dst, int DH, int DW) {
  static const int k[5] = {1, 4, 6, 4, 1};
  if (H <= 0 || W <= 0 || abs(DW * 2 - W) > 2 || abs(DH * 2 - H) > 2) return -1;
  for (int y = 0; y < DH; ++y)
    for (int x = 0; x < DW; ++x) {
      int acc = 0;
      for (int i = 0; i < 5; ++i) {
        const uint8_t* row = src + (size_t)reflect101(2 * y + i - 2, H) * W;
        int h = 0;
        for (int j = 0; j < 5; ++j) h += k[j] * row[reflect101(2 * x + j - 2, W)];
        acc += k[i] * h;
      }
      dst[(size_t)y * DW + x] = (uint8_t)((acc + 128) >> 8);
    }
  return 0;
}

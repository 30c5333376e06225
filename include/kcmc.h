/*
 * kcmc.h -- C ABI of the MI355X (gfx950) alignment hot path.
 *
 * Drop-in boundary for the per-frame hot path of VideoAligner
 * (reference: /root/reference/VideoAligner.py, cited as VA:<line>).  The reference
 * farms three per-frame functions out to a joblib process pool through
 * VideoAligner._parallelize (VA:460-471).  Each entry point below replaces one of
 * those per-frame calls with ONE batched call over all frames of a slab:
 *
 *   kcmc_match_frames      <- _get_frame_keypoints matching part (VA:194-214):
 *                             cv2.BFMatcher(crossCheck=False).knnMatch(des_t, des_q, k=2),
 *                             best-match reorder, ratio filter, median filter.
 *   kcmc_knn2_l2u8         <- cv2.BFMatcher().knnMatch(..., k=2) alone (VA:194-195).
 *   kcmc_consensus         <- _get_consensus_kps + _lookup_consensus_kps (VA:224-286),
 *                             host-only, reproducing CPython set/Counter ordering.
 *   kcmc_consensus_vote / _merge / _lookup  <- the same consensus in three parts, the
 *                             per-frame parts on the device (frame-sharded jobs exchange
 *                             only the O(n_tpl) votes).
 *   kcmc_ransac_rigid      <- _compute_euclidean_affine (VA:288-323), i.e. skimage 0.18.3
 *                             ransac(EuclideanTransform, 2, 2, max_trials, random_state).
 *   kcmc_ransac_similarity <- the same call with SimilarityTransform (an extension: the
 *                             reference fits EuclideanTransform only).
 *   kcmc_warp_affine_u16   <- _apply_affine (VA:455-458): cv2.warpAffine(img, M, (W,H),
 *                             INTER_LINEAR), BORDER_CONSTANT 0, classic fixed-point path.
 *   kcmc_warp_affine_cubic_u16 <- nothing in the reference (an extension): the same warp
 *                             with OpenCV's classic INTER_CUBIC restated, grayscale.
 *   kcmc_stack_sum_u16 / kcmc_frame_stats_u16  <- nothing in the reference (an extension):
 *                             the mean image of the aligned stack and every frame's
 *                             correlation moments with it.
 *   kcmc_temporal_sums_u16 <- nothing in the reference (an extension): per pixel over time,
 *                             the sums behind the max projection, the temporal standard
 *                             deviation and the local correlation image of the aligned stack.
 *   kcmc_shift_search_u16  <- nothing in the reference (an extension): the same moments at
 *                             every integer shift in a window, for the intensity fallback
 *                             of frames without a model.
 *   kcmc_gradient_sums_u16 <- nothing in the reference (an extension): the right-hand side
 *                             of one least-squares step of every frame against the mean
 *                             image, for the intensity refinement of the frames' maps.
 *   kcmc_tile_gradient_sums_u16 <- nothing in the reference (an extension): the same
 *                             right-hand side on every patch of a tiling from one read of
 *                             the stack, for the non-rigid intensity refinement.
 *   kcmc_bidi_phase_sums_u16 / kcmc_shift_rows_u16 <- nothing in the reference (an extension):
 *                             the offset of the odd rows of a bidirectionally scanned stack
 *                             against its even rows, measured and undone before registration.
 *   kcmc_box_bandpass_u16  <- nothing in the reference (an extension): the detection copy of a
 *                             stack, box-smoothed with a box background removed.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Pointers named *_dev are device (HBM) pointers
 *     owned by the caller (e.g. torch ROCm tensors' data_ptr()); *_host are host
 *     pointers.  The library never frees caller memory.
 *   - Launch entry points are asynchronous on `stream` (a hipStream_t; NULL = the
 *     null stream) and perform no synchronisation.  The warp, float-matcher and
 *     detector entry points take a per-call workspace from the context's private
 *     stream-ordered memory pool (hipMallocFromPoolAsync / hipFreeAsync on `stream`);
 *     outside stream capture one block per stream is kept and reused in stream order.
 *     Under hipGraph capture the workspace is the graph's own allocation node (never
 *     the per-stream block), so the launches are capturable and a replay never touches
 *     memory that later eager calls may free.  kcmc_ransac_prepare allocates and
 *     synchronises.
 *   - Return value: KCMC_OK (0) or an error code; kcmc_last_error() returns the
 *     calling thread's last message.  Per-frame model failure is NOT an error: it is
 *     NaN in the output parameters, as in the reference (VA:321-322).
 *   - One kcmc_ctx per device; contexts are independent (no global mutable state
 *     except the thread-local error string).
 */
#ifndef KCMC_H_
#define KCMC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KCMC_ABI_VERSION 2

enum {
  KCMC_OK = 0,
  KCMC_EINVAL = 1,       /* bad argument (maps to ValueError on the Python side) */
  KCMC_EHIP = 2,         /* HIP runtime / launch failure */
  KCMC_ENOMEM = 3,       /* allocation failure */
  KCMC_EUNSUPPORTED = 4, /* shape outside what the kernels implement */
  KCMC_EALIGN = 5        /* too few consensus keypoints (VideoAligner.AlignmentError, VA:241-244) */
};

typedef struct kcmc_ctx kcmc_ctx;
typedef void* kcmc_stream_t; /* hipStream_t */

int kcmc_abi_version(void);
const char* kcmc_last_error(void);

/* hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, stream): the pinned-host <-> device
 * transfers of a pipelined caller (e.g. kcmc_amd.pipeline) without a runtime binding of its own. */
int kcmc_memcpy_async(void* dst, const void* src, size_t bytes, kcmc_stream_t stream);

/* Create / destroy the per-device context (holds the uploaded RANSAC hypothesis
 * tables).  `device` is a HIP device ordinal. */
int kcmc_create(int device, kcmc_ctx** out);
int kcmc_destroy(kcmc_ctx* ctx);

/* ---------------------------------------------------------------- K1: matching
 * Brute-force k=2 nearest neighbours under OpenCV NORM_L2 on uint8 descriptors
 * (cv2.BFMatcher default normType, VA:194), batched over frames.
 *   des_tpl_dev [n_tpl, D] u8      template ("query" in OpenCV terms), shared
 *   des_q_dev   [P, D] u8          all frames' descriptors, frame f = rows
 *                                  q_off[f] .. q_off[f+1]-1 ("train" in OpenCV terms)
 *   q_off_dev   [n_frames+1] i32   CSR offsets (device)
 *   max_nq                          max_f (q_off[f+1]-q_off[f]) (host-known bound)
 *   out_idx_dev [n_frames, n_tpl, 2] i32   train index of best / second best (-1: none)
 *   out_dist_dev[n_frames, n_tpl, 2] f32   sqrtf of the exact integer SSD (FLT_MAX: none)
 * Ties go to the lower frame-keypoint index, as OpenCV's K-insertion does.
 * 1 <= D <= 64. */
int kcmc_knn2_l2u8(kcmc_ctx* ctx, const uint8_t* des_tpl_dev, int n_tpl, int D,
                   const uint8_t* des_q_dev, const int32_t* q_off_dev, int n_frames, int max_nq,
                   int32_t* out_idx_dev, float* out_dist_dev, kcmc_stream_t stream);

/* kcmc_knn2_l2u8 + VA:196-214 per frame:
 *   out_kp_ordered_dev [n_frames, n_tpl, 2] f64 = kp_q[best match] for every template row
 *   out_keep_bits_dev  [n_frames, ceil(n_tpl/32)] u32  bit i = template row i survived the
 *                      ratio filter (d0 < ratio*d1, in double) and the displacement filter
 *                      (d_lo*median <= |kp_t - kp_q| <= d_hi*median over ratio survivors)
 *   out_counts_dev     [n_frames, 4] i32 = the four numbers of the reference's per-frame
 *                      debug log (VA:215-221): len(kp_query) (== n_tpl after the reorder),
 *                      len(matches), #ratio survivors, #distance survivors.
 * kp_tpl_dev [n_tpl, 2] f64, kp_q_dev [P, 2] f64 (cv2 KeyPoint.pt promoted to f64).
 * Every frame must have >= 2 keypoints (the reference raises otherwise, VA:203). */
int kcmc_match_frames(kcmc_ctx* ctx, const uint8_t* des_tpl_dev, const double* kp_tpl_dev, int n_tpl,
                      int D, const uint8_t* des_q_dev, const double* kp_q_dev,
                      const int32_t* q_off_dev, int n_frames, int max_nq, double ratio, double d_lo,
                      double d_hi, int32_t* out_idx_dev, float* out_dist_dev,
                      double* out_kp_ordered_dev, uint32_t* out_keep_bits_dev,
                      int32_t* out_counts_dev, kcmc_stream_t stream);

/* VA:196-214 alone, on knn results of any of the matchers (out_idx / out_dist of
 * kcmc_knn2_l2u8 / _hamming / _l2f32): the outputs of kcmc_match_frames after its knn, so that
 * the filter can run on another stream than the knn (ordered after it by the caller). */
int kcmc_match_filter(kcmc_ctx* ctx, const int32_t* idx_dev, const float* dist_dev, const double* kp_tpl_dev,
                      const double* kp_q_dev, const int32_t* q_off_dev, int n_frames, int n_tpl, double ratio,
                      double d_lo, double d_hi, double* out_kp_ordered_dev, uint32_t* out_keep_bits_dev,
                      int32_t* out_counts_dev, kcmc_stream_t stream);

/* -------------------------------------------------- K1 opt-in: binary descriptors, NORM_HAMMING
 * BFMatcher(NORM_HAMMING).knnMatch(k=2): distance = number of differing bits (as a float),
 * ties to the lower frame index.  NOT the reference's matcher (VA:194 uses the default
 * NORM_L2, kcmc_knn2_l2u8); for binary ORB/BRIEF/AKAZE descriptors where Hamming is
 * wanted.  1 <= D <= 64 bytes, fewer than 2^21 rows per frame.  Arguments as
 * kcmc_knn2_l2u8 / kcmc_match_frames (the filters VA:196-214 are the same). */
int kcmc_knn2_hamming(kcmc_ctx* ctx, const uint8_t* des_tpl_dev, int n_tpl, int D, const uint8_t* des_q_dev,
                      const int32_t* q_off_dev, int n_frames, int max_nq, int32_t* out_idx_dev,
                      float* out_dist_dev, kcmc_stream_t stream);
int kcmc_match_frames_hamming(kcmc_ctx* ctx, const uint8_t* des_tpl_dev, const double* kp_tpl_dev, int n_tpl,
                              int D, const uint8_t* des_q_dev, const double* kp_q_dev, const int32_t* q_off_dev,
                              int n_frames, int max_nq, double ratio, double d_lo, double d_hi,
                              int32_t* out_idx_dev, float* out_dist_dev, double* out_kp_ordered_dev,
                              uint32_t* out_keep_bits_dev, int32_t* out_counts_dev, kcmc_stream_t stream);

/* -------------------------------------------------- K1 extension: float descriptors
 * BFMatcher(NORM_L2).knnMatch(k=2) on float32 descriptors (BASELINE config 5,
 * SIFT-style; the reference's AKAZE/BRISK descriptors are uint8, VA:22-25).  Distance:
 * dist = sqrtf((float)sum_k ((double)a_k - (double)b_k)^2) (sequential fp64 sum; OpenCV's
 * own float accumulation order is build-dependent), ties to the lower
 * frame index.  1 <= D <= 128.  Arguments as kcmc_knn2_l2u8 / kcmc_match_frames. */
int kcmc_knn2_l2f32(kcmc_ctx* ctx, const float* des_tpl_dev, int n_tpl, int D, const float* des_q_dev,
                    const int32_t* q_off_dev, int n_frames, int max_nq, int32_t* out_idx_dev,
                    float* out_dist_dev, kcmc_stream_t stream);
int kcmc_match_frames_f32(kcmc_ctx* ctx, const float* des_tpl_dev, const double* kp_tpl_dev, int n_tpl,
                          int D, const float* des_q_dev, const double* kp_q_dev,
                          const int32_t* q_off_dev, int n_frames, int max_nq, double ratio,
                          double d_lo, double d_hi, int32_t* out_idx_dev, float* out_dist_dev,
                          double* out_kp_ordered_dev, uint32_t* out_keep_bits_dev,
                          int32_t* out_counts_dev, kcmc_stream_t stream);

/* ------------------------------------------------------- host: keypoint consensus
 * VA:224-286 on the host, reproducing CPython 3 set/Counter iteration order exactly:
 *   keep_bits_host [n_frames, ceil(n_tpl/32)] u32 (output of kcmc_match_frames)
 *   out_consensus_host [n_kp_global] i32  template indices in Counter.most_common order
 *   out_votes_host     [n_kp_global] i32  their vote counts
 *   *out_n_consensus   number of entries written (<= n_kp_global)
 *   out_pt_off_host [n_frames+1] i32, out_pt_idx_host [n_frames * n_kp_global] i32:
 *       per-frame template indices of list(consensus_set.intersection(frame_set)),
 *       i.e. the RANSAC point order of VA:274.
 * Returns KCMC_EALIGN if fewer than n_min keypoints received any vote (VA:241-244). */
int kcmc_consensus(const uint32_t* keep_bits_host, int n_frames, int n_tpl, int n_kp_global,
                   int n_min, int32_t* out_consensus_host, int32_t* out_votes_host,
                   int* out_n_consensus, int32_t* out_pt_off_host, int32_t* out_pt_idx_host);
/* The same consensus (from all n_frames frames' bitmasks) with the per-frame lists of
 * frames [f_begin, f_end) only: out_pt_off_host [f_end - f_begin + 1] (starting at 0),
 * out_pt_idx_host [(f_end - f_begin) * n_kp_global].  A rank of a frame-sharded job
 * calls it with its own frame range after the bitmask all-gather, so that its host
 * work per step does not grow with the number of ranks. */
int kcmc_consensus_slice(const uint32_t* keep_bits_host, int n_frames, int n_tpl, int n_kp_global,
                         int n_min, int f_begin, int f_end, int32_t* out_consensus_host,
                         int32_t* out_votes_host, int* out_n_consensus, int32_t* out_pt_off_host,
                         int32_t* out_pt_idx_host);

/* ------------------------------------- keypoint consensus in three parts (VA:224-286)
 * The same consensus split so that each rank of a frame-sharded job works on its own
 * frames and exchanges O(n_tpl) numbers instead of every frame's bitmask:
 *   vote   (per rank)   votes [2, n_tpl] i64: row 0 = Counter count of every template over
 *                        the rank's frames (VA:239); row 1 = its first-occurrence key
 *                        (frame_base + f) << 32 | slot, f the first frame whose set holds it
 *                        and slot its position in that CPython set's table (iteration order),
 *                        INT64_MAX if no frame holds it.
 *   merge  (host)       counts summed over ranks, keys min'ed: Counter.most_common(n_kp_global)
 *                        (VA:240) and the iteration order of set(consensus) (VA:248).
 *   lookup (per rank)   list(consensus_set.intersection(frame_set)) per frame (VA:274) as the
 *                        CSR RANSAC point lists.
 * frame_base = global index of the rank's first frame (0 on one device). */
int kcmc_consensus_vote(kcmc_ctx* ctx, const uint32_t* keep_bits_dev, int n_frames, int n_tpl,
                        long long frame_base, int64_t* out_votes_dev, kcmc_stream_t stream);
int kcmc_consensus_vote_host(const uint32_t* keep_bits_host, int n_frames, int n_tpl, long long frame_base,
                             int64_t* out_votes_host);
/* votes_host [world, 2, n_tpl] (the ranks' vote outputs, any order).  out_consensus_host /
 * out_votes_host [n_kp_global] as kcmc_consensus; out_cons_pack_host [n_kp_global + ceil(n_tpl/32)]
 * i32: set(consensus)'s iteration order in [0, nc), its bitmask (u32 words) in [nc, nc + words)
 * -- the input of kcmc_consensus_lookup.  KCMC_EALIGN if fewer than n_min templates were voted. */
int kcmc_consensus_merge(const int64_t* votes_host, int world, int n_tpl, int n_kp_global, int n_min,
                         int32_t* out_consensus_host, int32_t* out_votes_host, int* out_n_consensus,
                         int32_t* out_cons_pack_host);
/* Device lookup: cons_pack_dev = kcmc_consensus_merge's pack (nc entries + bitmask words);
 * out_pt_off_dev [n_frames + 1], out_pt_idx_dev [n_frames * nc]; scratch_dev of at least
 * kcmc_consensus_lookup_scratch_bytes(n_frames, nc) bytes (the CPython set emulation tables
 * that do not fit in LDS; 0 bytes -- scratch_dev may be NULL -- while nc < 308). */
long long kcmc_consensus_lookup_scratch_bytes(int n_frames, int nc);
int kcmc_consensus_lookup(kcmc_ctx* ctx, const uint32_t* keep_bits_dev, int n_frames, int n_tpl,
                          const int32_t* cons_pack_dev, int nc, int32_t* out_pt_off_dev,
                          int32_t* out_pt_idx_dev, void* scratch_dev, kcmc_stream_t stream);
int kcmc_consensus_lookup_host(const uint32_t* keep_bits_host, int n_frames, int n_tpl,
                               const int32_t* cons_iter_host, int nc, int32_t* out_pt_off_host,
                               int32_t* out_pt_idx_host);

/* The boundary of a slab's RANSAC output for NaN-gap filling across ranks (VA:347-407):
 * params_dev [n_frames, E] f64 (E = 6 for [F,2,3], 9 for [F,3,3]); out_dev [2 + 2E] f64 =
 * (first frame without NaN or -1, last such frame or -1, its E params, the last one's E params). */
int kcmc_params_boundary(kcmc_ctx* ctx, const double* params_dev, int n_frames, int E, double* out_dev,
                         kcmc_stream_t stream);

/* --------------------------------------------------------------- K2: RANSAC
 * The seeded sample stream skimage 0.18.3 consumes: trial t of a frame with n points
 * uses np.random.RandomState(seed).choice(n, min_samples, replace=False) drawn t+1-th
 * (fit.py:791, 819-826), i.e. the first min_samples entries of the t-th legacy
 * MT19937 permutation.  out_host [trials, min_samples] i32.  Host only. */
int kcmc_hypothesis_table(int n, int trials, uint32_t seed, int min_samples, int32_t* out_host);

/* Build (host, cached per context) and upload the rigid (min_samples = 2) tables for
 * the point counts n_values_host[0..count) (each in [3, 65535]).  Allocates and
 * synchronises when a new count appears; call before kcmc_ransac_rigid with every
 * point count that frame batch will run RANSAC on. */
int kcmc_ransac_prepare(kcmc_ctx* ctx, const int32_t* n_values_host, int count, int trials, uint32_t seed);

/* Batched rigid RANSAC, one frame per workgroup.
 * Point k of frame f (k < N_f = pt_off[f+1]-pt_off[f]):
 *   pt_idx_dev == NULL: src = src_dev[pt_off[f]+k], dst = dst_dev[pt_off[f]+k]
 *   pt_idx_dev != NULL: q = pt_idx[pt_off[f]+k]; src = src_dev[f*src_frame_stride + q],
 *                       dst = dst_dev[q]        (src = kcmc_match_frames' kp_ordered,
 *                                                dst = template keypoints: VA:275-276)
 * src = frame keypoints, dst = template keypoints (VA:310).  Frames with
 * N_f < n_skip (VideoAligner.N_KP_FRAME_SKIP) or with no inlier get NaN params.
 *   out_params_dev   [n_frames, 2, 3] f64  model.params[:2], translation * spatial_rate
 *   out_inliers_dev  [P] u8                best hypothesis' inlier mask (skimage ransac's
 *                                          second return value), CSR like the points
 *   out_n_inliers_dev[n_frames] i32, out_best_trial_dev[n_frames] i32 (-1: none)
 * max_n >= every N_f; every N_f >= max(n_skip, 3) must have been prepared with the same
 * `trials` (kcmc_ransac_prepare); a missing table yields NaN for that frame and
 * n_inliers = -1. */
int kcmc_ransac_rigid(kcmc_ctx* ctx, const double* src_dev, const double* dst_dev,
                      const int32_t* pt_idx_dev, const int32_t* pt_off_dev, int src_frame_stride,
                      int n_frames, int max_n, int trials, double residual_threshold,
                      double spatial_rate, int n_skip, double* out_params_dev,
                      uint8_t* out_inliers_dev, int32_t* out_n_inliers_dev,
                      int32_t* out_best_trial_dev, kcmc_stream_t stream);

/* K2s: batched similarity RANSAC (rotation, translation and one scale), i.e. skimage 0.18.3
 * ransac(..., SimilarityTransform, min_samples=2, ...): _umeyama(estimate_scale=True) for
 * the 2-point hypotheses and for the refit on the inliers.  The same kernel as
 * kcmc_ransac_rigid (its scorer, selection and early exit), the same parameter list, the
 * same hypothesis tables (kcmc_ransac_prepare) and the same outputs and NaN conventions:
 *   out_params_dev   [n_frames, 2, 3] f64  model.params[:2] = [scale * R | t],
 *                                          translation * spatial_rate
 * Its parity with skimage rests on an operation-for-operation numpy restatement
 * (tests/test_similarity_host.py), not on a golden from skimage itself.  The bit-exact
 * yardstick of the selection (winning trial, inlier count and mask) is the C oracle
 * kcmc_oracle_ransac_similarity (oracle/kcmc_oracle.c, test infrastructure), the same
 * closed form, itself pinned to that restatement. */
int kcmc_ransac_similarity(kcmc_ctx* ctx, const double* src_dev, const double* dst_dev,
                           const int32_t* pt_idx_dev, const int32_t* pt_off_dev, int src_frame_stride,
                           int n_frames, int max_n, int trials, double residual_threshold,
                           double spatial_rate, int n_skip, double* out_params_dev,
                           uint8_t* out_inliers_dev, int32_t* out_n_inliers_dev,
                           int32_t* out_best_trial_dev, kcmc_stream_t stream);

/* ------------------------------------------------- K2 extension: affine / projective
 * The reference only fits EuclideanTransform (VA:311).  BASELINE configs 3-5 need the
 * other scikit-image 0.18.3 models through the same ransac call (fit.py:621-881):
 *   KCMC_MODEL_AFFINE      ransac(..., AffineTransform,     min_samples=3, ...)
 *   KCMC_MODEL_PROJECTIVE  ransac(..., ProjectiveTransform, min_samples=4, ...)
 * with the same seeded sample stream (RandomState(seed).choice(N, min_samples, False)
 * per trial) and skimage's total-least-squares refit on the inliers
 * (_geometric.py:596-703). */
enum { KCMC_MODEL_EUCLIDEAN = 0, KCMC_MODEL_AFFINE = 1, KCMC_MODEL_PROJECTIVE = 2, KCMC_MODEL_SIMILARITY = 3 };

/* kcmc_ransac_prepare for min_samples in {2, 3, 4} (2 is kcmc_ransac_prepare itself).
 * Every point count must exceed min_samples (skimage raises otherwise, fit.py:798). */
int kcmc_ransac_prepare_samples(kcmc_ctx* ctx, int min_samples, const int32_t* n_values_host, int count,
                                int trials, uint32_t seed);

/* Batched affine / projective RANSAC (model = KCMC_MODEL_AFFINE or _PROJECTIVE); points,
 * pt_idx/pt_off/src_frame_stride, outputs and NaN conventions as kcmc_ransac_rigid,
 * except:
 *   out_params_dev [n_frames, 3, 3] f64  model.params (affine: last row 0 0 1), scaled for
 *                                         spatial downsampling as S H S^-1, S = diag(r, r, 1)
 *                                         (affine: translation * r, like VA:320)
 * Frames with N_f < max(n_skip, min_samples + 1) get NaN.  Tables for every other N_f
 * must have been prepared with kcmc_ransac_prepare_samples(ctx, min_samples, ...). */
int kcmc_ransac_model(kcmc_ctx* ctx, int model, const double* src_dev, const double* dst_dev,
                      const int32_t* pt_idx_dev, const int32_t* pt_off_dev, int src_frame_stride,
                      int n_frames, int max_n, int trials, double residual_threshold,
                      double spatial_rate, int n_skip, double* out_params_dev,
                      uint8_t* out_inliers_dev, int32_t* out_n_inliers_dev,
                      int32_t* out_best_trial_dev, kcmc_stream_t stream);

/* ------------------------------------------------------------------ K3: warp
 * cv2.warpAffine(frame, M_f, (W, H), flags=INTER_LINEAR [| WARP_INVERSE_MAP]) for
 * every frame: src_dev/dst_dev [n_frames, H, W, C] u16 (C interleaved, C=1 for the
 * reference's grayscale stacks), M_dev [n_frames, 2, 3] f64 forward maps (inverted
 * in double exactly as OpenCV does unless inverse_map != 0).  Out-of-image taps
 * read 0.  Bit-exact to the classic OpenCV fixed-point algorithm on platforms
 * without FMA contraction.  A frame whose map holds a NaN is zeros.
 * Alignment: src_dev and dst_dev need only the natural 2-byte alignment of uint16_t -- any
 * element of a larger allocation may be the first (a tensor view, a frame range of a stack
 * with odd W).  The kernels choose their 16-byte staging loads (W % 8 == 0), their buffer
 * loads and stores through descriptors based at src_dev / dst_dev (the fast path) and their
 * 4-byte pixel-pair stores (W even, or C = 3 / 4) from W alone, never from the pointers, so
 * off the 16- / 4-byte grid these accesses are unaligned; that they return and write the right
 * bytes rests on gfx950's unaligned global and buffer memory access (the driver's default
 * unaligned access mode), not on code here.  Measured, not assumed: the seeded sweeps
 * tests/test_gpu_sweeps.py::test_warp_affine_sweep / test_warp_perspective_sweep run both
 * entries with sources 0, 2, 8 and 16 bytes and outputs 0 and 2 bytes off the grids on every
 * staging and store path (tests/test_sweep_cases_host.py lists them), bit for bit against
 * the oracle, the sources and outputs between sentinels.  The pipeline's own slabs start on
 * frame boundaries of aligned allocations and never take the unaligned case. */
int kcmc_warp_affine_u16(kcmc_ctx* ctx, const uint16_t* src_dev, uint16_t* dst_dev,
                         const double* M_dev, int n_frames, int H, int W, int C, int inverse_map,
                         kcmc_stream_t stream);

/* cv2.warpPerspective(frame, M_f, (W, H), flags=INTER_LINEAR [| WARP_INVERSE_MAP]) for
 * every frame -- the warp of the homography extension (BASELINE config 5; the
 * reference's own warp is warpAffine, VA:458).  M_dev [n_frames, 3, 3] f64 forward maps,
 * inverted like cv::invert (closed-form 3x3) unless inverse_map != 0; classic
 * WarpPerspectiveInvoker fixed-point coordinates (per-block double evaluation, 1/32 px)
 * and the remapBilinear blend of kcmc_warp_affine_u16; out-of-image taps read 0; a frame
 * whose map holds a NaN is zeros.  Alignment as kcmc_warp_affine_u16: src_dev and dst_dev
 * need only 2-byte alignment (the 16-byte staging loads with W % 8 == 0 and the 4-byte
 * pixel-pair stores are then unaligned device accesses; pinned by the same sweep). */
int kcmc_warp_perspective_u16(kcmc_ctx* ctx, const uint16_t* src_dev, uint16_t* dst_dev,
                              const double* M_dev, int n_frames, int H, int W, int C, int inverse_map,
                              kcmc_stream_t stream);

/* K3f: the piecewise-rigid field warp -- kcmc_warp_affine_u16 (grayscale, C = 1) with a smooth
 * per-pixel residual source displacement added to the fixed-point source coordinate.  The
 * reference has no such mode: the semantics are BUILD-DEFINED, in exact integer arithmetic,
 * and pinned by a numpy restatement (tests/test_piecewise_host.py), not by a golden.
 *   M_dev     [n_frames, 2, 3] f64   forward maps (or inverse maps with inverse_map != 0),
 *                                    exactly as kcmc_warp_affine_u16 takes them
 *   field_dev [n_frames, gy, gx, 2] i32   q: the residual displacement (x, y) at the nodes of
 *                                    a gy x gx grid, in 1/1024 px; 1 <= gy, gx <= 16,
 *                                    gy <= H, gx <= W.  Contract |q| <= 2^20: beyond it the
 *                                    pixels are unspecified (never an out-of-bounds access).
 * Node (i, j) sits at pixel-index coordinates cx_j = (j + 0.5) W / gx - 0.5,
 * cy_i = (i + 0.5) H / gy - 0.5.  For output pixel (x, y):
 *   X_aff, Y_aff: kcmc_warp_affine_u16's 1/1024-px coordinates adelta[x] + X0(y) (the same
 *     inversion, the same cvRounds, the same + 16).
 *   Along an axis of length L with g nodes, at pixel index p (integer divisions):
 *     g == 1: k0 = 0, w = 0; otherwise
 *     num = clamp((2p + 1) g - L, 0, 2L (g - 1)), k0 = min(num / (2L), g - 2),
 *     w = ((num - k0 2L) 1024 + L) / (2L)   in [0, 1024]
 *     (the field is held constant outside the outermost node centres).
 *   (i0, wy) from (y, H, gy), (j0, wx) from (x, W, gx); per component, arithmetic shifts:
 *     v_j = (q[i0][j] (1024 - wy) + q[i0 + 1][j] wy + 512) >> 10        (vertical first)
 *     val = (v_j0 (1024 - wx) + v_{j0 + 1} wx + 512) >> 10              (then horizontal)
 *     (a term with weight 0 is dropped: q[i0 + 1] / v_{j0 + 1} need not exist)
 *   X = X_aff + val_x, Y = Y_aff + val_y; then kcmc_warp_affine_u16 again: integer part
 *   sat_short(X >> 10), fraction (X >> 5) & 31, OpenCV's float blend, cvRound with
 *   saturation, taps outside the image read 0, a frame whose map holds a NaN is zeros.
 * So a field of equal nodes q moves every pixel by exactly q, and a zero field gives
 * kcmc_warp_affine_u16's output bit for bit.  Asynchronous on `stream`, capturable under the
 * affine warp's workspace rules; n_frames == 0 returns KCMC_OK; a NULL ctx or pointer,
 * H or W < 1 or a grid outside the limits return KCMC_EINVAL before any device work. */
int kcmc_warp_field_u16(kcmc_ctx* ctx, const uint16_t* src_dev, uint16_t* dst_dev, const double* M_dev,
                        const int32_t* field_dev, int n_frames, int H, int W, int gy, int gx,
                        int inverse_map, kcmc_stream_t stream);

/* K3c: bicubic warpAffine of grayscale frames -- kcmc_warp_affine_u16 with INTER_CUBIC in place
 * of INTER_LINEAR.  The reference never resamples cubically: the semantics are BUILD-DEFINED, a
 * restatement of OpenCV's classic algorithm (WarpAffineInvoker + remapBicubic<Cast<float,
 * ushort>, float, 1>, BORDER_CONSTANT 0) pinned by a numpy restatement
 * (tests/test_warp_cubic_host.py); PARITY WITH cv2 IS UNPINNED.  For output pixel (x, y) of a
 * frame with 2 x 3 map M (forward, or inverse with inverse_map != 0):
 *   1. Coordinates: exactly kcmc_warp_affine_u16's -- the same inversion, the same cvRounds,
 *      the same + 16, X and Y in 1/1024 px; sx = sat_short(X >> 10), fx = (X >> 5) & 31,
 *      likewise sy, fy.  A frame whose map holds a NaN is zeros.
 *   2. 1-D weights: the cubic-convolution kernel with A = -3/4 at t = f / 32,
 *        c0 = ((A (t + 1) - 5A)(t + 1) + 8A)(t + 1) - 4A
 *        c1 = ((A + 2) t - (A + 3)) t^2 + 1
 *        c2 = ((A + 2)(1 - t) - (A + 3))(1 - t)^2 + 1
 *        c3 = 1 - c0 - c1 - c2
 *      OpenCV evaluates them in float32; for all 32 fractions every intermediate is exact and
 *      each weight is an integer multiple of 2^-17 (f = 0: [0, 1, 0, 0]; f = 16:
 *      [-3, 19, 19, -3] / 32; f = 1: [-2883, 130789, 3259, -93] / 2^17).
 *   3. 2-D weights: w[i][j] = fl32(c_i(fy) c_j(fx)), one float32 rounding of the exact product
 *      (OpenCV's BicubicTab_f entry).
 *   4. Taps S[sy - 1 + i][sx - 1 + j], i, j = 0..3, as float32; a tap outside the image reads
 *      0.  Every product p_ij = fl32(S w) and every sum is a separate float32 operation (no FMA
 *      contraction).
 *        interior pixel (0 <= sx - 1, sx + 2 <= W - 1, the same in y; never when W or H < 4):
 *          r_i = ((p_i0 + p_i1) + p_i2) + p_i3,  sum = ((r_0 + r_1) + r_2) + r_3
 *        any other pixel: sum = 0, then sum = sum + p_ij for i = 0..3 and within that j = 0..3
 *   5. Output: saturate_cast<ushort>(sum) -- rintf, then a clamp to [0, 65535]; the negative
 *      lobes make the clamp reachable on both sides.
 * So an identity map returns the source bit for bit and an integer shift is a copy with zeros
 * shifted in.  Arguments and limits as kcmc_warp_affine_u16 (H, W < 32768, at most 65535 frames,
 * in-place refused), except: a NULL ctx or pointer and H or W < 1 return KCMC_EINVAL before any
 * device work, n_frames == 0 returns KCMC_OK, C == 3 or 4 return KCMC_EUNSUPPORTED (grayscale
 * only in this version) and any other C != 1 KCMC_EINVAL.  Asynchronous on `stream`, capturable
 * under the affine warp's workspace rules. */
int kcmc_warp_affine_cubic_u16(kcmc_ctx* ctx, const uint16_t* src_dev, uint16_t* dst_dev,
                               const double* M_dev, int n_frames, int H, int W, int C,
                               int inverse_map, kcmc_stream_t stream);

/* ------------------------------------------- f2: normalisation front end (VA:100-104)
 * brightest = np.percentile(images, 99.99) (VA:479-482) needs two order statistics of
 * the flattened uint16 stack; they come from two streaming 256-bin histogram passes:
 *   kcmc_histogram_u16(..., shift = 8, match = -1, ...)   counts of every value's high byte
 *   kcmc_histogram_u16(..., shift = 0, match = h, ...)    counts of the low byte of the values
 *                                                          whose high byte is h
 * out_hist_dev [256] u64 (overwritten).  src_dev 16-byte aligned, n elements. */
int kcmc_histogram_u16(kcmc_ctx* ctx, const uint16_t* src_dev, unsigned long long n, int shift, int match,
                       unsigned long long* out_hist_dev, kcmc_stream_t stream);

/* images_u8 = lut[images] for every element: the host evaluates the reference's
 * np.clip(v / brightest * 255, 0, 255).astype(uint8) (VA:484-492) once per uint16 value
 * (lut_dev [65536] u8); all buffers 16-byte aligned. */
int kcmc_lut_u16_to_u8(kcmc_ctx* ctx, const uint16_t* src_dev, unsigned long long n, const uint8_t* lut_dev,
                       uint8_t* dst_dev, kcmc_stream_t stream);

/* ------------------------------------------------------ f1: keypoint detection
 * The build's exact ORB-style detector (replaces the host OpenCV
 * detectAndCompute of VA:114-116 / VA:190-192, parity vs OpenCV unpinned): FAST-9
 * score > threshold, 3x3 NMS, the n_features largest integer-Harris responses
 * (harris_k), intensity-centroid orientation in 32 bins, steered BRIEF on a 5x5
 * binomial smoothing.  frames_dev [n_frames, H, W] u8 (e.g. kcmc_lut_u16_to_u8 output);
 * pattern_dev [32][512][2] i8 and bin_cs_dev [32][2] f64 from kcmc_amd/orb.py;
 * edge >= 16.  Outputs per frame, in candidate order (64x16 tiles row-major, raster
 * inside a tile): out_kp_dev [n_frames, n_features, 2] f64 (x, y),
 * out_des_dev [n_frames, n_features, 32] u8, out_count_dev [n_frames] i32.
 * frames_dev needs no alignment (4-byte staging loads are used only when W % 4 == 0 and
 * frames_dev is 4-byte aligned; otherwise byte loads, same result).  n_features == 0
 * needs only frames_dev and out_count_dev (zeroed); the other pointers may then be NULL. */
int kcmc_orb_detect(kcmc_ctx* ctx, const uint8_t* frames_dev, int n_frames, int H, int W, int threshold,
                    int n_features, double harris_k, int edge, const int8_t* pattern_dev,
                    const double* bin_cs_dev, double* out_kp_dev, uint8_t* out_des_dev,
                    int32_t* out_count_dev, kcmc_stream_t stream);

/* ------------------------------------------------------ f1: the scale pyramid
 * Build-defined like the detector; the host computes every size and quota as integers
 * (kcmc_amd/orb.py level_sizes / level_quotas) and the kernels receive integers only.
 *
 * The exact bilinear resize that makes level l from level l - 1: src_dev [n_frames, H, W]
 * u8 -> dst_dev [n_frames, dst_h, dst_w] u8, any sizes in [1, 65535] (upscaling too), no
 * alignment requirement, at most 65535 frames per call.  Per axis, source length n,
 * destination length m, destination index x:
 *   num = (2x + 1) n - m, den = 2m, i = floor(num / den),
 *   a = ((num - i den) 2048 + m) / den (integer division);
 *   i < 0 -> i = 0, a = 0;  i >= n - 1 -> i = n - 1, a = 0 (second tap clamped to n - 1);
 *   dst = (sum of the 4 taps x (2048 - a | a)(2048 - b | b) + 2^21) >> 22.
 * m == n is the identity; an exact 2:1 is (sum of the 2x2 + 2) >> 2. */
int kcmc_resize_u8(kcmc_ctx* ctx, const uint8_t* src_dev, int n_frames, int H, int W, uint8_t* dst_dev,
                   int dst_h, int dst_w, kcmc_stream_t stream);

/* kcmc_orb_detect on every level of a scale pyramid.  Host arrays level_h, level_w,
 * level_quota [n_levels], n_levels in [1, 8]: level 0 must be (H, W), sizes >= 1 and
 * non-increasing, quotas >= 0 with sum n_features (else KCMC_EINVAL, before any launch).
 * orb.py: H_l = rint(H / scale_factor^l) (half to even, doubles), W_l alike; with
 * f = 1 / scale_factor and d_0 = n_features (1 - f) / (1 - f^n_levels), level
 * l < n_levels - 1 gets rint(d_l), d_{l+1} = d_l f, the last max(n_features - sum, 0).
 * Level l is kcmc_resize_u8 of level l - 1 (level 0: frames_dev).  Every level runs the
 * detector above unchanged on its image with its quota as the budget (same threshold,
 * harris_k, edge, tables); a level with H_l or W_l < 2 edge + 1, or quota 0, yields nothing
 * and its quota is not redistributed.  Output rows: level 0 first, each level in its
 * candidate order, packed without gaps; out_count_dev = the sum of the levels' counts; rows
 * at or past it are undefined.  Coordinates are mapped to level 0 through the resize's own
 * pixel map, one correctly rounded double division per axis:
 *   x0 = ((2 x_l + 1) W - W_l) / (2 W_l),  y0 = ((2 y_l + 1) H - H_l) / (2 H_l)
 * (level 0: x0 = x_l exactly; not OpenCV's x * scale, which the rounding of the level sizes
 * biases).  out_level_dev [n_frames, n_features] u8 names each row's level.  The levels
 * live in the context workspace; frames are batched so that it stays bounded. */
int kcmc_orb_detect_pyramid(kcmc_ctx* ctx, const uint8_t* frames_dev, int n_frames, int H, int W, int threshold,
                            int n_features, double harris_k, int edge, const int8_t* pattern_dev,
                            const double* bin_cs_dev, int n_levels, const int32_t* level_h,
                            const int32_t* level_w, const int32_t* level_quota, double* out_kp_dev,
                            uint8_t* out_des_dev, uint8_t* out_level_dev, int32_t* out_count_dev,
                            kcmc_stream_t stream);

/* ----------------------------------------------------- f4: spatial downsample
 * cv2.pyrDown(frame, dstsize=(dst_w, dst_h)) of every uint8 frame (replaces the per-frame
 * host calls of VideoAligner._downsample, VA:501-503): 5x5 binomial (1,4,6,4,1)^2 / 256,
 * BORDER_REFLECT_101, (sum + 128) >> 8.  src_dev [n_frames, H, W] u8, dst_dev
 * [n_frames, dst_h, dst_w] u8, both 4-byte aligned.  KCMC_EINVAL (OpenCV's assertion)
 * unless |2 dst_w - W| <= 2 and |2 dst_h - H| <= 2. */
int kcmc_pyr_down_u8(kcmc_ctx* ctx, const uint8_t* src_dev, int n_frames, int H, int W, uint8_t* dst_dev,
                     int dst_h, int dst_w, kcmc_stream_t stream);

/* ------------------------------------------------ q1: registration quality metrics
 * Two streaming reductions of a grayscale uint16 stack, exact in 64-bit integers (the
 * results do not depend on the order in which workgroups finish).  Asynchronous on
 * `stream`, capturable, no allocation; each zeroes its own output first.
 *
 * out_sum_dev [n_px] i64 = the per-pixel sum over the frames f with sel_dev[f] != 0
 * (sel_dev [n_frames] u8; NULL = every frame) of frames_dev [n_frames, n_px] u16.  Any
 * n_frames, n_px and alignment of frames_dev; the 16-byte path needs n_px % 8 == 0 and a
 * 16-byte aligned frames_dev. */
int kcmc_stack_sum_u16(kcmc_ctx* ctx, const uint16_t* frames_dev, int n_frames, unsigned long long n_px,
                       const uint8_t* sel_dev, long long* out_sum_dev, kcmc_stream_t stream);

/* out_dev [n_frames, 5] i64 = (sum a, sum b, sum a^2, sum b^2, sum a*b) over the pixels of
 * rows [y0, y1) and columns [x0, x1), a = frame f of frames_dev [n_frames, H, W] u16 and
 * b = ref_dev [H, W] u16: the integer moments of Pearson's correlation of every frame with
 * a reference image.  H * W < 2^31 (sum a*b <= 65535^2 * H * W fits 63 bits); an empty
 * rectangle is KCMC_EINVAL.  The 16-byte path needs W % 8 == 0 and 16-byte aligned
 * frames_dev / ref_dev. */
int kcmc_frame_stats_u16(kcmc_ctx* ctx, const uint16_t* frames_dev, int n_frames, int H, int W,
                         const uint16_t* ref_dev, int y0, int y1, int x0, int x1, long long* out_dev,
                         kcmc_stream_t stream);

/* ------------------------------------------------ q2: summary images (temporal sums)
 * Build-defined: the reference reports nothing about the aligned stack, and has nothing
 * like this pass.
 *
 * One streaming reduction of frames_dev [n_frames, H, W] u16 per pixel over time, over the
 * frames f with sel_dev[f] != 0 (sel_dev [n_frames] u8; NULL = every frame; unselected
 * frames are not loaded) and the pixels p = (y, x) of rows [y0, y1) and columns [x0, x1).
 * With a_f the value of p in frame f and b_f the value of a partner pixel in the same frame:
 *
 *   out_sums_dev [K, H, W] i64, K = 2 + neighbours / 2
 *     plane 0   sum_f a_f
 *     plane 1   sum_f a_f^2
 *     plane 2   sum_f a_f * b_f,  partner (y, x + 1)
 *     plane 3   sum_f a_f * b_f,  partner (y + 1, x)
 *     plane 4   sum_f a_f * b_f,  partner (y + 1, x + 1)     neighbours = 8 only
 *     plane 5   sum_f a_f * b_f,  partner (y + 1, x - 1)     neighbours = 8 only
 *   out_max_dev [H, W] u16 = max_f a_f
 *
 * A pair sum is 0 where the partner lies outside the rectangle (column x1 - 1 never pairs
 * with column x0 of the next row).  Every output element outside the rectangle is 0; with no
 * selected frame everything is 0 and the call succeeds.  The other four (eight) neighbours
 * of a pixel are the same sums read at the partner: sum a(y, x) a(y, x - 1) is plane 2 at
 * (y, x - 1), and so on.  From these, exactly: the mean and the max projection, the temporal
 * variance n * plane 1 - plane 0^2, and Pearson's r over time of every pixel with each
 * neighbour (kcmc_amd.summary).
 *
 * Contract (KCMC_EINVAL before any device work otherwise, as for a NULL ctx or pointer):
 * neighbours 4 or 8; 0 <= y0 < y1 <= H, 0 <= x0 < x1 <= W, H * W < 2^31; out_sums_dev 8-byte
 * and out_max_dev 4-byte aligned.  out_max_dev is updated in aligned 32-bit words (compare
 * and swap: the hardware has no 16-bit integer atomics), so when H * W is odd the buffer must
 * extend 2 bytes past the last pixel; those bytes keep their value.  KCMC_EUNSUPPORTED when
 * tiles times frame chunks reach 2^31.  Any n_frames (plane 1 and the pair planes stay below
 * 2^31 * 65535^2 < 2^63), any W and alignment of frames_dev: the 16-byte path needs
 * W % 8 == 0 and a 16-byte aligned frames_dev, everything else is read element by element.
 *
 * Exact: every sum is a 64-bit integer (the results do not depend on the order in which
 * workgroups finish).  Asynchronous on `stream`, capturable, no allocation; zeroes its own
 * outputs first. */
int kcmc_temporal_sums_u16(kcmc_ctx* ctx, const uint16_t* frames_dev, int n_frames, int H, int W,
                           const uint8_t* sel_dev, int y0, int y1, int x0, int x1, int neighbours,
                           long long* out_sums_dev, uint16_t* out_max_dev, kcmc_stream_t stream);

/* ------------------------------------- s1: exact shift search (intensity fallback)
 * Build-defined: the reference never registers a frame RANSAC gave no model (it
 * interpolates the frame's map from its neighbours, VA:347-437) and has no intensity mode.
 *
 * out_dev [n_sel, 2R + 1, 2R + 1, 5] i64: entry [s][dy + R][dx + R] = (sum a, sum b, sum a^2,
 * sum b^2, sum a*b) over rows [y0, y1) and columns [x0, x1), with
 *   a = frames_dev[frame_idx_dev[s]][y + dy][x + dx]   (frames_dev [n_frames, H, W] u16),
 *   b = ref_dev[y][x]                                  (ref_dev [H, W] u16),
 * i.e. the moments of kcmc_frame_stats_u16 (same layout and meaning) at every integer shift
 * of the frame in [-R, R]^2; entry (0, 0) equals that function's row for the same frame and
 * rectangle.  A shift (dy, dx) with a high correlation says frame(p + d) ~ ref(p).
 *
 * frame_idx_dev [n_sel] i32; NULL = frames 0 .. n_sel - 1.  An index outside [0, n_frames)
 * gives an all-zero row and is never read through; repeated and unordered indices are fine.
 *
 * Contract (KCMC_EINVAL before any device work otherwise, as for a NULL ctx or pointer):
 * 1 <= R <= 16, y0 < y1, x0 < x1, y0 - R >= 0, y1 + R <= H, x0 - R >= 0, x1 + R <= W,
 * H * W < 2^31, out_dev 8-byte aligned.  n_sel == 0 is KCMC_OK.  Any alignment of frames_dev /
 * ref_dev and any W: the 16-byte path needs W % 8 == 0 and 16-byte aligned frames_dev and
 * ref_dev, everything else is staged element by element.
 *
 * Exact: every sum is a 64-bit integer (no floating point, no dependence on the order in
 * which workgroups finish; narrower partial sums are bounded for all-65535 input).
 * Asynchronous on `stream`, no allocation; zeroes its own output first. */
int kcmc_shift_search_u16(kcmc_ctx* ctx, const uint16_t* frames_dev, int n_frames, int H, int W,
                          const int32_t* frame_idx_dev, int n_sel, const uint16_t* ref_dev, int y0, int y1,
                          int x0, int x1, int R, long long* out_dev, kcmc_stream_t stream);

/* ----------------------------- g1: gradient sums (intensity refinement of the maps)
 * Build-defined: the reference registers frames on keypoints only and has no dense step.
 *
 * One linearised least-squares (Gauss-Newton) step of an aligned frame a against a
 * reference image b models a(p) ~ alpha b(p - u(p)) + beta, u(p) = (tx - theta y', ty + theta x'),
 * as a ~ alpha b + beta + qx gx + qy gy + qt gr with the integer gradients (twice the central
 * difference)
 *   gx(y, x) = b(y, x + 1) - b(y, x - 1),   gy(y, x) = b(y + 1, x) - b(y - 1, x),
 *   gr = x' gy - y' gx,   x' = x - (x0 + x1) / 2,   y' = y - (y0 + y1) / 2   (integer division),
 * and tx = -2 qx / alpha, ty = -2 qy / alpha, theta = -2 qt / alpha.  The normal matrix depends on
 * b and the rectangle only (host, kcmc_amd.refine.gram); this entry point gives what
 * depends on the frame.
 *
 * out_dev [n_sel, n_bands, 7] i64, n_bands = ceil((y1 - y0) / band_rows): row [s][k] = (sum a,
 * sum a^2, sum a b, sum a gx, sum a gy, sum x' a gy, sum y' a gx) over the rows [y0 + k band_rows,
 * min(y1, y0 + (k + 1) band_rows)) and the columns [x0, x1), a = frames_dev[frame_idx_dev[s]]
 * (frames_dev [n_frames, H, W] u16), b = ref_dev [H, W] u16.  The caller adds the bands (the
 * sum over bands may pass 2^63).  sum a gr = sum x' a gy - sum y' a gx.  Pixels outside the
 * rectangle contribute nothing as a; as b they are read where the gradient at the
 * rectangle's edge needs them.
 *
 * frame_idx_dev [n_sel] i32; NULL = frames 0 .. n_sel - 1.  An index outside [0, n_frames)
 * gives all-zero rows and is never read through; repeated and unordered indices are fine.
 *
 * Contract (KCMC_EINVAL before any device work otherwise, as for a NULL ctx or pointer):
 * 1 <= y0 < y1 <= H - 1 and 1 <= x0 < x1 <= W - 1 (the gradient reads +-1), H * W < 2^31,
 * out_dev 8-byte aligned, band_rows >= 1 and
 *   band_rows * (x1 - x0) * max(x1 - x0, y1 - y0) < 2^32.
 * That bound keeps every band sum below 2^63 for any input: a band has at most
 * band_rows * (x1 - x0) pixels, a <= 65535 and |gx|, |gy| <= 65535 make every product a^2, a b,
 * a g smaller than 2^32, and |x'| <= (x1 - x0) / 2, |y'| <= (y1 - y0) / 2, so the largest sum is
 * below band_rows * (x1 - x0) * (max / 2) * 2^32 < 2^63.  (1080p: one band would do; 4K needs
 * several.)  n_sel == 0 is KCMC_OK; KCMC_EUNSUPPORTED when n_sel * n_bands >= 2^31.  Any
 * alignment of frames_dev / ref_dev and any W: the 16-byte path needs W % 8 == 0 and 16-byte
 * aligned frames_dev and ref_dev, everything else is read element by element.
 *
 * Exact: every value is a signed 64-bit integer (no floating point); one workgroup owns
 * each (frame, band) and writes its row with plain stores, so nothing depends on the order
 * in which workgroups finish.  Asynchronous on `stream`, no allocation, no memset: every
 * row of out_dev is written. */
int kcmc_gradient_sums_u16(kcmc_ctx* ctx, const uint16_t* frames_dev, int n_frames, int H, int W,
                           const int32_t* frame_idx_dev, int n_sel, const uint16_t* ref_dev, int y0, int y1,
                           int x0, int x1, int band_rows, long long* out_dev, kcmc_stream_t stream);

/* ----------------------------- g2: gradient sums per tile (non-rigid intensity refinement)
 * Build-defined: the reference has no dense step and no non-rigid mode.
 *
 * g1's right-hand side on every patch of a tiling, from one read of the stack: the translation
 * part of g1's model, a ~ alpha b + beta + qx gx + qy gy with the same integer gradients gx, gy of
 * b (twice the central difference), fitted per patch (host, kcmc_amd.refine_field) gives a
 * displacement per grid node instead of one per frame.
 *
 * row_edges_host [ty + 1], col_edges_host [tx + 1] i32, HOST arrays (as level_h of
 * kcmc_orb_detect_pyramid), non-decreasing: tile (i, j) is the rows [row_edges[i],
 * row_edges[i + 1]) and the columns [col_edges[j], col_edges[j + 1]).  They are read and
 * validated before any device work and handed to the kernel by value: no upload, no
 * synchronisation, and the call can be captured into a graph.
 *
 * out_dev [n_sel, ty, tx, 5] i64: entry [s][i][j] = (sum a, sum a^2, sum a b, sum a gx, sum a gy)
 * over tile (i, j), a = frames_dev[frame_idx_dev[s]] (frames_dev [n_frames, H, W] u16),
 * b = ref_dev [H, W] u16; a, b, gx, gy exactly as in kcmc_gradient_sums_u16, so the sum over all
 * tiles equals the first five of its sums over the rectangle [row_edges[0], row_edges[ty]) x
 * [col_edges[0], col_edges[tx]).  A tile without pixels (two equal edges) gives zeros.  Pixels
 * outside the tiling contribute nothing as a; as b they are read where the gradient at the
 * tiling's edge needs them.
 *
 * frame_idx_dev [n_sel] i32; NULL = frames 0 .. n_sel - 1.  An index outside [0, n_frames)
 * gives all-zero rows and is never read through; repeated and unordered indices are fine.
 *
 * Contract (KCMC_EINVAL before any device work otherwise, as for a NULL ctx or pointer):
 * 1 <= ty, tx <= 32, both edge lists non-decreasing, 1 <= row_edges[0], row_edges[ty] <= H - 1,
 * 1 <= col_edges[0], col_edges[tx] <= W - 1 (the gradient reads +-1), H * W < 2^31, out_dev 8-byte
 * aligned.  n_sel == 0 is KCMC_OK; KCMC_EUNSUPPORTED when n_sel * ty >= 2^31.  Any alignment of
 * frames_dev / ref_dev and any W: the 16-byte path needs W % 8 == 0 and 16-byte aligned
 * frames_dev and ref_dev, everything else is read element by element.
 *
 * Exact: every value is a signed 64-bit integer (no floating point).  A tile has fewer than
 * 2^31 pixels and every product a^2, a b, a g is below 2^32 in magnitude, so no tile sum can
 * reach 2^63; there are no coordinate moments, so no bands.  One workgroup owns each (frame,
 * tile row), adds its threads' integer partial sums in LDS and writes its tx entries with
 * plain stores, so nothing depends on the order in which workgroups or waves finish.
 * Asynchronous on `stream`, no allocation, no memset: every entry of out_dev is written. */
int kcmc_tile_gradient_sums_u16(kcmc_ctx* ctx, const uint16_t* frames_dev, int n_frames, int H, int W,
                                const int32_t* frame_idx_dev, int n_sel, const uint16_t* ref_dev,
                                const int32_t* row_edges_host, int ty, const int32_t* col_edges_host, int tx,
                                long long* out_dev, kcmc_stream_t stream);

/* ----------------------------- b1: bidirectional-scan phase correction (row offset)
 * Build-defined: the reference has no such mode.  A microscope that scans bidirectionally
 * acquires the odd image rows on the return sweep; an error in its line clock displaces every
 * odd row horizontally against the even rows by a constant.  These two entry points measure
 * that offset in whole pixels and undo it (host part: kcmc_amd.bidi; numpy restatement:
 * tests/test_bidi_host.py).
 *
 * out_dev [n_sel, 2R + 1, 5] u64: for the selected frame F = frames_dev[frame_idx_dev[s]]
 * (frames_dev [n_frames, H, W] u16) and every d in [-R, R], entry [s][d + R] = (sum a, sum b,
 * sum a^2, sum b^2, sum a*b) -- the layout of kcmc_frame_stats_u16 -- over the samples
 *   one vertically adjacent row pair (y, y + 1), 0 <= y < H - 1, at one column x in [R, W - R):
 *   a = F[the pair's odd row][x + d],  b = F[the pair's even row][x].
 * There are n = (H - 1) (W - 2R) samples for every d; an interior row is in two pairs and counts
 * twice.  A high correlation at d says odd(x + d) ~ even(x): the odd rows are corrected by
 * kcmc_shift_rows_u16(..., parity = 1, d).
 *
 * frame_idx_dev [n_sel] i32; NULL = frames 0 .. n_sel - 1.  An index outside [0, n_frames)
 * gives an all-zero row and is never read through; repeated and unordered indices are fine.
 *
 * Contract (KCMC_EINVAL before any device work otherwise, as for a NULL ctx or pointer):
 * 0 <= R <= 16, H >= 2, W >= 2R + 1, H * W < 2^31 (every sum stays below 2^63), out_dev 8-byte
 * aligned.  n_sel == 0 is KCMC_OK.  Any alignment of frames_dev and any W: the 16-byte path needs
 * W % 8 == 0 and a 16-byte aligned frames_dev, everything else is read element by element.  No
 * load leaves the image.
 *
 * Exact: every sum is a 64-bit integer (no floating point), added into the zeroed output with
 * 64-bit integer atomics, so nothing depends on the order in which workgroups finish.
 * Asynchronous on `stream`, no allocation; zeroes its own output first. */
int kcmc_bidi_phase_sums_u16(kcmc_ctx* ctx, const uint16_t* frames_dev, int n_frames, int H, int W,
                             const int32_t* frame_idx_dev, int n_sel, int R, uint64_t* out_dev,
                             kcmc_stream_t stream);

/* dst_dev[f][y][x] = src_dev[f][y][clamp(x + d, 0, W - 1)] for the rows with (y & 1) == parity and
 * src_dev[f][y][x] for the others; src_dev / dst_dev [n_frames, H, W] u16.  The edge pixel is
 * replicated, not zero-filled (a comb of zeros at the border would hand the detector corners).
 * parity is 0 or 1; |d| <= 16, also when that exceeds W (the clamp covers it: the shifted rows are
 * then filled with their edge pixel); H, W < 32768.
 * src_dev == dst_dev is allowed -- in place, and then only the rows of the parity are touched (with
 * d == 0 nothing is launched); any other overlap of the two stacks is KCMC_EINVAL.  Out of place
 * every row is written (d == 0: a copy) and src_dev is only read.  n_frames == 0 is KCMC_OK; a NULL
 * ctx or pointer and arguments outside the limits are KCMC_EINVAL before any device work.  Any
 * alignment and any W: 16-byte loads and stores need W % 8 == 0 and 16-byte aligned stacks (and a
 * row of at most 32728 pixels), everything else moves element by element.  A workgroup reads a row
 * completely before any of it is written.  Asynchronous on `stream`, no allocation. */
int kcmc_shift_rows_u16(kcmc_ctx* ctx, const uint16_t* src_dev, uint16_t* dst_dev, int n_frames, int H, int W,
                        int parity, int d, kcmc_stream_t stream);

/* ----------------------------- p1: box band-pass prefilter in front of keypoint detection
 * Build-defined: the reference has no such mode.  The detection copy of a uint16 stack: a small
 * box smoothing minus a large box background, floored at 0 (host part: kcmc_amd.prefilter; numpy
 * restatement: tests/test_prefilter_host.py).  Two integer radii: s = smooth_radius in [0, 4], r =
 * background_radius, 0 or in [s + 1, 32]; not both 0.  For one frame src[H][W], a radius rho and the
 * pixel (y, x) the window is clipped to the image (rho = 0: the pixel itself):
 *
 *   rows y0 = max(0, y - rho) .. y1 = min(H - 1, y + rho), columns x0 = max(0, x - rho) .. x1 = min(W - 1, x + rho)
 *   n_rho = (y1 - y0 + 1) (x1 - x0 + 1)
 *   S_rho = the sum of src over the window              <= 65535 * 65^2 < 2^32
 *   m_rho = (S_rho + n_rho / 2) / n_rho                 the rounded mean, integer division
 *
 *   a = m_s,  b = r > 0 ? m_r : 0,  dst[y][x] = max(a - b, 0)
 *
 * The box of ones in the denominator makes a constant frame filter to 0 right up to the border
 * (r > 0; to itself with r = 0); the floor at 0 keeps the bright features for the percentile
 * scaling that follows.  Once r >= max(H, W) - 1 every pixel's background is the rounded mean of
 * the whole frame.  Frames are independent; src_dev / dst_dev [n_frames, H, W] u16.
 *
 * Contract (KCMC_EINVAL before any device work otherwise): ctx not NULL, n_frames >= 0, H >= 1,
 * W >= 1 (frames smaller than the window are fine), the radii as above; with n_frames > 0 also
 * src_dev and dst_dev not NULL and the two stacks must not overlap (a neighbourhood filter cannot
 * run in place).  n_frames == 0 is KCMC_OK once the shape and the radii have passed: nothing is
 * touched and the two pointers are not looked at (they may be NULL).  Any 2-byte aligned pointers
 * and any W; frame offsets are 64-bit.  No load or store leaves the two stacks.  Exact integers
 * throughout, so the result does not depend on how the work is cut.  Asynchronous on `stream`, no
 * allocation. */
int kcmc_box_bandpass_u16(kcmc_ctx* ctx, const uint16_t* src_dev, uint16_t* dst_dev, int n_frames, int H, int W,
                          int smooth_radius, int background_radius, kcmc_stream_t stream);

/* How kcmc_box_bandpass_u16 cuts that call's work, for tests and tools that want shapes at the
 * kernel's seams: plan_host[4] = (output columns of one workgroup's strip, strips per frame, row
 * chunks per frame, rows per chunk).  Every chunk holds at least one row: (chunks - 1) * rows < H <=
 * chunks * rows.  The same checks of the shape and the radii; host only, no context, no device
 * work. */
int kcmc_box_bandpass_plan(int n_frames, int H, int W, int smooth_radius, int background_radius, int* plan_host);

#ifdef __cplusplus
}
#endif
#endif /* KCMC_H_ */

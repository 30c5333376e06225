// K1: batched k=2 L2 matching of uint8 descriptors (the per-frame match filters that
// follow it are in match_filter.hip).
//
// Reference: VA:194-195 (cv2.BFMatcher(crossCheck=False).knnMatch(des_template,
// des_query, k=2)).
//
// knn2_l2u8_kernel -- persistent: a workgroup keeps 256 / 512 template rows in registers
//   and matches them against a strided set of frames.
//   The distance is an exact integer contraction, so it runs on the int8 matrix
//   cores.  With x = a - 128 (template) and y = 127 - b (frame), both int8,
//   a - b = x + y + 1, so SSD = T + Q + 2 x.y with T = sum(x^2 + 2x) + D per template
//   row and Q = sum(y^2 + 2y) per frame row.  One v_mfma_i32_32x32x32_i8 pass per
//   32-deep k-step gives x.y (accumulator from zero).  T is constant along a template
//   column, so a column's frame rows are ordered by SSD - T + B = Q + 2 x.y + B, with
//   B = 2^20 = max T; the key is non-negative because SSD >= 0 (and < 2^23).  A operand = 32 frame
//   descriptors (rows j), B operand = 32 template descriptors (columns i): each lane
//   owns one template column and 16 frame rows of the 32x32 tile and keeps a running
//   top-2 in registers.
//   The top-2 runs on 32-bit keys ((SSD - T + B) << 8 | j - q0) local to a 256-row
//   chunk of frame descriptors: for D <= 64 bytes sqrtf is strictly increasing on the
//   integer SSD range, so integer keys order exactly like OpenCV's float
//   distances, and the low bits make ties go to the lower frame index like OpenCV's
//   K-insertion.  2.5 VALU ops per distance (the kernel is bound by integer VALU issue,
//   4 cycles per wave64 op): key = acc << 9 + qk (v_lshl_add, qk = (Q + B) << 8 | j - q0
//   from LDS) for two rows of a column, then b2 = min(b2, med3(b1, ka, kb)),
//   b1 = min3(b1, ka, kb), on two independent top-2 pairs per column so that consecutive
//   pairs do not wait on each other.  Each chunk's top-2 is merged into a 64-bit
//   (ssd << 32 | j) top-2 with SSD = (key >> 8) + T - B.  Frame descriptors are staged
//   through LDS (converted to int8, zero-padded to DP, rows padded by 16 B so the
//   ds_read_b128 fragment reads are bank-conflict free).
#include <cfloat>
#include <climits>

#include <atomic>

#include "match_common.h"

namespace kcmc {

// CU count of the calling thread's current device, cached per device id.
int device_cus() {
  static std::atomic<int> cache[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  int cus = cache[dev].load(std::memory_order_relaxed);
  if (cus <= 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    cache[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kBlocksPerWave = 2;                         // 32-row template blocks per wave
template <int WAVES>
struct KnnShape {
  static constexpr int kThreads = 64 * WAVES;
  static constexpr int kTplPerWG = WAVES * kBlocksPerWave * 32;  // template rows per workgroup
};
constexpr int kQChunk = 256;                              // frame descriptors per LDS chunk (8-bit local index)
constexpr uint32_t kNoKey = 0xffffffffu;                  // chunk keys of real rows are < 2^31
constexpr uint32_t kPad = 0xc0000000u;                    // key of the padding rows of a tile (acc = 0)
// Bias of the frame-row term: B = 2^20 = max T (T = sum (x + 1)^2 over D <= 64 bytes with
// x = a - 128 in [-128, 127]: 64 * 128^2).  The biased keys stay >= 0 only because the SSD
// they encode is >= 0; the asserts keep every real key below the padding key.
constexpr int kBias = 1 << 20;
static_assert(64 * 128 * 128 <= kBias, "kBias must cover the largest template term T");
static_assert(((64ull * 255 * 255) << 8 | 0xffull) < kPad, "real keys (SSD << 8 | row) must stay below kPad");
constexpr unsigned long long kNoKey64 = ~0ull;

__device__ __forceinline__ uint32_t min3_u32(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// b1 <= b2 always; new b2 = median(b1, b2, key), new b1 = min(b1, key).
__device__ __forceinline__ void top2_insert(uint32_t& b1, uint32_t& b2, uint32_t key) {
  b2 = med3_u32(b1, b2, key);
  b1 = b1 < key ? b1 : key;
}

// two keys at once (3 ops): the second smallest of {b1, b2, ka, kb} is
// min(b2, median(b1, ka, kb)) because b2 >= b1.  Exact when the keys are distinct or
// equal keys are interchangeable (the per-chunk keys carry their row).
__device__ __forceinline__ void top2_insert2(uint32_t& b1, uint32_t& b2, uint32_t ka, uint32_t kb) {
  const uint32_t m = med3_u32(b1, ka, kb);
  b1 = min3_u32(b1, ka, kb);
  b2 = b2 < m ? b2 : m;
}

__device__ __forceinline__ void top2_insert64(unsigned long long& b1, unsigned long long& b2, unsigned long long key) {
  const unsigned long long hi = b1 > key ? b1 : key;
  b2 = b2 < hi ? b2 : hi;
  b1 = b1 < key ? b1 : key;
}

// 4 consecutive descriptor bytes at column `col`, each XORed with `x` (0x80: a - 128,
// 0x7f: 127 - b as int8), zero past D.
__device__ __forceinline__ uint32_t load4_xor(const uint8_t* row, int col, int D, uint32_t x) {
  uint32_t w = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    uint32_t v = (col + b < D) ? (uint32_t)(row[col + b] ^ x) : 0u;
    w |= v << (8 * b);
  }
  return w;
}

// sum(v^2 + 2v) over the four int8 lanes of w, accumulated into acc
__device__ __forceinline__ int sq2(uint32_t w, int acc) {
  acc = __builtin_amdgcn_sdot4((int)w, (int)w, acc, false);
  return __builtin_amdgcn_sdot4((int)w, 0x02020202, acc, false);
}

// Chunk staging, one frame descriptor row per thread (row q0 + tid of a 256-row chunk):
// 16-byte loads at offsets 0, 16, ... of the row (rows are not 16-byte aligned unless
// D % 16 == 0; unaligned global loads are allowed), the last one running up to 15 bytes
// into the next row (masked off when landing).  The rows at the end of des_q whose last
// load would run past the buffer (staged_row_overruns: the last row, and for D <= 7 the few
// before it) read that piece bytewise (load_row_pieces).  The loads of the next chunk are issued
// before the current chunk's MFMA tiles so that their latency hides behind them.
// Landing turns them into the padded int8 row (127 - b, zero past D), its key part
// (Q + B) << 8 | row and the LDS writes, all in registers.
template <int DP>
struct RowPieces {
  static constexpr int kNP = DP / 16;
};

template <int DP>
__device__ __forceinline__ void land_row(uint8_t* qrow, uint32_t* qk, int r, bool real, int D,
                                         const uint4 (&pf)[RowPieces<DP>::kNP]) {
  int nb = kBias;
#pragma unroll
  for (int k = 0; k < RowPieces<DP>::kNP; ++k) {
    uint4 v = pf[k];
    // int8 127 - b inside the row, zero past D (the masks are uniform)
    v.x = (v.x ^ 0x7f7f7f7fu) & byte_mask(D, k, 0);
    v.y = (v.y ^ 0x7f7f7f7fu) & byte_mask(D, k, 1);
    v.z = (v.z ^ 0x7f7f7f7fu) & byte_mask(D, k, 2);
    v.w = (v.w ^ 0x7f7f7f7fu) & byte_mask(D, k, 3);
    if (!real) v = make_uint4(0u, 0u, 0u, 0u);
    nb = sq2(v.x, nb);
    nb = sq2(v.y, nb);
    nb = sq2(v.z, nb);
    nb = sq2(v.w, nb);
    *reinterpret_cast<uint4*>(qrow + 16 * k) = v;
  }
  // padding rows of the last tile (zero descriptors, so acc = 0) get the key kPad
  *qk = real ? (((uint32_t)nb << 8) | (uint32_t)r) : kPad;
}

// Persistent, template-stationary: workgroup (tg, g) keeps template rows
// [tg * kTplPerWG, +kTplPerWG) in registers for the whole launch and walks frames g,
// g + G, g + 2G, ... (G workgroups per template group), so the template is loaded once per
// workgroup instead of once per frame, and the loads of the next 256-row chunk -- which
// may be the next frame's first -- are in flight while the current chunk is matched.
// WAVES = 8: 512 template rows share each staged chunk (n_tpl > 256); WAVES = 4 otherwise.
template <int DP, int WAVES>
__global__ __launch_bounds__(KnnShape<WAVES>::kThreads) void knn2_l2u8_kernel(
    const uint8_t* __restrict__ des_tpl, int n_tpl, int D, const uint8_t* __restrict__ des_q,
    const int32_t* __restrict__ q_off, int n_frames, int n_tg, int32_t* __restrict__ out_idx,
    float* __restrict__ out_dist) {
  constexpr int KSTEPS = DP / 32;
  constexpr int ROWB = DP + 16;  // padded LDS row stride (bytes)
  // double-buffered chunks: one barrier per chunk (a wave writes chunk c + 1 only after
  // every wave has passed the barrier of chunk c, i.e. finished chunk c - 1)
  __shared__ __attribute__((aligned(16))) uint8_t qbuf[2][kQChunk * ROWB];
  __shared__ __attribute__((aligned(16))) uint32_t qkey[2][kQChunk];

  // the template groups of a frame get consecutive ids of one XCD's run: they stage the
  // same frame rows, which then stay in that XCD's L2
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int tg = id % n_tg, g = id / n_tg, G = gridDim.x / n_tg;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int c = lane & 31;   // MFMA column (template row within a block)
  const int h = lane >> 5;   // k-half of the fragment / row group of the output
  const int last_global = q_off[n_frames] - 1;  // des_q's last row

  // ---- template fragments (B operand) and T = sum(x^2 + 2x) + D, kept in registers
  v4i bfrag[kBlocksPerWave][KSTEPS];
  int tk[kBlocksPerWave];
  int tpl_row[kBlocksPerWave];
#pragma unroll
  for (int b = 0; b < kBlocksPerWave; ++b) {
    const int i = tg * KnnShape<WAVES>::kTplPerWG + (wave * kBlocksPerWave + b) * 32 + c;
    tpl_row[b] = i;
    int na = 0;
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (i < n_tpl) {
        const uint8_t* row = des_tpl + (size_t)i * D;
#pragma unroll
        for (int d = 0; d < 4; ++d) w[d] = load4_xor(row, 32 * kk + 16 * h + 4 * d, D, 0x80u);
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) na = sq2(w[d], na);
      bfrag[b][kk] = v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    }
    na += __shfl_xor(na, 32);
    tk[b] = na + D;
  }

  // ---- the item sequence: the 256-row chunks of frames g, g + G, ... that have rows
  // (a frame without rows still gets its epilogue).  nxt = the item whose loads are in
  // flight: frame nf, first row nq0 (nf >= n_frames: none).
  auto advance = [&](int f, int q0) -> int2 {  // the item after (f, q0)
    if (q0 + kQChunk < q_off[f + 1] - q_off[f]) return make_int2(f, q0 + kQChunk);
    for (f += G; f < n_frames && q_off[f + 1] == q_off[f]; f += G) {
    }
    return make_int2(f, 0);
  };
  auto issue = [&](int2 it, uint4 (&pf)[RowPieces<DP>::kNP]) {
    if (it.x < n_frames && tid < kQChunk) {
      const int qb = q_off[it.x], nq = q_off[it.x + 1] - qb;
      const int r = qb + it.y + min(tid, nq - it.y - 1);
      load_row_pieces(des_q + (size_t)r * D, D, staged_row_overruns(D, last_global - r), pf);
    }
  };
  uint4 pf[RowPieces<DP>::kNP];
  int2 nxt = make_int2(g, 0);  // the first item: frame g's first chunk, or the next frame with rows
  if (g < n_frames && q_off[g + 1] == q_off[g]) nxt = advance(g, 0);
  issue(nxt, pf);
  int buf = 0;
  for (int f = g; f < n_frames; f += G) {
    const int n_q = q_off[f + 1] - q_off[f];
    unsigned long long g1[kBlocksPerWave], g2[kBlocksPerWave];
#pragma unroll
    for (int b = 0; b < kBlocksPerWave; ++b) g1[b] = g2[b] = kNoKey64;
    for (int q0 = 0; q0 < n_q; q0 += kQChunk, buf ^= 1) {
      const int cnt = min(kQChunk, n_q - q0);
      const int rows = (cnt + 31) & ~31;
      // ---- stage frame descriptors [q0, q0+cnt) as int8 127 - b, zero-padded to DP columns
      if (tid < rows) land_row<DP>(&qbuf[buf][tid * ROWB], &qkey[buf][tid], tid, tid < cnt, D, pf);
      __syncthreads();
      nxt = advance(f, q0);
      issue(nxt, pf);
      const uint8_t* qb = qbuf[buf];
      const uint32_t* qkb = qkey[buf];
      uint32_t b1[kBlocksPerWave][2], b2[kBlocksPerWave][2];  // [even | odd accumulator]
#pragma unroll
      for (int b = 0; b < kBlocksPerWave; ++b) b1[b][0] = b2[b][0] = b1[b][1] = b2[b][1] = kNoKey;
      // ---- MFMA tiles of 32 frame rows
      for (int t0 = 0; t0 < rows; t0 += 32) {
        v4i afrag[KSTEPS];
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk)
          afrag[kk] = *reinterpret_cast<const v4i*>(&qb[(t0 + c) * ROWB + 32 * kk + 16 * h]);
        // rows of this lane's 16 accumulators: t0 + (r&3) + 8*(r>>2) + 4*h
        uint32_t qk[16];
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
#pragma unroll
          for (int s2 = 0; s2 < 4; ++s2) qk[4 * gg + s2] = qkb[t0 + 8 * gg + 4 * h + s2];
        // every block's MFMAs first, so that block b + 1's matrix work overlaps block b's
        // top-2 epilogue instead of the epilogue waiting out each chain's latency
        v16i acc[kBlocksPerWave];
#pragma unroll
        for (int b = 0; b < kBlocksPerWave; ++b) {
          acc[b] = v16i{};
#pragma unroll
          for (int kk = 0; kk < KSTEPS; ++kk)  // acc = x.y
            acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[kk], bfrag[b][kk], acc[b], 0, 0, 0);
        }
#pragma unroll
        for (int b = 0; b < kBlocksPerWave; ++b)
#pragma unroll
          for (int p = 0; p < 8; ++p)
            top2_insert2(b1[b][p & 1], b2[b][p & 1], ((uint32_t)acc[b][2 * p] << 9) + qk[2 * p],
                         ((uint32_t)acc[b][2 * p + 1] << 9) + qk[2 * p + 1]);
      }
      // ---- fold the chunk's top-2 (local indices) into the frame's 64-bit top-2: the
      // even / odd pairs merge in 32 bits first (c1 <= c2 = the chunk's two smallest keys)
#pragma unroll
      for (int b = 0; b < kBlocksPerWave; ++b) {
        const uint32_t c1 = min(b1[b][0], b1[b][1]);
        const uint32_t c2 = min(max(b1[b][0], b1[b][1]), min(b2[b][0], b2[b][1]));
        const uint32_t ks[2] = {c1, c2};
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (ks[k] < kPad) {
            const uint32_t ssd = (ks[k] >> 8) + (uint32_t)(tk[b] - kBias);
            top2_insert64(g1[b], g2[b], ((unsigned long long)ssd << 32) | (uint32_t)(q0 + (int)(ks[k] & 255u)));
          }
      }
    }
    // ---- merge the two row halves (lanes l and l^32 own the same template column)
#pragma unroll
    for (int b = 0; b < kBlocksPerWave; ++b) {
      const unsigned long long o1 = (unsigned long long)__shfl_xor((long long)g1[b], 32);
      const unsigned long long o2 = (unsigned long long)__shfl_xor((long long)g2[b], 32);
      unsigned long long m1 = g1[b], m2 = g2[b];
      top2_insert64(m1, m2, o1);
      top2_insert64(m1, m2, o2);
      const int i = tpl_row[b];
      if (h == 0 && i < n_tpl) {
        const size_t o = ((size_t)f * n_tpl + i) * 2;
        const unsigned long long ms[2] = {m1, m2};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (ms[k] == kNoKey64) {
            out_idx[o + k] = -1;
            out_dist[o + k] = FLT_MAX;
          } else {
            out_idx[o + k] = (int32_t)(ms[k] & 0xffffffffull);
            out_dist[o + k] = sqrtf((float)(ms[k] >> 32));
          }
        }
      }
    }
  }
}

// persistent grid: n_tg template groups x G frame strides, G = the resident workgroups
// per template group (workgroups never wait on each other, so a wrong residency count
// costs balance, not progress).  tests/test_gpu_matcher_paths.py sizes its frame counts by
// the bound G <= 8 * CUs / n_tg (2048 threads per CU): a policy past it moves that bound too.
int knn_grid(int n_tg, int n_frames, int wgs_per_cu) {
  const int G = std::max(1, std::min(n_frames, device_cus() * std::max(1, wgs_per_cu) / n_tg));
  return n_tg * G;
}

template <typename K>
int resident_wgs(K kernel, int threads) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, 0) != hipSuccess || n <= 0) n = 1;
  return n;
}

template <int DP, int WAVES>
int launch_knn_row(const uint8_t* des_tpl, int n_tpl, int D, const uint8_t* des_q, const int32_t* q_off,
                   int n_frames, int32_t* out_idx, float* out_dist, hipStream_t s) {
  auto* k = knn2_l2u8_kernel<DP, WAVES>;
  static const int per_cu = resident_wgs(k, KnnShape<WAVES>::kThreads);
  const int n_tg = ceil_div(n_tpl, KnnShape<WAVES>::kTplPerWG);
  hipLaunchKernelGGL(k, dim3(knn_grid(n_tg, n_frames, per_cu)), dim3(KnnShape<WAVES>::kThreads), 0, s, des_tpl,
                     n_tpl, D, des_q, q_off, n_frames, n_tg, out_idx, out_dist);
  return launch_check("knn2_l2u8_kernel");
}

int launch_knn(const uint8_t* des_tpl, int n_tpl, int D, const uint8_t* des_q, const int32_t* q_off,
               int n_frames, int max_nq, int32_t* out_idx, float* out_dist, hipStream_t s) {
  if (n_frames == 0 || n_tpl == 0) return KCMC_OK;
  (void)max_nq;
  const bool wide = n_tpl > 256;  // 512 template rows share each staged chunk
  if (D <= 32)
    return wide ? launch_knn_row<32, 8>(des_tpl, n_tpl, D, des_q, q_off, n_frames, out_idx, out_dist, s)
                : launch_knn_row<32, 4>(des_tpl, n_tpl, D, des_q, q_off, n_frames, out_idx, out_dist, s);
  return wide ? launch_knn_row<64, 8>(des_tpl, n_tpl, D, des_q, q_off, n_frames, out_idx, out_dist, s)
              : launch_knn_row<64, 4>(des_tpl, n_tpl, D, des_q, q_off, n_frames, out_idx, out_dist, s);
}

int check_match_args(const void* des_tpl, int n_tpl, int D, const void* des_q, const void* q_off,
                     int n_frames, int max_nq, const void* o1, const void* o2) {
  return check_knn_args("match", 64, des_tpl, n_tpl, D, des_q, q_off, n_frames, max_nq, o1, o2, [&] {
    return max_nq > (1 << 30) ? fail(KCMC_EUNSUPPORTED, "match: max_nq too large") : KCMC_OK;
  });
}

}  // namespace
}  // namespace kcmc

using namespace kcmc;

extern "C" int kcmc_knn2_l2u8(kcmc_ctx* ctx, const uint8_t* des_tpl, int n_tpl, int D, const uint8_t* des_q,
                              const int32_t* q_off, int n_frames, int max_nq, int32_t* out_idx,
                              float* out_dist, kcmc_stream_t stream) {
  if (!ctx) return fail(KCMC_EINVAL, "kcmc_knn2_l2u8: ctx is NULL");
  KCMC_TRY(check_match_args(des_tpl, n_tpl, D, des_q, q_off, n_frames, max_nq, out_idx, out_dist));
  return launch_knn(des_tpl, n_tpl, D, des_q, q_off, n_frames, max_nq, out_idx, out_dist, (hipStream_t)stream);
}

extern "C" int kcmc_match_frames(kcmc_ctx* ctx, const uint8_t* des_tpl, const double* kp_tpl, int n_tpl, int D,
                                 const uint8_t* des_q, const double* kp_q, const int32_t* q_off, int n_frames,
                                 int max_nq, double ratio, double d_lo, double d_hi, int32_t* out_idx,
                                 float* out_dist, double* out_kp_ordered, uint32_t* out_keep_bits,
                                 int32_t* out_counts, kcmc_stream_t stream) {
  if (!ctx) return fail(KCMC_EINVAL, "kcmc_match_frames: ctx is NULL");
  KCMC_TRY(check_match_args(des_tpl, n_tpl, D, des_q, q_off, n_frames, max_nq, out_idx, out_dist));
  hipStream_t s = (hipStream_t)stream;
  return match_frames_tail(
      "kcmc_match_frames",
      [&] { return launch_knn(des_tpl, n_tpl, D, des_q, q_off, n_frames, max_nq, out_idx, out_dist, s); }, kp_tpl,
      kp_q, q_off, n_frames, n_tpl, max_nq, ratio, d_lo, d_hi, out_idx, out_dist, out_kp_ordered, out_keep_bits,
      out_counts, s);
}

"""A/B edit (tools/ab_build.py KCMC_AB_PATCH): phase timestamps of the rigid scorer, a
timing instrument (never the product library; tools/debug/ransac_stamps.py reads them).

Thread 0 of every frame's workgroup records s_memtime right after the barriers that end
each phase, plus two counters kept in LDS (trials re-counted by phase A2, phase-B
candidates) and whether the frame fell back to exact scoring:
  0 entry   1 staged (points + magnitudes in LDS)   2 phase A (fp32 counts + brackets)
  3 phase A2 (fp64 re-counts)   4 best count known   6 phase B + selection (the barriers
  between them are inside ransac_common.h's select_best; slot 5 is unused)
  7 end (inlier mask + refit)   8 A2 trials   9 phase-B candidates   10 exact path
Stamps go to a __device__ array through ordinary vector stores; kcmc_debug_ransac_stamps
copies them out (hipMemcpyFromSymbol)."""
import os
import sys

p = os.path.join(sys.argv[1], "ransac.hip")
s = open(p).read()


def sub(a, b, count=1):
    global s
    assert s.count(a) == count, (a, s.count(a))
    s = s.replace(a, b)


sub("using namespace ransac_common;\n",
    "using namespace ransac_common;\n\n"
    "constexpr int kStampFrames = 8192, kStamps = 12;\n"
    "__device__ unsigned long long g_stamps[kStampFrames * kStamps];\n"
    "#define STAMP(i) do { if (tid == 0 && f < kStampFrames) g_stamps[(size_t)f * kStamps + (i)] = "
    "__builtin_amdgcn_s_memtime(); } while (0)\n"
    "#define STAMP_V(i, v) do { if (tid == 0 && f < kStampFrames) g_stamps[(size_t)f * kStamps + (i)] = "
    "(unsigned long long)(v); } while (0)\n")
# entry (before the early returns of skipped frames: those record only the entry)
sub("  const int tid = threadIdx.x;\n  const int lane = tid & 63, wave = tid >> 6;\n  int p0, N, hoff;\n",
    "  const int tid = threadIdx.x;\n  const int lane = tid & 63, wave = tid >> 6;\n  STAMP(0);\n"
    "  __shared__ int s_na2, s_nb;\n  if (tid == 0) { s_na2 = 0; s_nb = 0; }\n  int p0, N, hoff;\n")
sub("  stage_points<LARGE>(gather, N, sx, sy, dxs, dys, pk32, red, mg);\n",
    "  stage_points<LARGE>(gather, N, sx, sy, dxs, dys, pk32, red, mg);\n  STAMP(1);\n")
sub("    __syncthreads();  // sc.cnt is reused\n", "    __syncthreads();  // sc.cnt is reused\n    STAMP(2);\n")
sub("          const Model m = fit_of(tc);\n          int c = 0;\n",
    "          const Model m = fit_of(tc);\n          if (lane == 0) atomicAdd(&s_na2, 1);\n          int c = 0;\n")
sub("    __syncthreads();  // the A2 results of the other waves' lanes\n",
    "    __syncthreads();  // the A2 results of the other waves' lanes\n    STAMP(3);\n")
sub("  const bool exact = flag != 0 || mcount <= 0;\n",
    "  const bool exact = flag != 0 || mcount <= 0;\n  STAMP(4);\n  STAMP_V(10, exact ? 1 : 0);\n")
sub("          const Model m = fit_of(tc);\n          const double S = wave_pairwise<LARGE>(\n",
    "          const Model m = fit_of(tc);\n          if (lane == 0) atomicAdd(&s_nb, 1);\n"
    "          const double S = wave_pairwise<LARGE>(\n")
sub("  select_best(best, any_zero, T, tS, tC, sc, s_any_zero, best_t, best_c);\n",
    "  select_best(best, any_zero, T, tS, tC, sc, s_any_zero, best_t, best_c);\n  STAMP(6);\n")
sub("    out_nin[f] = (int32_t)u.n_in;\n    out_best[f] = best_t;\n  }\n",
    "    out_nin[f] = (int32_t)u.n_in;\n    out_best[f] = best_t;\n  }\n  STAMP(7);\n  STAMP_V(8, s_na2);\n"
    "  STAMP_V(9, s_nb);\n")
s += ("\nextern \"C\" int kcmc_debug_ransac_stamps(void* dst, int n_frames) {\n"
      "  const size_t n = (size_t)(n_frames < kcmc::kStampFrames ? n_frames : kcmc::kStampFrames) * kcmc::kStamps;\n"
      "  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(kcmc::g_stamps), n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess"
      " ? 0 : -1;\n}\n")
open(p, "w").write(s)

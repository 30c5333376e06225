"""The outward rounding of the compact RANSAC records (ransac_common.h f32_below / f32_above:
a trial's bracket of S kept as two floats) on the host: a small program compiled from the
header prints both roundings of every probe, and numpy checks each against its definition --
f32_below(d) is the largest float <= d, f32_above(d) the smallest float >= d -- so a bracket
stays a bound after the rounding.  Also the byte encoding of the counts and the LDS formula
(ransac_common.h rigid_small_lds) at the sizes the slot argument names.  No GPU."""
import os
import shutil
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "keypoint-consensus-motion-correction_amd", "csrc")
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "ransac_common.h"
using namespace kcmc::ransac_common;
int main(int argc, char** argv) {
  if (argc == 1) {
    std::printf("%zu %zu %zu %d %d %d %d\n", rigid_small_lds(128, 1000), rigid_small_lds(100, 1000), rigid_small_lds(3, 1000),
                cnt_of8(0), cnt_of8(128), cnt_of8(kNoModel), cnt_of8(kDeferred));
    return 0;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  double d;
  while (f && std::fread(&d, sizeof d, 1, f) == 1) {
    const float lo = f32_below(d), hi = f32_above(d);
    std::fwrite(&lo, sizeof lo, 1, stdout);
    std::fwrite(&hi, sizeof hi, 1, stdout);
  }
  return f ? 0 : 1;
}
"""


def _probes():
    rng = np.random.default_rng(5)
    f = np.array([1.0, 2.0, 1e-30, 1e30, 3.0e-38, 1.17549435e-38, 3.4028235e38, 1e-45, 0.1, 1234.5678], np.float32)
    exact = np.concatenate([f, -f, [0.0]]).astype(np.float64)  # floats: both roundings return them
    near = np.concatenate([np.nextafter(exact, np.inf), np.nextafter(exact, -np.inf)])  # one double ulp off a float
    rand = np.concatenate([10.0 ** rng.uniform(-44, 38, 4000) * rng.choice([-1.0, 1.0], 4000), rng.normal(0, 1, 1000)])
    beyond = np.array([1e39, -1e39, 1e300, -1e300, 1e-50, -1e-50, 5e-324, np.inf, -np.inf])
    return np.concatenate([exact, near, rand, beyond])


def test_outward_rounding_counts_and_lds_formula(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe, probes = tmp_path / "outward.cpp", tmp_path / "outward", tmp_path / "probes.bin"
    src.write_text(PROGRAM)
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", f"-I{CSRC}",
                    f"-I{os.path.join(REPO, 'include')}", str(src), "-o", str(exe)], check=True, timeout=300)
    d = _probes()
    d.tofile(probes)
    out = np.frombuffer(subprocess.run([str(exe), str(probes)], check=True, capture_output=True, timeout=60).stdout,
                        np.float32).reshape(-1, 2)
    assert len(out) == len(d)
    lo, hi = out[:, 0], out[:, 1]
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    assert not np.isnan(out).any()
    assert (lo64 <= d).all() and (hi64 >= d).all()  # outward: [lo, hi] contains d
    # and tight: the next float inward is already on the other side of d
    with np.errstate(over="ignore"):
        up, down = np.nextafter(lo, np.float32(np.inf)), np.nextafter(hi, np.float32(-np.inf))
    assert ((up.astype(np.float64) > d) | np.isposinf(lo)).all()
    assert ((down.astype(np.float64) < d) | np.isneginf(hi)).all()
    with np.errstate(over="ignore"):
        is_f32 = d.astype(np.float32).astype(np.float64) == d
    assert (lo64[is_f32] == d[is_f32]).all() and (hi64[is_f32] == d[is_f32]).all() and is_f32.sum() >= 21
    # a NaN bound stays NaN (the brackets' validity test then sends the frame to the exact path)
    np.array([np.nan]).tofile(probes)
    assert np.isnan(np.frombuffer(subprocess.run([str(exe), str(probes)], check=True, capture_output=True,
                                                 timeout=60).stdout, np.float32)).all()
    # 18,336 B at (128, 1000): with the 224 B of static LDS inside one warp tile's 20,480 B
    v = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert v[:3] == [32 * 128 + 32 * 128 + 10000 + 128 + 16, 32 * 100 + 32 * 100 + 10000 + 100 + 16, 96 + 12000 + 3 + 16]
    assert v[0] + 224 <= 20480
    assert v[3:] == [0, 128, -1, -1]

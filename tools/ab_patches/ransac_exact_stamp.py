"""Debug stamp for tools/ab_build.py (KCMC_AB_PATCH): the rigid / similarity RANSAC kernel
reports a frame that took the exact single-phase loop (`exact` in ransac.hip) as
n_inliers = -1000 - n_inliers, so a `bench.py --dump-outputs` run counts such frames:

    KCMC_AB_PATCH=tools/ab_patches/ransac_exact_stamp.py python tools/ab_build.py exact_stamp
    KCMC_TEST_ONLY_ALT_LIB=1 KCMC_LIB_PATH=ab/exact_stamp.so python bench.py --dump-outputs DIR
    python -c "import numpy as np; print((np.load('DIR/ransac_n_inliers.npy') <= -1000).sum())"
"""
import os
import sys

path = os.path.join(sys.argv[1], "ransac.hip")
src = open(path).read()
old = "out_nin[f] = (int32_t)u.n_in;"
assert src.count(old) == 1, "ransac.hip: the n_inliers store moved"
open(path, "w").write(src.replace(old, "out_nin[f] = exact ? -1000 - (int32_t)u.n_in : (int32_t)u.n_in;"))

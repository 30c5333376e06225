"""The N <= 128 rigid and similarity RANSAC kernels with the compact per-trial records (a
bracket of S as two floats rounded outward, the two counts as bytes; ransac.hip) against the C
oracle: winning trial, inlier count and mask bit for bit, parameters at the rigid fuzz's
tolerance (rtol 1e-10, atol 1e-10 max(1, |template|max)).  Every case runs both models
through the package's entries (stages.ransac_rigid / ransac_similarity).

Wider brackets may only add phase-B candidates, never change an output, so the cases are the
ones where a bracket decides something: every point count at which the one-wave staging
changes (and a launch of each count alone, whose LDS is laid out for that count), data
nearly free of noise and exact data (brackets at or below the validity range), a NaN point
(skimage's comparisons with every S NaN), coordinates of 3e5 px with
residuals within ulps of the threshold (trials deferred to the fp64 phase A), and a frame
where most trials tie at the top count with S closer together than one float ulp."""
import numpy as np
import pytest
import torch

import oracle
from kcmc_amd import stages, synthetic

pytestmark = pytest.mark.gpu
MODELS = {"rigid": (stages.ransac_rigid, oracle.ransac_rigid),
          "similarity": (stages.ransac_similarity, oracle.ransac_similarity)}
SLOT_NS = [2, 3, 63, 64, 65, 100, 127, 128]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off


def _run(dev, model, tpls, qs, **kw):
    off = _csr(qs)
    r = MODELS[model][0](_t(np.concatenate(qs).reshape(-1, 2), dev), _t(np.concatenate(tpls).reshape(-1, 2), dev),
                         _t(off, dev), off, **kw)
    return (off, r.params.cpu().numpy(), r.inliers.cpu().numpy().astype(bool), r.n_inliers.cpu().numpy(),
            r.best_trial.cpu().numpy())


def _check(model, tpls, qs, got, trials=1000, thresh=2.0, ctx=()):
    """Every frame against the oracle; returns the number of frames with a fitted model."""
    off, params, inl, nin, best = got
    n_fit = 0
    for f, (tpl, q) in enumerate(zip(tpls, qs)):
        m = inl[off[f]:off[f + 1]]
        if len(q) < 3:  # below n_skip: NaN, no inliers, no trial
            assert np.isnan(params[f]).all() and nin[f] == 0 and best[f] == -1 and not m.any(), (ctx, f)
            continue
        p, i_ref, bt, ni = MODELS[model][1](q, tpl, trials, thresh)
        assert best[f] == bt and nin[f] == ni, (ctx, f, len(q), best[f], bt, nin[f], ni)
        assert np.array_equal(m, i_ref), (ctx, f)
        sc = max(1.0, float(np.nanmax(np.abs(tpl))))
        np.testing.assert_allclose(params[f], p, rtol=1e-10, atol=1e-10 * sc, equal_nan=True, err_msg=str((ctx, f)))
        n_fit += not np.isnan(p).any()
    return n_fit


def _noisy_frame(rng, N, scale=None):
    """test_gpu_kernels.test_ransac_bit_exact_selection_vs_oracle's frames (float32-valued
    points, noise 0.1 .. 1.5 px, up to 60 % outliers), with a scale in [0.5, 2] if asked."""
    tpl = rng.uniform(0, 1000, (N, 2))
    A = synthetic.rigid(rng.normal(0, 0.02), rng.normal(0, 5), rng.normal(0, 5))
    q = (tpl - A[:, 2]) @ A[:, :2] / (scale or 1.0) + rng.normal(0, rng.uniform(0.1, 1.5), (N, 2))
    out = rng.random(N) < rng.uniform(0, 0.6)
    q[out] = rng.uniform(0, 1000, (int(out.sum()), 2))
    return tpl.astype(np.float32).astype(np.float64), q.astype(np.float32).astype(np.float64)


def _clean_frame(rng, N, noise, lo=100.0, hi=900.0):
    tpl = rng.uniform(lo, hi, (N, 2))
    A = synthetic.rigid(rng.normal(0, 0.02), rng.normal(0, 5), rng.normal(0, 5))
    q = (tpl - A[:, 2]) @ A[:, :2]
    return tpl, q + rng.normal(0, noise, (N, 2)) if noise else q


@pytest.mark.parametrize("model", sorted(MODELS))
def test_point_counts_each_alone_and_together(dev, model):
    """N = 2 (below n_skip), 3, the one- and two-points-per-lane staging (63, 64, 65), the
    flagship's 100 and the largest small frames (127, 128), 1000 trials: every count in a
    launch of its own (max_n = N sizes the LDS) and all in one launch."""
    rng = np.random.default_rng(41)
    frames = [_noisy_frame(rng, N, rng.uniform(0.5, 2.0) if model == "similarity" else None) for N in SLOT_NS]
    tpls, qs = [t for t, _ in frames], [q for _, q in frames]
    assert _check(model, tpls, qs, _run(dev, model, tpls, qs), ctx=(model, "together")) == len(SLOT_NS) - 1
    for tpl, q in frames:
        _check(model, [tpl], [q], _run(dev, model, [tpl], [q]), ctx=(model, "alone", len(q)))


@pytest.mark.parametrize("model", sorted(MODELS))
def test_large_path_untouched_at_129_points_37_trials(dev, model):
    rng = np.random.default_rng(42)
    frames = [_noisy_frame(rng, N) for N in (129, 128, 100)]
    tpls, qs = [t for t, _ in frames], [q for _, q in frames]
    assert _check(model, tpls, qs, _run(dev, model, tpls, qs, trials=37), trials=37, ctx=(model, 129)) == 3


@pytest.mark.parametrize("model", sorted(MODELS))
def test_large_path_point_counts_each_alone(dev, model):
    """129, 136 and 257 points at 1000 trials, every count in a launch of its own: max_n = N
    sizes the large kernel's LDS (ransac_common.h RigidLargeLds) for exactly that frame."""
    rng = np.random.default_rng(47)
    for N in (129, 136, 257):
        tpl, q = _noisy_frame(rng, N, rng.uniform(0.5, 2.0) if model == "similarity" else None)
        assert _check(model, [tpl], [q], _run(dev, model, [tpl], [q]), ctx=(model, "large alone", N)) == 1


@pytest.mark.parametrize("model", sorted(MODELS))
def test_skipped_frame_and_nan_point(dev, model):
    """A frame below n_skip between two scored ones, and a frame with one NaN coordinate (its
    bounding boxes are infinite, every trial's S is NaN: the frame takes the exact path, where
    skimage's comparisons pick the first trial that reaches the best count)."""
    rng = np.random.default_rng(43)
    a, b, c = _noisy_frame(rng, 70), _noisy_frame(rng, 2), _noisy_frame(rng, 90)
    c[1][17, 0] = np.nan
    tpls, qs = [a[0], b[0], c[0]], [a[1], b[1], c[1]]
    got = _run(dev, model, tpls, qs)
    assert _check(model, tpls, qs, got, ctx=(model, "skip, nan")) == 2
    off, _, inl, nin, _ = got
    assert nin[2] > 0 and not inl[off[2] + 17]


@pytest.mark.parametrize("model", sorted(MODELS))
def test_near_noise_free_and_exact_data(dev, model):
    """Noise of 1e-6 px on coordinates in the hundreds: S is small next to the fp32 error
    term, so the brackets' low bounds reach the validity limit.  And exact data (integer
    points, integer shift: every S == 0), where skimage's early exit picks the trial."""
    rng = np.random.default_rng(44)
    frames = [_clean_frame(rng, N, 1e-6) for N in (100, 128, 40)]
    tpl = np.array([[x, y] for x in range(0, 50, 7) for y in range(0, 40, 9)], np.float64)
    frames.append((tpl, tpl - np.array([4.0, -2.0])))
    tpls, qs = [t for t, _ in frames], [q for _, q in frames]
    got = _run(dev, model, tpls, qs)
    assert _check(model, tpls, qs, got, ctx=(model, "clean")) == 4
    assert got[4][3] == 0 and got[3][3] == len(tpl)  # S == 0 at trial 0: skimage stops there
    assert (got[3][:3] == [100, 128, 40]).all()


@pytest.mark.parametrize("model", sorted(MODELS))
def test_scale_3e5_residuals_within_ulps_of_the_threshold(dev, model):
    """Coordinates up to 3e5 px (the fp32 band is too wide: trials run the fp64 phase A) with
    points whose residual under the true map is the 2 px threshold times 1 + j 2^-50, j in
    -3 .. 3, or within 1e-12 .. 1e-2 of it."""
    rng = np.random.default_rng(45)
    tpls, qs = [], []
    for f in range(4):
        n_exact, n_band, n_out = 30 + 20 * f, 28, 10
        tpl = rng.uniform(0.2, 1.0, (n_exact + n_band + n_out, 2)) * 3e5
        a = rng.normal(0, 0.02)
        A = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        t = rng.normal(0, 5, 2)
        q = (tpl - t) @ np.linalg.inv(A).T  # A q + t = tpl
        rad = np.concatenate([2.0 * (1 + (np.arange(14) % 7 - 3) * 2.0 ** -50),
                              2.0 + rng.choice([-1e-2, -1e-5, -1e-9, -1e-12, 1e-12, 1e-9, 1e-5, 1e-2], 14)])
        ang = rng.uniform(0, 2 * np.pi, n_band)
        tpl[n_exact:n_exact + n_band] += rad[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        tpl[n_exact + n_band:] += rng.uniform(5, 50, (n_out, 2))
        tpls.append(tpl)
        qs.append(q)
    assert max(len(q) for q in qs) == 128
    assert _check(model, tpls, qs, _run(dev, model, tpls, qs), ctx=(model, 3e5)) == 4


def _tied_frame(rng, N, n_off):
    """N - n_off points that map onto the template up to fp64 rounding and n_off points 0.5 ..
    1.5 px away (inliers at 2 px).  Every trial whose pair lies among the first kind -- most
    trials -- fits the true map up to ~1e-13 and counts all N points, and their S = the sum of
    the squared offsets differ by ~1e-12 relative: far less than a float ulp (6e-8)."""
    tpl, q = _clean_frame(rng, N, 0.0)
    k = rng.permutation(N)[:n_off]
    ang = rng.uniform(0, 2 * np.pi, n_off)
    tpl[k] += rng.uniform(0.5, 1.5, n_off)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    return tpl, q


@pytest.mark.parametrize("model", sorted(MODELS))
def test_many_trials_tied_within_a_float_ulp(dev, model):
    rng = np.random.default_rng(46)
    frames = [_tied_frame(rng, 100, 12), _tied_frame(rng, 128, 10), _tied_frame(rng, 64, 6)]
    tpls, qs = [t for t, _ in frames], [q for _, q in frames]
    # the frames are what the docstring says: under the oracle's own winner every point is an
    # inlier, and most pairs of the hypothesis table lie among the points on the map
    for tpl, q in frames:
        N = len(q)
        _, i_ref, _, ni = MODELS[model][1](q, tpl, 1000, 2.0)
        assert ni == N and i_ref.all()
        on_map = np.ones(N, bool)
        p, _, _, _ = oracle.ransac_rigid(q, tpl)
        on_map[np.hypot(*(q @ p[:, :2].T + p[:, 2] - tpl).T) > 0.1] = False
        pairs = oracle.hypothesis_table(N, 1000)
        assert on_map[pairs].all(1).mean() > 0.6
    assert _check(model, tpls, qs, _run(dev, model, tpls, qs), ctx=(model, "ties")) == 3

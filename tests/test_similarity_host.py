"""The similarity model (K2s) on the host: the operation-for-operation numpy restatement
of scikit-image 0.18.3's ransac(..., SimilarityTransform, min_samples=2, ...), a plain
closed-form version of the same loop (what the kernel computes), their agreement on every
input set the GPU tests use, and the host pieces of the model (summary, gap filling,
binding tables, header).

scikit-image is not installed where these tests run, so no golden from skimage itself
exists for this model: the restatement below is the yardstick.  tests/test_gpu_similarity.py
imports the input sets and the (cached) restatement results from here."""
import functools
import os
import re

import numpy as np
import pytest

import oracle
from kcmc_amd import _lib, affines as _aff, pipeline, synthetic

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kcmc.h")
RTOL, ATOL = 1e-8, 1e-9  # the parameter bound of tests/test_gpu_models.py (closed form vs SVD)


# ------------------------------------------------------------------ the restatement
def umeyama_similarity_numpy(src, dst):
    """skimage _umeyama(src, dst, estimate_scale=True), _geometric.py:72-144."""
    num, dim = src.shape
    src_mean = src.mean(axis=0)
    dst_mean = dst.mean(axis=0)
    src_demean = src - src_mean
    dst_demean = dst - dst_mean
    A = dst_demean.T @ src_demean / num
    d = np.ones((dim,), dtype=np.double)
    if np.linalg.det(A) < 0:
        d[dim - 1] = -1
    T = np.eye(dim + 1, dtype=np.double)
    U, S, V = np.linalg.svd(A)
    rank = np.linalg.matrix_rank(A)
    if rank == 0:
        return np.nan * T
    elif rank == dim - 1:
        if np.linalg.det(U) * np.linalg.det(V) > 0:
            T[:dim, :dim] = U @ V
        else:
            s = d[dim - 1]
            d[dim - 1] = -1
            T[:dim, :dim] = U @ np.diag(d) @ V
            d[dim - 1] = s
    else:
        T[:dim, :dim] = U @ np.diag(d) @ V
    scale = 1.0 / src_demean.var(axis=0).sum() * (S @ d)
    T[:dim, dim] = dst_mean - scale * (T[:dim, :dim] @ src_mean.T)
    T[:dim, :dim] *= scale
    return T


def _apply(T, coords):
    """ProjectiveTransform._apply_mat (_geometric.py:548-562)."""
    x, y = np.transpose(coords)
    s = np.vstack((x, y, np.ones_like(x)))
    d = s.T @ T.T
    d[d[:, 2] == 0, 2] = np.finfo(float).eps
    d[:, :2] /= d[:, 2:3]
    return d[:, :2]


def _ransac_loop(src, dst, estimate, residuals, trials, thresh, seed):
    """skimage 0.18.3 ransac (fit.py:784-881) around a model's estimate / residuals.
    Returns (params [2, 3] (NaN: none), inliers bool [N], winning sample pair as a frozenset
    (None: no trial was ever selected), n_inliers)."""
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    n = len(src)
    rs = np.random.RandomState(seed)
    best_n, best_S, best_inl, best_pair = 0, np.inf, None, None
    spl = rs.choice(n, 2, replace=False)
    with np.errstate(all="ignore"):
        for _ in range(trials):
            cur = spl
            spl = rs.choice(n, 2, replace=False)
            T = estimate(src[cur], dst[cur])
            r = residuals(T, src, dst)
            inl = r < thresh
            S = np.sum(r ** 2)
            ni = np.sum(inl)
            if ni > best_n or (ni == best_n and S < best_S):
                best_n, best_S, best_inl, best_pair = ni, S, inl, frozenset(int(k) for k in cur)
                if best_S <= 0:
                    break
        if best_inl is not None and any(best_inl):
            T = estimate(src[best_inl], dst[best_inl])
            return T[:2].copy(), best_inl, best_pair, int(best_inl.sum())
    return np.full((2, 3), np.nan), np.zeros(n, bool), best_pair, 0


def ransac_similarity_skimage(src, dst, trials=1000, thresh=2.0, seed=42):
    """The restatement: per-trial SVD like skimage.  src = frame keypoints, dst = template."""
    return _ransac_loop(src, dst, umeyama_similarity_numpy,
                        lambda T, s, d: np.abs(np.sqrt(np.sum((_apply(T, s) - d) ** 2, axis=1))), trials, thresh, seed)


# ------------------------------------------------------------------ the closed form
def fit_similarity_closed(src, dst):
    """_umeyama(estimate_scale=True) without the SVD: with a = a00 + a11, b = a10 - a01 of the
    covariance sums and v = sum |src_d|^2, scale * R = [[a, -b], [b, a]] / v."""
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    u, w = src - ms, dst - md
    a = np.sum(w[:, 0] * u[:, 0]) + np.sum(w[:, 1] * u[:, 1])
    b = np.sum(w[:, 1] * u[:, 0]) - np.sum(w[:, 0] * u[:, 1])
    T = np.eye(3)
    if a == 0.0 and b == 0.0:
        return np.nan * T
    v = np.sum(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1])
    c, s = a / v, b / v
    T[0] = c, -s, md[0] - (c * ms[0] - s * ms[1])
    T[1] = s, c, md[1] - (s * ms[0] + c * ms[1])
    return T


def _residuals_closed(T, src, dst):
    ex = (src[:, 0] * T[0, 0] + src[:, 1] * T[0, 1] + T[0, 2]) - dst[:, 0]
    ey = (src[:, 0] * T[1, 0] + src[:, 1] * T[1, 1] + T[1, 2]) - dst[:, 1]
    return np.sqrt(ex * ex + ey * ey)


def ransac_similarity_closed(src, dst, trials=1000, thresh=2.0, seed=42):
    return _ransac_loop(src, dst, fit_similarity_closed, _residuals_closed, trials, thresh, seed)


# ------------------------------------------------------------------ the input sets
def _sim_map(rng, scale_lo=0.9, scale_hi=1.1):
    s = rng.uniform(scale_lo, scale_hi)
    A = synthetic.rigid(np.deg2rad(rng.normal(0, 2.0)), rng.normal(0, 5), rng.normal(0, 5))
    A[:, :2] *= s
    return A


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


SELECTION_NS = [2, 3, 4, 8, 9, 63, 64, 65, 127, 128, 129, 136, 257, 300]


def selection_frames(seed=91):
    """float32-rounded coordinates in [0, 1000), scale in [0.9, 1.1], 0-60 % outliers; every
    N at which the kernel changes path (skip, one wave / two halves, one leaf / split plan)."""
    rng = np.random.default_rng(seed)
    tpls, qs = [], []
    for N in SELECTION_NS:
        tpl = rng.uniform(0, 1000, (N, 2))
        A = _sim_map(rng)
        q = synthetic.apply_map(np.linalg.inv(np.vstack([A, [0, 0, 1.0]])), tpl)
        q = q + rng.normal(0, rng.uniform(0.1, 1.5), (N, 2))
        out = rng.random(N) < rng.uniform(0, 0.6)
        q[out] = rng.uniform(0, 1000, (int(out.sum()), 2))
        tpls.append(_f32(np.clip(tpl, 0, 999.99)))
        qs.append(_f32(np.clip(q, 0, 999.99)))
    return tpls, qs


def exact_frames():
    """dst = 2 src + t on small integers (every hypothesis has S == 0: skimage's early exit and
    the kernel's replay) and one frame with all points coincident (no model)."""
    rng = np.random.default_rng(92)
    tpls, qs, maps = [], [], []
    for N, t in [(5, (3.0, -1.0)), (40, (-7.0, 2.0)), (130, (0.0, 11.0))]:
        q = rng.permutation(64 * 64)[:N]
        q = np.stack([q % 64, q // 64], 1).astype(np.float64)
        tpls.append(2.0 * q + np.array(t))
        qs.append(q)
        maps.append(np.array([[2.0, 0.0, t[0]], [0.0, 2.0, t[1]]]))
    qs.append(np.full((9, 2), 5.0))
    tpls.append(np.full((9, 2), 7.0))
    maps.append(np.full((2, 3), np.nan))
    return tpls, qs, maps


def rigid_frames():
    """Rigid data (scale exactly 1) with noise and outliers, for similarity vs rigid."""
    rng = np.random.default_rng(93)
    tpls, qs = [], []
    for N in [30, 90, 200]:
        tpl = rng.uniform(0, 1000, (N, 2))
        A = _sim_map(rng, 1.0, 1.0)
        q = (tpl - A[:, 2]) @ A[:, :2] + rng.normal(0, 0.3, (N, 2))
        out = rng.random(N) < 0.2
        q[out] = rng.uniform(0, 1000, (int(out.sum()), 2))
        tpls.append(_f32(tpl))
        qs.append(_f32(q))
    return tpls, qs


THRESHOLDS = [1e-120, 5e-5]


def threshold_frames():
    """Frames for the thresholds 1e-120 (tq out of range: exact scoring only) and 5e-5 (the
    fp32 phase A with points inside its undecided band around the threshold).

    At 1e-120 a point is an inlier only if its residual is exactly 0, so SVD and closed form
    can agree only where neither ever computes an exact 0.  The frames are therefore template
    points in [0, 1)^2 seen by a frame whose points lie near (1000, 1000): the map's products
    and translation are ~1000 and cancel to ~1, so a mapped point carries rounding errors of
    ulp(1000) = 1.1e-13 against template coordinates given to 1.1e-16, and matches one exactly
    with probability ~1e-3 per coordinate (~2e-3 over the 2000 sample points of a frame's
    trials; on ordinary frames it is ~0.1 per sample point and some trial always has one).
    The same geometry keeps the centred fp32 coordinates small, so at 5e-5 the fp32 bound is
    well below the threshold and the noise levels around 5e-5 put points inside the band."""
    rng = np.random.default_rng(94)
    tpls, qs = [], []
    for N, noise in [(40, 1e-9), (90, 5e-5), (90, 1e-2), (150, 3e-5), (12, 5e-5)]:
        tpl = rng.uniform(0, 1, (N, 2))
        A = _sim_map(rng, 0.98, 1.02)
        A[:, 2] = 0.0
        q = synthetic.apply_map(np.linalg.inv(np.vstack([A, [0, 0, 1.0]])), tpl) + 1000.0
        q = q + rng.normal(0, noise, (N, 2))
        tpls.append(tpl)
        qs.append(q)
    return tpls, qs


PIPE = dict(F=24, n_tpl=64, D=32, size=(64, 96), n_kp_global=40, blank=(9, 10))


def pipeline_keypoints():
    """synthetic.make_keypoints(model="similarity") with two frames' keypoints blanked: all
    their descriptors are one row, so no match passes the ratio test (d1 == d2) and the
    frames get no model."""
    ks = synthetic.make_keypoints(PIPE["F"], PIPE["n_tpl"], PIPE["D"], PIPE["size"], seed=95, model="similarity")
    rng = np.random.default_rng(96)
    for f in PIPE["blank"]:
        ks.des_q[ks.q_off[f]:ks.q_off[f + 1]] = rng.integers(0, 256, (1, PIPE["D"]), dtype=np.uint8)
    return ks


def pipeline_frames():
    """The pipeline set's per-frame consensus point lists, made with the CPU oracle (match,
    filters, consensus, lookup: what the device stages reproduce bit for bit)."""
    ks = pipeline_keypoints()
    sets, kqs = [], []
    for f in range(PIPE["F"]):
        a, b = ks.q_off[f], ks.q_off[f + 1]
        idx, dist = oracle.knn2_l2u8(ks.des_tpl, ks.des_q[a:b])
        s, kq, _ = oracle.filter_matches(idx, dist, ks.kp_tpl, ks.kp_q[a:b])
        sets.append(set(s))
        kqs.append(kq)
    cset, _, _ = oracle.consensus(sets, PIPE["n_kp_global"])
    lists = oracle.lookup(cset, sets)
    assert all(len(lists[f]) == 0 for f in PIPE["blank"])
    return [ks.kp_tpl[L] for L in lists], [kqs[f][L] for f, L in enumerate(lists)]


@functools.lru_cache(maxsize=None)
def input_sets():
    """name -> (template points per frame, frame points per frame, trials, threshold)."""
    sets = {"selection": selection_frames() + (1000, 2.0), "selection200": selection_frames() + (200, 2.0),
            "exact": exact_frames()[:2] + (1000, 2.0), "rigid": rigid_frames() + (1000, 2.0),
            "pipeline": pipeline_frames() + (1000, 2.0)}
    for th in THRESHOLDS:
        sets[f"thresh{th:g}"] = threshold_frames() + (1000, th)
    return sets


SET_NAMES = ["selection", "selection200", "exact", "rigid", "pipeline"] + [f"thresh{th:g}" for th in THRESHOLDS]


FUZZ_SEEDS = range(6)
FUZZ_FRAMES = 24
FUZZ_THRESHOLDS = [2.0, 0.5, 5.0, 1e-3]


def fuzz_frames(rng, n_frames, extra_n=(), extra_noise=()):
    """Random (template, frame) point sets: 3 to 400 points, coordinate scales 1e-2 to 1e4,
    any rotation, scales 0.25 to 4, noise from 1e-9 to 1.5 px (scaled with large coordinates),
    up to half outliers, mirrored frames (refit with det < 0) and duplicated halves.  No frame
    is noise-free by default: with S == 0 the SVD and the closed form legitimately stop at
    different trials.  extra_n / extra_noise widen the choices of N and of the noise for the
    comparison of two closed forms (tests/test_gpu_similarity.py)."""
    for _ in range(n_frames):
        N = int(rng.choice([3, 4, 5, int(rng.integers(6, 60)), int(rng.integers(60, 400))] + list(extra_n)))
        scale = 10.0 ** rng.uniform(-2, 4)
        tpl = rng.uniform(0, scale, (N, 2))
        a = rng.uniform(-np.pi, np.pi) if rng.random() < 0.5 else rng.normal(0, 0.05)
        k = float(rng.choice([0.25, 0.5, 0.8, 1.0, 1.25, 2.0, 4.0])) * rng.uniform(0.95, 1.05)
        A = k * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        q = tpl @ A.T + rng.normal(0, scale * 0.01, 2)
        noise = rng.choice([1e-9, 0.3, 1.5] + list(extra_noise)) * (scale / 1000.0 if scale > 1000 else 1.0)
        q = q + rng.normal(0, noise, (N, 2))
        out = rng.random(N) < rng.uniform(0, 0.5)
        q[out] = rng.uniform(0, scale, (int(out.sum()), 2))
        if rng.random() < 0.15:
            q[:, 1] = -q[:, 1]                      # mirrored frame
        if N > 10 and rng.random() < 0.3:
            q[N // 2:], tpl[N // 2:] = q[: N - N // 2], tpl[: N - N // 2]
        yield tpl, q


def fuzz_set(s, **widen):
    """Seed 5000 + s: the threshold (drawn before the frames) and the 24 frames."""
    rng = np.random.default_rng(5000 + s)
    thresh = float(rng.choice(FUZZ_THRESHOLDS))
    tpls, qs = zip(*fuzz_frames(rng, FUZZ_FRAMES, **widen))
    return list(tpls), list(qs), thresh


DEGENERATE_KINDS = ["frame_third_identical", "template_third_identical", "quarter_turn_scale3", "mirrored_x"]


def degenerate_frames():
    """(kind, N, template points, frame points) for N = 30 and 140: both sides share a
    0.03 rad, scale 1.07 map with 0.4 px noise, then a third of the frame points coincide,
    a third of the template points coincide, the map is a rotation by pi/2 + 0.01 with
    scale 3, or the frame's x is mirrored (the refit's covariance has det < 0)."""
    rng = np.random.default_rng(97)
    out = []
    for N in (30, 140):
        for kind in DEGENERATE_KINDS:
            a, k = (np.pi / 2 + 0.01, 3.0) if kind == "quarter_turn_scale3" else (0.03, 1.07)
            A = k * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            q = rng.uniform(0, 300, (N, 2))
            tpl = q @ A.T + rng.normal(0, 5, 2) + rng.normal(0, 0.4, (N, 2))
            if kind == "frame_third_identical":
                q[: N // 3] = q[0]
            elif kind == "template_third_identical":
                tpl[: N // 3] = tpl[0]
            elif kind == "mirrored_x":
                q[:, 0] = -q[:, 0]
            out.append((kind, N, tpl, q))
    return out


def large_frame(N=1024):
    """One frame well above the other sets' 300 points (numpy's split plan three levels deep)."""
    rng = np.random.default_rng(98)
    tpl = rng.uniform(0, 1000, (N, 2))
    A = _sim_map(rng, 0.7, 1.4)
    q = synthetic.apply_map(np.linalg.inv(np.vstack([A, [0, 0, 1.0]])), tpl) + rng.normal(0, 0.7, (N, 2))
    out = rng.random(N) < 0.3
    q[out] = rng.uniform(0, 1000, (int(out.sum()), 2))
    return tpl, q


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's result for every frame of an input set (computed once per session;
    frames with fewer than 3 points are skipped by the caller, VA:306-307: NaN, no inliers)."""
    tpls, qs, trials, thresh = input_sets()[name]
    out = []
    for tpl, q in zip(tpls, qs):
        if len(q) < 3:
            out.append((np.full((2, 3), np.nan), np.zeros(len(q), bool), None, 0))
        else:
            out.append(ransac_similarity_skimage(q, tpl, trials, thresh))
    return out


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", SET_NAMES)
def test_closed_form_agrees_with_the_restatement(name):
    """Every frame of every input set the GPU tests use: equal inlier masks, equal winning
    sample (as a set of two indices: another draw of the same pair is the same hypothesis, and
    the SVD's rounding decides between them) and parameters within the closed-form-vs-SVD
    bound.  On the exact-data set every hypothesis fits with S == 0 in exact arithmetic and
    the winner is whichever trial's rounding says so (the closed form stops at the first
    S == 0, the SVD's S is a few ulps above): the pair is then compared on neither side."""
    tpls, qs, trials, thresh = input_sets()[name]
    ref = reference(name)
    assert len(ref) == len(qs)
    n_fit = 0
    for f, (tpl, q) in enumerate(zip(tpls, qs)):
        p_ref, inl_ref, pair_ref, ni_ref = ref[f]
        if len(q) < 3:
            continue
        p, inl, pair, ni = ransac_similarity_closed(q, tpl, trials, thresh)
        assert np.array_equal(inl, inl_ref), (name, f)
        assert ni == ni_ref, (name, f)
        if name != "exact":
            assert pair == pair_ref, (name, f)
        np.testing.assert_allclose(p, p_ref, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=f"{name} {f}")
        n_fit += not np.isnan(p_ref).any()
    if not name.startswith("thresh1e-120"):
        assert n_fit >= len(qs) - 3, name  # the sets exercise fits, not only failures


# ------------------------------------------------------ the C oracle against the restatement
def _sample_rows(tpl, q, pair):
    """A sample as the set of its (frame point, template point) coordinate rows: duplicated
    rows make different index pairs the same hypothesis."""
    return None if pair is None else frozenset((*map(float, q[k]), *map(float, tpl[k])) for k in pair)


def check_oracle_vs_restatement(tpl, q, trials, thresh, ref=None, compare_pair=True, ctx=None):
    """oracle.ransac_similarity (C, closed form) against ransac_similarity_skimage on one
    frame: inlier mask and count exact, the winning sample as coordinate rows, parameters at
    RTOL with atol = ATOL max(1, |tpl|max).  Returns the largest parameter deviation divided
    by max(1, |tpl|max) (0 when there is no model)."""
    p_ref, inl_ref, pair_ref, ni_ref = ref if ref is not None else ransac_similarity_skimage(q, tpl, trials, thresh)
    p, inl, bt, ni = oracle.ransac_similarity(q, tpl, trials, thresh)
    assert np.array_equal(inl, inl_ref), ctx
    assert ni == ni_ref, ctx
    if compare_pair:
        pair = None if bt < 0 else [int(k) for k in oracle.hypothesis_table(len(q), trials)[bt]]
        assert _sample_rows(tpl, q, pair) == _sample_rows(tpl, q, pair_ref), (ctx, bt)
    sc = max(1.0, float(np.abs(tpl).max()))
    np.testing.assert_allclose(p, p_ref, rtol=RTOL, atol=ATOL * sc, equal_nan=True, err_msg=str(ctx))
    return 0.0 if np.isnan(p_ref).any() else float(np.abs(p - p_ref).max()) / sc


@pytest.mark.parametrize("name", SET_NAMES)
def test_oracle_agrees_with_the_restatement_on_the_input_sets(name):
    """Every frame of every existing input set, under the rule of
    test_closed_form_agrees_with_the_restatement (no pair comparison on "exact").  A frame of
    two points, which every caller skips, is compared as well: both loops accept it (the
    pipeline set's two blanked frames have no point at all, so no sample can be drawn)."""
    tpls, qs, trials, thresh = input_sets()[name]
    worst = 0.0
    assert sum(len(q) < 2 for q in qs) == (len(PIPE["blank"]) if name == "pipeline" else 0)
    for f, (tpl, q, ref) in enumerate(zip(tpls, qs, reference(name))):
        if len(q) < 2:
            continue
        worst = max(worst,check_oracle_vs_restatement(tpl, q, trials, thresh, ref=ref if len(q) >= 3 else None,
                                                       compare_pair=name != "exact", ctx=(name, f)))
    print(f"{name}: {len(qs)} frames, max |dp| / scale {worst:.3g}")


@pytest.mark.parametrize("s", FUZZ_SEEDS)
def test_oracle_agrees_with_the_restatement_on_the_fuzz(s):
    tpls, qs, thresh = fuzz_set(s)
    assert len(qs) == FUZZ_FRAMES
    worst = 0.0
    for f, (tpl, q) in enumerate(zip(tpls, qs)):
        worst = max(worst, check_oracle_vs_restatement(tpl, q, 1000, thresh, ctx=(s, f, len(q), thresh)))
    print(f"fuzz seed {5000 + s} thresh {thresh:g}: max |dp| / scale {worst:.3g}")


def test_oracle_agrees_with_the_restatement_on_degenerate_and_large_frames():
    frames = degenerate_frames()
    assert len(frames) == 8
    worst = 0.0
    for kind, N, tpl, q in frames:
        worst = max(worst, check_oracle_vs_restatement(tpl, q, 1000, 2.0, ctx=(kind, N)))
        p, inl, _, ni = oracle.ransac_similarity(q, tpl)
        assert not np.isnan(p).any(), (kind, N)
        if kind == "mirrored_x":  # no similarity maps a mirrored frame onto the template
            assert 2 <= ni < N // 2, (kind, N, ni)
        else:
            assert ni >= N // 2, (kind, N, ni)
    tpl, q = large_frame()
    assert len(q) == 1024
    worst = max(worst, check_oracle_vs_restatement(tpl, q, 1000, 2.0, ctx="N1024"))
    print(f"degenerate + N1024: max |dp| / scale {worst:.3g}")


def test_oracle_entry_has_the_rigid_signature_and_no_model_cases():
    L = oracle.lib()
    assert L.kcmc_oracle_ransac_similarity.argtypes == L.kcmc_oracle_ransac_rigid.argtypes
    # all frame points coincident: a == b == 0 in every trial, so no model (rank(A) == 0 in skimage)
    p, inl, bt, ni = oracle.ransac_similarity(np.full((9, 2), 5.0), np.arange(18.0).reshape(9, 2))
    assert np.isnan(p).all() and not inl.any() and bt == -1 and ni == 0
    # dst = 2 R src + t exactly representable: the first trial wins with S == 0
    q = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 8.0], [4.0, 8.0], [2.0, 2.0]])
    p, inl, bt, ni = oracle.ransac_similarity(q, 2.0 * q[:, ::-1] * [-1.0, 1.0] + [3.0, -1.0])
    assert inl.all() and bt == 0 and ni == 5
    assert np.array_equal(p, [[0.0, -2.0, 3.0], [2.0, 0.0, -1.0]])


def test_exact_set_is_exact_and_coincident_points_have_no_model():
    tpls, qs, maps = exact_frames()
    for tpl, q, M, (p, inl, _, ni) in zip(tpls, qs, maps, reference("exact")):
        if np.isnan(M).any():
            assert np.isnan(p).all() and ni == 0 and not inl.any()
        else:
            assert inl.all() and ni == len(q)
            np.testing.assert_allclose(p, M, rtol=0, atol=1e-9)


def test_swapping_the_sample_points_gives_the_same_model():
    rng = np.random.default_rng(5)
    for _ in range(50):
        s, d = rng.uniform(0, 1000, (2, 2)), rng.uniform(0, 1000, (2, 2))
        assert np.array_equal(fit_similarity_closed(s, d), fit_similarity_closed(s[::-1], d[::-1]))


def test_similarity_transforms_summary():
    th, sc = np.array([0.3, -0.2, 0.0, 3.0]), np.array([1.0, 0.9, 1.1, 2.0])
    A = np.stack([s * synthetic.rigid(t, 0.0, 0.0) for t, s in zip(th, sc)])
    A[:, :, 2] = [[4.0 + k, -2.0 * k] for k in range(4)]
    out = _aff.similarity_transforms(A)
    assert out.shape == (4, 4)
    np.testing.assert_allclose(out[:, 0], [4, 5, 6, 7])
    np.testing.assert_allclose(out[:, 1], [0, -2, -4, -6])
    np.testing.assert_allclose(out[:, 2], th, atol=1e-15)
    np.testing.assert_allclose(out[:, 3], sc, rtol=1e-15)
    assert _aff.euclidean_transforms(A).shape == (4, 3)  # the reference's summary is untouched
    assert np.isnan(_aff.similarity_transforms(np.full((1, 2, 3), np.nan))).all()


def test_postprocess_affines_similarity_fills_gaps_linearly():
    cfg = pipeline.AlignConfig(n_kp_global=10, ransac_model="similarity")
    assert cfg.effective_frame_skip == 3
    assert pipeline.AlignConfig(n_kp_global=10, ransac_model="similarity", n_kp_frame_skip=5).effective_frame_skip == 5
    a = np.full((7, 2, 3), np.nan)
    a[1] = 1.05 * synthetic.rigid(0.1, 0, 0) + [[0, 0, 2.0], [0, 0, 4.0]]
    a[4] = 0.95 * synthetic.rigid(-0.2, 0, 0) + [[0, 0, 8.0], [0, 0, -2.0]]
    affines, skipped, interpolated, summary = pipeline.postprocess_affines(a, cfg)
    assert skipped == [0, 2, 3, 5, 6] and interpolated == [0, 2, 3]  # trailing frames: VA:400
    assert np.array_equal(affines[0], a[1]) and np.array_equal(affines[5], a[4]) and np.array_equal(affines[6], a[4])
    for k in (2, 3):  # entry-wise linear, scaled entries included (the reference's arccos lerp gives NaN here)
        np.testing.assert_allclose(affines[k], a[1] + (a[4] - a[1]) * (k - 1) / 3.0, rtol=1e-15, atol=1e-15)
    assert summary.shape == (7, 4)
    np.testing.assert_allclose(summary[[1, 4], 3], [1.05, 0.95], rtol=1e-15)
    np.testing.assert_allclose(summary[[1, 4], 2], [0.1, -0.2], atol=1e-15)
    # no gap: the one-copy path returns the [n, 4] summary too, the other models keep [n, 3]
    full = np.stack([a[1], a[4]])
    assert pipeline.postprocess_affines(full, cfg)[3].shape == (2, 4)
    affine = pipeline.AlignConfig(n_kp_global=10, ransac_model="affine")
    assert pipeline.postprocess_affines(full, affine)[3].shape == (2, 3)


def test_binding_tables_and_header_declare_the_similarity_entry():
    assert _lib.MODEL_IDS["similarity"] == _lib.KCMC_MODEL_SIMILARITY == 3
    assert _lib.MODEL_MIN_SAMPLES["similarity"] == 2
    assert "kcmc_ransac_similarity" in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGNATURES["kcmc_ransac_similarity"] == _lib._SIGNATURES["kcmc_ransac_rigid"]
    assert _lib.ABI_VERSION == 2  # additive
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+kcmc_ransac_similarity\s*\(", src)
    assert re.search(r"KCMC_MODEL_SIMILARITY\s*=\s*3\b", src)
    assert re.search(r"#define\s+KCMC_ABI_VERSION\s+2\b", src)
    params = lambda name: re.sub(r"\s+", " ", re.search(name + r"\s*\(([^)]*)\)", src).group(1))  # noqa: E731
    assert params("kcmc_ransac_similarity") == params("kcmc_ransac_rigid")


def test_library_validates_the_similarity_entry_before_touching_the_gpu():
    L = _lib.load()
    assert L.kcmc_ransac_similarity(None, None, None, None, None, 0, 1, 10, 1000, 2.0, 1.0, 3, None, None, None,
                                    None, None) == _lib.KCMC_EINVAL
    assert b"kcmc_ransac_similarity" in L.kcmc_last_error()
    # kcmc_ransac_model keeps accepting affine and projective only
    assert L.kcmc_ransac_model(None, 3, None, None, None, None, 0, 1, 10, 1000, 2.0, 1.0, 3, None, None, None,
                               None, None) == _lib.KCMC_EINVAL


def test_synthetic_similarity_ground_truth():
    ks = pipeline_keypoints()
    assert ks.gt.shape == (PIPE["F"], 2, 3)
    sc = np.hypot(ks.gt[:, 0, 0], ks.gt[:, 1, 0])
    assert (np.abs(sc - 1) <= 0.01 + 1e-12).all() and np.ptp(sc) > 1e-3
    # scale * rotation: equal diagonal, opposite off-diagonal
    assert np.allclose(ks.gt[:, 0, 0], ks.gt[:, 1, 1]) and np.allclose(ks.gt[:, 0, 1], -ks.gt[:, 1, 0])
    # the rigid fixtures are unchanged by the new branch
    a = synthetic.make_keypoints(3, 20, 8, (64, 96), seed=4)
    assert np.allclose(np.hypot(a.gt[:, 0, 0], a.gt[:, 1, 0]), 1.0, atol=1e-15)

"""The similarity RANSAC (K2s, kcmc_ransac_similarity: the rigid kernel with the scale
estimated) against the numpy restatement of scikit-image 0.18.3's
ransac(..., SimilarityTransform, min_samples=2, ...) in tests/test_similarity_host.py, and
the model through the pipeline and the VideoAligner API.  Inlier sets and the winning sample
pair exact, parameters within the closed-form-vs-SVD bound (rtol 1e-8, atol 1e-9), warped
pixels bit-exact to the oracle.

And against the C oracle (oracle.ransac_similarity, the same closed form, pinned to the
restatement on the host): winning trial index, inlier count and mask bit for bit on a fuzz
over sizes, coordinate scales, rotations and scales 0.25 to 4, on points within 1e-12 of
the threshold under scales 0.4 and 2.5, on every path size up to N = 2000 and on degenerate
frames; parameters at rtol 1e-10, atol 1e-10 max(1, |template|max)."""
import numpy as np
import pytest
import torch

import oracle
import test_similarity_host as host
from kcmc_amd import stages, synthetic

pytestmark = pytest.mark.gpu
RTOL, ATOL = host.RTOL, host.ATOL


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off


def _run(dev, tpls, qs, fn=None, **kw):
    off = _csr(qs)
    fn = fn or stages.ransac_similarity
    r = fn(_t(np.concatenate(qs).reshape(-1, 2), dev), _t(np.concatenate(tpls).reshape(-1, 2), dev), _t(off, dev),
           off, **kw)
    return (off, r.params.cpu().numpy(), r.inliers.cpu().numpy().astype(bool), r.n_inliers.cpu().numpy(),
            r.best_trial.cpu().numpy())


def _check_vs_reference(name, off, params, inl, nin, best, trials, rate=1.0):
    tpls, qs, tr, _ = host.input_sets()[name]
    assert tr == trials
    for f, (p_ref, inl_ref, pair_ref, ni_ref) in enumerate(host.reference(name)):
        N = len(qs[f])
        assert np.array_equal(inl[off[f]:off[f + 1]], inl_ref), (name, f)
        assert nin[f] == ni_ref, (name, f)
        if N < 3:  # below N_KP_FRAME_SKIP: NaN, no inliers, no trial
            assert np.isnan(params[f]).all() and best[f] == -1, (name, f)
            continue
        pair = None if best[f] < 0 else frozenset(int(k) for k in oracle.hypothesis_table(N, trials)[best[f]])
        assert pair == pair_ref, (name, f, best[f])
        ref = p_ref.copy()
        ref[:, 2] *= rate
        print(f"{name} frame {f} N {N}: inliers {nin[f]}, max |dp| "
              f"{np.nanmax(np.abs(params[f] - ref)) if not np.isnan(ref).any() else float('nan'):.3g}")
        np.testing.assert_allclose(params[f], ref, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=f"{name} {f}")


def test_selection_matches_the_restatement(dev):
    """One launch over every N at which the kernel changes path: N = 2 (skipped), one wave
    with one and with two points per lane (<= 64, <= 128), the workgroup form and numpy's
    split plan (> 128), leaf lengths that are no multiple of 8."""
    tpls, qs = host.selection_frames()
    assert [len(q) for q in qs] == [2, 3, 4, 8, 9, 63, 64, 65, 127, 128, 129, 136, 257, 300]
    off, params, inl, nin, best = _run(dev, tpls, qs)
    assert np.isnan(params[0]).all() and nin[0] == 0
    _check_vs_reference("selection", off, params, inl, nin, best, 1000)


def _gathered(tpls, qs):
    """The frames in the pt_idx / src_frame_stride form: frame f's points are scattered rows
    of kp_ord[f] (a [F, stride] array), the template's the same rows of one shared array."""
    rng = np.random.default_rng(7)
    stride = sum(len(q) for q in qs) + 5
    kp_tpl = rng.uniform(0, 1000, (stride, 2))
    kp_ord = rng.uniform(0, 1000, (len(qs), stride, 2))
    lists, at = [], 0
    for f, (tpl, q) in enumerate(zip(tpls, qs)):
        rows = (at + rng.permutation(len(q))).astype(np.int32)  # list order = the frame's point order
        at += len(q)
        kp_tpl[rows] = tpl
        kp_ord[f, rows] = q
        lists.append(rows)
    return kp_ord, kp_tpl, lists, stride


def test_selection_with_gather_addressing_rate_and_fewer_trials(dev):
    """trials = 200, spatial_rate = 2 and the pt_idx / src_frame_stride addressing form."""
    kp_ord, kp_tpl, lists, stride = _gathered(*host.selection_frames())
    off = _csr(lists)
    r = stages.ransac_similarity(_t(kp_ord.reshape(-1, 2), dev), _t(kp_tpl, dev), _t(off, dev), off,
                                 pt_idx=_t(np.concatenate(lists), dev), src_frame_stride=stride, trials=200,
                                 spatial_rate=2.0)
    _check_vs_reference("selection200", off, r.params.cpu().numpy(), r.inliers.cpu().numpy().astype(bool),
                        r.n_inliers.cpu().numpy(), r.best_trial.cpu().numpy(), 200, rate=2.0)


def test_device_lists_equal_host_lists(dev):
    """ransac_lists("similarity") (the pipeline's entry: device point lists whose sizes the
    host does not read, tables for every count up to max_n) on the same points: bit-identical
    to ransac_similarity."""
    tpls, qs = host.selection_frames()
    kp_ord, kp_tpl, lists, stride = _gathered(tpls, qs)
    off = _csr(lists)
    args = (_t(kp_ord.reshape(-1, 2), dev), _t(kp_tpl, dev), _t(off, dev))
    idx = _t(np.concatenate(lists), dev)
    a = stages.ransac_similarity(*args, off, pt_idx=idx, src_frame_stride=stride)
    max_n = int(np.diff(off).max())
    stages.ransac_prepare_range(dev, "similarity", 3, max_n)
    b = stages.ransac_lists("similarity", *args, idx, stride, max_n)
    assert b.params.shape == (len(qs), 2, 3)
    for name in ("params", "n_inliers", "best_trial", "inliers"):
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        assert np.array_equal(x, y, equal_nan=name == "params"), name
    # and both are the contiguous form's result
    _, params, _, nin, best = _run(dev, tpls, qs)
    assert np.array_equal(params, b.params.cpu().numpy(), equal_nan=True)
    assert np.array_equal(nin, b.n_inliers.cpu().numpy()) and np.array_equal(best, b.best_trial.cpu().numpy())


def test_exact_data_and_coincident_points(dev):
    """dst = 2 src + t on small integers: every hypothesis has S == 0, so the kernel replays
    the trial sequence for skimage's early exit; all points coincident: no model."""
    tpls, qs, maps = host.exact_frames()
    off, params, inl, nin, best = _run(dev, tpls, qs)
    for f, M in enumerate(maps):
        m = inl[off[f]:off[f + 1]]
        if np.isnan(M).any():
            assert np.isnan(params[f]).all() and nin[f] == 0 and not m.any() and best[f] == -1, f
            continue
        assert m.all() and nin[f] == len(qs[f]), f
        np.testing.assert_allclose(params[f], M, rtol=0, atol=1e-9, err_msg=str(f))
        # the first trial with a model already has S == 0: skimage stops there
        assert best[f] == 0, f


def test_scale_one_reduces_to_rigid(dev):
    """Rigid data with noise: the similarity and the rigid kernel find the same inlier sets
    and the recovered scale is 1 up to the noise (guards against a transposed sign)."""
    tpls, qs = host.rigid_frames()
    off, ps, inl_s, nin_s, _ = _run(dev, tpls, qs)
    _, pr, inl_r, nin_r, _ = _run(dev, tpls, qs, fn=stages.ransac_rigid)
    assert np.array_equal(inl_s, inl_r) and np.array_equal(nin_s, nin_r)
    assert (nin_s > 0.6 * np.diff(off)).all()
    scale = np.hypot(ps[:, 0, 0], ps[:, 1, 0])
    print("recovered scales", scale)
    assert np.abs(scale - 1).max() < 1e-2
    np.testing.assert_allclose(ps[:, 0, 0], ps[:, 1, 1], rtol=0, atol=0)
    np.testing.assert_allclose(ps[:, 0, 1], -ps[:, 1, 0], rtol=0, atol=0)
    assert np.abs(np.arctan2(ps[:, 1, 0], ps[:, 0, 0]) - np.arctan2(pr[:, 1, 0], pr[:, 0, 0])).max() < 1e-2


@pytest.mark.parametrize("thresh", host.THRESHOLDS)
def test_thresholds_exact_only_path_and_undecided_band(dev, thresh):
    """1e-120: tq is out of the fast range, every trial is scored exactly; 5e-5: the fp32
    phase A with points inside its undecided band (host.threshold_frames)."""
    assert host.THRESHOLDS == [1e-120, 5e-5]
    tpls, qs = host.threshold_frames()
    off, params, inl, nin, best = _run(dev, tpls, qs, residual_threshold=thresh)
    _check_vs_reference(f"thresh{thresh:g}", off, params, inl, nin, best, 1000)


# ------------------------------------------------------------- the kernel against the C oracle
# oracle.ransac_similarity is the closed form the kernel computes (pinned to the restatement
# in tests/test_similarity_host.py), so the comparison is bit for bit on selection: winning
# trial index, inlier count and mask.  Only the refit's summation order differs: parameters
# at the rigid fuzz's tolerance.
def _check_vs_oracle(tpls, qs, got, thresh=2.0, trials=1000, ctx=()):
    off, params, inl, nin, best = got
    worst, n_fit = 0.0, 0
    for f, (tpl, q) in enumerate(zip(tpls, qs)):
        m = inl[off[f]:off[f + 1]]
        if len(q) < 3:  # below N_KP_FRAME_SKIP: NaN, no inliers, no trial
            assert np.isnan(params[f]).all() and nin[f] == 0 and best[f] == -1 and not m.any(), (ctx, f)
            continue
        p, i_ref, bt, ni = oracle.ransac_similarity(q, tpl, trials, thresh)
        assert best[f] == bt and nin[f] == ni, (ctx, f, len(q), best[f], bt, nin[f], ni)
        assert np.array_equal(m, i_ref), (ctx, f)
        sc = max(1.0, float(np.abs(tpl).max()))
        np.testing.assert_allclose(params[f], p, rtol=1e-10, atol=1e-10 * sc, equal_nan=True, err_msg=str((ctx, f)))
        if not np.isnan(p).any():
            worst = max(worst, float(np.abs(params[f] - p).max()) / sc)
            n_fit += 1
    print(f"{ctx}: {len(qs)} frames, {n_fit} fitted, kernel vs oracle max |dp| / scale {worst:.3g}")
    return n_fit


def _fuzz_set(s):
    """host.fuzz_set widened for two closed forms: N = 0, 1, 2 (skipped frames) and noise-free
    frames (S rounds to 0 in some trials: the early exit must agree)."""
    return host.fuzz_set(s, extra_n=(0, 1, 2), extra_noise=(0.0,))


@pytest.mark.parametrize("s", host.FUZZ_SEEDS)
def test_fuzz_vs_oracle(dev, s):
    tpls, qs, thresh = _fuzz_set(s)
    assert len(qs) == 24
    n_fit = _check_vs_oracle(tpls, qs, _run(dev, tpls, qs, residual_threshold=thresh), thresh, ctx=("fuzz", s, thresh))
    assert n_fit >= 8  # 3 of the 8 choices of N are skipped frames: a third of the 24 at least is fitted


@pytest.mark.parametrize("k", [0.4, 2.5])
@pytest.mark.parametrize("scale", [1.0, 2000.0, 3e5])
def test_threshold_band_vs_oracle(dev, scale, k):
    """test_gpu_fuzz.test_ransac_threshold_band_vs_oracle's frames under a similarity of scale
    k (|a|, |b| of the fp32 phase A's bound |a| h_x + |b| h_y above and far below 1), with
    2.0 rad more rotation on odd frames: points within 1e-12 .. 1e-2 of the 2 px threshold,
    coordinates up to 3e5 px (wide band, trials deferred to the fp64 phase A).  The band lies
    inside the SVD's rounding, so only the closed-form oracle can be the yardstick here."""
    rng = np.random.default_rng(int(scale) + int(10 * k))
    tpls, qs = [], []
    for f in range(6):
        n_exact, n_band, n_out = 12 + 3 * f, 20, 10
        tpl = rng.uniform(0.2, 1.0, (n_exact + n_band + n_out, 2)) * scale
        a = rng.normal(0, 0.02) + (2.0 if f % 2 else 0.0)
        A = k * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        t = rng.normal(0, 5, 2)
        q = (tpl - t) @ np.linalg.inv(A).T  # q maps onto tpl exactly: A q + t = tpl
        d = rng.choice([-1e-2, -1e-5, -1e-9, -1e-12, 0.0, 1e-12, 1e-9, 1e-5, 1e-2], n_band)
        ang = rng.uniform(0, 2 * np.pi, n_band)
        sl = slice(n_exact, n_exact + n_band)
        tpl[sl] += (2.0 + d)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        tpl[n_exact + n_band:] += rng.uniform(5, 50, (n_out, 2))
        tpls.append(tpl)
        qs.append(q)
    assert _check_vs_oracle(tpls, qs, _run(dev, tpls, qs), ctx=("band", scale, k)) == 6


PATH_NS = [3, 4, 5, 8, 9, 50, 63, 64, 65, 100, 127, 128, 129, 136, 200, 255, 256, 257, 300, 500, 777, 1024, 2000]


def test_path_sizes_winning_trial_vs_oracle(dev):
    """test_gpu_kernels.test_ransac_bit_exact_selection_vs_oracle's frames with a per-frame
    scale in [0.5, 2]: every N at which the kernel changes path, up to the 2000 points of the
    rigid list (numpy's split plan four levels deep), and the winning trial by its index."""
    rng = np.random.default_rng(21)
    tpls, qs = [], []
    for N in PATH_NS:
        tpl = rng.uniform(0, 1000, (N, 2))
        A = synthetic.rigid(rng.normal(0, 0.02), rng.normal(0, 5), rng.normal(0, 5))
        s = rng.uniform(0.5, 2.0)
        q = (tpl - A[:, 2]) @ A[:, :2] / s + rng.normal(0, rng.uniform(0.1, 1.5), (N, 2))
        out = rng.random(N) < rng.uniform(0, 0.6)
        q[out] = rng.uniform(0, 1000, (int(out.sum()), 2))
        tpls.append(host._f32(tpl))
        qs.append(host._f32(q))
    assert _check_vs_oracle(tpls, qs, _run(dev, tpls, qs), ctx="path sizes") == len(PATH_NS)


def test_degenerate_frames_vs_oracle(dev):
    """host.degenerate_frames (coincident thirds on either side, a quarter turn with scale 3, a
    mirrored frame: refit with det < 0) and a frame whose points all coincide: no trial has a
    model, so NaN, no inliers, trial -1."""
    frames = host.degenerate_frames()
    tpls, qs = [t for _, _, t, _ in frames], [q for _, _, _, q in frames]
    rng = np.random.default_rng(23)
    tpls.append(rng.uniform(0, 100, (10, 2)))
    qs.append(np.repeat(rng.uniform(0, 100, (1, 2)), 10, 0))
    got = _run(dev, tpls, qs)
    assert _check_vs_oracle(tpls, qs, got, ctx="degenerate") == 8
    off, params, inl, nin, best = got
    assert np.isnan(params[-1]).all() and nin[-1] == 0 and best[-1] == -1 and not inl[off[-2]:].any()


@pytest.mark.parametrize("thresh", host.THRESHOLDS)
def test_fuzz_first_seed_at_extreme_thresholds_vs_oracle(dev, thresh):
    """1e-120 (exact scoring only: a point is an inlier only at residual 0, and a trial with
    no inlier can still win on S) and 5e-5 on frames of every coordinate scale."""
    tpls, qs, _ = _fuzz_set(0)
    _check_vs_oracle(tpls, qs, _run(dev, tpls, qs, residual_threshold=thresh), thresh, ctx=("fuzz 0", thresh))


def _pipeline_inputs(dev):
    ks = host.pipeline_keypoints()
    P = host.PIPE
    H, W = P["size"]
    base = synthetic.make_texture((H, W), seed=96)
    imgs = np.ascontiguousarray(np.stack([np.roll(base, (5 * f, 7 * f), axis=(0, 1)) for f in range(P["F"])]))
    return ks, imgs


def test_pipeline_end_to_end(dev):
    """match -> consensus -> similarity RANSAC -> linear gap filling -> warpAffine, frame by
    frame against the restatement on that frame's consensus list and the oracle's warp."""
    from kcmc_amd import pipeline

    ks, imgs = _pipeline_inputs(dev)
    P = host.PIPE
    inp = pipeline.SlabInputs(_t(imgs, dev), _t(ks.des_tpl, dev), _t(ks.kp_tpl, dev), _t(ks.des_q, dev),
                              _t(ks.kp_q, dev), _t(ks.q_off, dev), ks.q_off)
    cfg = pipeline.AlignConfig(n_kp_global=P["n_kp_global"], ransac_model="similarity")
    res = pipeline.align_slab(inp, cfg, keep_intermediates=True)
    torch.cuda.synchronize()
    assert res.affines.shape == (P["F"], 2, 3) and res.euclidean.shape == (P["F"], 4)
    kq = res.match.kp_ordered.cpu().numpy()
    po, pi = res.consensus.pt_off, res.consensus.pt_idx
    raw = res.ransac.params.cpu().numpy()
    tpls, qs, _, _ = host.input_sets()["pipeline"]
    ref = host.reference("pipeline")
    out = res.aligned.cpu().numpy()
    for f in range(P["F"]):
        L = pi[po[f]:po[f + 1]]
        # the device consensus lists are the oracle's (the restatement ran on those)
        assert np.array_equal(kq[f][L], qs[f]) and np.array_equal(ks.kp_tpl[L], tpls[f]), f
        p_ref = ref[f][0]
        if f in P["blank"]:
            assert np.isnan(raw[f]).all() and np.isnan(p_ref).all(), f
        else:
            np.testing.assert_allclose(raw[f], p_ref, rtol=RTOL, atol=ATOL, err_msg=str(f))
            assert np.array_equal(res.affines[f], raw[f]), f
            assert np.abs(res.affines[f][:, 2] - ks.gt[f][:, 2]).max() < 1.0, f
            assert abs(res.euclidean[f, 3] - np.hypot(ks.gt[f][0, 0], ks.gt[f][1, 0])) < 5e-3, f
        assert np.array_equal(out[f], oracle.warp_affine_u16(imgs[f], res.affines[f])), f
    a, b = P["blank"][0] - 1, P["blank"][-1] + 1  # the gap's neighbours
    assert res.skipped == list(P["blank"]) and res.interpolated == list(P["blank"])
    for f in P["blank"]:
        want = res.affines[a] + (res.affines[b] - res.affines[a]) * ((f - a) / float(b - a))
        np.testing.assert_allclose(res.affines[f], want, rtol=1e-15, atol=1e-15)


def test_video_aligner_similarity(dev):
    from kcmc_amd import VideoAligner

    class One(VideoAligner):
        RANSAC_MODEL = "similarity"
        DEVICES = [0]

    class Two(One):
        DEVICES = [0, 0]

    ks, imgs = _pipeline_inputs(dev)
    P = host.PIPE
    kps = [ks.kp_q[ks.q_off[f]:ks.q_off[f + 1]] for f in range(P["F"])]
    des = [ks.des_q[ks.q_off[f]:ks.q_off[f + 1]] for f in range(P["F"])]
    a1, t1, s1 = One().align_keypoints(imgs, ks.kp_tpl, ks.des_tpl, kps, des, n_kp_global=P["n_kp_global"])
    a2, t2, s2 = Two().align_keypoints(imgs, ks.kp_tpl, ks.des_tpl, kps, des, n_kp_global=P["n_kp_global"])
    assert t1.shape == (P["F"], 4) and a1.shape == imgs.shape and s1 == list(P["blank"])
    assert np.array_equal(a1, a2) and np.array_equal(t1, t2) and s1 == s2
    tpls, qs, _, _ = host.input_sets()["pipeline"]
    f = 3
    row = One._compute_similarity_affine(tpls[f], qs[f], 1)
    assert row.shape == (2, 3)
    from kcmc_amd import affines

    assert np.array_equal(t1[f], affines.similarity_transforms(row[None])[0])  # the batch row, bit for bit
    np.testing.assert_allclose(row, host.reference("pipeline")[f][0], rtol=RTOL, atol=ATOL)
    assert np.isnan(One._compute_similarity_affine(tpls[f][:2], qs[f][:2], 1)).all()  # below N_KP_FRAME_SKIP

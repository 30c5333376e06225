"""The similarity RANSAC (K2s, kcmc_ransac_similarity: the rigid kernel with the scale
estimated) against the numpy restatement of scikit-image 0.18.3's
ransac(..., SimilarityTransform, min_samples=2, ...) in tests/test_similarity_host.py, and
the model through the pipeline and the VideoAligner API.  Inlier sets and the winning sample
pair exact, parameters within the closed-form-vs-SVD bound (rtol 1e-8, atol 1e-9), warped
pixels bit-exact to the oracle."""
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

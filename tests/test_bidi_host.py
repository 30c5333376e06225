"""The bidirectional-scan phase correction (kcmc_amd.bidi, csrc/bidi_phase.hip) restated in numpy:
what the two kernels compute (ref_bidi_sums, ref_shift_rows), known answers of the restatement,
the estimator's rules, the planted offsets it recovers, the sampled frames, the switch's
checks and the ABI -- all without a GPU.  tests/test_gpu_bidi.py holds the kernels to the
restatement bit for bit.

Build-defined semantics (include/kcmc.h).  A sample is one vertically adjacent
row pair (y, y + 1) at one column x in [R, W - R); a = the pair's odd row at x + d, b = its even
row at x; the five sums are (sum a, sum b, sum a^2, sum b^2, sum a*b), n = (H - 1)(W - 2R)."""
import ctypes
import math
import os

import numpy as np
import pytest

from kcmc_amd import _lib, bidi, quality, synthetic

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kcmc.h")


# ------------------------------------------------------------------------ the restatements
def ref_bidi_sums(frames, idx, R):
    """[len(idx), 2R + 1, 5] of Python ints (dtype object): sample by sample as the header states
    them, one row pair at a time.  idx None: every frame; an index outside the stack: zeros."""
    frames = np.asarray(frames)
    F, H, W = frames.shape
    idx = list(range(F)) if idx is None else [int(i) for i in idx]
    out = np.zeros((len(idx), 2 * R + 1, 5), dtype=object)
    for k, f in enumerate(idx):
        if not 0 <= f < F:
            continue
        fr = frames[f].astype(np.int64)
        for d in range(-R, R + 1):
            s = [0] * 5
            for y in range(H - 1):
                yo, ye = (y, y + 1) if y & 1 else (y + 1, y)
                a = [int(v) for v in fr[yo, R + d:W - R + d]]
                b = [int(v) for v in fr[ye, R:W - R]]
                assert len(a) == len(b) == W - 2 * R
                s[0] += sum(a)
                s[1] += sum(b)
                s[2] += sum(v * v for v in a)
                s[3] += sum(v * v for v in b)
                s[4] += sum(p * q for p, q in zip(a, b))
            out[k, d + R] = s
    return out


def ref_shift_rows(frames, d, parity=1):
    """dst[f][y][x] = src[f][y][clamp(x + d, 0, W - 1)] on the rows with (y & 1) == parity."""
    frames = np.asarray(frames)
    out = frames.copy()
    W = frames.shape[-1]
    cols = np.clip(np.arange(W) + int(d), 0, W - 1)
    out[..., parity::2, :] = frames[..., parity::2, :][..., cols]
    return out


def ref_r(sums_row, n):
    """Pearson's r of one entry, as quality.pearson: exact integers, one rounding each."""
    sa, sb, saa, sbb, sab = (int(v) for v in sums_row)
    va, vb = n * saa - sa * sa, n * sbb - sb * sb
    if va == 0 or vb == 0:
        return math.nan
    return float(n * sab - sa * sb) / (math.sqrt(float(va)) * math.sqrt(float(vb)))


def random_u16(shape, seed):
    return np.random.default_rng(seed).integers(0, 65536, shape).astype(np.uint16)


# --------------------------------------------------------------------------- known answers
def test_module_is_exported():
    import kcmc_amd

    assert kcmc_amd.bidi is bidi
    for name in ("phase_sums", "sample_indices", "estimate_offset", "shift_rows"):
        assert callable(getattr(bidi, name))


def test_shift_restatement_known_answers():
    x = random_u16((3, 7, 11), 1)
    np.testing.assert_array_equal(ref_shift_rows(x, 0), x)
    for d in (1, -1, 3, -4):
        back = ref_shift_rows(ref_shift_rows(x, d), -d)
        k = abs(d)
        np.testing.assert_array_equal(back[..., k:11 - k], x[..., k:11 - k])
        assert (back != x).any()
        y = ref_shift_rows(x, d)
        np.testing.assert_array_equal(y[:, 0::2], x[:, 0::2])  # even rows untouched
        if d > 0:
            np.testing.assert_array_equal(y[:, 1::2, :11 - d], x[:, 1::2, d:])
            assert (y[:, 1::2, 11 - d:] == x[:, 1::2, -1:]).all()  # the edge replicated
        else:
            np.testing.assert_array_equal(y[:, 1::2, -d:], x[:, 1::2, :11 + d])
            assert (y[:, 1::2, :-d] == x[:, 1::2, :1]).all()
    for d, edge in ((11, -1), (16, -1), (-11, 0), (-16, 0)):  # |d| >= W: the edge pixel everywhere
        y = ref_shift_rows(x, d)
        assert (y[:, 1::2] == x[:, 1::2, edge][..., None]).all()
    p0, p1 = ref_shift_rows(x, 2, parity=0), ref_shift_rows(x, 2, parity=1)
    np.testing.assert_array_equal(p0[:, 1::2], x[:, 1::2])
    np.testing.assert_array_equal(p1[:, 0::2], x[:, 0::2])
    assert (p0[:, 0::2] != x[:, 0::2]).any() and (p1[:, 1::2] != x[:, 1::2]).any()


def test_sums_restatement_known_answers():
    R, H, W = 3, 6, 19
    row = random_u16((W,), 2)
    same = np.repeat(row[None], H, 0)[None]
    s = ref_bidi_sums(same, None, R)
    n = (H - 1) * (W - 2 * R)
    assert ref_r(s[0, R], n) == 1.0
    assert int(s[0, R, 0]) == int(s[0, R, 1]) == (H - 1) * int(row[R:W - R].astype(np.int64).sum())
    # an interior row counts twice: one bright odd row of a dark frame
    one = np.zeros((1, 5, 9), np.uint16)
    one[0, 1, :] = 7
    one[0, 4, :] = 3
    s = ref_bidi_sums(one, None, 1)
    assert [int(v) for v in s[0, 1]] == [2 * 7 * 7, 3 * 7, 2 * 49 * 7, 9 * 7, 0]
    # b does not depend on d; a out-of-range index is zeros
    x = random_u16((2, 5, 12), 3)
    s = ref_bidi_sums(x, [1, 5, -1], 2)
    assert (s[0, :, 1] == s[0, 0, 1]).all() and (s[0, :, 3] == s[0, 0, 3]).all()
    assert not s[1].any() and not s[2].any()
    # all-65535: every r is NaN, the estimate is (0, ..., False)
    full = np.full((2, 9, 40), 65535, np.uint16)
    s = ref_bidi_sums(full, None, 8)
    off, r, ok = bidi.estimate_offset(s, bidi.sample_count(9, 40, 8))
    assert off == 0 and ok is False and np.isnan(r).all() and r.shape == (17,)
    assert int(s[0, 0, 4]) == 8 * 24 * 65535 * 65535


def test_pearson_of_the_sums_is_the_correlation_of_the_samples():
    R, H, W = 2, 7, 23
    x = random_u16((1, H, W), 4)
    s = ref_bidi_sums(x, None, R)
    n = bidi.sample_count(H, W, R)
    assert n == (H - 1) * (W - 2 * R)
    for d in range(-R, R + 1):
        a, b = [], []
        for y in range(H - 1):
            yo, ye = (y, y + 1) if y & 1 else (y + 1, y)
            a.append(x[0, yo, R + d:W - R + d])
            b.append(x[0, ye, R:W - R])
        want = np.corrcoef(np.concatenate(a).astype(np.float64), np.concatenate(b).astype(np.float64))[0, 1]
        got = quality.pearson(s[0, d + R][None], n)[0]
        assert got == ref_r(s[0, d + R], n)
        assert abs(got - want) < 1e-12


# ----------------------------------------------------------------------- the estimator's rules
def sums_with_r(rs, n=1000):
    """[1, S, 5] sums whose correlations are (about) ``rs``: a and b zero-mean-free integers with
    va = vb = n^2 and the covariance set per entry (NaN: a constant a)."""
    out = np.zeros((1, len(rs), 5), dtype=object)
    for j, r in enumerate(rs):
        if r is None:
            out[0, j] = (5 * n, 7 * n, 25 * n, 49 * n + n, 35 * n)  # va = 0
        else:
            out[0, j] = (0, 0, n, n, int(round(r * n)))
    return out


def test_estimator_tie_order_border_and_gain():
    est = bidi.estimate_offset
    # the peak
    off, r, ok = est(sums_with_r([0.1, 0.2, 0.3, 0.9, 0.3, 0.2, 0.1][::-1]), 1000)
    assert (off, ok) == (0, True) and r.dtype == np.float64 and abs(r[3] - 0.9) < 1e-12
    assert est(sums_with_r([0.1, 0.8, 0.3, 0.5, 0.3, 0.2, 0.1]), 1000)[::2] == (-2, True)
    assert est(sums_with_r([0.1, 0.2, 0.3, 0.5, 0.3, 0.8, 0.1]), 1000)[::2] == (2, True)
    # ties: the smaller |d|, then the negative d
    assert est(sums_with_r([0.1, 0.8, 0.3, 0.5, 0.8, 0.2, 0.1]), 1000)[::2] == (1, True)
    assert est(sums_with_r([0.1, 0.2, 0.8, 0.5, 0.8, 0.2, 0.1]), 1000)[::2] == (-1, True)
    assert est(sums_with_r([0.1, 0.8, 0.3, 0.8, 0.3, 0.8, 0.1]), 1000)[::2] == (0, True)
    # the border: rejected; an interior entry that ties with it wins on |d|
    assert est(sums_with_r([0.9, 0.2, 0.3, 0.5, 0.3, 0.2, 0.1]), 1000)[::2] == (0, False)
    assert est(sums_with_r([0.1, 0.2, 0.3, 0.5, 0.3, 0.2, 0.9]), 1000)[::2] == (0, False)
    assert est(sums_with_r([0.9, 0.2, 0.9, 0.5, 0.3, 0.2, 0.1]), 1000)[::2] == (-1, True)
    # R = 0: the only entry is no border
    assert est(sums_with_r([0.4]), 1000)[::2] == (0, True)
    # NaN entries are skipped; all NaN: rejected
    off, r, ok = est(sums_with_r([None, 0.2, None, 0.5, 0.7, None, None]), 1000)
    assert (off, ok) == (1, True) and np.isnan(r[[0, 2, 5, 6]]).all()
    assert est(sums_with_r([None] * 5), 1000)[::2] == (0, False)
    # min_gain: r(peak) - r(0) <= min_gain rejects a peak off 0, never one at 0
    s = sums_with_r([0.1, 0.2, 0.3, 0.5, 0.75, 0.2, 0.1])
    assert est(s, 1000)[::2] == (1, True)
    assert est(s, 1000, min_gain=0.2)[::2] == (1, True)
    assert est(s, 1000, min_gain=0.25)[::2] == (0, False)
    assert est(s, 1000, min_gain=0.5)[::2] == (0, False)
    assert est(sums_with_r([0.1, 0.2, 0.3, 0.9, 0.3, 0.2, 0.1]), 1000, min_gain=5.0)[::2] == (0, True)
    with pytest.raises(ValueError):
        est(np.zeros((1, 4, 5), np.int64), 10)
    with pytest.raises(ValueError):
        est(np.zeros((3, 5), np.int64), 10)


def test_estimator_pools_exactly_near_2_63():
    """Sums of 64 frames near 2^62 each: their total passes 2^63, n * sum(ab) passes 2^100; the
    result is the exact-integer one, and int64 wrap-around would change it."""
    n1 = (1 << 31) - 1
    K = 64
    big = np.zeros((K, 3, 5), np.int64)
    for k in range(K):
        for j, sab in enumerate((n1 * 65535 * 20000 + k, n1 * 65535 * 30000 + 7 * k, n1 * 65535 * 25000)):
            # a = 65535 or 0 half of the time, b likewise: sums of that magnitude
            big[k, j] = (n1 * 32768, n1 * 30000, n1 * 32768 * 65535, n1 * 30000 * 65535, sab)
    assert int(big[:, 0, 2].astype(object).sum()) > 1 << 63
    off, r, ok = bidi.estimate_offset(big, n1)
    pooled = big.astype(object).sum(axis=0)
    want = [ref_r(pooled[j], K * n1) for j in range(3)]
    assert [float(v) for v in r] == want
    assert (off, ok) == (0, True) and want[1] > want[2] > want[0]
    assert (big.sum(axis=0).astype(object) != pooled).any()  # int64 wraps


def planted(H, W, k, sigma, frames=4):
    base = synthetic.make_texture((H, W), seed=5)
    rng = np.random.default_rng(0)
    out = []
    for f in range(frames):
        fr = np.roll(base, (3 * f, 5 * f), (0, 1)).copy()
        fr[1::2] = np.roll(fr[1::2], k, axis=1)  # the odd rows displaced by k: odd(x) = scene(x - k)
        if sigma:
            fr = np.clip(np.rint(fr + rng.normal(0, sigma, fr.shape)), 0, 65535)
        out.append(fr.astype(np.uint16))
    return np.stack(out)


def fast_bidi_sums(frames, R):
    """ref_bidi_sums of every frame, vectorised (int64 is exact here: small frames)."""
    fr = np.asarray(frames).astype(np.int64)
    F, H, W = fr.shape
    out = np.zeros((F, 2 * R + 1, 5), np.int64)
    yo = np.array([y if y & 1 else y + 1 for y in range(H - 1)])
    ye = np.array([y + 1 if y & 1 else y for y in range(H - 1)])
    b = fr[:, ye, R:W - R]
    for d in range(-R, R + 1):
        a = fr[:, yo, R + d:W - R + d]
        out[:, d + R] = np.stack([a.sum((1, 2)), b.sum((1, 2)), (a * a).sum((1, 2)), (b * b).sum((1, 2)),
                                  (a * b).sum((1, 2))], 1)
    return out


def test_fast_restatement_is_the_restatement():
    x = random_u16((2, 6, 21), 6)
    assert (ref_bidi_sums(x, None, 3) == fast_bidi_sums(x, 3)).all()


@pytest.mark.parametrize("sigma", [0, 2000])
@pytest.mark.parametrize("H,W", [(96, 160), (57, 129), (64, 136)])
def test_estimator_recovers_planted_offsets(H, W, sigma):
    R = 8
    for k in range(-6, 7):
        off, r, ok = bidi.estimate_offset(fast_bidi_sums(planted(H, W, k, sigma), R), bidi.sample_count(H, W, R))
        assert (off, ok) == (k, True), (k, r)


# --------------------------------------------------------------------------- sample_indices
def test_sample_indices():
    assert bidi.sample_indices(5, 64) == [0, 1, 2, 3, 4]        # n < k
    assert bidi.sample_indices(4, 4) == [0, 1, 2, 3]            # n == k
    assert bidi.sample_indices(10, 4) == [0, 3, 6, 9]           # n > k: (i (n - 1)) // (k - 1)
    assert bidi.sample_indices(2000, 64) == [(i * 1999) // 63 for i in range(64)]
    assert bidi.sample_indices(2000, 64)[0] == 0 and bidi.sample_indices(2000, 64)[-1] == 1999
    assert bidi.sample_indices(11, 2) == [0, 10]
    assert bidi.sample_indices(9, 1) == [4] and bidi.sample_indices(10, 1) == [5]  # k == 1: n // 2
    assert bidi.sample_indices(1, 1) == [0] and bidi.sample_indices(0, 3) == []
    with pytest.raises(ValueError):
        bidi.sample_indices(5, 0)


# ------------------------------------------------------------------ the switch without a GPU
def _va(**kw):
    from kcmc_amd import VideoAligner

    return type("VA", (VideoAligner,), kw)()


def test_switch_defaults_and_results():
    from kcmc_amd import VideoAligner

    assert VideoAligner.BIDI_PHASE == "none"
    assert (VideoAligner.BIDI_PHASE_RADIUS, VideoAligner.BIDI_PHASE_FRAMES, VideoAligner.BIDI_PHASE_MIN_GAIN) == \
        (8, 64, 0.0)
    va = VideoAligner()
    assert va.bidi_offset is None and va.bidi_correlations is None and va.bidi_frames is None
    assert va.bidi_accepted is None
    assert va._bidi_on() is None and _va(BIDI_PHASE="auto")._bidi_on() == "auto"
    assert _va(BIDI_PHASE=-16)._bidi_on() == -16 and _va(BIDI_PHASE=np.int64(3))._bidi_on() == 3
    assert _va(BIDI_PHASE=0)._bidi_on() == 0


def test_switch_checks_fail_before_any_work():
    stack4 = np.zeros((2, 4, 4, 3), np.uint16)
    cases = [(dict(BIDI_PHASE=v), ValueError, "BIDI_PHASE", None) for v in ("Auto", True, 17, -17, 1.5, None)]
    cases += [(dict(BIDI_PHASE="auto", BIDI_PHASE_RADIUS=v), ValueError, "BIDI_PHASE_RADIUS", None)
              for v in (0, 17, 2.0, True)]
    cases += [(dict(BIDI_PHASE="auto", BIDI_PHASE_FRAMES=v), ValueError, "BIDI_PHASE_FRAMES", None) for v in (0, -1, 1.5)]
    cases += [(dict(BIDI_PHASE=2, BIDI_PHASE_MIN_GAIN="x"), ValueError, "BIDI_PHASE_MIN_GAIN", None)]
    cases += [(dict(BIDI_PHASE="auto"), NotImplementedError, "grayscale", stack4),
              (dict(BIDI_PHASE=3), NotImplementedError, "grayscale", stack4)]
    for kw, err, match, images in cases:
        va = _va(**kw)
        va.bidi_offset = 5  # a stale result: reset at the start of every call
        with pytest.raises(err, match=match):
            va.align_images(images, 10, "orb", 30)
        assert va.bidi_offset is None
        with pytest.raises(err, match=match):
            _va(**kw).align_keypoints(images, None, None, None, None, 10)


# -------------------------------------------------------------------------------- the ABI
def test_header_and_binding_table_name_the_entry_points():
    with open(HEADER) as f:
        header = f.read()
    for name in ("kcmc_bidi_phase_sums_u16", "kcmc_shift_rows_u16"):
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGNATURES
        assert f"int {name}(" in header
    assert len(_lib._SIGNATURES["kcmc_bidi_phase_sums_u16"][0]) == 10
    assert len(_lib._SIGNATURES["kcmc_shift_rows_u16"][0]) == 9
    assert "#define KCMC_ABI_VERSION 2" in header and _lib.ABI_VERSION == 2
    assert _lib.load().kcmc_abi_version() == 2


def check_validation(ctx, good):
    """Every contract violation is KCMC_EINVAL before any device work.  ``ctx``: a context handle
    (never dereferenced by the checks); ``good``: device pointers (frames, idx, out, dst) of valid
    33 x 40 calls, or None on a box without a GPU (a host buffer stands in: nothing reads it)."""
    L = _lib.load()
    P = ctypes.c_void_p
    buf = np.zeros(64, np.int64)
    fr, idx, out, dst = good if good is not None else (buf.ctypes.data,) * 4
    p = lambda v: None if v is None else P(v)  # noqa: E731
    E, OK = _lib.KCMC_EINVAL, _lib.KCMC_OK

    def sums(ctx=ctx, fr=fr, n_frames=1, H=33, W=40, idx=idx, n_sel=1, R=8, out=out):
        return L.kcmc_bidi_phase_sums_u16(ctx, p(fr), n_frames, H, W, p(idx), n_sel, R, p(out), None)

    assert sums(ctx=None) == E and b"ctx" in L.kcmc_last_error()
    assert sums(fr=None) == E and b"NULL" in L.kcmc_last_error()
    assert sums(out=None) == E
    assert sums(out=out + 4) == E and b"aligned" in L.kcmc_last_error()
    for R in (-1, 17):
        assert sums(R=R) == E and b"R must" in L.kcmc_last_error()
    assert sums(H=1) == E and b"H must" in L.kcmc_last_error()
    assert sums(W=16) == E and b"W must" in L.kcmc_last_error()
    assert sums(H=1 << 16, W=1 << 15) == E and b"2^31" in L.kcmc_last_error()
    assert sums(n_sel=-1) == E and sums(n_frames=-1) == E and sums(H=0) == E and sums(W=0) == E
    assert sums(n_sel=0) == OK
    assert sums(n_sel=0, fr=None, idx=None, out=None) == OK

    def shift(ctx=ctx, src=fr, dst=dst, n_frames=1, H=33, W=40, parity=1, d=3):
        return L.kcmc_shift_rows_u16(ctx, p(src), p(dst), n_frames, H, W, parity, d, None)

    assert shift(ctx=None) == E and b"ctx" in L.kcmc_last_error()
    assert shift(src=None) == E and b"NULL" in L.kcmc_last_error()
    assert shift(dst=None) == E
    for parity in (-1, 2):
        assert shift(parity=parity) == E and b"parity" in L.kcmc_last_error()
    for d in (-17, 17):
        assert shift(d=d) == E and b"d must" in L.kcmc_last_error()
    assert shift(H=32768) == E and shift(W=32768) == E and b"32768" in L.kcmc_last_error()
    assert shift(H=0) == E and shift(W=0) == E and shift(n_frames=-1) == E
    for delta in (2, -2, 2 * (33 * 40 - 1), -2 * (33 * 40 - 1)):  # partial overlap, either way round
        assert shift(dst=fr + delta) == E and b"overlap" in L.kcmc_last_error(), delta
    assert shift(n_frames=0) == OK and shift(n_frames=0, src=None, dst=None) == OK
    assert shift(dst=fr, d=0) == OK  # in place, nothing to move: no launch
    if good is not None:
        assert sums() == OK and shift() == OK and shift(dst=fr) == OK


def test_entry_points_validate_before_touching_the_gpu():
    check_validation(ctypes.c_void_p(np.zeros(8, np.int64).ctypes.data), None)

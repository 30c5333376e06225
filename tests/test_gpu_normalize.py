"""The normalisation front end (csrc/normalize.hip behind stages.brightest_px / max_scale_u8) bit
for bit against numpy: np.percentile(x, q), the reference's scaling expression
np.clip(x / b * max_px, 0, max_px).astype(uint8) and np.bincount -- never stages.max_scale_lut,
which is the code under test.

Large stacks: the sizes of tests/test_normalize_host.py, where the capped grids of both histogram
passes and of the table kernel walk their grid-stride loops (two or more iterations, the single
load behind an iteration, both tails); that file proves from the kernel's constants which path
each size takes.  Directed ranks: small sorted multisets, shuffled, with q chosen so that numpy's
two ranks land on the first or last element of a bin, on the two sides of a coarse boundary, of a
run of empty bins, in bins 0 and 255 of either byte.  The C entries with every (shift, match) they
accept and every argument they refuse.  max_scale_u8's tails, ``out`` views and parameters.  A
side stream."""
import ctypes

import numpy as np
import pytest
import torch

import test_normalize_host as nhost
from kcmc_amd import _lib, stages

pytestmark = pytest.mark.gpu
QS = (99.99, 50.0, 0.0, 100.0)
FAMILIES = ("u12", "u16-patch", "concentrated")
P = ctypes.c_void_p


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _family(name, n, seed):
    rng = np.random.default_rng([seed, n])
    if name == "u12":
        return rng.integers(0, 4096, n, dtype=np.uint16)
    if name == "concentrated":  # two coarse bins: the fine pass counts about half the stack
        return rng.integers(0x0F00, 0x1100, n, dtype=np.uint16)
    v = rng.integers(0, 65536, n, dtype=np.uint16)
    m = max(1, n // 20000)  # with the values drawn as 65535, still fewer than the top 0.01 %
    a = int(rng.integers(0, n - m + 1))
    v[a:a + m] = 65535
    return v


def _scaled(x, b, max_px=255, chunk=1 << 22):
    """The reference's expression (VA:490), evaluated in chunks: x / b is float64."""
    flat = x.reshape(-1)
    out = np.empty(flat.size, np.uint8)
    for a in range(0, flat.size, chunk):
        out[a:a + chunk] = np.clip(flat[a:a + chunk] / b * max_px, a_min=0, a_max=max_px).astype(np.uint8)
    return out.reshape(x.shape)


def _histogram(dev, src, n, shift, match, fill=0x5A5A5A5A5A5A5A5A, src_ptr=None, out_null=False):
    """(status, the 256 counters) of kcmc_histogram_u16 into counters pre-filled with ``fill``."""
    h = torch.full((256,), fill, dtype=torch.int64, device=dev)
    ptr = src_ptr if src_ptr is not None else (src.data_ptr() if src is not None else 0)
    rc = _lib.load().kcmc_histogram_u16(stages._ctx(dev).handle, P(ptr), n, shift, match,
                                        P(0 if out_null else h.data_ptr()), stages._stream(dev))
    return rc, h.cpu().numpy()


# ------------------------------------------------------------------ large stacks
@pytest.mark.parametrize("n,family", [(nhost.SIZE_A, f) for f in FAMILIES] + [(nhost.SIZE_B, "u12")]
                         + [(nhost.EDGE_ONE_LOOP, f) for f in FAMILIES])
def test_large_stack(dev, n, family):
    """Sizes at which the grids are capped (test_normalize_host: A = three coarse and two fine
    main-loop iterations, the single load behind them and both tails, two table steps; B = three
    table steps and four coarse iterations; 4 194 312 = one thread looping once).  The raw
    histograms of both passes as well as the percentiles: a vector counted twice or not at all
    moves a counter even where it moves no percentile."""
    x = _family(family, n, 11)
    t = _t(x, dev).view(1, 1, n)
    rc, coarse = _histogram(dev, t, n, 8, -1)
    assert rc == _lib.KCMC_OK
    np.testing.assert_array_equal(coarse, np.bincount(x >> 8, minlength=256))
    hb = int(np.percentile(x, 99.99)) >> 8
    rc, fine = _histogram(dev, t, n, 0, hb)
    assert rc == _lib.KCMC_OK
    np.testing.assert_array_equal(fine, np.bincount(x[x >> 8 == hb] & 255, minlength=256))
    for q in QS:
        assert stages.brightest_px(t, q) == np.percentile(x, q), q
    b = np.percentile(x, 99.99)
    out = torch.full((1, 1, n), 0xA5, dtype=torch.uint8, device=dev)  # a pixel left unwritten shows
    got = stages.max_scale_u8(t, b, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = _scaled(x, b)
    assert (want != 0xA5).mean() > 0.9
    np.testing.assert_array_equal(got.cpu().numpy().reshape(-1), want)


# ------------------------------------------------------------------ directed ranks
def _check_ranks(dev, s, k, lo_value=None, hi_value=None, seed=0):
    """np.percentile == brightest_px on the shuffled multiset ``s`` (sorted) for the two q whose
    floor rank is k, with gamma below and above 0.5 (numpy's two interpolation branches)."""
    s = np.asarray(s, np.uint16)
    assert (np.diff(s.astype(np.int64)) >= 0).all()
    if lo_value is not None:
        assert (s[k], s[k + 1]) == (lo_value, hi_value)
    x = np.random.default_rng(seed).permutation(s)
    t = _t(x, dev)
    for frac in (0.25, 0.75):
        q = nhost.q_for_rank(s.size, k, frac)
        want = np.percentile(x, q)
        if s[k] != s[k + 1]:
            assert s[k] < want < s[k + 1]
        assert stages.brightest_px(t, q) == want, (k, frac, q)


def _bin(rng, hb, count, lo=0, hi=256):
    return np.sort((hb << 8) | rng.integers(lo, hi, count))


def test_ranks_on_the_two_sides_of_a_coarse_boundary(dev):
    rng = np.random.default_rng(1)
    below, above = _bin(rng, 0x12, 700), _bin(rng, 0x13, 900)
    below[-1], above[0] = 0x12FF, 0x1300
    _check_ranks(dev, np.concatenate([_bin(rng, 0x03, 50), below, above]), 749, 0x12FF, 0x1300)
    # the last element of bin 0x12 and the first of bin 0x17: four empty coarse bins between them
    far = _bin(rng, 0x17, 300)
    s = np.concatenate([below, far, _bin(rng, 0x90, 41)])
    _check_ranks(dev, s, 699, 0x12FF, int(far[0]))
    # and with empty bins below the lower rank's bin as well (nothing under 0x12)
    _check_ranks(dev, s, 0, int(below[0]), int(below[1]))


def test_ranks_across_empty_fine_bins_of_one_coarse_bin(dev):
    rng = np.random.default_rng(2)
    lo, hi = _bin(rng, 0x12, 500, 0, 0x11), _bin(rng, 0x12, 400, 0xF0, 0x100)
    s = np.concatenate([_bin(rng, 0x00, 123), lo, hi, _bin(rng, 0xFF, 77)])
    assert lo[-1] < 0x1211 and hi[0] >= 0x12F0
    _check_ranks(dev, s, 123 + 499, int(lo[-1]), int(hi[0]))


def test_both_ranks_on_the_first_and_on_the_last_elements_of_a_bin(dev):
    """Runs of equal values: ranks k, k + 1 as the first two elements of a coarse bin and of a fine
    bin, as the last two, and one on each side of the border between two runs."""
    s = np.concatenate([np.full(5, 0x0042), np.full(6, 0x1234), np.full(4, 0x1235), np.full(7, 0x1301),
                        np.full(3, 0x2000)])
    starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    for a in starts:  # the first two elements of every run
        _check_ranks(dev, s, int(a), int(s[a]), int(s[a]))
    for e in list(starts[1:]) + [s.size]:  # the last two
        _check_ranks(dev, s, int(e) - 2, int(s[e - 1]), int(s[e - 1]))
    for e in starts[1:]:  # the last of one run, the first of the next
        _check_ranks(dev, s, int(e) - 1, int(s[e - 1]), int(s[e]))


def test_every_rank_of_a_multiset_in_bins_0_and_255_of_both_bytes(dev):
    values = (0, 255, 256, 0x01FF, 0x7F00, 0xFF00, 0xFFFE, 65535)
    s = np.repeat(np.asarray(values), (3, 2, 1, 2, 1, 3, 1, 4))
    for k in range(s.size - 1):
        _check_ranks(dev, s, k, seed=k)
    x = np.random.default_rng(9).permutation(s).astype(np.uint16)
    for q in QS:
        assert stages.brightest_px(_t(x, dev), q) == np.percentile(x, q), q
    for value in values:  # and each of them as every order statistic
        one = np.full(19, value, np.uint16)
        assert stages.brightest_px(_t(one, dev), 99.99) == np.percentile(one, 99.99) == value


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 15, 16, 17])
def test_tail_only_one_vector_and_vector_plus_tail(dev, n):
    rng = np.random.default_rng(n)
    for hi in (65536, 300):
        x = rng.integers(0, hi, n).astype(np.uint16)
        t = _t(x, dev).view(1, 1, n)
        for q in QS + (float(rng.uniform(0, 100)),):
            assert stages.brightest_px(t, q) == np.percentile(x, q), (hi, q)
        b = max(np.percentile(x, 99.99), 1.0)
        np.testing.assert_array_equal(stages.max_scale_u8(t, b).cpu().numpy(), _scaled(x, b).reshape(1, 1, n))


def test_constant_stacks(dev):
    """All zeros: the percentile is 0 (max-scaling by it is the caller's to refuse, as
    VideoAligner does: the expression divides by zero).  All 65535: every pixel scales to max_px."""
    zeros = np.zeros(1000, np.uint16)
    full = np.full(1003, 65535, np.uint16)
    for q in QS:
        assert stages.brightest_px(_t(zeros, dev), q) == np.percentile(zeros, q) == 0.0
        assert stages.brightest_px(_t(full, dev), q) == np.percentile(full, q) == 65535.0
    got = stages.max_scale_u8(_t(full, dev), 65535.0).cpu().numpy()
    np.testing.assert_array_equal(got, _scaled(full, 65535.0))
    assert (got == 255).all()
    np.testing.assert_array_equal(stages.max_scale_u8(_t(zeros, dev), 65535.0).cpu().numpy(), zeros.astype(np.uint8))


def test_part_list_with_empty_misaligned_and_every_tail(dev):
    rng = np.random.default_rng(3)
    lengths = [0, 1001] + [8 * int(rng.integers(1, 40)) + r for r in range(8)]
    xs = [rng.integers(0, 5000, m).astype(np.uint16) for m in lengths]
    parts = [_t(x, dev) for x in xs]
    holder = _t(np.concatenate([[7], xs[1]]).astype(np.uint16), dev)
    parts[1] = holder[1:]  # 2 bytes off the 16-byte grid: stages._aligned16 copies it
    assert parts[0].numel() == 0 and parts[1].data_ptr() % 16 == 2 and parts[1].is_contiguous()
    assert {p.numel() % 8 for p in parts[2:]} == set(range(8))
    whole = np.concatenate(xs)
    for q in QS + (73.0,):
        assert stages.brightest_px(parts, q) == np.percentile(whole, q), q
    assert stages.brightest_px(parts[1], 99.99) == np.percentile(xs[1], 99.99)
    with pytest.raises(ValueError, match="empty"):
        stages.brightest_px([parts[0]])


def test_percentile_outside_0_100_raises_where_numpy_raises(dev):
    x = np.arange(100, dtype=np.uint16)
    t = _t(x, dev)
    raised = 0
    for q in (-1.0, -1e-300, 100.001, 1e9, np.inf, -np.inf, np.nan, np.nextafter(100.0, 200.0),
              np.nextafter(0.0, -1.0), -0.0, np.nextafter(100.0, 0.0)):
        try:
            want = np.percentile(x, q)
        except ValueError:
            raised += 1
            with pytest.raises(ValueError, match="range"):
                stages.brightest_px(t, q)
        else:
            assert stages.brightest_px(t, q) == want, q
    assert raised >= 7


# ------------------------------------------------------------------ the C entries
def test_histogram_entry_every_shift_and_match(dev):
    rng = np.random.default_rng(4)
    n = 4099  # 512 vectors and a tail of 3
    x = np.concatenate([rng.integers(0, 256, 600), 0x1200 + rng.integers(0, 256, 1500),
                        0xFF00 + rng.integers(0, 256, 700), rng.integers(0x8000, 0xC000, n - 2800)])
    x = rng.permutation(x).astype(np.uint16)
    t = _t(x, dev)
    hi, lo = x >> 8, x & 255
    assert not (hi == 0x40).any() and (hi == 0x12).any()

    def want(shift, match):
        sel = np.ones(n, bool) if match < 0 else hi == match
        return np.bincount((hi if shift == 8 else lo)[sel], minlength=256)

    for shift, match in [(8, -1), (0, -1), (0, 0x12), (0, 0x40), (0, 0), (0, 255), (8, 0x12), (8, 0x40), (8, 0),
                         (8, 255)]:
        for fill in (0x5A5A5A5A5A5A5A5A, -1):  # out_hist is overwritten, never added to
            rc, got = _histogram(dev, t, n, shift, match, fill)
            assert rc == _lib.KCMC_OK, (shift, match)
            np.testing.assert_array_equal(got, want(shift, match), err_msg=str((shift, match)))
    assert want(8, 0x12)[0x12] == (hi == 0x12).sum() == want(8, 0x12).sum()
    for src in (t, None):  # n == 0: all 256 counters cleared, src not read
        rc, got = _histogram(dev, src, 0, 8, -1)
        assert rc == _lib.KCMC_OK and not got.any()


def test_histogram_entry_refuses_bad_arguments(dev):
    t = _t(np.arange(64, dtype=np.uint16), dev)
    assert t.data_ptr() % 16 == 0
    for shift in (1, 4, 7, 16, -8):
        assert _histogram(dev, t, 64, shift, -1)[0] == _lib.KCMC_EINVAL, shift
    assert _histogram(dev, t, 64, 8, 256)[0] == _lib.KCMC_EINVAL
    assert _histogram(dev, t, 64, 8, -1, out_null=True)[0] == _lib.KCMC_EINVAL
    assert _histogram(dev, t, 48, 8, -1, src_ptr=t.data_ptr() + 2)[0] == _lib.KCMC_EINVAL
    assert _histogram(dev, None, 64, 8, -1)[0] == _lib.KCMC_EINVAL  # NULL src with n > 0
    assert b"kcmc_histogram_u16" in _lib.load().kcmc_last_error()
    rc, got = _histogram(dev, t, 64, 8, -1)  # and the entry works after the refusals
    assert rc == _lib.KCMC_OK and got[0] == 64 and got.sum() == 64


def test_table_entry_refuses_bad_arguments_and_leaves_dst_alone_for_n_0(dev):
    n = 100
    x = np.random.default_rng(5).integers(0, 65536, n).astype(np.uint16)
    src = _t(np.concatenate([x, np.zeros(8, np.uint16)]), dev)
    lut = _t(np.concatenate([stages.max_scale_lut(40000.0), np.zeros(16, np.uint8)]), dev)
    buf = torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device=dev)
    dst = buf[64:64 + n]
    assert src.data_ptr() % 16 == 0 and lut.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    entry, ctx, stream = _lib.load().kcmc_lut_u16_to_u8, stages._ctx(dev).handle, stages._stream(dev)
    good = (src.data_ptr(), lut.data_ptr(), dst.data_ptr())
    for i in range(3):
        for bad in (good[i] + 2, good[i] + 8, 0):  # off the 16-byte grid, NULL
            a = list(good)
            a[i] = bad
            assert entry(ctx, P(a[0]), n, P(a[1]), P(a[2]), stream) == _lib.KCMC_EINVAL, (i, bad)
    assert entry(ctx, P(good[0]), 0, P(good[1]), P(good[2]), stream) == _lib.KCMC_OK
    assert (buf.cpu().numpy() == 0xA5).all()
    assert entry(ctx, P(good[0]), n, P(good[1]), P(good[2]), stream) == _lib.KCMC_OK
    flat = buf.cpu().numpy()
    np.testing.assert_array_equal(flat[64:64 + n], _scaled(x, 40000.0))
    assert (flat[:64] == 0xA5).all() and (flat[64 + n:] == 0xA5).all()


# ------------------------------------------------------------------ max_scale_u8's plumbing
def test_max_scale_every_length_mod_16(dev):
    rng = np.random.default_rng(6)
    for n in range(0, 50):
        x = rng.integers(0, 65536, n).astype(np.uint16)
        got = stages.max_scale_u8(_t(x, dev), 30000.5)
        assert got.dtype == torch.uint8 and got.shape == (n,)
        np.testing.assert_array_equal(got.cpu().numpy(), _scaled(x, 30000.5), err_msg=str(n))


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 8, 16), (1, 1, 1)])
def test_max_scale_into_an_out_view_one_byte_into_its_buffer(dev, shape):
    """data_ptr % 16 == 1: the kernel writes a temporary and the wrapper copies it in."""
    x = np.random.default_rng(7).integers(0, 65536, shape).astype(np.uint16)
    n = x.size
    for off in (1, 0):
        buf = torch.full((off + n + 33,), 0xA5, dtype=torch.uint8, device=dev)
        view = buf[off:off + n].view(*shape)
        assert view.data_ptr() % 16 == off
        got = stages.max_scale_u8(_t(x, dev), 41234.5, out=view)
        assert got.data_ptr() == view.data_ptr()
        flat = buf.cpu().numpy()
        np.testing.assert_array_equal(flat[off:off + n].reshape(shape), _scaled(x, 41234.5))
        assert (flat[:off] == 0xA5).all() and (flat[off + n:] == 0xA5).all()


def test_max_scale_refuses_a_wrong_out(dev):
    t = _t(np.zeros((2, 3, 4), np.uint16), dev)
    with pytest.raises(ValueError, match="shape"):
        stages.max_scale_u8(t, 100.0, out=torch.empty((2, 3, 5), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="shape"):
        stages.max_scale_u8(t, 100.0, out=torch.empty((24,), dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError, match="dtype"):
        stages.max_scale_u8(t, 100.0, out=torch.empty((2, 3, 4), dtype=torch.int8, device=dev))
    with pytest.raises(TypeError, match="dtype"):
        stages.max_scale_u8(t.to(torch.int32), 100.0)
    with pytest.raises(ValueError, match="contiguous"):
        stages.max_scale_u8(t, 100.0, out=torch.empty((2, 3, 8), dtype=torch.uint8, device=dev)[:, :, ::2])


@pytest.mark.parametrize("max_px", nhost.SCALE_MAX_PX)
@pytest.mark.parametrize("b", nhost.SCALE_B)
def test_max_scale_parameters(dev, b, max_px):
    """b fractional, b = 0.5 (every nonzero pixel clips), b = 65535, max_px other than 255: over
    every uint16 value and a tail."""
    x = np.concatenate([np.arange(65536), [0, 1, 65535, 32768, 4095]]).astype(np.uint16)
    got = stages.max_scale_u8(_t(x, dev), b, max_px=max_px).cpu().numpy()
    np.testing.assert_array_equal(got, _scaled(x, b, max_px))
    assert got.max() == max_px and got[0] == 0


# ------------------------------------------------------------------ streams
def test_on_a_side_stream(dev):
    x = _family("u12", 300007, 8)
    t = _t(x, dev)
    torch.cuda.synchronize(dev)
    b1 = stages.brightest_px(t)
    u1 = stages.max_scale_u8(t, b1)
    s2 = torch.cuda.Stream(dev)
    with torch.cuda.stream(s2):
        b2 = stages.brightest_px(t)
        b50 = stages.brightest_px(t, 50.0)
        u2 = stages.max_scale_u8(t, b2)
    s2.synchronize()
    assert b1 == b2 == np.percentile(x, 99.99) and b50 == np.percentile(x, 50.0)
    want = _scaled(x, b1)
    np.testing.assert_array_equal(u1.cpu().numpy(), want)
    np.testing.assert_array_equal(u2.cpu().numpy(), want)

"""Piecewise-rigid correction on the host: the numpy restatement of the field warp
(``ref_warp_field``, the yardstick of tests/test_gpu_piecewise.py), the fixed-point weights,
kcmc_amd.piecewise's host functions against restatements written here, the binding and the
refusals.  The semantics are build-defined (include/kcmc.h): this file pins them."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import oracle
from kcmc_amd import VideoAligner, _lib, piecewise

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kcmc.h")


# ------------------------------------------------------------------ the restatement
def axis_weights(L, g):
    """(k0 [L], w [L]) of every pixel index along an axis of length L with g nodes."""
    p = np.arange(L, dtype=np.int64)
    if g == 1:
        return np.zeros(L, np.int64), np.zeros(L, np.int64)
    num = np.clip((2 * p + 1) * g - L, 0, 2 * L * (g - 1))
    k0 = np.minimum(num // (2 * L), g - 2)
    w = ((num - k0 * 2 * L) * 1024 + L) // (2 * L)
    return k0, w


def interp_field(q, H, W):
    """val [H, W, 2] int64 of q [gy, gx, 2]: vertical step first, then horizontal, arithmetic
    right shifts (numpy's >> on signed integers)."""
    q = np.asarray(q).astype(np.int64)
    gy, gx = q.shape[:2]
    i0, wy = axis_weights(H, gy)
    j0, wx = axis_weights(W, gx)
    i1, j1 = np.minimum(i0 + 1, gy - 1), np.minimum(j0 + 1, gx - 1)
    v = (q[i0] * (1024 - wy)[:, None, None] + q[i1] * wy[:, None, None] + 512) >> 10        # [H, gx, 2]
    return (v[:, j0] * (1024 - wx)[None, :, None] + v[:, j1] * wx[None, :, None] + 512) >> 10


def _invert(M):
    """OpenCV warpAffine's in-place inversion, operation by operation."""
    M = np.array(M, np.float64).reshape(6)
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return M


def _ref_one(img, M, q, inverse_map):
    H, W = img.shape
    if np.isnan(np.asarray(M, np.float64)).any():
        return np.zeros((H, W), np.uint16)
    m = np.asarray(M, np.float64).reshape(6) if inverse_map else _invert(M)
    if np.isnan(m).any():
        return np.zeros((H, W), np.uint16)
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    adelta = np.rint(m[0] * x * 1024).astype(np.int64)
    bdelta = np.rint(m[3] * x * 1024).astype(np.int64)
    X0 = np.rint((m[1] * y + m[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((m[4] * y + m[5]) * 1024).astype(np.int64) + 16
    val = interp_field(q, H, W)
    X = X0[:, None] + adelta[None, :] + val[..., 0]
    Y = Y0[:, None] + bdelta[None, :] + val[..., 1]
    sx, sy = np.clip(X >> 10, -32768, 32767), np.clip(Y >> 10, -32768, 32767)
    fx, fy = ((X >> 5) & 31).astype(np.float32), ((Y >> 5) & 31).astype(np.float32)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.where(ok, img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0).astype(np.float32)

    one, s = np.float32(1.0), np.float32(1.0 / 32.0)
    ax, bx, ay, by = one - fx * s, fx * s, one - fy * s, fy * s  # exact in float32
    w0, w1, w2, w3 = ay * ax, ay * bx, by * ax, by * bx          # OpenCV's BilinearTab_f (exact)
    acc = ((tap(sy, sx) * w0 + tap(sy, sx + 1) * w1) + tap(sy + 1, sx) * w2) + tap(sy + 1, sx + 1) * w3
    assert acc.dtype == np.float32
    return np.clip(np.rint(acc.astype(np.float64)), 0, 65535).astype(np.uint16)


def ref_warp_field(frames, M, q, grid=None, inverse_map=False):
    """Section 1 of the definition for frames [F, H, W] u16, M [F, 2, 3] f64, q [F, gy, gx, 2]."""
    frames, M, q = np.asarray(frames), np.asarray(M, np.float64), np.asarray(q)
    if grid is not None:
        assert tuple(q.shape[1:3]) == tuple(grid)
    return np.stack([_ref_one(frames[f], M[f], q[f], inverse_map) for f in range(frames.shape[0])])


def rot_about_centre(deg, H, W, tx=0.0, ty=0.0, scale=1.0):
    a = math.radians(deg)
    c, s = scale * math.cos(a), scale * math.sin(a)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty]])


def random_frames(F, H, W, seed, hi=65536, n_sat=5):
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, hi, (F, H, W)).astype(np.uint16)
    if n_sat:
        fr[rng.integers(0, F, n_sat), rng.integers(0, H, n_sat), rng.integers(0, W, n_sat)] = 65535
    return fr


@pytest.mark.parametrize("H,W", [(61, 75), (56, 136)])
def test_restatement_with_a_zero_field_is_the_oracle_warp(H, W):
    fr = random_frames(1, H, W, seed=H)
    maps = [np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([[1.0, 0, 3.3], [0, 1.0, -2.7]]),
            rot_about_centre(2.0, H, W, 1.4, -0.6), rot_about_centre(0.0, H, W, scale=1.03)]
    for g in ((1, 1), (3, 4)):
        q = np.zeros((1,) + g + (2,), np.int32)
        for M in maps:
            for inv in (False, True):
                np.testing.assert_array_equal(ref_warp_field(fr, M[None], q, g, inverse_map=inv)[0],
                                              oracle.warp_affine_u16(fr[0], M, inverse_map=inv))


@pytest.mark.parametrize("L,g", [(75, 1), (75, 2), (75, 5), (136, 16), (16, 16), (7, 7)])
def test_weights(L, g):
    k0, w = axis_weights(L, g)
    assert k0.min() >= 0 and k0.max() <= max(g - 2, 0)
    assert w.min() >= 0 and w.max() <= 1024
    assert (np.diff(k0 * 1024 + w) >= 0).all()  # the position in node units never goes back
    # along x (a [1, g] grid on a 1 x L frame) and along y (a [g, 1] grid on an L x 1 frame)
    for c in (-8192, -1, 0, 1, 8191):
        assert (interp_field(np.full((1, g, 2), c), 1, L) == c).all()
        assert (interp_field(np.full((g, 1, 2), c), L, 1) == c).all()
    rng = np.random.default_rng(L * 17 + g)
    inc = np.cumsum(rng.integers(0, 3000, g)) - 7000
    qx = np.stack([inc, inc[::-1]], -1)[None]          # x increasing, y decreasing along the axis
    vx = interp_field(qx, 1, L)[0]
    assert (np.diff(vx[:, 0]) >= 0).all() and (np.diff(vx[:, 1]) <= 0).all()
    assert vx[:, 0].min() >= inc.min() and vx[:, 0].max() <= inc.max()
    vy = interp_field(qx.reshape(g, 1, 2), L, 1)[:, 0]
    np.testing.assert_array_equal(vy, vx)  # the same weights along either axis


def test_device_weight_formula_matches_on_a_2d_grid():
    """Vertical first, then horizontal: a 2-D field against a per-pixel scalar evaluation."""
    H, W, gy, gx = 23, 31, 3, 4
    q = np.random.default_rng(5).integers(-9000, 9000, (gy, gx, 2))
    val = interp_field(q, H, W)
    (i0, wy), (j0, wx) = axis_weights(H, gy), axis_weights(W, gx)
    for y, x in ((0, 0), (11, 17), (22, 30), (5, 29), (20, 3)):
        for c in range(2):
            va = (int(q[i0[y], j0[x], c]) * (1024 - wy[y]) + int(q[i0[y] + 1, j0[x], c]) * wy[y] + 512) >> 10
            vb = (int(q[i0[y], j0[x] + 1, c]) * (1024 - wy[y]) + int(q[i0[y] + 1, j0[x] + 1, c]) * wy[y] + 512) >> 10
            assert val[y, x, c] == (va * (1024 - wx[x]) + vb * wx[x] + 512) >> 10


# ------------------------------------------------------------------ host functions
def test_node_centres_and_membership_edges():
    H, W, grid = 200, 264, (2, 3)
    cy, cx = piecewise.node_centres(H, W, grid)
    np.testing.assert_array_equal(cx, [(j + 0.5) * W / 3 - 0.5 for j in range(3)])
    np.testing.assert_array_equal(cy, [(i + 0.5) * H / 2 - 0.5 for i in range(2)])
    hx, hy = 1.0 * W / 3, 1.0 * H / 2
    kp = np.array([[cx[1] + hx, cy[0]],                      # on the right edge of cell (0, 1): inside
                   [cx[1] + hx + 1e-9, cy[0]],                # just past it: outside
                   [cx[1], cy[0] - hy],                      # on the upper edge: inside
                   [cx[1], cy[0] - hy - 1e-9],
                   [cx[0] - hx, cy[1] + hy],                 # a corner of cell (1, 0)
                   [10.0, 10.0]])
    m = piecewise.cell_membership(kp, H, W, grid, 1.0).reshape(2, 3, -1)
    assert m[0, 1].tolist() == [True, False, True, False, False, False]
    assert m[1, 0, 4] and not m[0, 0, 4]
    assert m[:, :, 5].tolist() == [[True, False, False], [False, False, False]]
    # restated per point
    rng = np.random.default_rng(2)
    kp = np.stack([rng.uniform(0, W, 80), rng.uniform(0, H, 80)], 1)
    got = piecewise.cell_membership(kp, H, W, grid, 0.75).reshape(2, 3, -1)
    for i in range(2):
        for j in range(3):
            want = [abs(x - cx[j]) <= 0.75 * W / 3 and abs(y - cy[i]) <= 0.75 * H / 2 for x, y in kp]
            assert got[i, j].tolist() == want


def test_acceptance_rule():
    for n, thr in ((5, 3), (6, 3), (7, 4)):
        for ni in (2, 3, 4):
            assert bool(piecewise.accept_fit(n, ni, True)) == (ni >= max(3, (n + 1) // 2)) == (ni >= thr)
            assert not piecewise.accept_fit(n, ni, False)
    np.testing.assert_array_equal(piecewise.accept_fit([5, 6, 7, 7], [3, 2, 3, 4], [True] * 4),
                                  [True, False, False, True])


def _rigid(deg, tx, ty):
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), tx], [math.sin(a), math.cos(a), ty]])


def test_residual_field_against_hand_made_models():
    H, W, grid = 96, 160, (2, 2)
    cy, cx = piecewise.node_centres(H, W, grid)
    G = _rigid(0.7, 2.5, -1.25)
    cells = np.stack([np.stack([_rigid(0.7, 2.5, -1.25), _rigid(0.2, 3.0, -1.0)]),
                      np.stack([_rigid(1.0, 14.0, 0.0), np.full((2, 3), np.nan)])])
    fitted = np.array([[True, True], [True, True]])
    r = piecewise.residual_field(cells, fitted, G, H, W, grid, 8.0)
    gi = oracle.invert_affine(G)
    for i in range(2):
        for j in range(2):
            if np.isnan(cells[i, j]).any():
                want = np.zeros(2)                      # NaN model: the node follows the global one
            else:
                ai = oracle.invert_affine(cells[i, j])
                want = np.array([ai[0, 0] * cx[j] + ai[0, 1] * cy[i] + ai[0, 2] - (gi[0, 0] * cx[j] + gi[0, 1] * cy[i] + gi[0, 2]),
                                 ai[1, 0] * cx[j] + ai[1, 1] * cy[i] + ai[1, 2] - (gi[1, 0] * cx[j] + gi[1, 1] * cy[i] + gi[1, 2])])
                if np.abs(want).max() > 8.0:
                    want = np.zeros(2)
            np.testing.assert_array_equal(r[i, j], want)
    assert (r[0, 0] == 0).all() and (r[0, 1] != 0).all()
    assert (r[1, 0] == 0).all()  # |r| ~ 11.5 px > MAX_RESIDUAL: rejected
    assert (piecewise.residual_field(cells, fitted, G, H, W, grid, 20.0)[1, 0] != 0).all()
    # not fitted: zero whatever the parameters say
    nf = piecewise.residual_field(cells, np.array([[True, False], [True, True]]), G, H, W, grid, 8.0)
    assert (nf[0, 1] == 0).all()
    # exactly at MAX_RESIDUAL is kept (the comparison is "greater than")
    m = np.abs(r[0, 1]).max()
    assert (piecewise.residual_field(cells, fitted, G, H, W, grid, m)[0, 1] != 0).all()
    assert (piecewise.residual_field(cells, fitted, G, H, W, grid, np.nextafter(m, 0))[0, 1] == 0).all()
    # batched over frames
    rb = piecewise.residual_field(np.stack([cells, cells]), np.stack([fitted, fitted]), np.stack([G, G]), H, W, grid)
    np.testing.assert_array_equal(rb[1], r)


def test_host_inversion_is_the_oracle_inversion():
    rng = np.random.default_rng(8)
    for _ in range(20):
        M = _rigid(rng.uniform(-5, 5), rng.uniform(-9, 9), rng.uniform(-9, 9)) * rng.uniform(0.9, 1.1)
        np.testing.assert_array_equal(piecewise.invert_affine(M), oracle.invert_affine(M))
        np.testing.assert_array_equal(_invert(M).reshape(2, 3), oracle.invert_affine(M))
    np.testing.assert_array_equal(piecewise.invert_affine(np.zeros((2, 3))), oracle.invert_affine(np.zeros((2, 3))))


def test_interpolate_fields_gaps():
    F = 10
    rng = np.random.default_rng(4)
    r = rng.normal(0, 2, (F, 2, 3, 2))
    have = np.zeros(F, bool)
    have[[2, 3, 6]] = True  # leading gap 0-1, inner gap 4-5, trailing gap 7-9
    out = piecewise.interpolate_fields(r, have)
    np.testing.assert_array_equal(out[[2, 3, 6]], r[[2, 3, 6]])
    np.testing.assert_array_equal(out[0], r[2])
    np.testing.assert_array_equal(out[1], r[2])
    for f in (7, 8, 9):
        np.testing.assert_array_equal(out[f], r[6])
    for e in np.ndindex(2, 3, 2):
        np.testing.assert_array_equal(out[(slice(None),) + e], np.interp(np.arange(F), [2, 3, 6], r[(slice(None),) + e][[2, 3, 6]]))
    np.testing.assert_allclose(out[4], r[3] + (r[6] - r[3]) / 3, rtol=0, atol=1e-12)
    assert (piecewise.interpolate_fields(r, np.zeros(F, bool)) == 0).all()


def test_quantise_rounds_half_to_even():
    r = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.49, -2.51]) / 1024
    np.testing.assert_array_equal(piecewise.quantise(r), [0, 2, 2, 0, -2, 3, -3])
    assert piecewise.quantise(r).dtype == np.int32
    np.testing.assert_array_equal(piecewise.quantise(np.array([1.0, -8.0])), [1024, -8192])


def test_fields_from_fits_places_and_interpolates():
    """Sample frames at f * rate, frames without a global model and the non-sample frames
    interpolated; a cell that took the whole list over gives exactly zero."""
    H, W, grid, rate = 96, 160, (2, 2), 2
    S = 4
    G = np.stack([_rigid(0.1 * f, f, -f) for f in range(S)])
    G[2] = np.nan
    params = np.broadcast_to(G[:, None, None], (S, 2, 2, 2, 3)).copy()  # every cell = the global model ...
    params[0, 0, 1] = _rigid(0.0, 0.5, -0.25)                          # ... except one
    params[3, 1, 0] = _rigid(0.3, 3.0, -2.0)
    fitted = np.ones((S, 2, 2), bool)
    fitted[2] = False
    fits = piecewise.CellFits(np.full((S, 2, 2), 9, np.int32), fitted, params, np.full((S, 2, 2), -1, np.int32),
                              np.zeros((S, 2, 2), bool))
    q = piecewise.fields_from_fits(fits, G, 7, rate, H, W, grid, 8.0)
    assert q.shape == (7, 2, 2, 2) and q.dtype == np.int32
    r = np.zeros((8, 2, 2, 2))
    for f in (0, 1, 3):
        r[f * rate] = piecewise.residual_field(params[f], fitted[f], G[f], H, W, grid, 8.0)
    have = np.zeros(8, bool)
    have[[0, 2, 6]] = True
    np.testing.assert_array_equal(q, piecewise.quantise(piecewise.interpolate_fields(r, have))[:7])
    assert (q[0, 1] == 0).all() and (q[0, 0, 1] != 0).any() and (q[6, 1, 0] != 0).any()
    assert (q[4, 1, 0] == piecewise.quantise(r[6, 1, 0] / 2)).all()  # frame 4 (sample 2: no model) is half-way 2 -> 6


def cell_stack(seed, F=6, n_tpl=60, H=200, W=264):
    """Template points, and per frame their positions under a global rigid motion plus a
    per-quadrant translation of up to 1.5 px and 0.2 px noise; every frame lists a shuffled
    subset of the template points."""
    rng = np.random.default_rng(seed)
    kp_tpl = np.stack([rng.uniform(0, W, n_tpl), rng.uniform(0, H, n_tpl)], 1)
    kp_ordered = np.zeros((F, n_tpl, 2))
    lists = []
    for f in range(F):
        a = math.radians(rng.uniform(-0.5, 0.5))
        R = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
        quad = (kp_tpl[:, 0] >= W / 2).astype(int) + 2 * (kp_tpl[:, 1] >= H / 2).astype(int)
        extra = rng.uniform(-1.5, 1.5, (4, 2))[quad]
        kp_ordered[f] = kp_tpl @ R.T + rng.uniform(-4, 4, 2) + extra + rng.normal(0, 0.2, (n_tpl, 2))
        lists.append(rng.permutation(n_tpl)[:rng.integers(45, n_tpl + 1)].astype(np.int32))
    off = np.zeros(F + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return kp_tpl, kp_ordered, lists, off


def restate_cells(kp_tpl, kp_ordered, lists, G, H, W, grid, min_points=6, window=1.0, max_residual=8.0):
    gy, gx = grid
    F = len(lists)
    cy, cx = [(i + 0.5) * H / gy - 0.5 for i in range(gy)], [(j + 0.5) * W / gx - 0.5 for j in range(gx)]
    points, fitted = np.zeros((F, gy, gx), np.int32), np.zeros((F, gy, gx), bool)
    params, r = np.full((F, gy, gx, 2, 3), np.nan), np.zeros((F, gy, gx, 2))
    for f in range(F):
        own = not np.isnan(G[f]).any()
        gi = oracle.invert_affine(G[f]) if own else None
        for i in range(gy):
            for j in range(gx):
                cell = [q for q in lists[f] if abs(kp_tpl[q, 0] - cx[j]) <= window * W / gx
                        and abs(kp_tpl[q, 1] - cy[i]) <= window * H / gy]
                n = points[f, i, j] = len(cell)
                if n < min_points or not own:
                    continue
                if n == len(lists[f]):
                    params[f, i, j], fitted[f, i, j] = G[f], True
                else:
                    p, _, _, n_inl = oracle.ransac_rigid(kp_ordered[f, cell], kp_tpl[cell], 1000, 2.0, 42)
                    if np.isfinite(p).all() and n_inl >= max(3, (n + 1) // 2):
                        params[f, i, j], fitted[f, i, j] = p, True
                if fitted[f, i, j]:
                    ai = oracle.invert_affine(params[f, i, j])
                    v = np.array([ai[0, 0] * cx[j] + ai[0, 1] * cy[i] + ai[0, 2] - (gi[0, 0] * cx[j] + gi[0, 1] * cy[i] + gi[0, 2]),
                                  ai[1, 0] * cx[j] + ai[1, 1] * cy[i] + ai[1, 2] - (gi[1, 0] * cx[j] + gi[1, 1] * cy[i] + gi[1, 2])])
                    if np.isfinite(v).all() and np.abs(v).max() <= max_residual:
                        r[f, i, j] = v
    return points, fitted, params, r


CELL_SEED = 11  # keeps r * 1024 of the restatement clear of half-integers (asserted below)


@pytest.mark.parametrize("grid", [(2, 2), (3, 4)])
def test_cell_restatement_premises(grid):
    """What tests/test_gpu_piecewise.py relies on, checked on the restatement alone: most cells
    run a fit of their own, most fits are accepted, the per-quadrant motion shows in the
    residuals, and at most 1 % of the field's entries lie within 1e-4 of a rounding tie."""
    H, W = 200, 264
    kp_tpl, kp_ordered, lists, off = cell_stack(CELL_SEED)
    G = np.stack([oracle.ransac_rigid(kp_ordered[f, l], kp_tpl[l])[0] for f, l in enumerate(lists)])
    assert np.isfinite(G).all()
    G[4] = np.nan
    points, fitted, params, r = restate_cells(kp_tpl, kp_ordered, lists, G, H, W, grid)
    assert (points[4] > 0).any() and not fitted[4].any()
    assert (points >= 6).sum() >= 0.75 * points.size and fitted.sum() >= 0.5 * (points >= 6).sum()
    assert np.abs(r).max() > 0.25
    x = piecewise.interpolate_fields(r, ~np.isnan(G.reshape(len(lists), 6)).any(1)) * 1024
    band = np.abs((x - np.floor(x)) - 0.5) < 1e-4
    assert band.sum() <= 0.01 * band.size


# ------------------------------------------------------------------ binding and header
def test_binding_and_header():
    assert "kcmc_warp_field_u16" in _lib.EXPORTED_SYMBOLS and "kcmc_warp_field_u16" in _lib._SIGNATURES
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+kcmc_warp_field_u16\s*\(", src)
    assert _lib.ABI_VERSION == 2 and re.search(r"#define\s+KCMC_ABI_VERSION\s+2\b", src)
    L = _lib.load()
    assert hasattr(L, "kcmc_warp_field_u16") and L.kcmc_abi_version() == 2


def test_entry_validates_before_touching_the_gpu():
    L = _lib.load()
    P = ctypes.c_void_p
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data_as(P)
    p2 = np.zeros(64, np.int64).ctypes.data_as(P)
    fake_ctx = P(buf.ctypes.data)  # never dereferenced: the argument checks come first
    f = L.kcmc_warp_field_u16

    def bad(*args, word):
        assert f(*args) == _lib.KCMC_EINVAL
        assert word in L.kcmc_last_error(), L.kcmc_last_error()

    bad(None, p, p2, p, p, 1, 8, 8, 2, 2, 0, None, word=b"ctx")
    bad(fake_ctx, None, p2, p, p, 1, 8, 8, 2, 2, 0, None, word=b"NULL")
    bad(fake_ctx, p, None, p, p, 1, 8, 8, 2, 2, 0, None, word=b"NULL")
    bad(fake_ctx, p, p2, None, p, 1, 8, 8, 2, 2, 0, None, word=b"NULL")
    bad(fake_ctx, p, p2, p, None, 1, 8, 8, 2, 2, 0, None, word=b"NULL")
    bad(fake_ctx, p, p2, p, p, 1, 0, 8, 1, 1, 0, None, word=b"H, W")
    bad(fake_ctx, p, p2, p, p, 1, 8, 0, 1, 1, 0, None, word=b"H, W")
    bad(fake_ctx, p, p2, p, p, -1, 8, 8, 1, 1, 0, None, word=b"n_frames")
    for gy, gx in ((0, 1), (1, 0), (17, 1), (1, 17), (9, 2), (2, 9), (-1, -1)):
        bad(fake_ctx, p, p2, p, p, 1, 8, 8, gy, gx, 0, None, word=b"grid")
    bad(fake_ctx, p, p, p, p, 1, 8, 8, 2, 2, 0, None, word=b"in-place")
    assert f(fake_ctx, p, p2, p, p, 0, 8, 8, 2, 2, 0, None) == _lib.KCMC_OK  # no frames: nothing to do
    assert f(fake_ctx, p, p2, p, p, 0, 8, 8, 0, 2, 0, None) == _lib.KCMC_EINVAL  # ... but the grid is still checked


# ------------------------------------------------------------------ refusals
def _cls(**kw):
    return type("VA", (VideoAligner,), kw)


def _both(cls, exc, match=None):
    with pytest.raises(exc, match=match):
        cls().align_images(None, 10, "orb", 30)
    with pytest.raises(exc, match=match):
        cls().align_keypoints(None, None, None, None, None, 10)


def test_refusals_come_before_the_inputs_are_looked_at():
    _both(_cls(PIECEWISE_GRID=(2, 2), RANSAC_MODEL="projective"), NotImplementedError, "projective")
    _both(_cls(PIECEWISE_GRID=(2, 2), QUALITY_METRICS=True), NotImplementedError, "QUALITY_METRICS")
    _both(_cls(PIECEWISE_GRID=(2, 2), TEMPLATE_REFINE_ITERS=1), (NotImplementedError, ValueError))
    with pytest.raises(NotImplementedError, match="QUALITY_METRICS"):
        _cls(PIECEWISE_GRID=(2, 2), TEMPLATE_REFINE_ITERS=1)().align_images(None, 10, "orb", 30)
    for grid in ((0, 2), (2, 17), (2,), (2, 2, 2), 4, (1.5, 2), "22"):
        _both(_cls(PIECEWISE_GRID=grid), ValueError, "PIECEWISE_GRID")
    _both(_cls(PIECEWISE_GRID=(2, 2), PIECEWISE_MIN_POINTS=2), ValueError, "PIECEWISE_MIN_POINTS")
    rgb = np.zeros((3, 8, 8, 3), np.uint16)
    with pytest.raises(NotImplementedError, match="grayscale"):
        _cls(PIECEWISE_GRID=(2, 2))().align_images(rgb, 10, "orb", 30)
    with pytest.raises(NotImplementedError, match="grayscale"):
        _cls(PIECEWISE_GRID=(2, 2))().align_keypoints(rgb, None, None, None, None, 10)


def test_paths_without_the_mode_refuse_the_grid():
    from kcmc_amd import multidevice, pipeline

    cfg = pipeline.AlignConfig(n_kp_global=10, piecewise_grid=(2, 2))
    with pytest.raises(NotImplementedError, match="OverlappedSlabs"):
        pipeline.OverlappedSlabs(0, cfg)
    with pytest.raises(NotImplementedError, match="align_streamed"):
        pipeline.align_streamed(None, None, cfg)
    with pytest.raises(NotImplementedError, match="align_split"):
        multidevice.align_split([None], [None], cfg)
    pipeline.refuse_piecewise(pipeline.AlignConfig(n_kp_global=10), "anything")  # grid off: nothing


def test_grid_off_leaves_the_attributes_none_and_the_config_default():
    va = VideoAligner()
    assert va.patch_residuals is None and va.patch_points is None and va.patch_fitted is None
    assert VideoAligner.PIECEWISE_GRID is None and VideoAligner.PIECEWISE_WINDOW == 1.0
    assert VideoAligner.PIECEWISE_MIN_POINTS == 6 and VideoAligner.PIECEWISE_MAX_RESIDUAL == 8.0
    cfg = va._config(40)
    assert cfg.piecewise_grid is None and cfg.piecewise_window == 1.0
    assert cfg.piecewise_min_points == 6 and cfg.piecewise_max_residual == 8.0
    assert _cls(PIECEWISE_GRID=[3, 4])()._config(40).piecewise_grid == (3, 4)

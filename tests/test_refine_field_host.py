"""The non-rigid intensity refinement (kcmc_amd.refine_field, csrc/refine_tiles.hip) restated in
numpy / Python integers, and the host half of the module checked against the restatement
(no GPU).

Build-defined semantics (the reference has no such mode), pinned here:
  edges    edge k along x = clamp(k * W // (2 gx), x0, x1), k = 0 .. 2 gx; y alike: two tiles per
           grid cell and axis, clipped to the rectangle (y0, y1, x0, x1)
  sums     per frame a, reference b and tile: (Sa, Saa, Sab, Sagx, Sagy), gx = b(x + 1) - b(x - 1),
           gy = b(y + 1) - b(y - 1); an index outside the stack and an empty tile give zeros
  windows  node (i, j): tile rows 2i - 1 .. 2i + 2, tile columns 2j - 1 .. 2j + 2, clipped to the
           tiling; the restatement sums the window's PIXELS, the module its tiles' sums
  solve    regressors (b, 1, gx, gy) on the window: G p = (Sab, Sa, Sagx, Sagy) solved for
           p - (1, 0, 0, 0) with the right-hand side differenced in exact integers, G scaled by
           the powers of two 2^-rint(log2(G_ii) / 2), one float64 solve per node for all
           frames, t = -2 (p_2, p_3) / (1 + p_0); (0, 0) for an empty window, a diagonal entry
           <= 0, a singular matrix or one with 1 / cond_2 < 1e-8, alpha <= 0 or a non-finite
           value; else scaled by min(1, max_step / max(|tx|, |ty|))
  field    q = rint(1024 L^-1 u), L^-1 the linear part of the warp's inversion of the frame's map
  pass     per iteration: mean image of the sample frames with a model of their own, valid
           region shrunk by ceil(iters * max_step), sums, node steps, q = q_prev + q_step, the
           candidates warped from the SOURCE frames by the field warp, kept where r rose
The restatement shares no code with kcmc_amd.refine_field; tests/test_gpu_refine_field.py imports it.
"""
import ctypes
import math
import os

import numpy as np
import pytest

import oracle
import test_fallback_host as fhost
import test_piecewise_host as phost
import test_quality_host as qhost
import test_refine_host as rhost
from kcmc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def ref_tile_edges(H, W, grid, rect):
    gy, gx = grid
    y0, y1, x0, x1 = rect
    rows = [min(max(k * H // (2 * gy), y0), y1) for k in range(2 * gy + 1)]
    cols = [min(max(k * W // (2 * gx), x0), x1) for k in range(2 * gx + 1)]
    return rows, cols


def _terms(frame, ref, ya, yb, xa, xb):
    """(a, a a, a b, a gx, a gy) of the pixels [ya, yb) x [xa, xb) as int64 [5, h, w]."""
    B = np.asarray(ref).astype(np.int64)
    a = np.asarray(frame)[ya:yb, xa:xb].astype(np.int64)
    b = B[ya:yb, xa:xb]
    gx = B[ya:yb, xa + 1:xb + 1] - B[ya:yb, xa - 1:xb - 1]
    gy = B[ya + 1:yb + 1, xa:xb] - B[ya - 1:yb - 1, xa:xb]
    return np.stack([a, a * a, a * b, a * gx, a * gy])


def ref_tile_sums(frames, idx, ref, rows, cols):
    """[len(idx), ty, tx, 5] int64: what the entry point writes (a tile has fewer than 2^31
    pixels of terms below 2^32, so int64 holds every sum)."""
    ty, tx = len(rows) - 1, len(cols) - 1
    out = np.zeros((len(idx), ty, tx, 5), np.int64)
    for k, f in enumerate(idx):
        if not 0 <= f < len(frames):
            continue
        for i in range(ty):
            for j in range(tx):
                if rows[i] < rows[i + 1] and cols[j] < cols[j + 1]:
                    out[k, i, j] = _terms(frames[f], ref, rows[i], rows[i + 1], cols[j], cols[j + 1]).sum(axis=(1, 2))
    return out


def ref_window(i, j, grid, rows, cols):
    """(ya, yb, xa, xb): the pixels of node (i, j)'s window."""
    gy, gx = grid
    return rows[max(0, 2 * i - 1)], rows[min(2 * gy, 2 * i + 3)], cols[max(0, 2 * j - 1)], cols[min(2 * gx, 2 * j + 3)]


def ref_window_gram(ref, win):
    """The 4 x 4 normal matrix of (b, 1, gx, gy) over the window, Python ints; None when empty."""
    ya, yb, xa, xb = win
    if ya >= yb or xa >= xb:
        return None
    B = np.asarray(ref).astype(np.int64)
    b = B[ya:yb, xa:xb]
    gx = B[ya:yb, xa + 1:xb + 1] - B[ya:yb, xa - 1:xb - 1]
    gy = B[ya + 1:yb + 1, xa:xb] - B[ya - 1:yb - 1, xa:xb]
    cols = [b, np.ones_like(b), gx, gy]
    return [[int((u * v).sum()) for v in cols] for u in cols]


def ref_solve_window(G, full, max_step):
    """[F, 2]: the steps of one node from its matrix G (Python ints) and the frames'
    right-hand sides ``full`` (F rows (Sab, Sa, Sagx, Sagy) of Python ints)."""
    F = len(full)
    out = np.zeros((F, 2))
    if F == 0 or any(G[i][i] <= 0 for i in range(4)):
        return out
    scale = [2.0 ** -np.rint(np.log2(np.float64(G[i][i])) / 2) for i in range(4)]
    Gs = np.array([[float(G[i][j]) * scale[i] * scale[j] for j in range(4)] for i in range(4)])
    rhs = np.array([[float(int(row[i]) - G[i][0]) * scale[i] for row in full] for i in range(4)])  # [4, F]
    with np.errstate(all="ignore"):
        try:
            sv = np.linalg.svd(Gs, compute_uv=False)
            if not np.isfinite(sv).all() or not sv[0] > 0 or sv[-1] / sv[0] < 1e-8:
                return out
            p = np.linalg.solve(Gs, rhs) * np.array(scale)[:, None]
        except np.linalg.LinAlgError:
            return out
    for f in range(F):
        vals = [float(v) for v in p[:, f]]
        alpha = 1.0 + vals[0]
        if not all(math.isfinite(v) for v in vals) or not alpha > 0:
            continue
        tx, ty = -2.0 * vals[2] / alpha, -2.0 * vals[3] / alpha
        if not (math.isfinite(tx) and math.isfinite(ty)):
            continue
        m = max(abs(tx), abs(ty))
        s = min(1.0, max_step / m) if m > 0 else 1.0
        out[f] = tx * s + 0.0, ty * s + 0.0
    return out


def ref_solve_nodes(frames, ref, grid, rows, cols, max_step=1.0):
    """[F, gy, gx, 2] float64: every node's step of every frame, from the windows' pixels."""
    gy, gx = grid
    out = np.zeros((len(frames), gy, gx, 2))
    for i in range(gy):
        for j in range(gx):
            win = ref_window(i, j, grid, rows, cols)
            G = ref_window_gram(ref, win)
            if G is None:
                continue
            full = []
            for fr in frames:
                sa, _, sab, sagx, sagy = (int(v) for v in _terms(fr, ref, *win).sum(axis=(1, 2)))
                full.append((sab, sa, sagx, sagy))
            out[:, i, j] = ref_solve_window(G, full, max_step)
    return out


def ref_to_source_field(u, M):
    """q [gy, gx, 2] int32 of one frame's steps u [gy, gx, 2] and forward map M [2, 3]."""
    m = phost._invert(M)
    ux, uy = np.asarray(u, np.float64)[..., 0], np.asarray(u, np.float64)[..., 1]
    q = np.stack([m[0] * ux + m[1] * uy, m[3] * ux + m[4] * uy], -1)
    return np.rint(q * 1024).astype(np.int32)


def ref_shrunk_region(affines, H, W, iters, max_step):
    y0, y1, x0, x1 = qhost.ref_valid_region(affines, H, W)
    m = math.ceil(iters * max_step)
    if y0 + m >= y1 - m or x0 + m >= x1 - m:
        raise ValueError("no common valid region")
    return y0 + m, y1 - m, x0 + m, x1 - m


def ref_field_pass(aligned, sources, affines, skipped, grid, iters=1, max_step=1.0, rate=1):
    """The whole pass from what a run WITHOUT the grid returns (aligned frames, maps, skipped)
    and the source frames.  Returns (aligned', field [n, gy, gx, 2], correlations [n, iters + 1],
    idxs, steps: per iteration the steps u [n, gy, gx, 2] before the keep rule)."""
    aligned = np.array(aligned, copy=True)
    affines = np.asarray(affines, np.float64)
    n, H, W = aligned.shape
    gy, gx = grid
    field = np.zeros((n, gy, gx, 2))
    corr = np.full((n, iters + 1), np.nan)
    q_acc = np.zeros((n, gy, gx, 2), np.int32)
    sel = np.zeros(n, bool)
    sel[qhost.ref_sel0(n, rate, [int(i) for i in skipped])] = True
    changed, steps = set(), []
    for it in range(iters):
        try:
            mean0 = qhost.ref_mean_image(aligned, sel)
            rect = ref_shrunk_region(affines[:n], H, W, iters, max_step)
        except ValueError:
            break
        rows, cols = ref_tile_edges(H, W, grid, rect)
        r_old = qhost.ref_correlations(aligned, mean0, rect)
        corr[:, it] = corr[:, it + 1] = r_old
        u = ref_solve_nodes(aligned, mean0, grid, rows, cols, max_step)
        steps.append(u)
        for i in range(n):
            if not u[i].any():
                continue
            q = q_acc[i] + ref_to_source_field(u[i], affines[i])
            cand = phost.ref_warp_field(np.asarray(sources[i])[None], affines[i][None], q[None])[0]
            r_new = qhost.ref_correlations(cand[None], mean0, rect)[0]
            if r_new > r_old[i]:
                aligned[i], q_acc[i], corr[i, it + 1] = cand, q, r_new
                field[i] += u[i]
                changed.add(i)
    return aligned, field, corr, sorted(changed), steps


# --------------------------------------------------------------------- synthetic frames
def smooth_fields(n, grid, seed, base=(0.3, 0.45), slope=0.15):
    """[n, gy, gx, 2] node displacements of smooth fields: per frame a common offset of length
    base[0] .. base[1] in a random direction plus a linear variation A p over the nodes'
    positions p in [-0.5, 0.5]^2 (entries of A within +-slope), so every component stays
    within base[1] + slope; frame 2k + 1 carries the negative of frame 2k's, so the fields
    leave the mean image in place."""
    rng = np.random.default_rng(seed)
    gy, gx = grid
    ang = rng.uniform(0, 2 * np.pi, n)
    off = rng.uniform(base[0], base[1], n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    A = rng.uniform(-slope, slope, (n, 2, 2))
    py, px = np.meshgrid((np.arange(gy) + 0.5) / gy - 0.5, (np.arange(gx) + 0.5) / gx - 0.5, indexing="ij")
    pos = np.stack([px, py], -1)  # [gy, gx, 2]
    u = off[:, None, None, :] + np.einsum("fab,ijb->fija", A, pos)
    u[1::2] = -u[0:2 * (n // 2):2]
    return u


def displaced(frames, u):
    """frame(p) = content(p - u(p)), u the field warp's interpolation of the node values u: the
    frames whose exact correction (to first order) is the field u."""
    frames = np.asarray(frames)
    ident = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (len(frames), 1, 1))
    return phost.ref_warp_field(frames, ident, np.rint(-np.asarray(u) * 1024).astype(np.int32))


H, W, GRID = 96, 128, (2, 3)
RECT = (3, H - 3, 3, W - 3)
NF = 6
_CACHE = {}


def recovery_inputs():
    """The texture image, NF frames of it displaced by known smooth fields, noise of sigma 40."""
    if not _CACHE:
        tex = rhost.Texture(5)
        img = fhost.to_u16(np.rint(tex(*rhost.grid(H, W))))
        truth = smooth_fields(NF, GRID, 17)
        frames = displaced(np.repeat(img[None], NF, 0), truth)
        frames = fhost.to_u16(frames + np.random.default_rng(3).normal(0, 40, frames.shape))
        _CACHE.update(img=img, truth=truth, frames=np.ascontiguousarray(frames))
    return _CACHE


def node_errors(field, truth):
    """[n, gy, gx]: the distance of every node's displacement from the truth (px)."""
    return np.sqrt(((np.asarray(field) - np.asarray(truth)) ** 2).sum(axis=-1))


# The end-to-end stack of tests/test_gpu_refine_field.py (test_gpu_refine.py's kind): frames
# are integer crops of one sampling of the analytic texture, displaced further by a smooth
# field per frame; every frame's keypoints carry a common offset of 0.3 - 0.5 px in a random
# direction, which RANSAC reproduces and the global refinement takes out again.
EF, PAD = 12, 12
_E2E = {}


def e2e_stack():
    if not _E2E:
        rng = np.random.default_rng(29)
        tex = rhost.Texture(11)
        scene = fhost.to_u16(np.rint(tex(*rhost.grid(H + 2 * PAD, W + 2 * PAD))))
        n_tpl = 60
        kp_tpl = np.stack([rng.integers(10, W - 10, n_tpl), rng.integers(10, H - 10, n_tpl)], 1).astype(np.float64)
        des_tpl = rng.integers(0, 256, (n_tpl, 32), dtype=np.uint8)
        ang = rng.uniform(0, 2 * np.pi, EF)
        jit = rng.uniform(0.3, 0.5, EF)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        t = rng.integers(-3, 4, (EF, 2))
        crops, kq, dq = [], [], []
        for f in range(EF):
            tx, ty = (int(v) for v in t[f])
            crops.append(scene[PAD - ty:PAD - ty + H, PAD - tx:PAD - tx + W])
            perm = rng.permutation(n_tpl)
            kq.append(kp_tpl[perm] + [tx, ty] + jit[f])
            dq.append(des_tpl[perm])
        fields = smooth_fields(EF, GRID, 31, base=(0.0, 0.0), slope=0.8)
        frames = displaced(np.stack(crops), fields)
        frames = fhost.to_u16(frames + rng.normal(0, 40, frames.shape))
        truth = np.array([[[1, 0, -tx], [0, 1, -ty]] for tx, ty in t], np.float64)
        maps = truth.copy()
        maps[:, :, 2] -= jit  # what RANSAC makes of the offset keypoints
        _E2E.update(frames=np.ascontiguousarray(frames), kp_tpl=kp_tpl, des_tpl=des_tpl, kq=kq, dq=dq, truth=truth,
                    maps=maps, fields=fields)
    return _E2E


def check_first_iteration(steps, corr, idxs, n):
    """The end-to-end premise: in the first iteration every node of every frame took a
    non-zero step and every frame was kept (so nothing passes by rejecting everything)."""
    assert (steps[0] != 0).any(axis=-1).all()
    assert (corr[:, 1] > corr[:, 0]).all()
    assert idxs == list(range(n))


# ------------------------------------------------------------------------- the tests
def test_module_is_exported_with_the_switch_off():
    import kcmc_amd
    from kcmc_amd import refine_field

    assert kcmc_amd.refine_field is refine_field
    for name in ("tile_edges", "tile_gradient_sums", "tile_gram", "window_sums", "solve_nodes", "to_source_field",
                 "refine_field_frames"):
        assert callable(getattr(refine_field, name)), name
    va = kcmc_amd.VideoAligner
    assert va.REFINE_GRID is None and va.REFINE_GRID_ITERS == 1
    inst = va()
    for attr in ("refine_field", "refine_field_correlations", "refine_field_idxs"):
        assert getattr(inst, attr) is None, attr


def test_header_and_binding_table_name_the_entry_point():
    with open(os.path.join(REPO, "include", "kcmc.h")) as fh:
        header = fh.read()
    assert "int kcmc_tile_gradient_sums_u16(kcmc_ctx* ctx, const uint16_t* frames_dev, int n_frames, int H, int W," \
        in header
    assert "g2: gradient sums per tile" in header
    assert "#define KCMC_ABI_VERSION 2" in header
    assert "kcmc_tile_gradient_sums_u16" in _lib.EXPORTED_SYMBOLS
    assert len(_lib._SIGNATURES["kcmc_tile_gradient_sums_u16"][0]) == 14
    assert _lib.ABI_VERSION == 2
    L = _lib.load()
    assert L.kcmc_abi_version() == 2 and hasattr(L, "kcmc_tile_gradient_sums_u16")


def test_edges_by_hand():
    from kcmc_amd import refine_field

    # (H, W) = (37, 61), grid (2, 3), margin 3: k * 37 // 4 = 0, 9, 18, 27, 37 and k * 61 // 6 = 0, 10, 20, 30, 40,
    # 50, 61, clamped to [3, 34] and [3, 58]
    rows, cols = refine_field.tile_edges(37, 61, (2, 3), (3, 34, 3, 58))
    assert rows.dtype == np.int32 and cols.dtype == np.int32
    assert rows.tolist() == [3, 9, 18, 27, 34] and cols.tolist() == [3, 10, 20, 30, 40, 50, 58]
    assert ref_tile_edges(37, 61, (2, 3), (3, 34, 3, 58)) == (rows.tolist(), cols.tolist())
    # cell j's two tiles meet at the node: edge 2j + 1 = floor((j + 0.5) W / gx), so the boundary between its two
    # pixels (edge - 0.5) is less than a pixel left of the node's centre (j + 0.5) W / gx - 0.5
    from kcmc_amd import piecewise

    for (h, w), grid in (((37, 61), (2, 3)), ((96, 128), (2, 3)), ((1080, 1920), (8, 8)), ((50, 50), (16, 16))):
        rows, cols = refine_field.tile_edges(h, w, grid, (1, h - 1, 1, w - 1))
        cy, cx = piecewise.node_centres(h, w, grid)
        dy, dx = cy - (rows[1::2] - 0.5), cx - (cols[1::2] - 0.5)
        assert (dy >= 0).all() and (dy < 1).all() and (dx >= 0).all() and (dx < 1).all()
        assert rows[0] == 1 and rows[-1] == h - 1 and (np.diff(rows) >= 0).all()
        assert ref_tile_edges(h, w, grid, (1, h - 1, 1, w - 1)) == (rows.tolist(), cols.tolist())


def _module_nodes(frames, ref, grid, rect, max_step=1.0):
    """The module's host chain on the restatement's tile sums (the kernel's stand-in here)."""
    from kcmc_amd import refine_field

    h, w = ref.shape
    rows, cols = refine_field.tile_edges(h, w, grid, rect)
    sums = ref_tile_sums(frames, list(range(len(frames))), ref, rows.tolist(), cols.tolist())
    gram = refine_field.tile_gram(ref, (rows, cols))
    return refine_field.solve_nodes(refine_field.window_sums(gram, grid), refine_field.window_sums(sums, grid), max_step)


def test_tile_gram_and_windows_equal_the_restatement():
    from kcmc_amd import refine_field

    rng = np.random.default_rng(4)
    for (h, w), grid, rect in (((37, 61), (2, 3), (3, 34, 3, 58)), ((40, 72), (1, 1), (1, 39, 1, 71)),
                               ((40, 72), (3, 2), (15, 30, 20, 60)), ((34, 66), (16, 16), (1, 33, 1, 65))):
        ref = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        ref[5, 7] = 65535
        if grid == (16, 16):  # the largest gradients
            ref[:] = 0
            ref[:, 2::4] = ref[:, 3::4] = 65535
        rows, cols = refine_field.tile_edges(h, w, grid, rect)
        gram = refine_field.tile_gram(ref, (rows, cols))
        assert gram.dtype == np.int64 and gram.shape == (2 * grid[0], 2 * grid[1], 10)
        gw = refine_field.window_sums(gram, grid)
        for i in range(grid[0]):
            for j in range(grid[1]):
                win = ref_window(i, j, grid, rows.tolist(), cols.tolist())
                G = ref_window_gram(ref, win)
                n, sb, sbb, sgx, sgy, sbgx, sbgy, sgxx, sgyy, sgxy = (int(v) for v in gw[i, j])
                if G is None:
                    assert not gw[i, j].any()
                    continue
                assert n == (win[1] - win[0]) * (win[3] - win[2])
                assert [[sbb, sb, sbgx, sbgy], [sb, n, sgx, sgy], [sbgx, sgx, sgxx, sgxy],
                        [sbgy, sgy, sgxy, sgyy]] == G, (grid, i, j)
        # the frames' sums: the windows of the tiles' sums are the windows' pixels' sums
        frames = rng.integers(0, 65536, (2, h, w)).astype(np.uint16)
        sw = refine_field.window_sums(ref_tile_sums(frames, [0, 1], ref, rows.tolist(), cols.tolist()), grid)
        for i in range(grid[0]):
            for j in range(grid[1]):
                ya, yb, xa, xb = ref_window(i, j, grid, rows.tolist(), cols.tolist())
                if ya < yb and xa < xb:
                    for f in range(2):
                        np.testing.assert_array_equal(sw[f, i, j], _terms(frames[f], ref, ya, yb, xa, xb).sum(axis=(1, 2)))
    with pytest.raises(ValueError):
        refine_field.tile_gram(ref, (np.array([0, 5]), np.array([1, 5])))
    with pytest.raises(ValueError):
        refine_field.window_sums(np.zeros((3, 4, 5), np.int64), (2, 3))


def test_solve_nodes_equals_the_restatement_exactly():
    e = recovery_inputs()
    rows, cols = ref_tile_edges(H, W, GRID, RECT)
    for max_step in (1.0, 0.25):
        want = ref_solve_nodes(e["frames"], e["img"], GRID, rows, cols, max_step)
        got = _module_nodes(e["frames"], e["img"], GRID, RECT, max_step)
        np.testing.assert_array_equal(got, want)
        assert np.abs(got).max() <= max_step and (got != 0).any(axis=-1).all()
    assert np.abs(got).max() == 0.25  # the trust region binds


def test_a_margin_beyond_half_a_cell_empties_the_outer_tiles_and_the_nodes_still_solve():
    from kcmc_amd import refine_field

    e = recovery_inputs()
    rect = (30, H - 30, 30, W - 30)  # half a cell is 24 rows, 21 columns
    rows, cols = refine_field.tile_edges(H, W, GRID, rect)
    assert rows.tolist() == [30, 30, 48, 66, 66] and cols.tolist() == [30, 30, 42, 64, 85, 98, 98]
    got = _module_nodes(e["frames"], e["img"], GRID, rect)
    np.testing.assert_array_equal(got, ref_solve_nodes(e["frames"], e["img"], GRID, rows.tolist(), cols.tolist()))
    assert (got != 0).any(axis=-1).all()
    # a tiling whose first tile row is all there is: the lower nodes' windows are empty
    rect = (3, 20, 3, W - 3)
    rows, cols = refine_field.tile_edges(H, W, GRID, rect)
    assert rows.tolist() == [3, 20, 20, 20, 20]
    got = _module_nodes(e["frames"], e["img"], GRID, rect)
    np.testing.assert_array_equal(got, ref_solve_nodes(e["frames"], e["img"], GRID, rows.tolist(), cols.tolist()))
    assert (got[:, 0] != 0).any(axis=-1).all() and not got[:, 1].any()


def test_a_frame_equal_to_the_reference_gives_an_exactly_zero_field():
    e = recovery_inputs()
    got = _module_nodes(e["img"][None], e["img"], GRID, RECT)
    np.testing.assert_array_equal(got, np.zeros((1, 2, 3, 2)))
    assert not np.signbit(got).any()
    rows, cols = ref_tile_edges(H, W, GRID, RECT)
    np.testing.assert_array_equal(ref_solve_nodes(e["img"][None], e["img"], GRID, rows, cols), 0)


def test_a_constant_window_is_rejected_and_its_neighbours_are_not():
    e = recovery_inputs()
    rows, cols = ref_tile_edges(H, W, GRID, RECT)
    assert cols[3] == 64  # node column 0's window ends there; its gradient reads column 64
    ref = e["img"].copy()
    ref[:, :65] = 30000
    got = _module_nodes(e["frames"], ref, GRID, RECT)
    np.testing.assert_array_equal(got, ref_solve_nodes(e["frames"], ref, GRID, rows, cols))
    assert not got[:, :, 0].any()
    assert (got[:, :, 1:] != 0).any(axis=-1).all()
    # a reference that varies along x only: gy = 0 everywhere, every node is rejected
    ramp = np.tile((np.arange(W) * 300).astype(np.uint16), (H, 1))
    assert not _module_nodes(e["frames"], ramp, GRID, RECT).any()
    assert not ref_solve_nodes(e["frames"], ramp, GRID, rows, cols).any()


def test_to_source_field():
    from kcmc_amd import refine_field

    rng = np.random.default_rng(8)
    u = rng.uniform(-1, 1, (5, 2, 3, 2))
    M = np.stack([phost.rot_about_centre(d, H, W, tx, ty) for d, tx, ty in
                  ((0.0, 0.0, 0.0), (0.0, 3.0, -2.0), (7.0, 1.5, 0.5), (-90.0, 0.0, 0.0), (2.0, -4.0, 4.0))])
    got = refine_field.to_source_field(u, M)
    assert got.dtype == np.int32 and got.shape == u.shape
    for f in range(5):
        np.testing.assert_array_equal(got[f], ref_to_source_field(u[f], M[f]))
    # a translation leaves the step as it is; a rotation of the frame by -90 degrees turns it
    np.testing.assert_array_equal(got[1], np.rint(u[1] * 1024))
    np.testing.assert_allclose(got[3] / 1024.0, np.stack([-u[3, ..., 1], u[3, ..., 0]], -1), atol=1e-3)


def test_restated_pass_recovers_a_known_smooth_field():
    """Frames made from the texture by the field warp with known smooth fields (smooth_fields:
    every component within 0.6 px); the maps are the identity.  One iteration brings every node's
    error below its starting error (the length of its true displacement), a second brings
    the RMS lower still; no frame's correlation falls."""
    e = recovery_inputs()
    ident = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (NF, 1, 1))
    start = node_errors(np.zeros_like(e["truth"]), e["truth"])
    one = ref_field_pass(e["frames"], e["frames"], ident, [], GRID, iters=1)
    two = ref_field_pass(e["frames"], e["frames"], ident, [], GRID, iters=2)
    err1, err2 = node_errors(one[1], e["truth"]), node_errors(two[1], e["truth"])
    rms = lambda v: float(np.sqrt((v ** 2).mean()))  # noqa: E731
    print("RMS node error", rms(start), "->", rms(err1), "(one iteration)", rms(err2), "(two iterations)")
    print("worst node", float(start.max()), "->", float(err1.max()), float(err2.max()))
    assert (err1 < start).all()
    assert rms(err2) < rms(err1)
    check_first_iteration(one[4], one[2], one[3], NF)
    assert (two[2][:, 1:] >= two[2][:, :-1]).all()
    for f in range(NF):  # every kept frame is the field warp of its source with the quantised field
        np.testing.assert_array_equal(one[0][f], phost.ref_warp_field(e["frames"][f][None], ident[:1],
                                                                      ref_to_source_field(one[1][f], ident[0])[None])[0])


def test_end_to_end_premise_holds_for_the_restatement_alone():
    """The stack of the GPU end-to-end test through the restatements only: the maps RANSAC makes
    of the offset keypoints, the oracle's warp, the global refinement's pass, then the field
    pass -- in its first iteration every node of every frame steps and every frame is kept."""
    e = e2e_stack()
    aligned = np.stack([oracle.warp_affine_u16(s, M) for s, M in zip(e["frames"], e["maps"])])
    aligned, maps, _, _, _ = rhost.ref_refine_pass(aligned, e["frames"], e["maps"], [], oracle.warp_affine_u16, iters=2)
    _, field, corr, idxs, steps = ref_field_pass(aligned, e["frames"], maps, [], GRID, iters=1)
    check_first_iteration(steps, corr, idxs, EF)
    before = node_errors(np.zeros_like(field), e["fields"])
    after = node_errors(field, e["fields"])
    print("RMS node error", float(np.sqrt((before ** 2).mean())), "->", float(np.sqrt((after ** 2).mean())))
    assert np.sqrt((after ** 2).mean()) < np.sqrt((before ** 2).mean())


def test_entry_point_validates_before_touching_the_gpu():
    check_validation(ctypes.c_void_p(np.zeros(8, np.int64).ctypes.data), None)


def check_validation(ctx, good):
    """Every contract violation is KCMC_EINVAL before any device work.  ``ctx``: a context
    handle (never dereferenced by the checks); ``good``: device pointers (frames, idx, ref,
    out) of a valid 33 x 40 call with a 2 x 3 tiling, or None on a box without a GPU (a host
    buffer stands in: nothing reads it)."""
    L = _lib.load()
    P = ctypes.c_void_p
    buf = np.zeros(64, np.int64)
    fr, idx, ref, out = good if good is not None else (buf.ctypes.data,) * 4
    H, W = 33, 40

    def call(ctx=ctx, fr=fr, n_frames=1, H=H, W=W, idx=idx, n_sel=1, ref=ref, rows=(1, 16, 32), cols=(1, 9, 9, 39),
             ty=None, tx=None, out=out):
        p = lambda v: None if v is None else P(v)  # noqa: E731
        r = None if rows is None else np.asarray(rows, np.int32)
        c = None if cols is None else np.asarray(cols, np.int32)
        ty = (len(r) - 1 if r is not None else 1) if ty is None else ty
        tx = (len(c) - 1 if c is not None else 1) if tx is None else tx
        return L.kcmc_tile_gradient_sums_u16(ctx, p(fr), n_frames, H, W, p(idx), n_sel, p(ref),
                                             None if r is None else r.ctypes.data_as(P), ty,
                                             None if c is None else c.ctypes.data_as(P), tx, p(out), None)

    E = _lib.KCMC_EINVAL
    assert call(ctx=None) == E and b"ctx" in L.kcmc_last_error()
    assert call(fr=None) == E and b"NULL" in L.kcmc_last_error()
    assert call(ref=None) == E
    assert call(out=None) == E
    assert call(rows=None) == E and b"NULL" in L.kcmc_last_error()
    assert call(cols=None) == E
    assert call(out=out + 4) == E and b"aligned" in L.kcmc_last_error()
    big = list(range(1, 35))
    for ty, tx in ((0, 3), (2, 0), (-1, 3), (33, 3), (2, 33)):
        assert call(rows=big, cols=big, ty=ty, tx=tx) == E and b"[1, 32]" in L.kcmc_last_error(), (ty, tx)
    assert call(rows=(1, 17, 16)) == E and b"non-decreasing" in L.kcmc_last_error()
    assert call(cols=(1, 9, 8, 39)) == E and b"non-decreasing" in L.kcmc_last_error()
    for rows, cols in (((0, 16, 32), None), ((1, 16, 33), None), (None, (0, 9, 9, 39)), (None, (1, 9, 9, 40))):
        kw = dict(rows=rows) if rows is not None else dict(cols=cols)
        assert call(**kw) == E and b"leaves the image" in L.kcmc_last_error(), kw
    assert call(H=1 << 16, W=1 << 15) == E and b"2^31" in L.kcmc_last_error()
    assert call(n_sel=-1) == E and call(n_frames=-1) == E and call(H=0) == E
    assert call(n_sel=0) == _lib.KCMC_OK
    assert call(n_sel=0, fr=None, idx=None, ref=None, out=None) == _lib.KCMC_OK
    assert call(n_sel=0, rows=(1, 0, 32)) == E  # the edges are checked before the empty call returns
    # the limits pass the checks (and stop at the NULL frames): 32 x 32 tiles, an all-empty tiling
    assert call(H=40, W=72, rows=list(range(1, 34)), cols=list(range(2, 67, 2)), fr=None) == E \
        and b"NULL" in L.kcmc_last_error()
    assert call(rows=(5, 5), cols=(7, 7), fr=None) == E and b"NULL" in L.kcmc_last_error()
    if good is not None:
        assert call() == _lib.KCMC_OK


def test_switch_checks_fail_before_any_work():
    from kcmc_amd import VideoAligner

    def va(**kw):
        return type("VA", (VideoAligner,), {"REFINE": "intensity", "REFINE_GRID": (2, 3), **kw})()

    stack4 = np.zeros((2, 4, 4, 3), np.uint16)
    for make, err, match, images in (
            (lambda: va(REFINE="none"), ValueError, "REFINE_GRID needs REFINE", None),
            (lambda: va(REFINE_GRID=(0, 3)), ValueError, "REFINE_GRID", None),
            (lambda: va(REFINE_GRID=(2, 17)), ValueError, "REFINE_GRID", None),
            (lambda: va(REFINE_GRID=(2.5, 3)), ValueError, "REFINE_GRID", None),
            (lambda: va(REFINE_GRID=3), ValueError, "REFINE_GRID", None),
            (lambda: va(REFINE_GRID_ITERS=0), ValueError, "REFINE_GRID_ITERS", None),
            (lambda: va(REFINE_GRID_ITERS=1.5), ValueError, "REFINE_GRID_ITERS", None),
            (lambda: va(REFINE_GRID_ITERS=True), ValueError, "REFINE_GRID_ITERS", None),
            (lambda: va(QUALITY_METRICS=True), NotImplementedError, "REFINE_GRID", None),
            (lambda: va(TEMPLATE_REFINE_ITERS=1), NotImplementedError, "REFINE_GRID", None),
            (lambda: va(RANSAC_MODEL="projective"), NotImplementedError, "REFINE", None),
            (lambda: va(PIECEWISE_GRID=(2, 2)), NotImplementedError, "REFINE", None),
            (lambda: va(), NotImplementedError, "REFINE", stack4)):
        with pytest.raises(err, match=match):
            make().align_images(images, 10, "orb", 30)
        if "TEMPLATE_REFINE_ITERS" in make().__class__.__dict__:
            continue  # align_keypoints refuses the template refinement itself, first
        with pytest.raises(err, match=match):
            make().align_keypoints(images, None, None, None, None, 10)

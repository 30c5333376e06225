"""Which paths of the bilinear warps (csrc/warp.hip: warpAffine K3, warpPerspective K3p) the GPU
cases reach, worked out on the host in the manner of test_warp_tile_host.py: a numpy restatement
of the two plan kernels (source_box / persp_box / box_plan and the fast-path test) classifies
every tile of the cases of test_gpu_warp_staging.py, test_gpu_warp_tie_window.py and the warp
cases of test_gpu_kernels.py and test_gpu_models.py, and the blend of a tile is computed from the
case's data with the kernel's own rule (a 16-byte chunk is bright when one of its 8 pixels is
>= 16384; bright * 20 > rows * pitch / 8 takes the float blend).  The union must hold every path
of the tile kernels; a break in a path no case reaches would go unseen on the device."""
import collections

import numpy as np

import oracle
import test_gpu_kernels as gk
import test_gpu_models as gm
import test_gpu_warp_staging as gs
import test_gpu_warp_tie_window as gt
from kcmc_amd import synthetic

TILE_W, MAX_PITCH, FAST_PITCH, LIM, BRIGHT_SHARE = 128, 256, 144, 30000, 20


def config(C, H, perspective=False):
    """(tile rows, LDS elements, staged rows at most) of BlockCfg / Block64Cfg / ChanCfg."""
    if C > 1:
        return 24, 16384, 32
    return (64 if not perspective and H % 64 == 0 and H % 56 != 0 else 56), 10240, 72


# ------------------------------------------------------------------ the plans, restated
def box_plan(sx0, sx1, sy0, sy1, H, W, C, max_rows, small, stage_ok, budget):
    ax0 = (sx0 >> 3) << 3
    pitch, rows = ((sx1 - ax0 + 1) + 7) & ~7, sy1 - sy0 + 1
    mode = 2
    if small and (sx1 < 0 or sx0 > W - 1 or sy1 < 0 or sy0 > H - 1):
        mode = 1
    elif small and stage_ok and pitch <= MAX_PITCH and rows <= max_rows and pitch * rows * C <= budget:
        mode = 0
    return mode, ax0, sy0, pitch, rows


def affine_plan(m, xb, yb, H, W, C):
    """warp_plan_kernel's tile plan for the inverted map m: (mode, ax0, sy0, pitch, rows)."""
    th, lds, max_rows = config(C, H)
    xl, yl = min(xb + TILE_W, W) - 1, min(yb + th, H) - 1
    r = gs.cv_round
    a, b = [r(m[0] * x * 1024) for x in (xb, xl)], [r(m[3] * x * 1024) for x in (xb, xl)]
    x = [r((m[1] * y + m[2]) * 1024) + 16 for y in (yb, yl)]
    y = [r((m[4] * y + m[5]) * 1024) + 16 for y in (yb, yl)]
    sx0, sx1 = (min(x) + min(a)) >> 10, ((max(x) + max(a)) >> 10) + 1
    sy0, sy1 = (min(y) + min(b)) >> 10, ((max(y) + max(b)) >> 10) + 1
    small = all(-LIM < v < LIM for v in (sx0, sx1, sy0, sy1))
    mode, ax0, sy0, pitch, rows = box_plan(sx0, sx1, sy0, sy1, H, W, C, max_rows, small, True, lds)
    if W % 8 == 0 and mode == 0 and pitch <= FAST_PITCH and rows <= (lds - 8) // (C * FAST_PITCH):
        mode = 3
    return mode, ax0, sy0, pitch, rows


def persp_plan(m, xb, yb, H, W, C):
    """persp_plan_kernel's tile plan for the inverted homography m (9 values)."""
    th, lds, max_rows = config(C, H, True)
    xl, yl = min(xb + TILE_W, W) - 1, min(yb + th, H) - 1
    sx, sy, ws = [], [], []
    with np.errstate(all="ignore"):
        for cx, cy in ((xb, yb), (xl, yb), (xb, yl), (xl, yl)):
            w = np.float64(m[6] * cx + m[7] * cy + m[8])
            ws.append(w)
            sx.append((m[0] * cx + m[1] * cy + m[2]) / w)
            sy.append((m[3] * cx + m[4] * cy + m[5]) / w)
    one_sign = all(w > 0 for w in ws) or all(w < 0 for w in ws)
    wrange = all(2.0 ** -56 <= abs(w) <= 2.0 ** 56 for w in ws)
    if not one_sign or not (min(sx) > -LIM and max(sx) < LIM and min(sy) > -LIM and max(sy) < LIM):
        return 2, 0, 0, 0, 0
    fl = lambda v: int(np.floor(v))  # noqa: E731
    return box_plan(fl(min(sx)) - 1, fl(max(sx)) + 2, fl(min(sy)) - 1, fl(max(sy)) + 2, H, W, C, max_rows, True,
                    wrange, lds - 8 - th * 2 * 12)


def bright_chunk_map(img):
    """[H, ceil(W / 8)]: the aligned 8-pixel groups that hold a value >= 16384 in some channel."""
    H, W = img.shape[:2]
    hot = (img >= 16384).reshape(H, W, -1).any(2)
    pad = np.zeros((H, -W % 8), bool)
    return np.concatenate([hot, pad], 1).reshape(H, -1, 8).any(2)


def box_bright(chunks, ax0, sy0, pitch, rows):
    H, n = chunks.shape
    r0, r1, c0, c1 = max(sy0, 0), min(sy0 + rows, H), max(ax0 >> 3, 0), min((ax0 + pitch) >> 3, n)
    return int(chunks[r0:r1, c0:c1].sum()) if r0 < r1 and c0 < c1 else 0


def affine_paths(img, M, inverse_map=False):
    """The paths the tiles of one frame take in warp_affine_u16_kernel."""
    H, W = img.shape[:2]
    C = img.shape[2] if img.ndim == 3 else 1
    th = config(C, H)[0]
    paths = collections.Counter({f"tile{th}": 1, f"C{C}": 1})
    m = np.asarray(M, np.float64) if inverse_map else oracle.invert_affine(np.asarray(M, np.float64))
    m = [float(v) for v in m.reshape(6)]
    if np.isnan(m).any():
        paths["nan"] += 1
        return paths
    chunks = bright_chunk_map(img)
    kind = "1" if C == 1 else "C"
    for yb in range(0, H, th):
        for xb in range(0, W, TILE_W):
            mode, ax0, sy0, pitch, rows = affine_plan(m, xb, yb, H, W, C)
            paths[f"mode{mode}"] += 1
            if mode == 0:
                paths[("vec" if W % 8 == 0 else "elem") + kind] += 1
            if mode == 3:
                bright = box_bright(chunks, ax0, sy0, pitch, rows)
                blend = "dark" if bright == 0 else "mixed" if bright * BRIGHT_SHARE <= rows * (pitch >> 3) else "bright"
                where = "interior" if yb + th <= H and xb + TILE_W <= W else "edge"
                paths[f"fast{kind}-{blend}"] += 1
                paths[f"fast{kind}-{where}"] += 1
    return paths


def persp_paths(img, M, inverse_map=False):
    """The paths the tiles of one frame take in warp_perspective_u16_kernel."""
    H, W = img.shape[:2]
    C = img.shape[2] if img.ndim == 3 else 1
    th = config(C, H, True)[0]
    paths = collections.Counter({f"C{C}": 1})
    with np.errstate(all="ignore"):
        m = np.asarray(M, np.float64) if inverse_map else oracle.invert_perspective(np.asarray(M, np.float64))
    m = [float(v) for v in np.asarray(m).reshape(9)]
    bw0 = min(1024 // min(16, H), W)
    chunks, nan = bright_chunk_map(img), bool(np.isnan(m).any())
    for yb in range(0, H, th):
        for xb in range(0, W, TILE_W):
            mode, ax0, sy0, pitch, rows = (1, 0, 0, 0, 0) if nan else persp_plan(m, xb, yb, H, W, C)
            paths[f"mode{mode}"] += 1
            if nan:
                paths["nan"] += 1
            if mode != 1:
                paths["table" if bw0 == 64 else "no-table"] += 1
            if mode == 0:
                paths[("vec" if W % 8 == 0 else "elem") + ("1" if C == 1 else "C")] += 1
            if mode == 0 and bw0 == 64 and C == 1 and W % 8 == 0:
                paths["dark" if box_bright(chunks, ax0, sy0, pitch, rows) == 0 else "not-dark"] += 1
    return paths


# ------------------------------------------------------------------ the restatement's own answers
def test_restated_plans_on_known_tiles():
    z = np.zeros((56, 128), np.uint16)
    for dx, dy in gs.SHIFTS:  # the one-channel plan agrees with test_gpu_warp_staging's
        for H, W in gs.SHAPES:
            mi = oracle.invert_affine(gs.shift(dx, dy))
            for yb in range(0, H, gs.tile_h(H)):
                for xb in range(0, W, TILE_W):
                    assert affine_plan([float(v) for v in mi.reshape(6)], xb, yb, H, W, 1) == gs.source_box(mi, xb, yb, H, W)
    one = lambda *a, **k: set(affine_paths(*a, **k)) - {"tile56", "tile64", "tile24", "C1", "C3"}  # noqa: E731
    assert one(z, gs.shift(0, 0)) == {"mode3", "fast1-dark", "fast1-interior"}
    assert one(z + 16384, gs.shift(0, 0)) == {"mode3", "fast1-bright", "fast1-interior"}
    assert one(z[:, :120], gs.shift(0, 0)) == {"mode3", "fast1-dark", "fast1-edge"}
    assert one(z[:, :124], gs.shift(0, 0)) == {"mode0", "elem1"}
    assert one(z, gs.shift(300, 0)) == {"mode1"}
    assert one(z, gs.shift(-40000, 0)) == {"mode2"}  # beyond the coordinate limit
    assert one(z, synthetic.rigid(np.deg2rad(20), 0, 0)) == {"mode2"}
    assert one(z, gs.zoom_rot(0.8, 1.0, 0.0, 0, 0)) == {"mode0", "vec1"}  # a 160-px box: wider than the fast pitch
    assert one(z, gs.shift(np.nan, 0)) == {"nan"}
    z3 = np.zeros((24, 128, 3), np.uint16)
    assert one(z3, gs.shift(0, 0)) == {"mode3", "fastC-dark", "fastC-interior"}
    assert one(z3[:, :126], gs.shift(0, 0)) == {"mode0", "elemC"}
    one_bright = z.copy()
    one_bright[5, 9] = 16384  # 1 bright chunk of 17 x 58: mixed
    assert "fast1-mixed" in affine_paths(one_bright, gs.shift(0, 0))
    assert "tile64" in affine_paths(np.zeros((128, 8), np.uint16), gs.shift(0, 0))
    ident = np.eye(3)
    onep = lambda *a, **k: set(persp_paths(*a, **k)) - {"C1", "C3"}  # noqa: E731
    assert onep(z, ident) == {"mode0", "table", "vec1", "dark"}
    assert onep(one_bright, ident) == {"mode0", "table", "vec1", "not-dark"}
    assert onep(np.zeros((5, 7), np.uint16), ident) == {"mode0", "no-table", "elem1"}
    assert onep(z, np.array([[1.0, 0, 5000], [0, 1, 0], [0, 0, 1]])) == {"mode1"}
    assert onep(z, np.array([[1.0, 0, 0], [0, 1, 0], [0.02, 0, -1]])) == {"mode2", "table"}  # the horizon crosses the tile
    assert onep(z3, ident) == {"mode0", "table", "vecC"}


# ------------------------------------------------------------------ the GPU cases
def affine_cases():
    """(frame, map, inverse_map) of the affine GPU cases with inputs of their own."""
    for H, W in gs.SHAPES:  # test_gpu_warp_staging
        imgs = gs.frames(H, W)
        maps = [gs.shift(dx, dy) for dx, dy in gs.SHIFTS]
        maps += [gs.shift(dx, dy) for dx, dy in [(W + 40.5, 0.0), (0.0, -(H + 77.25)), (-(W + 3.0), H + 3.0),
                                                 (-(TILE_W - 0.5), 0.0), (W - 1.5, 0.0), (0.0, -(gs.tile_h(H) - 0.5)),
                                                 (0.0, H - 1.5)]]
        if (H, W) in gs.SHAPES[1:]:
            maps += gs.sweep()[::5]
        if (H, W) in gs.SHAPES[:2]:
            maps.append(np.full((2, 3), np.nan))
        for M in maps:
            for img in imgs:
                yield img, M, False
    for M in [gs.shift(0.0, 0.0), gs.shift(5.3, -3.2), gs.shift(-30.1, 20.6), synthetic.rigid(0.03, 2.3, -1.7)]:
        for img in gs.frames(60, 132):
            yield img, M, False
    for make in (gt.mixed_frames, gt.bright_frames):  # test_gpu_warp_tie_window
        F = len(gt.NEAR_MAPS)
        for H in (60, 64, 128):
            yield from ((img, M, False) for img, M in zip(make(F, H, gt.W0), gt.NEAR_MAPS))
        for C in (3, 4):
            yield from ((img, M, False) for img, M in zip(make(F, 48, gt.W0, C), gt.NEAR_MAPS))
        yield from ((img, M, False) for img, M in zip(make(8, gt.H0, gt.W0), gt.census_maps(8, seed=11)))
    for C in (3, 4):
        yield from ((img, M, False) for img, M in zip(gt.mixed_frames(8, 48, gt.W0, C, seed=9), gt.census_maps(8, seed=13)))
    img, M = gt.window_edge_frame()
    yield img, M, False
    img, M = gt.window_edge_frame(gt.H0, gt.W0, 3, gt.W0)
    yield img, M, False
    for shape in gk.WARP_SHAPES:  # test_gpu_kernels
        yield from ((img, M, False) for img, M in zip(*gk.warp_case(shape)))
    for C in (3, 4):
        yield from ((img, M, False) for img, M in zip(*gk.multichannel_case(C)))
    yield from ((img, M, False) for img, M in zip(*gk.all_tile_paths_case()))
    for values in gk.TILE64_VALUES:
        yield from ((img, M, False) for img, M in zip(*gk.tile64_case(values)))
    for shape in gk.VECTOR_STAGING_SHAPES:
        imgs, Ms, _ = gk.vector_staging_case(shape)
        yield from ((img, M, False) for img, M in zip(imgs, Ms))


def persp_cases():
    for data in (gt.mixed_frames, gt.bright_frames):  # test_gpu_warp_tie_window.test_perspective
        for C in (0, 3):
            Ms = [np.array([[1.0, 0.01, 2.3], [-0.01, 1.0, -1.6], [1e-5, 2e-5, 1.0]]),
                  np.array([[1.02, -0.02, -4.4], [0.015, 0.99, 3.2], [-2e-5, 1e-5, 1.0]])]
            yield from ((img, M, False) for img, M in zip(data(2, gt.H0, gt.W0, C), Ms))
    img, M = gt.window_edge_frame()
    yield img, np.concatenate([M, [[0.0, 0.0, 1.0]]]), False
    for shape in gm.PERSPECTIVE_SHAPES:  # test_gpu_models
        yield from ((img, M, False) for img, M in zip(*gm.perspective_case(shape)))
    for C in (3, 4):
        yield from ((img, M, False) for img, M in zip(*gm.perspective_multichannel_case(C)))
    img, Ms = gm.extreme_perspective_case()
    for inv in (False, True):
        yield from ((img, M, inv) for M in Ms)
    for shape in gk.VECTOR_STAGING_SHAPES:  # test_gpu_kernels
        imgs, _, Hs = gk.vector_staging_case(shape)
        yield from ((img, M, False) for img, M in zip(imgs, Hs))
    M = np.vstack([synthetic.rigid(0.01, 1.5, -2.0), [0.0, 0.0, 1.0]])  # test_warp_nan_map_gives_zeros
    M[0, 2] = np.nan
    yield np.ones((64, 136), np.uint16), M, False


AFFINE_PATHS = {"mode0", "mode1", "mode2", "mode3", "nan", "C1", "C3", "C4", "vec1", "vecC", "elem1", "elemC",
                "tile24", "tile56", "tile64"}
AFFINE_PATHS |= {f"fast{k}-{p}" for k in "1C" for p in ("interior", "edge", "dark", "mixed", "bright")}
PERSP_PATHS = {"mode0", "mode1", "mode2", "nan", "table", "no-table", "C1", "C3", "C4", "dark", "not-dark",
               "vec1", "vecC", "elem1", "elemC"}


def reached(cases, paths_of):
    total = collections.Counter()
    for img, M, inv in cases:
        for k in paths_of(img, M, inv):
            total[k] += 1  # frames with at least one tile on the path
    return total


def test_the_affine_gpu_cases_reach_every_path():
    total = reached(affine_cases(), affine_paths)
    print("affine, frames per path:", dict(sorted(total.items())))
    assert set(total) == AFFINE_PATHS, (AFFINE_PATHS - set(total), set(total) - AFFINE_PATHS)


def test_the_perspective_gpu_cases_reach_every_path():
    total = reached(persp_cases(), persp_paths)
    print("perspective, frames per path:", dict(sorted(total.items())))
    assert set(total) == PERSP_PATHS, (PERSP_PATHS - set(total), set(total) - PERSP_PATHS)

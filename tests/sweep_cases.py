"""Seeded random cases for the kernels added after the original hot path, and the code that
runs one case on the device and compares it with the numpy restatement, bit for bit.

    frame_stats         kcmc_frame_stats_u16 + kcmc_stack_sum_u16   (kcmc_amd.quality)
    shift_search        kcmc_shift_search_u16                       (kcmc_amd.fallback)
    gradient_sums       kcmc_gradient_sums_u16                      (kcmc_amd.refine)
    tile_gradient_sums  kcmc_tile_gradient_sums_u16, arbitrary edges (the C entry, through the
                        slab plumbing of kcmc_amd._intensity.run_indexed)
    phase_sums          kcmc_bidi_phase_sums_u16                    (kcmc_amd.bidi)
    warp_field          kcmc_warp_field_u16                         (kcmc_amd.stages)
    resize_u8           kcmc_resize_u8                              (kcmc_amd.stages)
    warp_affine         kcmc_warp_affine_u16, C = 1 / 3 / 4         (kcmc_amd.stages; against the C oracle)
    warp_perspective    kcmc_warp_perspective_u16, C = 1 / 3 / 4    (kcmc_amd.stages; against the C oracle)
    normalize           kcmc_histogram_u16 + kcmc_lut_u16_to_u8     (kcmc_amd.stages.brightest_px /
                        max_scale_u8; against np.percentile and the reference's scaling expression)

case_<kernel>(seed) draws one case from np.random.default_rng(seed): the inputs as numpy arrays
and the drawn parameters (describe(case): what a failure message prints).  expected(kernel, case)
is the restatement's answer, check(kernel, seed, dev) the device's answer compared with it.
tests/test_gpu_sweeps.py runs check over SEEDS and PINNED, tools/kernel_sweeps.py over any seed
range; tests/test_sweep_cases_host.py checks (without a GPU) that SEEDS reach the paths the sweeps
are for.  Not collected by pytest; importing it needs no GPU.

Shared draws.  Values: test_gpu_fuzz._values' three families and a full-range frame with a
rectangular patch of 65535.  Width: about half the cases have W % 8 == 0 (the 16-byte staging).
Slabs: the stack is cut into 1 to 3 slabs, each a contiguous view that starts ``off`` elements
into its own allocation (u16: 0, 1, 4 or 8 -- 0, 2, 8 or 16 bytes; u8: 0 to 3), the reference
image with an offset of its own.  Index lists: 0 to 8 entries with repeats, descending runs, -1
and values >= F; every fourth seed the plain range(F), every sixteenth the empty list.

The bilinear warps take any u16 pointer (include/kcmc.h): their sources sit between GUARD_U16
fills (in front of an offset view and at least _GUARD elements behind the data), so that a
staging load the device moved back onto the 16-byte grid, or one that strayed past the slab,
reads values that are neither the frame's nor the border's zero, inside the allocation.
"""
import ctypes

import numpy as np

import oracle
import test_bidi_host as bhost
import test_fallback_host as fhost
import test_gpu_fuzz as fuzz
import test_orb_pyramid_host as ohost
import test_piecewise_host as phost
import test_quality_host as qhost
import test_refine_field_host as tfhost
import test_refine_host as rhost

# _rng seeds from a kernel's position here: new kernels go at the end
KERNELS = ("frame_stats", "shift_search", "gradient_sums", "tile_gradient_sums", "phase_sums", "warp_field",
           "resize_u8", "warp_affine", "warp_perspective", "normalize")
# the seeds of tests/test_gpu_sweeps.py; tests/test_sweep_cases_host.py holds what they must reach
SEEDS = {k: tuple(range(16)) for k in KERNELS}
# seeds 0 to 15 hold no multichannel frame staged by mode 0 from a source 8 bytes off the 16-byte grid
SEEDS["warp_affine"] = tuple(range(4, 20))
# (kernel, seed) beyond SEEDS: cases a campaign (tools/kernel_sweeps.py) found failing, kept
PINNED = ()

OFFS_U16 = (0, 1, 4, 8)
OFFS_U8 = (0, 1, 2, 3)
FIELD_FAMILIES = ("zero", "2px", "40px", "constant", "2px+far")
LINEAR_FAMILIES = ("fuzz", "near", "zoom-out")
GUARD_U16, GUARD_U8 = 0xABCD, 0xA5
_GUARD = 64  # sentinel elements in front of and behind an output


def _rng(kernel, seed):
    return np.random.default_rng([KERNELS.index(kernel), int(seed)])


# ------------------------------------------------------------------ shared draws
def _values(rng, shape):
    if rng.integers(0, 4) < 3:
        return fuzz._values(rng, shape)
    v = rng.integers(0, 65536, shape).astype(np.uint16)
    H, W = shape[-2:]
    ya, xa = int(rng.integers(0, H)), int(rng.integers(0, W))
    yb, xb = int(rng.integers(ya + 1, H + 1)), int(rng.integers(xa + 1, W + 1))
    v[..., ya:yb, xa:xb] = 65535
    return v


def _values_u8(rng, shape):
    kind = rng.integers(0, 3)
    if kind == 0:
        return rng.integers(0, 256, shape).astype(np.uint8)
    if kind == 1:  # dark with hot pixels
        v = rng.integers(0, 32, shape)
        v[rng.random(shape) < 1e-2] = 255
        return v.astype(np.uint8)
    v = rng.integers(0, 256, shape).astype(np.uint8)
    H, W = shape[-2:]
    ya, xa = int(rng.integers(0, H)), int(rng.integers(0, W))
    v[..., ya:int(rng.integers(ya + 1, H + 1)), xa:int(rng.integers(xa + 1, W + 1))] = 255
    return v


def _width(rng, lo, hi):
    """W in [lo, hi]; about half the time a multiple of 8 in that range (when there is one)."""
    W = int(rng.integers(lo, hi + 1))
    if rng.random() < 0.5 and -(-lo // 8) <= hi // 8:
        W = 8 * int(rng.integers(-(-lo // 8), hi // 8 + 1))
    return W


def _layout(rng, F, offs):
    """[(first frame, end frame, offset)] of 1 to min(3, F) slabs without an empty one."""
    n = int(rng.integers(1, min(3, F) + 1))
    inner = rng.choice(np.arange(1, F), n - 1, replace=False) if n > 1 else []
    cuts = [0] + sorted(int(c) for c in inner) + [F]
    return [(cuts[i], cuts[i + 1], int(rng.choice(offs))) for i in range(n)]


def _index_list(rng, F, seed):
    if seed % 4 == 0:
        return list(range(F))
    n = 0 if seed % 16 == 7 else int(rng.integers(0, 9))
    idx = []
    while len(idx) < n:
        kind = int(rng.integers(0, 5))
        if kind == 0:
            idx.append(-1)
        elif kind == 1:
            idx.append(F + int(rng.integers(0, 3)))
        elif kind == 2 and idx:
            idx.append(idx[-1])
        elif kind == 3:  # a descending run
            a = int(rng.integers(0, F))
            idx.extend(range(a, max(a - 3, -1), -1))
        else:
            idx.append(int(rng.integers(0, F)))
    return idx[:n]


def _rect(rng, H, W, m, shape):
    """(y0, y1, x0, x1) non-empty with a margin of m inside H x W.  shape 0: one pixel; 1: the
    largest; else uniform among the rectangles."""
    if shape == 0:
        y0, x0 = int(rng.integers(m, H - m)), int(rng.integers(m, W - m))
        return y0, y0 + 1, x0, x0 + 1
    if shape == 1:
        return m, H - m, m, W - m
    y0, x0 = int(rng.integers(m, H - m)), int(rng.integers(m, W - m))
    return y0, int(rng.integers(y0 + 1, H - m + 1)), x0, int(rng.integers(x0 + 1, W - m + 1))


def _stack_case(rng, F, H, W, with_ref=True):
    case = {"F": F, "H": H, "W": W, "frames": _values(rng, (F, H, W)), "slabs": _layout(rng, F, OFFS_U16)}
    if with_ref:
        case["ref"] = _values(rng, (H, W))
        case["ref_off"] = int(rng.choice(OFFS_U16))
    return case


def vector_slabs(case):
    """Per slab: whether the kernels stage it with 16-byte loads (u16_rows.h rows_vectorizable:
    W % 8 == 0, the slab and the reference on 16-byte boundaries)."""
    ref_ok = case.get("ref_off", 0) % 8 == 0
    return [case["W"] % 8 == 0 and off % 8 == 0 and ref_ok for _, _, off in case["slabs"]]


def called_slabs(case):
    """The slabs run_indexed launches on: those that hold a listed frame, and the first."""
    idx = case["idx"]
    return [i for i, (a, b, _) in enumerate(case["slabs"]) if i == 0 or any(a <= f < b for f in idx)]


# ------------------------------------------------------------------ the generators
def case_frame_stats(seed):
    rng = _rng("frame_stats", seed)
    F, H, W = int(rng.integers(1, 10)), int(rng.integers(1, 141)), _width(rng, 1, 140)
    case = _stack_case(rng, F, H, W)
    case["rect"] = _rect(rng, H, W, 0, int(rng.integers(0, 8)))
    case["sel"] = None if rng.random() < 0.3 else rng.random(F) < 0.6
    return case


def case_shift_search(seed):
    rng = _rng("shift_search", seed)
    R = int(rng.integers(1, 17))
    if seed % 8 == 5:
        R = 16  # three shifts per thread
    F, H, W = int(rng.integers(1, 6)), int(rng.integers(2 * R + 1, 2 * R + 101)), _width(rng, 2 * R + 1, 2 * R + 260)
    case = _stack_case(rng, F, H, W)
    case["R"] = R
    case["rect"] = _rect(rng, H, W, R, int(rng.integers(0, 8)))
    case["idx"] = _index_list(rng, F, seed)
    return case


def case_gradient_sums(seed):
    from kcmc_amd import refine

    rng = _rng("gradient_sums", seed)
    F, H, W = int(rng.integers(1, 6)), int(rng.integers(3, 131)), _width(rng, 3, 300)
    case = _stack_case(rng, F, H, W)
    case["rect"] = _rect(rng, H, W, 1, int(rng.integers(0, 5)))
    kind = int(rng.integers(0, 3))
    band = refine.band_rows(H, W, case["rect"])
    case["rows"] = None if kind == 0 else 1 if kind == 1 else int(rng.integers(1, band + 1))
    case["idx"] = _index_list(rng, F, seed)
    return case


def _edges(rng, n, lo, hi, force):
    """n + 1 non-decreasing edges in [lo, hi]; force: an empty tile and a one-pixel tile where
    they fit (n >= 2 and hi > lo)."""
    e = np.sort(rng.integers(lo, hi + 1, n + 1))
    if rng.random() < 0.5:
        e[0], e[-1] = lo, hi
    if force and n >= 2 and hi > lo:
        k = int(rng.integers(0, n - 1))  # tiles k (one pixel) and k + 1 (empty)
        a = int(rng.integers(lo, hi))
        e[:k + 1] = np.minimum(e[:k + 1], a)
        e[k + 1] = e[k + 2] = a + 1
        e[k] = a
        e[k + 3:] = np.maximum(e[k + 3:], a + 1)
    return [int(v) for v in e]


def case_tile_gradient_sums(seed):
    """H in 3..130 and W in 3..330 (1 to 41 eight-pixel vectors: thread_columns_log2 3, 4 and 5);
    one case in six has W in 460..530 with the whole width covered, for 64 thread columns."""
    rng = _rng("tile_gradient_sums", seed)
    wide = seed % 6 == 5
    F, H = int(rng.integers(1, 6)), int(rng.integers(3, 131))
    W = _width(rng, 460, 530) if wide else _width(rng, 3, 330)
    case = _stack_case(rng, F, H, W)
    ty, tx = int(rng.integers(1, 33)), int(rng.integers(1, 33))
    if rng.random() < 0.2:
        ty, tx = (32, tx) if rng.random() < 0.5 else (ty, 32)
    force = seed % 3 == 1
    case["row_edges"] = _edges(rng, ty, 1, H - 1, force)
    case["col_edges"] = _edges(rng, tx, 1, W - 1, force)
    if wide:
        case["col_edges"][0], case["col_edges"][-1] = 1, W - 1
    case["idx"] = _index_list(rng, F, seed)
    return case


def case_phase_sums(seed):
    """One case in six has W in 1025..1100 (the second column tile) and then H in 2..16: the
    restatement walks the samples in Python, about a second for 3 x 16 x 1100 at R = 16."""
    rng = _rng("phase_sums", seed)
    R = int(rng.integers(0, 17))
    if seed % 8 in (4, 6):
        R = 16 if seed % 8 == 4 else 0
    F, H = int(rng.integers(1, 4)), int(rng.integers(2, 71))
    if seed % 6 == 3:
        H, W = int(rng.integers(2, 17)), _width(rng, 1025, 1100)
    elif seed % 8 == 1:
        W = 2 * R + 1
    else:
        W = _width(rng, 2 * R + 1, 2 * R + 300)
    case = _stack_case(rng, F, H, W, with_ref=False)
    case["R"] = R
    case["idx"] = _index_list(rng, F, seed)
    return case


def case_warp_field(seed):
    rng = _rng("warp_field", seed)
    F, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 301)), _width(rng, 1, 520)
    if seed % 8 == 2:
        H = int(rng.choice([64, 128, 192, 256]))  # the 64-row tiles (H % 64 == 0 and H % 56 != 0)
    full = seed % 6 == 1  # as many nodes as pixels along an axis
    if full:
        if seed // 6 % 2 == 0:
            H = int(rng.integers(1, 17))
        else:
            W = int(rng.integers(1, 17))
    gy, gx = int(rng.integers(1, min(16, H) + 1)), int(rng.integers(1, min(16, W) + 1))
    if full:
        gy, gx = (H, gx) if H <= 16 else (gy, W)
    case = {"F": F, "H": H, "W": W, "gy": gy, "gx": gx, "frames": _values(rng, (F, H, W))}
    case["slabs"] = _layout(rng, F, OFFS_U16)
    case["out_offs"] = [int(rng.choice(OFFS_U16)) for _ in case["slabs"]]
    fam = FIELD_FAMILIES[int(rng.integers(0, len(FIELD_FAMILIES)))]
    shape = (F, gy, gx, 2)
    if fam == "zero":
        q = np.zeros(shape, np.int64)
    elif fam == "40px":
        q = rng.integers(-40 * 1024, 40 * 1024 + 1, shape)
    elif fam == "constant":
        q = np.broadcast_to(rng.integers(-8 * 1024, 8 * 1024 + 1, 2), shape).copy()
    else:
        q = rng.integers(-2 * 1024, 2 * 1024 + 1, shape)
        if fam == "2px+far":  # the contract's edge, |q| = 2^20, at one node
            q[int(rng.integers(0, F)), int(rng.integers(0, gy)), int(rng.integers(0, gx)),
              int(rng.integers(0, 2))] = int(rng.choice([-1, 1])) << 20
    case["family"], case["q"] = fam, q.astype(np.int32)
    assert np.abs(case["q"]).max(initial=0) <= 1 << 20  # beyond it the pixels are unspecified
    M = np.stack([fuzz._affine(rng, H, W) for _ in range(F)])
    if seed % 5 == 4:
        M[F - 1, int(rng.integers(0, 2)), int(rng.integers(0, 3))] = np.nan
    case["M"] = M
    case["inverse_map"] = bool(rng.integers(0, 2))
    return case


def _log_uniform(rng, lo, hi):
    return int(min(hi, max(lo, np.floor(np.exp(rng.uniform(np.log(lo), np.log(hi + 1)))))))


def case_resize_u8(seed):
    rng = _rng("resize_u8", seed)
    F = int(rng.integers(1, 4))
    H, W, dh, dw = (_log_uniform(rng, 1, 400) for _ in range(4))
    if rng.random() < 0.5:
        W = max(8, W // 8 * 8)
    sizes = [H, W, dh, dw]
    if seed % 5 == 2:
        sizes[int(rng.integers(0, 4))] = 1
    H, W, dh, dw = sizes
    if seed % 5 == 3:  # one axis keeps its length
        dh, dw = (H, dw) if rng.random() < 0.5 else (dh, W)
    case = {"F": F, "H": H, "W": W, "dst_h": dh, "dst_w": dw, "frames": _values_u8(rng, (F, H, W))}
    case["slabs"] = _layout(rng, F, OFFS_U8)
    case["out_offs"] = [int(rng.choice(OFFS_U8)) for _ in case["slabs"]]
    return case


def _linear_map(rng, fam, H, W, C, persp, inverse_map):
    """One frame's map of the bilinear sweeps.
    fuzz: test_gpu_fuzz's families (for the perspective warp with its last rows, the one whose
    denominator changes sign inside the frame among them: the direct gather).
    near: a rotation of about 0.004 rad and a shift within 6 px (perspective: a last row of about
    1e-5) -- a 128-px tile's box fits the 144-px fast pitch: mode 3 of the affine kernel, the
    staged box and (H >= 16, W >= 64) the row table of the perspective one.
    zoom-out: columns scaled by about 0.8 from the frame to the output (by its reciprocal in a map
    that is passed as the inverse), so that a full tile's box is about 160 px wide, beyond
    the fast pitch: the affine kernel's generic staging (mode 0); narrower edge tiles of the same
    frame stay on mode 3.  The rows are zoomed in by about 1.3, or a full tile's box would not fit
    its budget and the tile would gather (mode 2): a 64-row tile's 66 box rows x 168 exceed the 10240
    elements of one channel, a 24-row tile's 26 x 168 x 4 the 16384 of four; 52 and 21 rows fit."""
    if fam == "fuzz":
        return (fuzz._perspective if persp else fuzz._affine)(rng, H, W)
    a, t = rng.normal(0, 0.004), rng.uniform(-6, 6, 2)
    sx, sy = 1.0, 1.0
    if fam == "zoom-out":
        sx, sy = rng.uniform(0.78, 0.84), rng.uniform(1.25, 1.4)
        if inverse_map:
            sx, sy = 1.0 / sx, 1.0 / sy
    c, n = np.cos(a), np.sin(a)
    M = np.array([[sx * c, -sy * n, t[0]], [sx * n, sy * c, t[1]]])
    if persp:
        M = np.vstack([M, [0.0, 0.0, 1.0]])
        M[2, :2] = rng.normal(0, 1e-5, 2)
    return M


def _case_linear(kernel, seed):
    """F in 1..3, H in 1..130, W in 1..300: up to three tile columns (128 px) and six tile rows (56
    rows with one channel, 24 with three or four), interior, edge and partial tiles.  C follows
    (1, 1, 3, 4)[seed % 4].  Every other seed is forced to W % 8 == 0 (the vector staging, mode 3),
    the phase alternating every four seeds so that C = 1, 3 and 4 all get such seeds (of 0 to 15:
    1, 4, 9, 12; 6, 14; 3, 11).  Those have W in 136..296, the first frame of every slab of the
    zoom-out family (full tiles on mode 0 and, where the edge column is narrow, an edge tile on
    mode 3: both stagings at the slab's offset) and the others of the near one; on the other
    seeds W is _width's and every frame's family is drawn.  Affine with one channel: seed % 16 in
    (1, 12) takes H in {64, 128} (the 64-row tiles).  seed % 5 == 4: a NaN entry in the last
    frame's map.  inverse_map is drawn."""
    persp = kernel == "warp_perspective"
    rng = _rng(kernel, seed)
    C = (1, 1, 3, 4)[seed % 4]
    w8 = (seed + seed // 4) % 2 == 1
    F, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 131)), _width(rng, 1, 300)
    if w8:
        W = 8 * int(rng.integers(17, 38))
    if not persp and C == 1 and seed % 16 in (1, 12):
        H = int(rng.choice([64, 128]))
    frames = _values(rng, (F, H, W * C)).reshape((F, H, W) if C == 1 else (F, H, W, C))
    case = {"F": F, "H": H, "W": W, "C": C, "frames": frames, "slabs": _layout(rng, F, OFFS_U16)}
    case["out_offs"] = [int(rng.choice(OFFS_U16)) for _ in case["slabs"]]
    heads = {a for a, _, _ in case["slabs"]}
    fams = [("zoom-out" if f in heads else "near") if w8 else LINEAR_FAMILIES[int(rng.integers(0, 3))]
            for f in range(F)]
    case["inverse_map"] = bool(rng.integers(0, 2))
    M = np.stack([_linear_map(rng, fam, H, W, C, persp, case["inverse_map"]) for fam in fams])
    if seed % 5 == 4:
        M[F - 1, int(rng.integers(0, M.shape[1])), int(rng.integers(0, 3))] = np.nan
    case["families"], case["M"] = fams, M
    return case


def case_warp_affine(seed):
    return _case_linear("warp_affine", seed)


def case_warp_perspective(seed):
    return _case_linear("warp_perspective", seed)


NORMALIZE_Q = (99.99, 0.0, 100.0, 50.0)


def case_normalize(seed):
    """F in 1..6, H in 1..300, W in 1..300 (_width's rule): up to 540 000 values, below every grid
    cap (the capped grids are tests/test_gpu_normalize.py's).  Values: the shared families, one
    case in four the concentrated one ([0x0F00, 0x10FF]: two coarse bins, the fine pass counts
    about half the stack).  The slabs go to brightest_px as a part list, each at its OFFS_U16
    offset (1 and 4 elements: copied for alignment); max_scale_u8 writes each slab into an ``out``
    view 0, 1, 4 or 8 bytes into a sentinel-filled buffer.  q is drawn from NORMALIZE_Q and one
    uniform value; seed % 8 == 3 and 7 instead take the q whose two ranks lie on the two sides of
    the stack's first coarse-bin boundary, with gamma about 0.25 and 0.75 (kept as drawn when all
    values share a coarse bin)."""
    rng = _rng("normalize", seed)
    F, H, W = int(rng.integers(1, 7)), int(rng.integers(1, 301)), _width(rng, 1, 300)
    if rng.integers(0, 4) == 0:
        frames, family = rng.integers(0x0F00, 0x1100, (F, H, W)).astype(np.uint16), "concentrated"
    else:
        frames, family = _values(rng, (F, H, W)), "shared"
    case = {"F": F, "H": H, "W": W, "family": family, "frames": frames, "slabs": _layout(rng, F, OFFS_U16)}
    case["out_offs"] = [int(rng.choice(OFFS_U16)) for _ in case["slabs"]]
    uniform = float(rng.uniform(0, 100))
    case["percentile"] = (NORMALIZE_Q + (uniform,))[int(rng.integers(0, 5))]
    case["max_px"] = int(rng.choice((255, 127)))
    if seed % 8 in (3, 7):
        hb = np.sort(frames.reshape(-1) >> 8)
        edge = np.flatnonzero(hb[1:] != hb[:-1])
        if len(edge):
            case["percentile"] = 100.0 * (int(edge[0]) + (0.25 if seed % 8 == 3 else 0.75)) / (frames.size - 1)
    return case


def frame_slab(case, f):
    """(source offset, output offset) of the slab that holds frame f."""
    return next((off, o) for (a, b, off), o in zip(case["slabs"], case.get("out_offs", [0] * 3)) if a <= f < b)


GENERATORS = {"frame_stats": case_frame_stats, "shift_search": case_shift_search, "gradient_sums": case_gradient_sums,
              "tile_gradient_sums": case_tile_gradient_sums, "phase_sums": case_phase_sums,
              "warp_field": case_warp_field, "resize_u8": case_resize_u8, "warp_affine": case_warp_affine,
              "warp_perspective": case_warp_perspective, "normalize": case_normalize}


def describe(case):
    """The drawn parameters without the pixels."""
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in case.items()
            if k not in ("frames", "ref", "q")}


# ------------------------------------------------------------------ the restatements' answers
def _per_frame(fn, idx, F):
    """fn(list of frames) -> [n, ...] evaluated once per distinct listed frame of the stack and
    laid out over ``idx``; an index outside the stack keeps fn's zeros."""
    uniq = sorted({int(f) for f in idx if 0 <= f < F})
    got = fn(uniq + [-1])  # the last row: what an index outside the stack gives
    rows = [uniq.index(int(f)) if 0 <= f < F else len(uniq) for f in idx]
    return got[rows]


def expected(kernel, case):
    """A dict of the outputs of ``kernel`` on ``case`` as the restatements give them."""
    fr, F = case["frames"], case["F"]
    if kernel == "frame_stats":
        return {"stats": qhost.ref_frame_stats(fr, case["ref"], case["rect"]).astype(np.int64),
                "sum": qhost.ref_stack_sum(fr, case["sel"])}
    if kernel == "shift_search":
        fn = lambda idx: fhost.ref_shift_search(fr, idx, case["ref"], case["rect"], case["R"])  # noqa: E731
        out = {"sums": _per_frame(fn, case["idx"], F).astype(np.int64)}
        out["centre"] = qhost.ref_frame_stats(fr, case["ref"], case["rect"]).astype(np.int64)
        return out
    if kernel == "gradient_sums":
        fn = lambda idx: rhost.ref_gradient_sums(fr, idx, case["ref"], case["rect"])  # noqa: E731
        return {"sums": _per_frame(fn, case["idx"], F)}
    if kernel == "tile_gradient_sums":
        fn = lambda idx: tfhost.ref_tile_sums(fr, idx, case["ref"], case["row_edges"], case["col_edges"])  # noqa: E731
        return {"sums": _per_frame(fn, case["idx"], F)}
    if kernel == "phase_sums":
        fn = lambda idx: bhost.ref_bidi_sums(fr, idx, case["R"])  # noqa: E731
        return {"sums": _per_frame(fn, case["idx"], F).astype(np.int64)}
    if kernel == "warp_field":
        return {"out": phost.ref_warp_field(fr, case["M"], case["q"], (case["gy"], case["gx"]), case["inverse_map"])}
    if kernel == "resize_u8":
        return {"out": ohost.resize_np(fr, case["dst_h"], case["dst_w"])}
    if kernel in ("warp_affine", "warp_perspective"):
        # a frame whose map holds a NaN is zeros (include/kcmc.h; test_gpu_kernels.test_warp_nan_map_gives_zeros):
        # the oracle, like OpenCV, converts the NaN coordinates to integers, which C leaves undefined
        ref = oracle.warp_affine_u16 if kernel == "warp_affine" else oracle.warp_perspective_u16
        return {"out": np.stack([np.zeros_like(fr[f]) if np.isnan(case["M"][f]).any() else
                                 ref(fr[f], case["M"][f], inverse_map=case["inverse_map"]) for f in range(F)])}
    if kernel == "normalize":
        # numpy's own percentile and the reference's expression (VA:481, VA:490), never stages.max_scale_lut
        b, max_px = np.percentile(fr, case["percentile"]), case["max_px"]
        return {"brightest": b, "out": np.clip(fr / scale_divisor(b) * max_px, a_min=0, a_max=max_px).astype(np.uint8)}
    raise KeyError(kernel)


def scale_divisor(b):
    """What the normalize sweep scales by: the percentile's value, or 1.0 where that is 0 (q = 0 on
    a stack that holds a zero), which the reference's expression would divide by."""
    return b if b > 0 else np.float64(1.0)


# ------------------------------------------------------------------ the device's answers
def _view(arr, off, dev, fill=0, tail=0):
    """``arr`` on the device as a contiguous view that starts ``off`` elements into its allocation;
    the ``off`` elements in front of it and ``tail`` elements behind it hold ``fill``."""
    import torch

    flat = np.full(off + arr.size + tail, fill, arr.dtype)
    flat[off:off + arr.size] = arr.reshape(-1)
    return torch.from_numpy(flat).to(dev)[off:off + arr.size].view(*arr.shape)


def _parts(case, dev):
    parts = [_view(case["frames"][a:b], off, dev) for a, b, off in case["slabs"]]
    for p, (_, _, off) in zip(parts, case["slabs"]):
        assert p.is_contiguous() and p.data_ptr() % 16 == (off * p.element_size()) % 16
    return parts[0] if len(parts) == 1 else parts  # the wrappers take one tensor or the slabs


def _guarded(shape, off, dtype, fill, dev):
    """(buffer, view): a flat sentinel-filled buffer and the view of ``shape`` in its middle,
    _GUARD + off elements in."""
    import torch

    n = int(np.prod(shape))
    buf = torch.full((2 * _GUARD + off + n,), fill, dtype=dtype, device=dev)
    return buf, buf[_GUARD + off:_GUARD + off + n].view(*shape)


def _per_slab(case, dev, dtype, fill, out_shape, call, src_guard=None):
    """call(slab tensor, first frame, end frame, out view) per slab into guarded outputs ->
    (the outputs joined [F, ...], whether every sentinel survived).  src_guard: (fill, tail) of
    the sources (_view); zeros in front and nothing behind without it."""
    outs, intact = [], True
    for (a, b, off), o_off in zip(case["slabs"], case["out_offs"]):
        src = _view(case["frames"][a:b], off, dev, *(src_guard or ()))
        buf, view = _guarded((b - a,) + out_shape, o_off, dtype, fill, dev)
        for t, o in ((src, off), (view, o_off)):  # the 16-byte phases the case asks for
            assert t.is_contiguous() and t.data_ptr() % 16 == (o * t.element_size()) % 16
        got = call(src, a, b, view)
        assert got.data_ptr() == view.data_ptr()
        flat, lo, n = buf.cpu().numpy(), _GUARD + o_off, view.numel()
        intact = intact and bool((flat[:lo] == fill).all() and (flat[lo + n:] == fill).all())
        outs.append(flat[lo:lo + n].reshape(view.shape))
    return np.concatenate(outs), intact


def run(kernel, case, dev):
    """The outputs of ``kernel`` on ``case`` from the device, keyed as expected()'s; "guards":
    whether the sentinels around an ``out`` argument survived."""
    import torch

    from kcmc_amd import _intensity, _lib, bidi, fallback, quality, refine, stages

    if kernel in ("warp_affine", "warp_perspective"):
        fn = stages.warp_affine_u16 if kernel == "warp_affine" else stages.warp_perspective_u16
        M = torch.from_numpy(case["M"]).to(dev)
        call = lambda src, a, b, o: fn(src, M[a:b].contiguous(), out=o, inverse_map=case["inverse_map"])  # noqa: E731
        out, ok = _per_slab(case, dev, torch.uint16, GUARD_U16, case["frames"].shape[1:], call,
                            src_guard=(GUARD_U16, _GUARD))
        return {"out": out, "guards": ok}
    if kernel in ("warp_field", "resize_u8"):
        if kernel == "warp_field":
            M, q = torch.from_numpy(case["M"]).to(dev), torch.from_numpy(case["q"]).to(dev)
            call = lambda src, a, b, o: stages.warp_field_u16(  # noqa: E731
                src, M[a:b].contiguous(), q[a:b].contiguous(), out=o, inverse_map=case["inverse_map"])
            out, ok = _per_slab(case, dev, torch.uint16, GUARD_U16, (case["H"], case["W"]), call)
        else:
            call = lambda src, a, b, o: stages.resize_u8(src, case["dst_h"], case["dst_w"], out=o)  # noqa: E731
            out, ok = _per_slab(case, dev, torch.uint8, GUARD_U8, (case["dst_h"], case["dst_w"]), call)
        return {"out": out, "guards": ok}
    parts = _parts(case, dev)
    if kernel == "normalize":
        b = stages.brightest_px(parts, case["percentile"])
        call = lambda src, a, b_, o: stages.max_scale_u8(src, scale_divisor(b), out=o, max_px=case["max_px"])  # noqa: E731
        out, ok = _per_slab(case, dev, torch.uint8, GUARD_U8, (case["H"], case["W"]), call)
        return {"brightest": b, "out": out, "guards": ok}
    if kernel == "phase_sums":
        return {"sums": bidi.phase_sums(parts, case["idx"], case["R"])}
    ref = _view(case["ref"], case["ref_off"], dev)
    if kernel == "frame_stats":
        return {"stats": quality.frame_stats(parts, ref, case["rect"]),
                "sum": quality.stack_sum(parts, case["sel"]).cpu().numpy()}
    if kernel == "shift_search":
        return {"sums": fallback.shift_search(parts, case["idx"], ref, case["rect"], case["R"]),
                "centre": quality.frame_stats(parts, ref, case["rect"])}
    if kernel == "gradient_sums":
        return {"sums": refine.gradient_sums(parts, case["idx"], ref, case["rect"], case["rows"])}
    if kernel == "tile_gradient_sums":
        rows, cols = np.asarray(case["row_edges"], np.int32), np.asarray(case["col_edges"], np.int32)
        ty, tx = len(rows) - 1, len(cols) - 1
        idx = np.asarray(case["idx"], np.int64).reshape(-1)
        edges = (rows.ctypes.data_as(ctypes.c_void_p), ty, cols.ctypes.data_as(ctypes.c_void_p), tx)
        out = np.zeros((len(idx), ty, tx, 5), np.int64)
        slabs = parts if isinstance(parts, list) else [parts]
        for mine, o in _intensity.run_indexed(_lib.load().kcmc_tile_gradient_sums_u16, slabs, idx, ref, (), edges,
                                              (ty, tx, 5)):
            if len(mine):
                out[mine] = o.cpu().numpy()
        return {"sums": out}
    raise KeyError(kernel)


def compare(kernel, case, got, want, seed=None):
    """assert_array_equal of every output, and the kernel's further checks; the message names
    the kernel, the seed and the drawn parameters."""
    msg = f"{kernel} seed {seed}: {describe(case)}"
    for key, w in want.items():
        np.testing.assert_array_equal(got[key], w, err_msg=f"[{key}] {msg}")
    assert got.get("guards", True), f"a sentinel beside the output was overwritten: {msg}"
    if kernel == "shift_search":  # entry [R][R] is quality.frame_stats on the same rectangle
        R = case["R"]
        for k, f in enumerate(case["idx"]):
            if 0 <= f < case["F"]:
                np.testing.assert_array_equal(got["sums"][k, R, R], got["centre"][f],
                                              err_msg=f"[R][R] of row {k}: {msg}")
    if kernel == "phase_sums":  # Sb and Sbb do not depend on d
        s = got["sums"]
        np.testing.assert_array_equal(s[:, :, [1, 3]], np.broadcast_to(s[:, :1, [1, 3]], s[:, :, [1, 3]].shape),
                                      err_msg=f"Sb, Sbb across d: {msg}")


def check(kernel, seed, dev):
    case = GENERATORS[kernel](seed)
    compare(kernel, case, run(kernel, case, dev), expected(kernel, case), seed)
    return case

"""Paths of the three k=2 matchers (csrc/match.hip, match_hamming.hip, match_f32.hip) that
the parity tests' small shapes never reach, every frame bit for bit against the oracle:

A. the persistent frame walk of the u8 L2 and Hamming kernels: more frames than any
   residency can hold at once, so every workgroup walks g, g + G, g + 2G, ... over empty,
   one-row and multi-chunk frames;
B. the float matcher's exact fallback, forced by construction (8+ bit-identical frame rows
   fill a template row's top-8 with one value, so the row cannot be certified), its slot
   counters, batches and the grid-strides of its two kernels;
C. the float phase 1 at the fp16 range boundary, at extreme descriptor scales, on all-zero
   descriptors and on buffers that are not 16-byte aligned.

The frame counts of A come from an upper bound on the walk's stride G that the tests compute
themselves: a CU holds 2048 threads, at most 8 workgroups of 256 threads (4 of 512), so
G <= 8 * CUs / n_tg whatever the launcher's residency figure (knn_grid in match.hip,
launch_knn_hamming in match_hamming.hip).  A launcher that could exceed it moves _bound()."""
import numpy as np
import pytest
import torch

import oracle
from kcmc_amd import stages

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _csr(sizes):
    off = np.zeros(len(sizes) + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    return off


_KNN = {"u8": (stages.knn2_l2u8, oracle.knn2_l2u8), "hamming": (stages.knn2_hamming, oracle.knn2_hamming),
        "f32": (stages.knn2_l2u8, oracle.knn2_l2f32)}


def _assert_frames_equal_oracle(kind, idx, dist, tpl, des_q, off):
    """idx / dist [F, n_tpl, 2] (device results) == the oracle's, every frame, bit for bit.
    Returns the oracle's (idx, dist)."""
    ref = _KNN[kind][1]
    F, n_tpl = len(off) - 1, len(tpl)
    ri = np.empty((F, n_tpl, 2), np.int32)
    rd = np.empty((F, n_tpl, 2), np.float32)
    for f in range(F):
        ri[f], rd[f] = ref(tpl, des_q[off[f]:off[f + 1]])
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    bad = np.flatnonzero((idx != ri).any(axis=(1, 2)) | (dist.view(np.int32) != rd.view(np.int32)).any(axis=(1, 2)))
    assert bad.size == 0, (f"{bad.size} of {F} frames differ, first {bad[:8].tolist()} with "
                           f"{np.diff(off)[bad[:8]].tolist()} rows")
    return ri, rd


def _run_and_check(kind, dev, tpl, des_q, off, des_q_dev=None, tpl_dev=None):
    idx, dist = _KNN[kind][0](_t(tpl, dev) if tpl_dev is None else tpl_dev,
                              _t(des_q, dev) if des_q_dev is None else des_q_dev, _t(off, dev),
                              int(np.diff(off).max()))
    return _assert_frames_equal_oracle(kind, idx, dist, tpl, des_q, off)


# ------------------------------------------------------------- A. the persistent walk
def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _bound(dev, kind, n_tpl):
    """Upper bound on G, the frame stride of a workgroup's walk (module docstring)."""
    cus = _cus(dev)
    if kind == "hamming":
        n_tg = -(-n_tpl // 256)
    else:
        n_tg = -(-n_tpl // 512) if n_tpl > 256 else 1
    return 8 * cus // n_tg


_BIG = (255, 256, 257, 300, 520)  # one chunk, exactly one, two (odd / even row counts), three


def _walk_sizes(rng, F, layout, bound):
    u = rng.random(F)
    small = rng.integers(1, 9, F)
    sizes = np.where(u < 0.3, 0, np.where(u < 0.9, small, rng.choice(_BIG, F)))
    if layout == "head_empty":  # every workgroup starts on an empty frame
        sizes[:bound] = 0
    elif layout == "tail_empty":  # des_q's last row lies in an earlier frame; every walk ends on empties
        sizes[-bound:] = 0
    elif layout == "alternating":  # blocks of `bound` empty and `bound` non-empty frames
        block = np.arange(F) // bound
        sizes = np.where(block % 2 == 0, 0, np.where(sizes == 0, small, sizes))
    return sizes.astype(np.int64)


def _walk_case(kind, n_tpl, D, layout, dev):
    bound = _bound(dev, kind, n_tpl)
    F = 2 * bound + 37
    assert F > 2 * bound and F <= 65535  # every workgroup takes at least three frames
    rng = np.random.default_rng([n_tpl, D, len(layout), int(kind == "hamming")])
    sizes = _walk_sizes(rng, F, layout, bound)
    off = _csr(sizes)
    total = int(off[-1])
    tpl = rng.integers(0, 256, (n_tpl, D), dtype=np.uint8)
    des_q = rng.integers(0, 256, (total, D), dtype=np.uint8)
    copies = rng.random(total) < 0.3  # exact copies of template rows: distance 0, and ties between them
    des_q[copies] = tpl[rng.integers(0, n_tpl, int(copies.sum()))]
    # duplicated frame rows: a frame's last row repeats its first (in another chunk when the
    # frame has more than 256 rows), row 7 repeats row 3: ties go to the lower index
    dup_last = np.flatnonzero((sizes >= 2) & (rng.random(F) < 0.5))
    des_q[off[dup_last + 1] - 1] = des_q[off[dup_last]]
    big = np.flatnonzero(sizes >= 255)
    des_q[off[big] + 7] = des_q[off[big] + 3]

    # the layout this case is about
    n_empty, n_single, n_multi = int((sizes == 0).sum()), int((sizes == 1).sum()), int((sizes > 256).sum())
    assert n_empty >= F // 5 and n_single >= 1 and n_multi >= 3, (n_empty, n_single, n_multi)
    assert len(big) >= 5 and len(dup_last) >= 1 and ((sizes[dup_last] > 256).any() or layout != "mixed")
    assert total < 400_000
    if layout == "mixed":
        assert {255, 256, 257}.issubset(set(sizes.tolist()))  # odd and even chunk counts
        assert 0.2 * F < n_empty < 0.4 * F and (sizes[sizes > 0] <= 8).sum() > 0.5 * F
    elif layout == "head_empty":
        assert (sizes[:bound] == 0).all() and sizes[bound:].any()
    elif layout == "tail_empty":
        assert (sizes[-bound:] == 0).all() and sizes[-1] == 0 and sizes[:-bound].any()
    else:
        assert (sizes[:bound] == 0).all() and (sizes[bound:2 * bound] > 0).all() and (sizes[2 * bound:] == 0).all()
    _run_and_check(kind, dev, tpl, des_q, off)


# (kind, n_tpl, D): the six kernel instantiations, each at the sizes that select it
_WALK_SHAPES = [
    ("u8", 40, 7), ("u8", 256, 32),            # knn2_l2u8_kernel<32, 4>
    ("u8", 40, 61), ("u8", 256, 33),           # <64, 4>
    ("u8", 700, 32), ("u8", 8192, 7),          # <32, 8>
    ("u8", 700, 61), ("u8", 8192, 33),         # <64, 8>
    ("hamming", 40, 7), ("hamming", 256, 32), ("hamming", 700, 32), ("hamming", 8192, 32),  # knn2_hamming_kernel<32>
    ("hamming", 256, 33), ("hamming", 700, 61), ("hamming", 8192, 61),                      # <64>
]
_WALK_STRUCTURED = [("u8", 40, 7), ("u8", 256, 33), ("u8", 8192, 7), ("u8", 700, 61), ("hamming", 40, 7),
                    ("hamming", 700, 61)]  # one per instantiation


@pytest.mark.parametrize("kind,n_tpl,D", _WALK_SHAPES)
def test_walk_mixed_frame_sizes(dev, kind, n_tpl, D):
    """F = 2 bound + 37 frames, ~30 % empty, ~60 % of 1-8 rows, ~10 % of 255-520 rows: every
    workgroup walks at least three frames, skips empty ones along its stride, prefetches
    the next frame's first chunk under the current frame's last, and carries the buffer
    parity across frames with odd and even chunk counts."""
    _walk_case(kind, n_tpl, D, "mixed", dev)


@pytest.mark.parametrize("layout", ["head_empty", "tail_empty", "alternating"])
@pytest.mark.parametrize("kind,n_tpl,D", _WALK_STRUCTURED)
def test_walk_structured_empty_runs(dev, kind, n_tpl, D, layout):
    """The same mix with the first `bound` frames empty (every workgroup starts on an empty
    frame), the last `bound` empty (des_q's last row belongs to an earlier frame, every walk
    ends on empties) or alternating blocks of `bound` empty and non-empty frames."""
    _walk_case(kind, n_tpl, D, layout, dev)


# ---------------------------------------------------- B. float matcher: the exact fallback
# A template row u with c bit-identical frame rows equal to u: their phase-1 values are
# equal (equal images and C'), so with c >= 8 the merged top-8 holds one value, the 8th is
# not above the bound of the 2nd and the row is listed for the fallback; with c = 7 it is
# certified and all seven are re-ranked.  Either way the answer is the two lowest copies at
# distance 0.  A lane owns the tile rows with (row >> 2) & 1 == its half.
_SPREAD = [30, 33, 62, 65, 95, 96, 127, 128, 131, 140, 150, 159, 160, 170, 180, 190, 191, 192, 195, 199]


def _copy_rows(placement, c):
    if placement == "one_half":  # one lane half of tile 1
        rows = [64 + r for r in range(64) if (r >> 2) & 1 == 0][:c]
        assert all((r >> 2) & 1 == 0 and r // 64 == 1 for r in rows)
    elif placement == "alternating":  # both halves of tile 1 in turn
        rows = [64 + 8 * (k // 2 // 4) + 4 * (k % 2) + (k // 2) % 4 for k in range(c)]
        halves = [(r >> 2) & 1 for r in rows]
        assert halves == [k % 2 for k in range(c)] and all(r // 64 == 1 for r in rows)
    else:  # several tiles, both sides of the 32-row half-tile boundaries
        rows = _SPREAD[:c]
        assert len({r // 64 for r in rows}) >= 2 and len({r // 32 for r in rows}) >= 3
    assert len(set(rows)) == c
    return sorted(rows)


def _assert_copies(tpl, i, q, rows, ri, rd):
    """Frame q holds exactly the copies `rows` of template row i, and the oracle's answer
    for it is the two lowest of them at distance 0."""
    same = np.flatnonzero((q.view(np.int32) == tpl[i].view(np.int32)).all(axis=1))
    assert same.tolist() == sorted(rows)
    assert ri[i].tolist() == sorted(rows)[:2] and rd[i].tolist() == [0.0, 0.0]


def _far_rows(rng, n, D):
    return rng.normal(0, 1, (n, D)).astype(np.float32)


@pytest.mark.parametrize("D", [128, 27])
def test_f32_identical_rows_fill_the_top8(dev, D):
    """c = 7 (certified, seven candidates re-ranked) and c = 8, 9, 20 (listed) copies of a
    template row, in one lane half, alternating halves, and spread over tiles."""
    rng = np.random.default_rng(D)
    n_tpl, u, n_q = 40, 3, 230
    tpl = _far_rows(rng, n_tpl, D)
    frames, rows_of = [], []
    for placement in ("one_half", "alternating", "spread"):
        for c in (7, 8, 9, 20):
            q = _far_rows(rng, n_q, D)
            rows = _copy_rows(placement, c)
            q[rows] = tpl[u]
            frames.append(q)
            rows_of.append(rows)
    off = _csr([len(q) for q in frames])
    ri, rd = _run_and_check("f32", dev, tpl, np.concatenate(frames), off)
    for f, q in enumerate(frames):
        _assert_copies(tpl, u, q, rows_of[f], ri[f], rd[f])


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 17, 18, 19])
def test_f32_listed_and_certified_rows_share_a_frame(dev, L):
    """L template rows identical to u among ~300 ordinary ones: a frame with 8+ copies of u
    lists exactly those L (slots 0..L-1 of its counter), so the fallback's batch loop runs
    with nb = 4 and every remainder nb = 1, 2, 3, while the ordinary rows are certified."""
    rng = np.random.default_rng(1000 + L)
    n_tpl, D = 300, 128
    def int_rows(n):  # small integers: exact in fp16 at the matcher's scales (asserted below)
        return np.rint(rng.normal(0, 16, (n, D))).astype(np.float32)

    tpl = int_rows(n_tpl)
    twins = sorted(rng.choice(n_tpl, L, replace=False).tolist())  # both workgroups, any wave
    tpl[twins[0]] += np.float32(16)  # u lies off the cloud: its copies are no other row's near neighbours
    tpl[twins] = tpl[twins[0]]
    frames = [int_rows(150), int_rows(90), int_rows(100)]
    rows0, rows2 = _copy_rows("spread", 10), _copy_rows("one_half", 8)
    frames[0][rows0] = tpl[twins[0]]  # frame 1 holds no copy: it lists nothing
    frames[2][rows2] = tpl[twins[0]]
    off = _csr([len(q) for q in frames])
    des_q = np.concatenate(frames)
    # The ordinary rows are certified.  With v = (S + K - |a|^2) / 2 phase 1 lists values in
    # [v (1 - T), v + 2B] and certifies a row when the 8th listed value exceeds the 2nd
    # (1 + 2T) + 2B, which S(8) - S(2) > 8B + 8T (max S + K) implies.  B is the largest
    # beta_j of match_f32.hip's beta_of(); the fp16 images of these descriptors are exact, so
    # its rounding-error norms vanish and its third term is left (5 % slack for the fp32
    # evaluation of the norms).
    s_T = 2.0 ** (15 - np.frexp(np.abs(tpl).max())[1])
    for x, s in ((tpl, s_T), (des_q, s_T / 256)):
        with np.errstate(over="raise"):
            assert ((x * np.float32(s)).astype(np.float16).astype(np.float32) == x * np.float32(s)).all()
    ordinary = np.setdiff1d(np.arange(n_tpl), twins)
    a = tpl.astype(np.float64)
    K, T = (a * a).sum(1).max(), 2.0 ** (5 + 2 - 23)  # at most 3 tiles: key_bits = 7
    for q in frames:
        b = q.astype(np.float64)
        nb = np.sqrt((b * b).sum(1).max())
        B = 1.05 * 1.1 * (4 * D + 8) * 2.0 ** -24 * (np.sqrt(K) + nb) ** 2 + 1e-30
        S = np.sort((a * a).sum(1)[:, None] + (b * b).sum(1)[None] - 2.0 * a @ b.T, axis=1)
        assert (S[ordinary, 7] - S[ordinary, 1] > 4 * (8 * B + 8 * T * (S.max() + K))).all()
    ri, rd = _run_and_check("f32", dev, tpl, des_q, off)
    assert len({tpl[i].tobytes() for i in range(n_tpl)}) == n_tpl - L + 1
    for i in twins:
        _assert_copies(tpl, i, frames[0], rows0, ri[0], rd[0])
        _assert_copies(tpl, i, frames[2], rows2, ri[2], rd[2])
        assert rd[1][i, 0] > 1.0


def test_f32_listed_frames_with_fewer_rows_than_slices(dev):
    """Frames of 8..17 rows that are all copies of u, or copies plus one other row: fewer
    rows than the fallback's 16 slices per frame, so some slices are empty; every template
    row sees 8+ equal values and is listed."""
    rng = np.random.default_rng(77)
    n_tpl, D, u = 20, 128, 6
    tpl = _far_rows(rng, n_tpl, D)
    frames, rows_of = [], []
    for n_q in (8, 9, 15, 16, 17):
        for extra in (False, True):
            q = np.repeat(tpl[u][None], n_q, axis=0)
            rows = list(range(n_q))
            if extra:
                j = int(rng.integers(0, n_q))
                q[j] = _far_rows(rng, 1, D)[0]
                rows.remove(j)
            frames.append(q)
            rows_of.append(rows)
    assert min(len(q) for q in frames) == 8 and max(len(r) for r in rows_of) == 17
    off = _csr([len(q) for q in frames])
    ri, rd = _run_and_check("f32", dev, tpl, np.concatenate(frames), off)
    for f, q in enumerate(frames):
        _assert_copies(tpl, u, q, rows_of[f], ri[f], rd[f])


def test_f32_fallback_kernel_grid_stride(dev):
    """40 listed frames: 40 x 64 work items exceed the fallback kernel's grid of 4 x CUs
    workgroups, which strides over them."""
    rng = np.random.default_rng(78)
    n_tpl, D, u, F = 30, 64, 11, 40
    assert F * 64 > 4 * _cus(dev)
    tpl = _far_rows(rng, n_tpl, D)
    frames, rows_of = [], []
    for f in range(F):
        q = _far_rows(rng, 60 + f % 7, D)
        rows = sorted(rng.choice(len(q), 10, replace=False).tolist())
        q[rows] = tpl[u]
        frames.append(q)
        rows_of.append(rows)
    off = _csr([len(q) for q in frames])
    ri, rd = _run_and_check("f32", dev, tpl, np.concatenate(frames), off)
    for f, q in enumerate(frames):
        _assert_copies(tpl, u, q, rows_of[f], ri[f], rd[f])


def test_f32_fallback_out_kernel_grid_stride(dev):
    """1100 tiny listed frames (ten copies of u and two other rows) among frames of five
    rows, which list nothing (fewer than eight rows are always certified): more listed
    frames than the 1024 workgroups of the kernel that writes the fallback's results."""
    rng = np.random.default_rng(79)
    n_tpl, D, u = 5, 8, 2
    tpl = _far_rows(rng, n_tpl, D)
    frames, rows_of = [], []
    for f in range(1650):
        if f % 3 == 2:
            frames.append(_far_rows(rng, 5, D))
            rows_of.append(None)
            continue
        q = _far_rows(rng, 12, D)
        rows = sorted(rng.choice(12, 10, replace=False).tolist())
        q[rows] = tpl[u]
        frames.append(q)
        rows_of.append(rows)
    assert sum(r is not None for r in rows_of) == 1100 > 1024
    off = _csr([len(q) for q in frames])
    ri, rd = _run_and_check("f32", dev, tpl, np.concatenate(frames), off)
    for f, q in enumerate(frames):
        if rows_of[f] is not None:
            _assert_copies(tpl, u, q, rows_of[f], ri[f], rd[f])
        else:
            assert len(q) < 8 and rd[f][u, 0] > 0.0


def test_f32_coarse_keys_on_a_40000_row_frame(dev):
    """One frame of 40 000 rows (625 tiles: key_bits = 15, so a key keeps 8 bits below the
    value's leading one) with near rows and copies, next to a 3-row frame whose single tile
    sits in a 625-tile slot."""
    rng = np.random.default_rng(80)
    n_tpl, D, n_q = 64, 32, 40000
    tiles = -(-n_q // 64)
    assert 5 + int(np.ceil(np.log2(tiles))) == 15
    tpl = _far_rows(rng, n_tpl, D)
    q = _far_rows(rng, n_q, D)
    near = rng.choice(n_q, 2000, replace=False)
    q[near] = tpl[rng.integers(0, n_tpl, 2000)] + rng.normal(0, 0.02, (2000, D)).astype(np.float32)
    rows = sorted(rng.choice(np.setdiff1d(np.arange(n_q), near), 10, replace=False).tolist())
    q[rows] = tpl[5]
    small = _far_rows(rng, 3, D)
    small[1] = tpl[9]
    off = _csr([n_q, 3])
    ri, rd = _run_and_check("f32", dev, tpl, np.concatenate([q, small]), off)
    _assert_copies(tpl, 5, q, rows, ri[0], rd[0])
    assert ri[1][9, 0] == 1 and rd[1][9, 0] == 0.0 and (ri[1] >= 0).all()


# ------------------------------------------------- C. float matcher: range and layout edges
def test_f32_fp16_range_boundary(dev):
    """The template's largest element is exactly 1, so s_T = 2^14 and frames are scaled by
    s_f = 2^6: an element 1023.5 lands on 65504, fp16's largest value (the frame is not
    flagged), 1023.75 on 65520 (flagged: the whole frame falls back), either sign, with a
    healthy frame between them."""
    rng = np.random.default_rng(81)
    n_tpl, D = 50, 64
    tpl = rng.uniform(-0.9, 0.9, (n_tpl, D)).astype(np.float32)
    tpl[17, 5] = 1.0
    assert np.abs(tpl).max() == 1.0 and np.frexp(np.float32(1.0))[1] == 1  # 1 < 2^1: s_T = 2^(15 - 1)
    assert np.float32(1023.5) * np.float32(64) == np.float32(65504)
    assert np.float32(1023.75) * np.float32(64) == np.float32(65520)
    frames = []
    for v in (1023.5, None, 1023.75, -1023.5, None, -1023.75):
        q = rng.uniform(-1, 1, (100, D)).astype(np.float32)
        q[:20] = tpl[rng.integers(0, n_tpl, 20)] + rng.normal(0, 0.01, (20, D)).astype(np.float32)
        if v is not None:
            q[70, 9] = v
            q[3, 63] = v  # also in a row that is some template row's best match
        frames.append(q)
    off = _csr([len(q) for q in frames])
    _run_and_check("f32", dev, tpl, np.concatenate(frames), off)


@pytest.mark.parametrize("scale,D", [(1e-20, 24), (1e-12, 128), (1e17, 128), (1e18, 128), (1.3e18, 128)])
def test_f32_extreme_scales(dev, scale, D):
    """Template and frames scaled alike, with exact copies and rows one ulp off a template
    row.  1e-20 at D = 24: |a|^2, S and the phase-1 values are fp32 subnormals; 1e17: squared
    norms ~1e36; 1e18: K = 1.7e38, (sqrt K + |b|)^2 overflows fp32 and so do 0.7 % of the
    squared distances; 1.3e18: 96 % of them do (a distance of inf is never a neighbour, in
    the oracle as in the kernels: such rows answer -1 / FLT_MAX)."""
    rng = np.random.default_rng(D + 3)
    n_tpl = 100
    tpl = (rng.normal(0, 1, (n_tpl, D)) * scale).astype(np.float32)
    frames = []
    for n_q in (300, 70, 5):
        q = (rng.normal(0, 1, (n_q, D)) * scale).astype(np.float32)
        q[: n_q // 4] = tpl[rng.integers(0, n_tpl, n_q // 4)]
        for k in range(n_q // 4, n_q // 4 + min(3, n_q // 4)):  # near-ties with the copy of row 7 below
            q[k] = tpl[7]
            q[k, k % D] = np.nextafter(q[k, k % D], np.float32(np.inf), dtype=np.float32)
        q[-1] = tpl[7]
        frames.append(q)
    off = _csr([len(q) for q in frames])
    ri, rd = _run_and_check("f32", dev, tpl, np.concatenate(frames), off)
    assert np.isfinite(rd).all() and (rd[0] >= 0).all()
    if scale == 1e-20:  # the precondition: the distances' squares are fp32 subnormals
        assert 0 < np.median(rd[0][:, 1].astype(np.float64) ** 2) < np.finfo(np.float32).tiny


@pytest.mark.parametrize("zero", ["template", "frame", "both"])
def test_f32_all_zero_descriptors(dev, zero):
    """An all-zero template (K = 0, s_T = 1), an all-zero frame among random ones, and both:
    every distance ties, so every row answers indices 0 and 1."""
    rng = np.random.default_rng(82)
    n_tpl, D = 40, 64
    tpl = _far_rows(rng, n_tpl, D)
    frames = [_far_rows(rng, 100, D), _far_rows(rng, 100, D), _far_rows(rng, 5, D), _far_rows(rng, 70, D)]
    if zero in ("template", "both"):
        tpl[:] = 0
    if zero == "frame":
        frames[1][:] = 0
        frames[2][:] = 0
    if zero == "both":
        for q in frames:
            q[:] = 0
    off = _csr([len(q) for q in frames])
    ri, rd = _run_and_check("f32", dev, tpl, np.concatenate(frames), off)
    if zero == "both":
        assert (ri == [0, 1]).all() and (rd == 0).all()
    if zero == "frame":
        assert (ri[1] == [0, 1]).all() and (rd[1][:, 0] == rd[1][:, 1]).all()


@pytest.mark.parametrize("shifted", ["des_q", "des_tpl"])
def test_f32_buffers_off_16_byte_alignment(dev, shifted):
    """D = 100 (D % 4 == 0) with des_q or des_tpl starting 4 bytes into a larger buffer: the
    image, re-rank and fallback kernels take their scalar paths; same answer as aligned."""
    rng = np.random.default_rng(83)
    n_tpl, D = 60, 100
    tpl = _far_rows(rng, n_tpl, D)
    frames = [_far_rows(rng, 150, D), _far_rows(rng, 70, D)]
    frames[0][_copy_rows("spread", 9)] = tpl[4]  # a listed row: the fallback scan runs too
    frames[1][:30] = tpl[rng.integers(0, n_tpl, 30)] + rng.normal(0, 0.05, (30, D)).astype(np.float32)
    des_q = np.concatenate(frames)
    off = _csr([len(q) for q in frames])

    def shifted_copy(a):
        buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
        assert buf.data_ptr() % 16 == 0
        v = buf[1:1 + a.size].view(a.shape)
        v.copy_(_t(a, dev))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    q_dev, t_dev = _t(des_q, dev), _t(tpl, dev)
    assert q_dev.data_ptr() % 16 == 0 and t_dev.data_ptr() % 16 == 0
    _run_and_check("f32", dev, tpl, des_q, off, des_q_dev=q_dev, tpl_dev=t_dev)
    if shifted == "des_q":
        q_dev = shifted_copy(des_q)
    else:
        t_dev = shifted_copy(tpl)
    ri, rd = _run_and_check("f32", dev, tpl, des_q, off, des_q_dev=q_dev, tpl_dev=t_dev)
    _assert_copies(tpl, 4, frames[0], _copy_rows("spread", 9), ri[0], rd[0])

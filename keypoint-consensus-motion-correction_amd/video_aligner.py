"""VideoAligner with the reference's public surface, running the hot path on MI355X.

Mirror of /root/reference/VideoAligner.py (VA:15-510): same class names, class
constants, ``align_images`` signature/returns and per-frame static helpers.  The
per-frame joblib stages (VA:117-123, 137-142, 150) are replaced by one batched HIP
launch each (``pipeline.align_slab``); the helpers that the reference runs per frame
(``_get_frame_keypoints``, ``_compute_euclidean_affine``, ``_apply_affine``) run the
same kernels on a batch of one, so code written against the reference keeps working.

Differences, all deliberate:
  * Keypoint detection still needs an OpenCV-compatible detector object
    (``detectAndCompute(img, mask) -> (keypoints with .pt, uint8 descriptors)``).
    OpenCV is not part of this image; ``DETECTOR_CONSTRUCTOR_DICT`` uses cv2 when it is
    importable and accepts any registered factory.  ``align_keypoints`` is the hot-path
    entry for precomputed keypoints/descriptors.
  * numpy >= 1.24 made the reference crash on ragged per-frame point lists (VA:284-285);
    ``_lookup_consensus_kps`` returns numpy<1.24-style object arrays instead.
  * Constants are read from the instance's class, so subclass overrides take effect
    everywhere (the reference's static methods read ``VideoAligner.X``; defaults equal).
"""
from __future__ import annotations

import time
from collections import Counter
from logging import LoggerAdapter, getLogger
from multiprocessing import cpu_count
from typing import Callable, List, Optional, Sequence, Set, Tuple, Union

import numpy as np
import torch

from . import affines as _aff
from . import _intensity as _in
from . import bidi as _bd
from . import fallback as _fb
from . import multidevice as _md
from . import piecewise as _pw
from . import pipeline as _pl
from . import prefilter as _pf
from . import quality as _q
from . import refine as _rf
from . import refine_field as _rff
from . import stages
from . import summary as _sm
from .affines import AlignmentError


def _cv2_factory(name: str) -> Callable:
    def make():
        try:
            import cv2  # type: ignore
        except ImportError as e:  # pragma: no cover - cv2 absent in this image
            raise RuntimeError(
                f"OpenCV is not installed, so '{name}' is unavailable: register a detector factory in "
                "VideoAligner.DETECTOR_CONSTRUCTOR_DICT or call align_keypoints() with precomputed keypoints"
            ) from e
        return getattr(cv2, name)()

    make.__name__ = name
    return make


class _CvKeyPoint:
    __slots__ = ("pt",)

    def __init__(self, x: float, y: float):
        self.pt = (x, y)


class GpuOrbDetector:
    """The build's ORB-style detector (csrc/orb.hip) behind the OpenCV
    detector interface the reference uses (VA:114-116, VA:190-192):
    ``detectAndCompute(img_u8, mask) -> (keypoints with .pt, uint8 [n, 32] descriptors)``.
    ``align_images`` recognises it and detects on the whole device-resident stack at once."""

    def __init__(self, params=None):
        from . import orb

        self.params = params or orb.OrbParams()

    def detectAndCompute(self, image, mask=None):  # noqa: N802 (OpenCV's name)
        if mask is not None:
            raise NotImplementedError("detection masks are not supported by the GPU detector")
        dev = torch.device("cuda", torch.cuda.current_device())
        img = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image, np.uint8))
        k = stages.detect_orb(img.to(dev).reshape(1, *img.shape[-2:]).contiguous(), self.params)
        n = int(k.count.cpu()[0])
        kp = k.kp[0, :n].cpu().numpy()
        return [_CvKeyPoint(float(x), float(y)) for x, y in kp], k.des[0, :n].cpu().numpy()


def _gpu_orb_multiscale() -> GpuOrbDetector:
    """The same detector on an 8-level scale pyramid of ratio 1.2: keeps
    matching under the magnification changes the similarity model is there for."""
    from . import orb

    return GpuOrbDetector(orb.OrbParams(n_levels=8))


def _as_numpy(x) -> np.ndarray:
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


class VideoAligner:
    AlignmentError = AlignmentError

    FRAME_SAMPLE_RATE = 100  # Hz
    SPATIAL_DOWNSAMPLE_RATE = 1
    N_JOBS_PARALLEL = cpu_count()
    DETECTOR_CONSTRUCTOR_DICT = {
        "akaze": _cv2_factory("AKAZE_create"),
        "brisk": _cv2_factory("BRISK_create"),
        # New: the build's exact ORB-style detector on the GPU (no OpenCV needed).
        "orb": GpuOrbDetector,
        # New: the same on a scale pyramid (8 levels, ratio 1.2), for zoom drift / focus breathing.
        "orb_ms": _gpu_orb_multiscale,
    }
    N_KP_GLOBAL_MIN = 5
    N_KP_FRAME_SKIP = 3
    TEMPLATE_FRAME_LOC = 0.5
    MAX_FRAC_INTERPOLATED = 0.2
    DESCRIPTOR_DISTANCE_RATIO_THRESH = 0.75
    MEDIAN_KEYPOINT_INLIER_DISTANCE_RANGE = (0.5, 2.0)
    IMAGE_NORM_MAX_PERCENTILE = 99.99
    MAX_PIXEL_UINT8 = 255
    RANSAC_MIN_SAMPLES = 2
    RANSAC_RESIDUAL_THRESH = 2
    RANSAC_MAX_TRIALS = 1000
    RANDOM_SEED = 42
    # New: the GPUs align_images / align_keypoints spread the frames over, as the
    # reference's _parallelize spreads them over every core (VA:21, VA:460-471): None = every
    # visible device (the current one first; one contiguous frame slab per device, the
    # cross-frame consensus and gap interpolation made once on the host, kcmc_amd.multidevice);
    # a list pins them (a device may repeat: two slabs on one GPU).
    DEVICES: Optional[Sequence[int]] = None
    # New: one GPU for everything (used when DEVICES is None; None = as DEVICES).  The
    # per-frame helpers (_get_frame_keypoints, _compute_euclidean_affine, _apply_affine)
    # run on the first device.
    DEVICE: Optional[int] = None
    # New (extension, BASELINE configs 3-5): the skimage model class RANSAC fits --
    # "euclidean" (the reference's EuclideanTransform, VA:311), "similarity"
    # (SimilarityTransform, min_samples 2: rigid plus one scale; the second return value of
    # align_images / align_keypoints is then [n, 4] = (tx, ty, rotation, scale)), "affine"
    # (AffineTransform, min_samples 3) or "projective" (ProjectiveTransform, min_samples 4,
    # frames warped with warpPerspective).
    RANSAC_MODEL = "euclidean"
    # New (opt-in, not the reference's matcher): the BFMatcher norm -- "l2" (the
    # reference's cv2.BFMatcher() default, VA:194) or "hamming" (NORM_HAMMING, for binary
    # ORB/BRIEF/AKAZE descriptors; csrc/match_hamming.hip).
    MATCH_NORM = "l2"
    # New (opt-in, kcmc_amd.quality): after the alignment, the mean image of the registered
    # sample frames, the region valid in every frame and every frame's correlation with the
    # mean image over it (frame_correlations, mean_image, valid_region, correlation_history).
    QUALITY_METRICS = False
    # New (opt-in; > 0 implies the metrics): that many more passes of the hot path, each
    # against the mean of the best-registered TEMPLATE_REFINE_TOP_FRAC of the previous pass's
    # sample frames (template_image) instead of one raw frame.  The frames' normalisation,
    # detection and keypoints are reused; only the template is detected again.
    TEMPLATE_REFINE_ITERS = 0
    TEMPLATE_REFINE_TOP_FRAC = 0.5
    # New (opt-in, kcmc_amd.summary; build-defined, the reference reports nothing about the
    # aligned stack): the summary images of the last pass's aligned stack, over all its frames
    # and the region valid in every frame (summary_region, quality.valid_region of the final
    # maps) -- summary_mean_image, max_image (the max projection), std_image (the temporal
    # standard deviation), correlation_image (each pixel's mean correlation over time with its
    # SUMMARY_NEIGHBOURS = 4 or 8 neighbours) and crispness (the norm of the mean image's
    # gradient), from one more read of the stack (csrc/temporal_sums.hip).  Needs no
    # QUALITY_METRICS and leaves its results alone.  Grayscale stacks, 2 x 3 models, not with
    # PIECEWISE_GRID / REFINE_GRID.
    SUMMARY_IMAGES = False
    SUMMARY_NEIGHBOURS = 8
    # New (opt-in, kcmc_amd.piecewise; build-defined, the reference has no such mode):
    # piecewise-rigid correction.  (gy, gx), each in [1, 16]: after the global RANSAC every sample
    # frame fits one rigid model per grid cell from the consensus points in the cell's window
    # (PIECEWISE_WINDOW cell sizes to each side; cells with fewer than PIECEWISE_MIN_POINTS
    # points have none), the residual of each accepted cell model against the global map at
    # the cell's node (dropped above PIECEWISE_MAX_RESIDUAL px) becomes a displacement field,
    # and the frames are made by the field warp (affines, the transform summary and the
    # skipped list stay what they are without the grid).  Results: patch_residuals,
    # patch_points, patch_fitted.  Grayscale stacks, first device only.
    PIECEWISE_GRID: Optional[Tuple[int, int]] = None
    PIECEWISE_WINDOW = 1.0
    PIECEWISE_MIN_POINTS = 6
    PIECEWISE_MAX_RESIDUAL = 8.0
    # New (opt-in, kcmc_amd.fallback; build-defined, the reference has no such mode): what
    # happens to the sample frames RANSAC gave no model (skipped_idxs).  "interpolate": the
    # reference's behaviour, their maps are interpolated from their neighbours.  "correlation":
    # after that, each of them is searched against the mean image of the registered sample
    # frames at every integer shift within FALLBACK_RADIUS px (exact Pearson correlation over
    # the valid region shrunk by the radius, csrc/shift_search.hip); a peak above
    # FALLBACK_MIN_CORRELATION that is not on the window's border -- refined by a parabola per
    # axis with FALLBACK_SUBPIXEL -- corrects the frame's map, and the frame is warped again
    # from its source.  Only frames in skipped_idxs are touched; skipped_idxs and
    # interpolated_idxs stay what they are.  Results: fallback_shifts, fallback_correlations,
    # fallback_idxs.  Grayscale stacks, 2 x 3 models, not with PIECEWISE_GRID.
    FALLBACK = "interpolate"
    FALLBACK_RADIUS = 8             # 1..16 px
    FALLBACK_MIN_CORRELATION = 0.0  # r <= this: no resemblance, keep the interpolated map
    FALLBACK_SUBPIXEL = True
    # New (opt-in, kcmc_amd.refine; build-defined, the reference has no such mode): the dense
    # step after the keypoints.  "intensity": REFINE_ITERS times, every frame of the stack
    # (sample or not, skipped or not) takes one linearised least-squares step against the mean
    # image of the registered sample frames over the valid region -- gain, offset, translation
    # and, with REFINE_MOTION = "rigid", a small rotation about the region's centre, from
    # seven exact integer sums per frame (csrc/refine.hip); the step is limited to
    # REFINE_MAX_STEP px at the region's corners, composed into the frame's map, the frame is
    # warped again from its source, and the step is kept only where the frame's correlation
    # with the mean image rose.  Runs after the fallback when both are on; skipped_idxs and
    # interpolated_idxs stay what they are.  Results: refine_steps, refine_correlations,
    # refine_idxs.  Grayscale stacks, 2 x 3 models, not with PIECEWISE_GRID.
    REFINE = "none"
    REFINE_ITERS = 2
    REFINE_MOTION = "rigid"         # or "translation"
    REFINE_MAX_STEP = 1.0           # px
    # New (opt-in, kcmc_amd.refine_field; build-defined): the non-rigid step after that one,
    # with REFINE = "intensity" only.  (gy, gx), each in [1, 16]: REFINE_GRID_ITERS times, every
    # frame takes the same least-squares step (gain, offset, translation) on a window around
    # every node of the grid -- the node's cell and half a cell to each side -- from five exact
    # integer sums per tile of one read of the aligned stack (csrc/refine_tiles.hip), over the
    # valid region shrunk by ceil(REFINE_GRID_ITERS * REFINE_MAX_STEP); a node's step is
    # limited to REFINE_MAX_STEP px, added to the frame's field, the frame is made again from
    # its source by the field warp, and the field is kept only where the frame's correlation
    # with the mean image rose.  affines, the transform summary, skipped_idxs and
    # interpolated_idxs stay what they are.  Results: refine_field, refine_field_correlations,
    # refine_field_idxs.  Not with QUALITY_METRICS / TEMPLATE_REFINE_ITERS.
    REFINE_GRID: Optional[Tuple[int, int]] = None
    REFINE_GRID_ITERS = 1
    # New (opt-in, csrc/warp_cubic.hip; build-defined, the reference always resamples with
    # INTER_LINEAR): the interpolation of every warp of the frames.  "linear": the reference's.
    # "cubic": OpenCV's classic INTER_CUBIC restated (cubic convolution, A = -3/4, 4 x 4 taps;
    # include/kcmc.h; parity with cv2 unpinned) -- aligned_imgs, the fallback's and the
    # refinement's warps and _apply_affine resample bicubically and valid_region keeps the wider
    # footprint's margin; transforms, affines, skipped_idxs and interpolated_idxs are what they
    # are with "linear" (the intensity passes read the resampled frames, so their corrections may
    # differ).  Grayscale stacks, 2 x 3 models, not with PIECEWISE_GRID / REFINE_GRID (the field
    # warp stays bilinear).
    WARP_INTERPOLATION = "linear"
    # New (opt-in, kcmc_amd.bidi; build-defined, the reference has no such mode): the phase
    # correction of bidirectionally scanned stacks, whose odd rows are displaced horizontally
    # against the even rows by a constant.  "none": off.  "auto": the offset is measured on
    # bidi.sample_indices(n, BIDI_PHASE_FRAMES) of the raw frames -- Pearson's r of the odd rows
    # read at x + d with their even neighbours at x for every d within BIDI_PHASE_RADIUS, from
    # exact integer sums pooled over the frames (csrc/bidi_phase.hip) -- and the peak is taken
    # unless it sits on the window's border or gains no more than BIDI_PHASE_MIN_GAIN over
    # d = 0.  An int in [-16, 16]: applied as given.  A non-zero offset d replaces every odd row
    # by row[clamp(x + d)] (whole pixels, the edge pixel replicated; up to half a pixel
    # remains) once the frames are on their device(s) and before anything else: the corrected
    # stack is the source of the normalisation, the detection, the template frame, every warp
    # and every later pass, exactly as if the caller had passed it.  The aligner's own upload
    # is corrected in place, a caller's device tensor into a new one (memory the caller can see
    # is never written).  Results: bidi_offset, bidi_correlations, bidi_frames, bidi_accepted.
    # Grayscale stacks.
    BIDI_PHASE: Union[str, int] = "none"
    BIDI_PHASE_RADIUS = 8           # 1..16 px
    BIDI_PHASE_FRAMES = 64          # >= 1
    BIDI_PHASE_MIN_GAIN = 0.0
    # New (opt-in, kcmc_amd.prefilter; build-defined, the reference has no such mode): a box
    # band-pass in front of the keypoint detection, for one-photon / miniscope / widefield stacks
    # (cells a few hundred grey levels high on a background of tens of thousands: after the
    # max-scaling FAST sees the vignette only) and for shot-noise-limited frames.  Both 0: off,
    # nothing runs and nothing is allocated.  DETECT_SMOOTH_RADIUS s in [0, 4],
    # DETECT_BACKGROUND_RADIUS r either 0 or in [s + 1, 32]: align_images detects on a copy of the
    # stack with every pixel replaced by max(m_s - m_r, 0) -- m_rho the rounded mean over the
    # (2 rho + 1)^2 box clipped to the image, m_r = 0 with r = 0 (csrc/band_filter.hip,
    # include/kcmc.h) -- made after BIDI_PHASE has corrected the stack.  The copy feeds the
    # percentile, the max-scaling, the downsample and the detection (GPU or host detector); the
    # template frame is taken from it, a masked_template and the refined template of
    # TEMPLATE_REFINE_ITERS are filtered the same way (template_image stays the mean of the raw
    # aligned frames).  Every warp and every later pass -- the fallback, the refinements, the
    # metrics, the summary images -- reads the raw (phase-corrected) stack as without the switch:
    # the transforms, affines, skipped_idxs and interpolated_idxs are what the plain aligner
    # returns for the filtered stack, aligned_imgs is the raw stack warped by those maps.  The
    # copy is released once the uint8 stack exists: the peak device memory per slab is raw +
    # filtered + uint8.  A stack the filter flattens completely (its percentile is 0) is an
    # AlignmentError.  align_keypoints has no detection to feed: it validates the constants and
    # ignores them.  Results: prefilter_radii, prefilter_brightest_px.  Grayscale stacks.
    DETECT_SMOOTH_RADIUS = 0
    DETECT_BACKGROUND_RADIUS = 0

    def __init__(self, logger: LoggerAdapter = None):
        self.logger = logger
        if self.logger is None:
            self.logger = getLogger(self.__class__.__name__)
        self.affines = None
        self.aligned_imgs = None
        self.interpolated_idxs = None
        self._kp_template = None
        self._des_template = None
        self._logged_one_device = False
        self._reset_quality()
        self._reset_summary()
        self._reset_piecewise()
        self._reset_fallback()
        self._reset_refine()
        self._reset_bidi()
        self._reset_prefilter()

    # ------------------------------------------------------------------ helpers
    @classmethod
    def _all_devices(cls) -> List[int]:
        """The configured devices: DEVICES, else [DEVICE], else every visible device with the
        current one first."""
        if not torch.cuda.is_available():
            from ._lib import KcmcLibraryError

            raise KcmcLibraryError("no GPU visible: the kcmc hot path runs on MI355X only (no CPU fallback)")
        if cls.DEVICES is not None:
            devs = [int(d) for d in cls.DEVICES]
            if not devs:
                raise ValueError("VideoAligner.DEVICES is empty")
            return devs
        if cls.DEVICE is not None:
            return [int(cls.DEVICE)]
        cur = torch.cuda.current_device()
        return [cur] + [d for d in _md.visible_devices() if d != cur]

    @classmethod
    def _devices(cls) -> List[int]:
        """The devices of the hot path (_all_devices); the first one only with PIECEWISE_GRID
        (the piecewise-rigid mode runs on one device in this version)."""
        devs = cls._all_devices()
        return devs[:1] if cls.PIECEWISE_GRID is not None else devs

    @classmethod
    def _device(cls) -> torch.device:
        return torch.device("cuda", cls._devices()[0])

    def _config(self, n_kp_global: int, frame_downsample_rate: int = 1) -> _pl.AlignConfig:
        cls = type(self)
        d_lo, d_hi = (0.5, 2)  # hard-coded at VA:209 (MEDIAN_KEYPOINT_INLIER_DISTANCE_RANGE is unused there)
        return _pl.AlignConfig(
            n_kp_global=int(n_kp_global), n_kp_global_min=cls.N_KP_GLOBAL_MIN, n_kp_frame_skip=cls.N_KP_FRAME_SKIP,
            ratio=cls.DESCRIPTOR_DISTANCE_RATIO_THRESH, d_lo=d_lo, d_hi=d_hi, ransac_trials=cls.RANSAC_MAX_TRIALS,
            ransac_threshold=float(cls.RANSAC_RESIDUAL_THRESH), ransac_min_samples=cls.RANSAC_MIN_SAMPLES,
            seed=cls.RANDOM_SEED, spatial_rate=cls.SPATIAL_DOWNSAMPLE_RATE,
            frame_downsample_rate=int(frame_downsample_rate), ransac_model=cls.RANSAC_MODEL,
            match_norm=cls.MATCH_NORM,
            piecewise_grid=None if cls.PIECEWISE_GRID is None else _pw.check_grid(cls.PIECEWISE_GRID),
            piecewise_window=float(cls.PIECEWISE_WINDOW), piecewise_min_points=int(cls.PIECEWISE_MIN_POINTS),
            piecewise_max_residual=float(cls.PIECEWISE_MAX_RESIDUAL),
            warp_interpolation=stages.check_interpolation(cls.WARP_INTERPOLATION))

    # ------------------------------------------------------------- the warp's interpolation
    def _interpolation_on(self, images=None) -> str:
        """WARP_INTERPOLATION, after the checks that must fail before any work (``images``: only
        its number of dimensions is read, when it has one)."""
        try:
            interp = stages.check_interpolation(self.WARP_INTERPOLATION)
        except ValueError:
            raise ValueError("WARP_INTERPOLATION must be 'linear' or 'cubic', got "
                             f"{self.WARP_INTERPOLATION!r}") from None
        if interp == "linear":
            return interp
        if self.RANSAC_MODEL == "projective":
            raise NotImplementedError("WARP_INTERPOLATION = 'cubic' does not support RANSAC_MODEL = 'projective' "
                                      "(warpPerspective stays bilinear)")
        if getattr(images, "ndim", 3) != 3:
            raise NotImplementedError("WARP_INTERPOLATION = 'cubic' supports grayscale stacks [F, H, W] only")
        if self.PIECEWISE_GRID is not None:
            raise NotImplementedError("WARP_INTERPOLATION = 'cubic' does not run together with PIECEWISE_GRID (the "
                                      "field warp stays bilinear)")
        if self.REFINE_GRID is not None:
            raise NotImplementedError("WARP_INTERPOLATION = 'cubic' does not run together with REFINE_GRID (the "
                                      "field warp stays bilinear)")
        return interp

    # ------------------------------------------------- bidirectional-scan phase correction
    def _reset_bidi(self) -> None:
        self.bidi_offset = None
        self.bidi_correlations = None
        self.bidi_frames = None
        self.bidi_accepted = None

    def _bidi_on(self, images=None):
        """BIDI_PHASE -- None for "none", else "auto" or the int -- after the checks that must fail
        before any work (``images``: only its number of dimensions is read, when it has one)."""
        mode = self.BIDI_PHASE
        if isinstance(mode, str):
            if mode == "none":
                return None
            if mode != "auto":
                raise ValueError(f"BIDI_PHASE must be 'none', 'auto' or an integer in [-16, 16], got {mode!r}")
        else:
            try:
                mode = _bd.check_shift(mode)
            except ValueError:
                raise ValueError("BIDI_PHASE must be 'none', 'auto' or an integer in [-16, 16], got "
                                 f"{self.BIDI_PHASE!r}") from None
        radius, k, gain = self.BIDI_PHASE_RADIUS, self.BIDI_PHASE_FRAMES, self.BIDI_PHASE_MIN_GAIN
        if not (_bd._is_int(radius) and 1 <= int(radius) <= _bd.MAX_RADIUS):
            raise ValueError(f"BIDI_PHASE_RADIUS must be an integer in [1, {_bd.MAX_RADIUS}], got {radius!r}")
        if not (_bd._is_int(k) and int(k) >= 1):
            raise ValueError(f"BIDI_PHASE_FRAMES must be an integer >= 1, got {k!r}")
        if isinstance(gain, bool) or not isinstance(gain, (int, float, np.integer, np.floating)) or gain != gain:
            raise ValueError(f"BIDI_PHASE_MIN_GAIN must be a number, got {gain!r}")
        if getattr(images, "ndim", 3) != 3:
            raise NotImplementedError("BIDI_PHASE supports grayscale stacks [F, H, W] only")
        return mode

    def _bidi_correct(self, parts: List[torch.Tensor], own: bool) -> List[torch.Tensor]:
        """The slabs of the stack with the phase correction applied (``parts`` themselves with the
        switch off or an offset of 0).  ``own``: the slabs are the aligner's own upload and are
        corrected in place; otherwise into new tensors."""
        mode = self._bidi_on()
        if mode is None:
            return parts
        if not own:
            parts = [p.contiguous() for p in parts]
        if mode == "auto":
            R = int(self.BIDI_PHASE_RADIUS)
            H, W = parts[0].shape[1:]
            idx = _bd.sample_indices(sum(p.shape[0] for p in parts), int(self.BIDI_PHASE_FRAMES))
            off, r, ok = _bd.estimate_offset(_bd.phase_sums(parts, idx, R), _bd.sample_count(H, W, R),
                                             float(self.BIDI_PHASE_MIN_GAIN))
            self.bidi_correlations, self.bidi_frames, self.bidi_accepted = r, idx, ok
            self.logger.info(f"bidirectional phase: offset {off} px from {len(idx)} frames"
                             + ("" if ok else " (no acceptable peak)"))
        else:
            off = int(mode)
            self.bidi_correlations, self.bidi_frames, self.bidi_accepted = None, [], True
        self.bidi_offset = off
        if off != 0:
            parts = _bd.shift_rows(parts, off, 1, out=parts if own else None)
        return parts

    def _bidi_source(self, parts, own: bool, template, template_idx: Optional[int]):
        """(_bidi_correct(parts, own), the template): the template frame is taken again from the
        corrected stack when it came from the stack (``template_idx``; None: a masked_template,
        which is used as given)."""
        parts = self._bidi_correct(parts, own)
        if self.bidi_offset and template_idx is not None:
            f0 = 0
            for p in parts:
                if f0 <= template_idx < f0 + p.shape[0]:
                    template = _as_numpy(p[template_idx - f0])
                f0 += p.shape[0]
        return parts, template

    # ------------------------------------------------- band-pass prefilter of the detection
    def _reset_prefilter(self) -> None:
        self.prefilter_radii = None
        self.prefilter_brightest_px = None

    def _prefilter_on(self, images=None) -> Optional[Tuple[int, int]]:
        """(s, r) of DETECT_SMOOTH_RADIUS / DETECT_BACKGROUND_RADIUS, None with both 0, after the
        checks that must fail before any work (``images``: only its number of dimensions is read,
        when it has one)."""
        s, r = self.DETECT_SMOOTH_RADIUS, self.DETECT_BACKGROUND_RADIUS
        if _pf._is_int(s) and _pf._is_int(r) and int(s) == 0 and int(r) == 0:
            return None
        try:
            radii = _pf.check_radii(s, r)
        except ValueError as e:
            raise ValueError(f"DETECT_SMOOTH_RADIUS / DETECT_BACKGROUND_RADIUS: {e}") from None
        if getattr(images, "ndim", 3) != 3:
            raise NotImplementedError("DETECT_SMOOTH_RADIUS / DETECT_BACKGROUND_RADIUS support grayscale stacks "
                                      "[F, H, W] only")
        return radii

    def _prefilter_image(self, image_u16) -> np.ndarray:
        """One [H, W] uint16 image in the detection's intensity domain: filtered on the first device
        of the hot path with the switch on, as given with it off."""
        radii = self._prefilter_on()
        image = _as_numpy(image_u16)
        if radii is None:
            return image
        with torch.cuda.device(self._device()):
            t = torch.from_numpy(np.ascontiguousarray(image, np.uint16)[None]).to(self._device())
            return _pf.box_bandpass(t, *radii)[0].cpu().numpy()

    def _prefilter_source(self, parts: List[torch.Tensor], template, template_idx: Optional[int]):
        """(the slabs the detection reads, the template in their domain): ``parts`` and ``template``
        themselves with the switch off; with it on, the filtered copies of the slabs and the
        template frame taken from them (``template_idx``; None: a masked_template, filtered by the
        same call)."""
        radii = self._prefilter_on()
        if radii is None:
            return parts, template
        self.prefilter_radii = radii
        filtered = _pf.box_bandpass([p.contiguous() for p in parts], *radii)
        if template_idx is None:
            return filtered, self._prefilter_image(template)
        f0 = 0
        for p in filtered:
            if f0 <= template_idx < f0 + p.shape[0]:
                template = _as_numpy(p[template_idx - f0])
            f0 += p.shape[0]
        return filtered, template

    # ------------------------------------------------------------- piecewise-rigid correction
    def _reset_piecewise(self) -> None:
        self.patch_residuals = None
        self.patch_points = None
        self.patch_fitted = None

    def _piecewise_on(self, images=None) -> bool:
        """Whether the piecewise-rigid mode runs, after the checks that must fail before any
        work (``images``: only its number of dimensions is read, when it has one)."""
        if self.PIECEWISE_GRID is None:
            return False
        _pw.check_grid(self.PIECEWISE_GRID)
        _pw.check_options(self.PIECEWISE_MIN_POINTS, self.PIECEWISE_WINDOW, self.PIECEWISE_MAX_RESIDUAL)
        if self.RANSAC_MODEL == "projective":
            raise NotImplementedError("PIECEWISE_GRID does not support RANSAC_MODEL = 'projective' (the field "
                                      "warp adds its displacement to an affine source coordinate)")
        if bool(self.QUALITY_METRICS) or int(self.TEMPLATE_REFINE_ITERS) > 0:
            raise NotImplementedError("PIECEWISE_GRID does not run together with QUALITY_METRICS / "
                                      "TEMPLATE_REFINE_ITERS (the valid region of a field warp is not defined yet)")
        if getattr(images, "ndim", 3) != 3:
            raise NotImplementedError("PIECEWISE_GRID supports grayscale stacks [F, H, W] only")
        return True

    def _log_one_device(self) -> None:
        if self.PIECEWISE_GRID is not None and not self._logged_one_device and len(self._all_devices()) > 1:
            self._logged_one_device = True
            self.logger.info(f"PIECEWISE_GRID: the piecewise-rigid mode runs on device {self._devices()[0]} only")

    def _take_piecewise(self, res) -> None:
        ex = getattr(res, "extras", None) or {}
        self.patch_residuals = ex.get("patch_residuals")
        self.patch_points = ex.get("patch_points")
        self.patch_fitted = ex.get("patch_fitted")

    def _check_intensity_pass(self, switch: str, why: str, images) -> None:
        """What the fallback and the refinement both refuse (``why``: what rules a homography out)."""
        if self.RANSAC_MODEL == "projective":
            raise NotImplementedError(f"{switch} does not support RANSAC_MODEL = 'projective' ({why})")
        if self.PIECEWISE_GRID is not None:
            raise NotImplementedError(f"{switch} does not run together with PIECEWISE_GRID")
        if getattr(images, "ndim", 3) != 3:
            raise NotImplementedError(f"{switch} supports grayscale stacks [F, H, W] only")

    # ------------------------------------------- intensity fallback for frames without a model
    def _reset_fallback(self) -> None:
        self.fallback_shifts = None
        self.fallback_correlations = None
        self.fallback_idxs = None

    def _fallback_on(self, images=None) -> bool:
        """Whether the correlation fallback runs, after the checks that must fail before any
        work (``images``: only its number of dimensions is read, when it has one)."""
        if self.FALLBACK == "interpolate":
            return False
        if self.FALLBACK != "correlation":
            raise ValueError(f"FALLBACK must be 'interpolate' or 'correlation', got {self.FALLBACK!r}")
        _fb.check_radius(self.FALLBACK_RADIUS)
        self._check_intensity_pass("FALLBACK = 'correlation'", "the shift is composed with a 2 x 3 map", images)
        return True

    def _with_fallback(self, hot: Callable, slabs: Sequence[_pl.SlabInputs], n_images: int, rate: int) -> Callable:
        """``hot`` itself with the switch off; with it on, ``hot`` followed by the fallback pass
        over its result, so that every pass of _run_passes carries the correction."""
        if not self._fallback_on():
            return hot

        def corrected():
            res = hot()
            fb = _fb.correct_skipped(res, [inp.frames for inp in slabs], n_images, rate, self.RANSAC_MODEL,
                                     int(self.FALLBACK_RADIUS), float(self.FALLBACK_MIN_CORRELATION),
                                     bool(self.FALLBACK_SUBPIXEL), logger=self.logger,
                                     interpolation=self._interpolation_on())
            self.fallback_shifts, self.fallback_correlations = fb.shifts, fb.correlations
            self.fallback_idxs = fb.idxs
            return res

        return corrected

    # ------------------------------------------------ intensity refinement of every frame's map
    def _reset_refine(self) -> None:
        self.refine_steps = None
        self.refine_correlations = None
        self.refine_idxs = None
        self.refine_field = None
        self.refine_field_correlations = None
        self.refine_field_idxs = None

    def _refine_grid_on(self) -> bool:
        """Whether the field stage follows the refinement, after the checks of its own switches."""
        if self.REFINE_GRID is None:
            return False
        if self.REFINE == "none":
            raise ValueError("REFINE_GRID needs REFINE = 'intensity' (the field stage runs after the refinement "
                             "of the frames' maps)")
        _rff.check_grid(self.REFINE_GRID)
        _rff.check_iters(self.REFINE_GRID_ITERS)
        if bool(self.QUALITY_METRICS) or int(self.TEMPLATE_REFINE_ITERS) > 0:
            raise NotImplementedError("REFINE_GRID does not run together with QUALITY_METRICS / "
                                      "TEMPLATE_REFINE_ITERS (their valid region is the affine maps')")
        return True

    def _refine_on(self, images=None) -> bool:
        """Whether the intensity refinement runs, after the checks that must fail before any
        work (``images``: only its number of dimensions is read, when it has one)."""
        self._refine_grid_on()
        if self.REFINE == "none":
            return False
        if self.REFINE != "intensity":
            raise ValueError(f"REFINE must be 'none' or 'intensity', got {self.REFINE!r}")
        try:
            _rf.check_options(self.REFINE_ITERS, self.REFINE_MOTION, self.REFINE_MAX_STEP)
        except ValueError as e:
            raise ValueError(f"REFINE_ITERS / REFINE_MOTION / REFINE_MAX_STEP: {e}") from None
        self._check_intensity_pass("REFINE = 'intensity'", "the step is composed with a 2 x 3 map", images)
        return True

    def _with_refine(self, hot: Callable, slabs: Sequence[_pl.SlabInputs], n_images: int, rate: int) -> Callable:
        """``hot`` itself with the switch off; with it on, ``hot`` (the fallback included)
        followed by the refinement pass over its result, in every pass of _run_passes."""
        if not self._refine_on():
            return hot

        def refined():
            res = hot()
            rf = _rf.refine_frames(res, [inp.frames for inp in slabs], n_images, rate, self.RANSAC_MODEL,
                                   int(self.REFINE_ITERS), self.REFINE_MOTION, float(self.REFINE_MAX_STEP),
                                   logger=self.logger, interpolation=self._interpolation_on())
            self.refine_steps, self.refine_correlations, self.refine_idxs = rf.steps, rf.correlations, rf.idxs
            if self._refine_grid_on():
                ff = _rff.refine_field_frames(res, [inp.frames for inp in slabs], n_images, rate, self.REFINE_GRID,
                                              int(self.REFINE_GRID_ITERS), float(self.REFINE_MAX_STEP),
                                              logger=self.logger)
                self.refine_field, self.refine_field_correlations = ff.field, ff.correlations
                self.refine_field_idxs = ff.idxs
            return res

        return refined

    # ------------------------------------------------- quality metrics, template refinement
    def _reset_quality(self) -> None:
        self.frame_correlations = None
        self.mean_image = None
        self.valid_region = None
        self.template_image = None
        self.correlation_history = None

    def _quality_on(self, refine_supported: bool = True) -> bool:
        """Whether the metrics run, after the checks that must fail before any work."""
        iters = int(self.TEMPLATE_REFINE_ITERS)
        if iters < 0:
            raise ValueError("TEMPLATE_REFINE_ITERS must be >= 0")
        on = bool(self.QUALITY_METRICS) or iters > 0
        if on and self.RANSAC_MODEL == "projective":
            raise NotImplementedError("QUALITY_METRICS / TEMPLATE_REFINE_ITERS do not support RANSAC_MODEL = "
                                      "'projective' (a homography's displacement is not bounded by its corners)")
        if iters > 0 and not refine_supported:
            raise ValueError("TEMPLATE_REFINE_ITERS needs a detector for the refined template: use align_images "
                             "(align_keypoints supports QUALITY_METRICS only)")
        return on

    def _measure(self, res, n_images: int, rate: int) -> List[int]:
        """The metrics of one pass (res: a SlabResult or SplitResult, frames still on their
        devices and unpatched); returns sel0, the sample frames that got a model of their own."""
        parts = _in.parts_of(res)
        if parts[0].dim() != 3:
            raise NotImplementedError("QUALITY_METRICS / TEMPLATE_REFINE_ITERS support grayscale stacks [F, H, W] only")
        H, W = parts[0].shape[1:]
        sel = _in.sample_mask(n_images, rate, res.skipped)
        mean0 = _q.mean_image(parts, sel)
        region = _q.valid_region(np.asarray(res.affines)[:n_images], H, W,
                                 taps=4 if self._interpolation_on() == "cubic" else 2)
        corr = _q.frame_correlations(parts, mean0, region)
        self.mean_image = mean0.cpu().numpy()
        self.valid_region = region
        self.frame_correlations = corr
        self.correlation_history.append(corr)
        if np.isnan(corr).all():
            self.logger.info(f"pass {len(self.correlation_history)}: no frame has a defined correlation")
        else:
            self.logger.info(f"pass {len(self.correlation_history)}: mean frame correlation with the mean image "
                             f"{np.nanmean(corr):.6f} over rows [{region[0]}, {region[1]}), columns "
                             f"[{region[2]}, {region[3]})")
        return np.flatnonzero(sel).tolist()

    def _run_passes(self, hot: Callable, slabs: Sequence[_pl.SlabInputs], n_images: int, rate: int,
                    detect_template: Optional[Callable] = None):
        """The hot path (``hot()`` -> SlabResult / SplitResult over ``slabs``) once, and with
        the switches on the metrics after it and TEMPLATE_REFINE_ITERS more passes, each with
        the template keypoints ``detect_template(template_u16)`` -> (kp [n, 2], des [n, D])
        finds in the mean of the previous pass's best-registered sample frames."""
        res = hot()
        if not self._quality_on(detect_template is not None):
            return res
        iters = int(self.TEMPLATE_REFINE_ITERS)
        self.correlation_history = []
        for k in range(iters + 1):
            try:
                sel0 = self._measure(res, n_images, rate)
            except ValueError as e:
                if iters > 0:
                    raise AlignmentError(f"template refinement, pass {k + 1}: {e}") from e
                raise
            if k == iters:
                break
            best = np.zeros(n_images, bool)
            best[_q.select_top(self.frame_correlations, sel0, float(self.TEMPLATE_REFINE_TOP_FRAC))] = True
            self.template_image = _q.mean_image(_in.parts_of(res), best).cpu().numpy()
            kp, des = detect_template(self.template_image)
            self._kp_template = np.asarray(kp, np.float64).reshape(-1, 2)
            self._des_template = np.asarray(des, np.uint8)
            for inp in slabs:  # only the template changes between passes
                dev = inp.frames.device
                inp.kp_tpl = torch.from_numpy(np.ascontiguousarray(self._kp_template)).to(dev)
                inp.des_tpl = torch.from_numpy(np.ascontiguousarray(self._des_template)).to(dev)
            self.logger.info(f"template refined from {int(best.sum())} frames: {len(self._kp_template)} keypoints")
            res = hot()
        return res

    # ------------------------------------------------- summary images of the aligned stack
    def _reset_summary(self) -> None:
        self.summary_region = None
        self.summary_mean_image = None
        self.max_image = None
        self.std_image = None
        self.correlation_image = None
        self.crispness = None

    def _summary_on(self, images=None) -> bool:
        """Whether the summary images are made, after the checks that must fail before any work
        (``images``: only its number of dimensions is read, when it has one)."""
        if not self.SUMMARY_IMAGES:
            return False
        try:
            _sm.check_neighbours(self.SUMMARY_NEIGHBOURS)
        except ValueError:
            raise ValueError(f"SUMMARY_NEIGHBOURS must be 4 or 8, got {self.SUMMARY_NEIGHBOURS!r}") from None
        if self.RANSAC_MODEL == "projective":
            raise NotImplementedError("SUMMARY_IMAGES does not support RANSAC_MODEL = 'projective' (a homography's "
                                      "displacement is not bounded by its corners)")
        if self.PIECEWISE_GRID is not None or self.REFINE_GRID is not None:
            raise NotImplementedError("SUMMARY_IMAGES does not run together with PIECEWISE_GRID / REFINE_GRID (the "
                                      "valid region of a field warp is not defined yet)")
        if getattr(images, "ndim", 3) != 3:
            raise NotImplementedError("SUMMARY_IMAGES supports grayscale stacks [F, H, W] only")
        return True

    def _summarize(self, res, n_images: int) -> None:
        """The summary images of the final pass (res: a SlabResult or SplitResult, frames still on
        their devices and unpatched), over all frames."""
        parts = _in.parts_of(res)
        if parts[0].dim() != 3:
            raise NotImplementedError("SUMMARY_IMAGES supports grayscale stacks [F, H, W] only")
        H, W = parts[0].shape[1:]
        region = _q.valid_region(np.asarray(res.affines)[:n_images], H, W,
                                 taps=4 if self._interpolation_on() == "cubic" else 2)
        n, planes, top = _sm.temporal_sums(parts, region, None, int(self.SUMMARY_NEIGHBOURS))
        planes = planes.cpu().numpy()
        self.summary_region = region
        self.summary_mean_image = _sm.mean_image(planes, n, region)
        self.max_image = top.cpu().numpy()
        self.std_image = _sm.std_image(planes, n, region)
        self.correlation_image = _sm.correlation_image(planes, n, region)
        self.crispness = _sm.crispness(self.summary_mean_image, region)
        self.logger.info(f"summary images over {n} frames, rows [{region[0]}, {region[1]}), columns "
                         f"[{region[2]}, {region[3]}): crispness {self.crispness:.3f}")

    # ------------------------------------------------------------- public API
    def _begin(self, images, refine_supported: bool) -> None:
        """What align_images and align_keypoints open with: the results of the switches reset and
        every switch checked, before any work.  The order of the checks decides which of two
        conflicting switches is named."""
        self._interpolation_on(images)
        self._reset_bidi()
        self._bidi_on(images)
        self._reset_prefilter()
        self._prefilter_on(images)
        self._reset_quality()
        self._quality_on(refine_supported)
        self._reset_summary()
        self._summary_on(images)
        self._reset_piecewise()
        self._piecewise_on(images)
        self._reset_fallback()
        self._fallback_on(images)
        self._reset_refine()
        self._refine_on(images)
        self._log_one_device()

    def align_images(
        self,
        images: np.ndarray,
        n_kp_global: int,
        detector_algorithm: str,
        frame_rate: int,
        masked_template: Optional[np.ndarray] = None,
        patch: Optional[Tuple[float, float, float, float]] = None,
    ) -> Tuple[np.ndarray, np.ndarray, List[int]]:
        """Register a uint16 stack [frames, x, y] to a template frame (VA:57-158).

        Returns (aligned_imgs, euclidean_transforms [n, 3] = (tx, ty, rotation),
        skipped_idxs); with RANSAC_MODEL = "similarity" the transforms are [n, 4] = (tx, ty,
        rotation, scale).  A device tensor input yields a device tensor output.

        With BIDI_PHASE on, the template frame is taken from the corrected stack; a
        ``masked_template`` is used as given (the caller corrects it, bidi.shift_rows).  With
        DETECT_SMOOTH_RADIUS / DETECT_BACKGROUND_RADIUS set, the detection reads the band-passed
        copy of the stack and of the template (a ``masked_template`` is passed raw and filtered
        here); the returned frames are the raw stack warped.
        """
        self._begin(images, refine_supported=True)
        self.logger.info(f"aligning {len(images)} frames with n_kp_global: {n_kp_global} and {detector_algorithm}")
        if not 0 <= self.TEMPLATE_FRAME_LOC <= 1:
            raise ValueError("`template_frame_loc` must be between 0 and 1")
        on_device = isinstance(images, torch.Tensor)
        template_idx = None
        if masked_template is not None:
            template = _as_numpy(masked_template)
        else:
            template_idx = int(len(images) * self.TEMPLATE_FRAME_LOC)
            template = _as_numpy(images[template_idx])
            self.logger.info(f"no masked template provided. Using frame {template_idx} as template")

        rate = max(1, frame_rate // self.FRAME_SAMPLE_RATE)
        self.logger.info("normalizing frames...")
        t_start = time.time()
        # VA:100-108 on the device(s): each slab is uploaded once (and reused by the warp), the
        # 99.99th percentile of the whole stack comes from the summed per-device histograms and
        # the max-scaling runs per device; the uint8 copy comes back only for a host detector.
        assert (images.dtype == torch.uint16) if on_device else (np.asarray(images).dtype == np.uint16)  # VA:104
        parts, ranges = self._split(images, rate)
        parts, template = self._bidi_source(parts, not on_device, template, template_idx)
        # the detection's source: the stack itself, or its band-passed copy (the warps read `parts`)
        seen, template = self._prefilter_source(parts, template, template_idx)
        brightest_px = stages.brightest_px(seen, self.IMAGE_NORM_MAX_PERCENTILE)
        if self.prefilter_radii is not None:
            self.prefilter_brightest_px = brightest_px
            if not brightest_px > 0:
                raise AlignmentError(
                    f"the band-pass prefilter (DETECT_SMOOTH_RADIUS = {self.prefilter_radii[0]}, "
                    f"DETECT_BACKGROUND_RADIUS = {self.prefilter_radii[1]}) leaves nothing of the stack: its "
                    f"{self.IMAGE_NORM_MAX_PERCENTILE}th percentile is 0")
        u8_parts = []
        for p in seen:  # each slab's work under its own device (launches, workspaces, allocations)
            with _md._on(p):
                u8_parts.append(self._max_scale_images(p, None, brightest_px, np.uint8)[0])
        del seen, p  # a filtered copy is released here: raw + filtered + uint8 is the peak per slab
        _, template_i8 = self._max_scale_images(None, template, brightest_px, np.uint8)
        detector = self.DETECTOR_CONSTRUCTOR_DICT[detector_algorithm]()
        on_gpu = isinstance(detector, GpuOrbDetector) and parts[0].dim() == 3
        self.logger.info(f"normalized frames in: {round(time.time() - t_start)} s")

        self.logger.info("identifying keypoints...")
        t_start = time.time()
        cfg = self._config(n_kp_global, rate)
        out = images.device if on_device else None
        if not on_gpu:
            detect_template = self._host_template_detector(detector, brightest_px, rate)
            images_i8 = np.concatenate([u.cpu().numpy() for u in u8_parts])
            images_sample, template = self._downsample(images_i8, template_i8, rate, self.SPATIAL_DOWNSAMPLE_RATE)
            kp_t, des_t = detector.detectAndCompute(template, None)
            self._kp_template = np.array([p.pt for p in kp_t])
            self._des_template = des_t
            kp_list, des_list = [], []
            for img in images_sample:
                kq, dq = detector.detectAndCompute(img, None)
                kp_list.append(np.array([p.pt for p in kq], dtype=np.float64).reshape(-1, 2))
                des_list.append(np.asarray(dq, dtype=np.uint8).reshape(len(kq), -1))
            self.logger.info(f"identified keypoints in: {round(time.time() - t_start)} s")
            return self._align_detected(parts, ranges, self._kp_template, np.asarray(des_t, np.uint8), kp_list,
                                        des_list, cfg, patch, out, detect_template)
        # f1 per device: each slab's sample frames detected where they live (f4: downsampled there too)
        tpl_u8 = np.ascontiguousarray(template_i8)
        samples = []
        for u in u8_parts:
            with _md._on(u):
                samples.append(_pl.downsample_u8(u, torch.from_numpy(tpl_u8).to(u.device)[None], rate,
                                                 self.SPATIAL_DOWNSAMPLE_RATE))
        with _md._on(samples[0][1]):
            kt = stages.detect_orb(samples[0][1], detector.params)
        n_t = int(kt.count.cpu()[0])
        self._kp_template = kt.kp[0, :n_t].cpu().numpy()
        self._des_template = kt.des[0, :n_t].cpu().numpy()
        slabs = []
        for fr, (smp, _) in zip(parts, samples):
            with _md._on(smp):
                kp_q, des_q, q_off, q_off_host = stages.keypoints_csr(stages.detect_orb(smp, detector.params))
            dev = fr.device
            slabs.append(_pl.SlabInputs(fr, torch.from_numpy(self._des_template).to(dev),
                                        torch.from_numpy(self._kp_template).to(dev), des_q, kp_q, q_off, q_off_host))
        self.logger.info(f"identified keypoints in: {round(time.time() - t_start)} s")

        def detect_template(tpl_u16):  # as a masked_template enters, on the first slab's device
            tpl_u16 = self._prefilter_image(tpl_u16)
            t8 = np.ascontiguousarray(self._max_scale_images(None, tpl_u16, brightest_px, np.uint8)[1])
            with _md._on(u8_parts[0]):
                t8 = torch.from_numpy(t8).to(u8_parts[0].device)[None]
                k = stages.detect_orb(_pl.downsample_u8(t8, t8, rate, self.SPATIAL_DOWNSAMPLE_RATE)[1],
                                      detector.params)
            n = int(k.count.cpu()[0])
            return k.kp[0, :n].cpu().numpy(), k.des[0, :n].cpu().numpy()

        return self._finish(slabs, ranges, cfg, patch, out, detect_template)

    def _split(self, images, rate: int):
        """(parts, ranges): the stack's slabs on the devices of the hot path, one per device that
        gets a sample frame (kcmc_amd.multidevice; one device: a list of one), and their frame
        ranges.  An empty stack is one empty slab."""
        devices = self._devices()
        ranges = _md.split_frames(len(images), rate, len(devices)) or [_md.SlabRange(0, 0, 0, 0)]
        frames = images if isinstance(images, torch.Tensor) else np.asarray(images)
        return _md.split_to_devices(frames, ranges, devices[:len(ranges)]), ranges

    def _host_template_detector(self, detector, brightest_px, rate) -> Callable:
        """template_u16 -> (kp, des) with a host (OpenCV-style) detector, the way a
        masked_template enters align_images: the prefilter when it is on, max-scale, downsample,
        detectAndCompute."""
        def detect_template(tpl_u16):
            tpl_u16 = self._prefilter_image(tpl_u16)
            t8 = self._max_scale_images(None, tpl_u16, brightest_px, np.uint8)[1]
            t8 = self._downsample(t8[None], t8, rate, self.SPATIAL_DOWNSAMPLE_RATE)[1]
            kp_t, des_t = detector.detectAndCompute(t8, None)
            return np.array([p.pt for p in kp_t]), des_t

        return detect_template

    def _finish(self, slabs, ranges, cfg, patch, out, detect_template=None):
        """The tail of align_images and align_keypoints: the hot path over the slabs -- align_slab
        for one (the only one with the piecewise-rigid mode), align_split for several -- with the
        fallback, the refinement and the template passes around it; then the results.  ``out``:
        the device the aligned stack is returned on, None for a numpy array."""
        self.logger.info("generating keypoint consensus...")
        t_start = time.time()
        n_images, rate = ranges[-1].f1, int(cfg.frame_downsample_rate)
        if len(slabs) == 1:
            hot = lambda: _pl.align_slab(slabs[0], cfg, logger=self.logger)  # noqa: E731
        else:
            hot = lambda: _md.align_split(slabs, ranges, cfg, logger=self.logger)  # noqa: E731
        hot = self._with_refine(self._with_fallback(hot, slabs, n_images, rate), slabs, n_images, rate)
        # the metrics read the aligned slabs where they are, before they are gathered
        res = self._run_passes(hot, slabs, n_images, rate, detect_template)
        if self._summary_on():
            self._summarize(res, n_images)
        self.interpolated_idxs = res.interpolated
        self.logger.info(f"aligned frames in: {round(time.time() - t_start)} s")
        self._take_piecewise(res)
        self.affines = res.affines  # the maps the returned frames were resampled with, after every pass
        aligned = res.aligned if len(slabs) == 1 else _md.gather_aligned(res, out)
        if patch is not None:
            x_start, y_start, width, height = patch
            aligned = aligned[:, x_start:x_start + width, y_start:y_start + height]
        if isinstance(aligned, torch.Tensor):  # one slab: the result itself, or only its patch copied
            aligned = aligned.cpu().numpy() if out is None else aligned.to(out)
        return aligned, res.euclidean, res.skipped

    @staticmethod
    def _csr(kp_list, des_list, D):
        q_off = np.zeros(len(kp_list) + 1, np.int32)
        q_off[1:] = np.cumsum([len(k) for k in kp_list])
        kp_flat = np.concatenate(kp_list).astype(np.float64) if q_off[-1] else np.zeros((0, 2))
        des_flat = np.concatenate(des_list).astype(np.uint8) if q_off[-1] else np.zeros((0, D), np.uint8)
        return kp_flat, des_flat, q_off

    def align_keypoints(
        self,
        images,
        kp_template: np.ndarray,
        des_template: np.ndarray,
        kp_query: Sequence[np.ndarray],
        des_query: Sequence[np.ndarray],
        n_kp_global: int,
        frame_rate: int = 30,
        patch: Optional[Tuple[float, float, float, float]] = None,
    ):
        """The hot path with precomputed keypoints: per SAMPLE frame
        (images[::max(1, frame_rate // FRAME_SAMPLE_RATE)]) keypoint coordinates [n, 2]
        and uint8 descriptors [n, D]; template keypoints/descriptors likewise."""
        self._begin(images, refine_supported=False)
        if self._prefilter_on() is not None:
            self.logger.info("DETECT_SMOOTH_RADIUS / DETECT_BACKGROUND_RADIUS: ignored by align_keypoints (the "
                             "keypoints are given, there is no detection to filter for)")
        self._kp_template = np.asarray(kp_template, dtype=np.float64).reshape(-1, 2)
        self._des_template = np.asarray(des_template, dtype=np.uint8)
        rate = max(1, frame_rate // self.FRAME_SAMPLE_RATE)
        on_device = isinstance(images, torch.Tensor)
        parts, ranges = self._split(images, rate)
        parts = self._bidi_correct(parts, not on_device)  # the caller's frames: corrected here
        return self._align_detected(parts, ranges, self._kp_template, self._des_template, list(kp_query),
                                    list(des_query), self._config(n_kp_global, rate), patch,
                                    images.device if on_device else None)

    def _align_detected(self, parts, ranges, kp_template, des_template, kp_list, des_list, cfg, patch, out,
                        detect_template=None):
        """_finish over the slabs of host-side keypoints: one [n, 2] and one [n, D] array per sample
        frame of the whole stack, cut per slab (multidevice.make_slabs)."""
        kp_flat, des_flat, q_off = self._csr(kp_list, des_list, des_template.shape[1])
        slabs = _md.make_slabs(parts, ranges, des_template, kp_template, kp_flat, des_flat, q_off)
        return self._finish(slabs, ranges, cfg, patch, out, detect_template)

    # ------------------------------------------------ per-frame helpers (VA:160-458)
    @classmethod
    def _get_frame_keypoints(cls, i: int, image: np.ndarray, kp_template: np.ndarray, des_template: np.ndarray,
                             detector_algorithm: str) -> Tuple[Set[int], np.ndarray, str]:
        """VA:160-222 for one frame (detection on the host, matching on the GPU)."""
        detector = cls.DETECTOR_CONSTRUCTOR_DICT[detector_algorithm]()
        kq, dq = detector.detectAndCompute(image, None)
        kp_query = np.array([p.pt for p in kq], dtype=np.float64).reshape(-1, 2)
        return cls._match_frame(i, kp_query, np.asarray(dq, np.uint8), kp_template, des_template)

    @classmethod
    def _match_frame(cls, i, kp_query, des_query, kp_template, des_template):
        dev = cls._device()
        q_off = np.array([0, len(kp_query)], np.int32)
        m = stages.match_frames(
            torch.from_numpy(np.ascontiguousarray(des_template, np.uint8)).to(dev),
            torch.from_numpy(np.ascontiguousarray(kp_template, np.float64)).to(dev),
            torch.from_numpy(np.ascontiguousarray(des_query, np.uint8)).to(dev),
            torch.from_numpy(np.ascontiguousarray(kp_query, np.float64)).to(dev),
            torch.from_numpy(q_off).to(dev), q_off, ratio=cls.DESCRIPTOR_DISTANCE_RATIO_THRESH)
        n_tpl = len(kp_template)
        bits = m.keep_bits.cpu().numpy().view(np.uint32)[0]
        kept = [k for k in range(n_tpl) if (bits[k >> 5] >> (k & 31)) & 1]
        c = m.counts.cpu().numpy()[0]
        return set(kept), m.kp_ordered.cpu().numpy()[0], _pl.frame_counts_text(i, c)

    def _get_consensus_kps(self, kp_idxs_list: List[set], n_frames: int, n_kp_global: int) -> Set[int]:
        """VA:224-249: the n_kp_global most frequently matched template keypoints."""
        counts = Counter([x for s in kp_idxs_list for x in s])
        votes = [x for x in counts.most_common(n_kp_global)]
        if len(votes) < self.N_KP_GLOBAL_MIN:
            raise VideoAligner.AlignmentError(
                "Too few keypoints found. Try a higher quality video, or decrease `VideoAligner.N_KP_GLOBAL_MIN`")
        consensus_idxs, vote_match_rates = zip(*votes)
        vote_match_rates = np.array(vote_match_rates) / n_frames
        self.logger.info(f"top n keypoints match rates: {vote_match_rates}")
        return set(consensus_idxs)

    def _lookup_consensus_kps(self, consensus_idxs: Set[int], kp_idxs_list: List[Set[int]],
                              kp_query_list: List[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        """VA:251-286 (object arrays for ragged frames, as numpy < 1.24 produced)."""
        tk, qk = [], []
        for i in range(len(kp_query_list)):
            idx = list(consensus_idxs.intersection(kp_idxs_list[i]))
            tk.append(self._kp_template[idx])
            qk.append(np.asarray(kp_query_list[i])[idx])
            if len(qk[-1]) < self.N_KP_FRAME_SKIP:
                self.logger.info(
                    f"transform for frame {i} not estimated due to low keypoint count: "
                    f"({len(qk[-1])}). Will be interpolated based on other frames instead")

        def arr(lst):
            try:
                return np.array(lst)
            except ValueError:
                out = np.empty(len(lst), dtype=object)
                for k, v in enumerate(lst):
                    out[k] = v
                return out

        return arr(tk), arr(qk)

    @classmethod
    def _compute_euclidean_affine(cls, kp_template: np.ndarray, kp_query: np.ndarray,
                                  spatial_downsample_rate: Union[float, int]) -> Optional[np.ndarray]:
        """VA:288-323 for one frame: seeded rigid RANSAC on the GPU (NaN on failure)."""
        return cls._compute_frame_affine(stages.ransac_rigid, kp_template, kp_query, spatial_downsample_rate)

    @classmethod
    def _compute_similarity_affine(cls, kp_template: np.ndarray, kp_query: np.ndarray,
                                   spatial_downsample_rate: Union[float, int]) -> Optional[np.ndarray]:
        """_compute_euclidean_affine with SimilarityTransform: [scale R | t] for one frame."""
        return cls._compute_frame_affine(stages.ransac_similarity, kp_template, kp_query, spatial_downsample_rate)

    @classmethod
    def _compute_frame_affine(cls, ransac, kp_template, kp_query, spatial_downsample_rate):
        kp_query = np.asarray(kp_query, dtype=np.float64).reshape(-1, 2)
        kp_template = np.asarray(kp_template, dtype=np.float64).reshape(-1, 2)
        if len(kp_query) < cls.N_KP_FRAME_SKIP:
            return np.full((2, 3), np.nan)
        dev = cls._device()
        off = np.array([0, len(kp_query)], np.int32)
        r = ransac(
            torch.from_numpy(np.ascontiguousarray(kp_query)).to(dev),
            torch.from_numpy(np.ascontiguousarray(kp_template)).to(dev),
            torch.from_numpy(off).to(dev), off, trials=cls.RANSAC_MAX_TRIALS,
            residual_threshold=float(cls.RANSAC_RESIDUAL_THRESH), spatial_rate=spatial_downsample_rate,
            n_skip=cls.N_KP_FRAME_SKIP, seed=cls.RANDOM_SEED, min_samples=cls.RANSAC_MIN_SAMPLES)
        return r.params.cpu().numpy()[0]

    _process_affines = staticmethod(_aff.process_affines)
    _interpolate_affines = staticmethod(_aff.interpolate_affines)
    _get_euclidean_transforms = staticmethod(_aff.euclidean_transforms)

    @staticmethod
    def _interpolate_affines_frame_range(base_affines: np.ndarray, failed_idx_range: range) -> List[np.ndarray]:
        """VA:409-437."""
        xs = np.arange(failed_idx_range[0], failed_idx_range[-1] + 1)
        out = _aff._lerp_gap(base_affines[0], base_affines[1], failed_idx_range[0] - 1, failed_idx_range[-1] + 1, xs)
        return [a for a in out]

    @classmethod
    def _apply_affine(cls, image: np.ndarray, affine: np.ndarray) -> np.ndarray:
        """VA:455-458: cv2.warpAffine(image, affine, (W, H), INTER_LINEAR) on the GPU (the
        bicubic warp with WARP_INTERPOLATION = "cubic")."""
        dev = cls._device()
        img = torch.from_numpy(np.ascontiguousarray(image, np.uint16)[None]).to(dev)
        a = torch.from_numpy(np.ascontiguousarray(affine, np.float64).reshape(1, 2, 3)).to(dev)
        return stages.warp_affine_u16(img, a, interpolation=stages.check_interpolation(cls.WARP_INTERPOLATION)
                                      ).cpu().numpy()[0]

    def _parallelize(self, func: Callable, *sequences: Sequence, **kwargs) -> List:
        """VA:460-465: func over the equal-length sequences, results in order, in a joblib
        process pool of N_JOBS_PARALLEL workers (backend "multiprocessing", as the reference)
        -- for a subclass's own (picklable, CPU) per-frame function.  This package's functions
        run in this process instead: they are GPU-backed, a forked worker cannot use the
        parent's GPU context, and the hot path batches them anyway."""
        r = range(len(sequences[0]))
        mod = getattr(func, "__module__", "") or ""
        if mod.split(".")[0] == __name__.split(".")[0] or int(self.N_JOBS_PARALLEL) <= 1 or len(r) <= 1:
            return [func(*[x[i] for x in sequences], **kwargs) for i in r]
        from joblib import Parallel, delayed

        with Parallel(n_jobs=int(self.N_JOBS_PARALLEL), backend="multiprocessing") as parallel:
            return list(parallel(delayed(func)(*[x[i] for x in sequences], **kwargs) for i in r))

    def _parallelize_i(self, func: Callable, *sequences: Sequence, **kwargs) -> List:
        r = range(len(sequences[0]))
        return self._parallelize(func, r, *sequences, **kwargs)

    @staticmethod
    def _convert_to_array(*args: Sequence):
        return tuple(np.array(arg) for arg in args)

    @classmethod
    def _get_brightest_px(cls, images) -> Union[float, int]:
        """VA:479-482: np.percentile(images, 99.99).  A uint16 device tensor takes the exact
        HIP path (two histogram passes + numpy's interpolation); a host array is the
        reference's own numpy call."""
        if isinstance(images, torch.Tensor):
            return stages.brightest_px(images.contiguous(), cls.IMAGE_NORM_MAX_PERCENTILE)
        return np.percentile(images, cls.IMAGE_NORM_MAX_PERCENTILE)

    @classmethod
    def _max_scale_images(cls, images, template, brightest_px: float, output_dtype: type):
        """VA:484-492.  uint16 device tensors are scaled on the GPU through the table of
        the reference's expression (bit-exact); host arrays use the expression itself.
        Either argument may be None (returned as None)."""
        max_px = cls.MAX_PIXEL_UINT8

        def scale(x):
            if x is None:
                return None
            if isinstance(x, torch.Tensor) and x.dtype == torch.uint16 and output_dtype == np.uint8:
                return stages.max_scale_u8(x.contiguous(), brightest_px, max_px=max_px)
            x = _as_numpy(x)
            if x.dtype == np.uint16 and output_dtype == np.uint8:
                return stages.max_scale_lut(brightest_px, max_px)[x]
            return np.clip(x / brightest_px * max_px, a_min=0, a_max=max_px).astype(output_dtype)

        return scale(images), scale(template)

    @staticmethod
    def _downsample(images: np.ndarray, template: np.ndarray, frame_downsample_rate: int,
                    spatial_downsample_rate: Union[float, int]) -> Tuple[np.ndarray, np.ndarray]:
        """VA:494-506: every rate-th frame and, when the rate is not 1, cv2.pyrDown of the
        sample frames and the template -- here the device kernel (stages.pyr_down_u8, via
        pipeline.downsample_u8) with the reference's dstsize quirk kept."""
        if int(frame_downsample_rate) == 1:
            return images[::1], template
        dev = VideoAligner._device()
        f = torch.from_numpy(np.ascontiguousarray(images, np.uint8)).to(dev)
        t = torch.from_numpy(np.ascontiguousarray(template, np.uint8)).to(dev)[None]
        s, t = _pl.downsample_u8(f, t, frame_downsample_rate, spatial_downsample_rate)
        return s.cpu().numpy(), t[0].cpu().numpy()


class LoResVideoAligner(VideoAligner):
    SPATIAL_DOWNSAMPLE_RATE = 2

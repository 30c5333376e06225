"""Benchmark of the alignment hot path on BASELINE.json config[1]:
1080p grayscale uint16, 2000 frames per GPU, ORB-like keypoints (500 per template,
32-byte descriptors, ~550 per frame), rigid RANSAC (1000 trials), n_kp_global = 100.

One step = one pass of the hot path over the whole batch with inputs resident in HBM:
K1 match (GPU) -> survivor bitmasks to host -> consensus (host, native) -> K2 RANSAC
(GPU) -> affine post-processing (host) -> K3 warp of every uint16 frame (GPU).
Detection is not part of the path (no detector exists in this image; keypoints are
synthetic, see kcmc_amd/synthetic.py).

Steps are issued through pipeline.OverlappedSlabs, a software pipeline (kernel stream:
warp(k-1); analysis stream: match(k) -> lookup + RANSAC(k) beside it, or for c5 the match
on the kernel stream ahead of the warp): the host consensus of step k runs while step
k-1's frames are warped; every step still runs every stage, and the pipeline is drained
inside the timed region.  --serial runs the steps strictly one after another.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    torchrun --nproc-per-node N bench.py --gpus N ...   (one rank per GPU, RCCL)

A plain run sets up, warms up, times the K steps and prints the result line (the figures in
it beside `value` come from HIP events the timed steps record anyway).  --full adds what
takes runs of its own after the timed region: every GPU stage alone (`stage_ms_isolated`,
the RANSAC / match / isolated-warp rooflines, `ransac_hypotheses_per_s_per_gpu`) and the
CPU baseline (`cpu_baseline`, see --cpu-sample / --cpu-procs).  --dump-outputs DIR writes
what the last timed step returned to its caller as DIR/<name>.npy (dump_outputs below); the
inputs are seeded, so two builds run with the same arguments compare output for output.

Without torchrun, `--gpus N > 1` starts the N rank processes itself (spawn_ranks: before
any GPU call, one child per GPU with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*), and refuses
(exit 2) when fewer than N devices are visible -- it never reports one GPU for --gpus N.

Rank 0 prints ONE JSON line.  value = frames aligned by all ranks / max-over-ranks
wall time of the K timed steps.
"""
import argparse
import json
import os
import sys
import time
from dataclasses import dataclass

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import kcmc_amd  # noqa: E402,F401
from kcmc_amd import distributed as kdist  # noqa: E402
from kcmc_amd import multidevice as md  # noqa: E402
from kcmc_amd import pipeline, stages, synthetic  # noqa: E402

METRIC = "aligned frames/sec (whole node) at 1080p; RANSAC hypotheses scored/sec/GPU"
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
BF16_PEAK_TFLOPS = 2500.0  # dense bf16 / fp16 MFMA (MI355X_MICROARCH.md: the F16 forms take the same cycles)
I8_PEAK_TOPS = 5000.0  # dense i8 MFMA: 2x the bf16 rate per clock (MI355X_MICROARCH.md)
# wave64 VALU instructions per second per GPU: 256 CUs x 4 SIMDs x one per 4 cycles (the
# integer ops of the matcher epilogues issue at this rate: SQ_ACTIVE_INST_VALU = 4 cycles
# per instruction in the r03 PMC passes) x 2.4 GHz
VALU_INSTR_PER_S_PER_GPU = 1024 * 0.25 * 2.4e9
TRIALS = 1000
ISOLATED_HEAD_START_CYCLES = 2_000_000  # spin ahead of the isolated match / RANSAC reps


@dataclass
class BenchConfig:
    name: str
    workload: str
    H: int
    W: int
    C: int
    n_tpl: int
    D: int
    n_kp_global: int
    model: str
    frames_per_gpu: int
    cpu_sample: int
    descriptor: str = "u8"
    # the match + vote on the analysis stream beside the warp (OverlappedSlabs match_beside):
    # c2 / c3 / c4 at depth 2 (match(k), lookup + RANSAC(k) beside warp(k-1): +0.9 % / +3.9 %
    # / +3.5 %, profiles/r03_b9_*, r03_b10_*); c5's
    # 4 ms float match beside its 1.6 ms warp is 12 % slower
    match_beside: bool = False


# BASELINE.json configs.  c2 (configs[1]) is the headline line; the others are the
# extension workloads (affine / 4K RGB), reported with --config.  Frames per GPU are the
# config's frame count divided over the 8 GPUs it names (weak scaling per GPU).
CONFIGS = {
    "c2": BenchConfig("c2", "BASELINE config[1]: 1080p grayscale u16, 2000 frames per GPU, ORB-like keypoints "
                      "(n_tpl=500, D=32 B, ~550/frame), rigid RANSAC 1000 trials, n_kp_global=100",
                      1080, 1920, 1, 500, 32, 100, "euclidean", 2000, 240, match_beside=True),
    "c3": BenchConfig("c3", "BASELINE config[2]: 512x512 two-photon-style u16, 20000 frames over 8 GPUs (2500 per GPU), "
                      "n_tpl=500, D=61 B (AKAZE-sized), affine RANSAC 1000 trials, n_kp_global=50",
                      512, 512, 1, 500, 61, 50, "affine", 2500, 60, match_beside=True),
    "c4": BenchConfig("c4", "BASELINE config[3]: 4K RGB u16 (2160x3840x3), 5000 frames over 8 GPUs (625 per GPU), "
                      "4096 keypoints/frame template, D=61 B, affine RANSAC 1000 trials, n_kp_global=500",
                      2160, 3840, 3, 4096, 61, 500, "affine", 625, 4, match_beside=True),
    "c5": BenchConfig("c5", "BASELINE config[4]: 1080p u16, float SIFT-style descriptors (n_tpl=4096, D=128 f32, "
                      "~4500/frame), homography RANSAC 1000 trials, n_kp_global=200, warpPerspective; "
                      "500 frames per GPU", 1080, 1920, 1, 4096, 128, 200, "projective", 500, 2, "f32"),
}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def make_texture(bc: BenchConfig) -> np.ndarray:
    if bc.C == 1:
        return synthetic.make_texture((bc.H, bc.W), seed=0)
    return np.stack([synthetic.make_texture((bc.H, bc.W), seed=c) for c in range(bc.C)], axis=-1)


def make_inputs(bc: BenchConfig, frames_per_gpu: int, rank: int, dev: torch.device):
    ks = synthetic.make_keypoints(frames_per_gpu, bc.n_tpl, bc.D, (bc.H, bc.W), seed=3, frame_seed=rank,
                                  model=bc.model, descriptor=bc.descriptor)
    base_t = torch.from_numpy(make_texture(bc)).to(dev)
    src = base_t.expand((frames_per_gpu,) + tuple(base_t.shape)).contiguous()
    gt = torch.from_numpy(ks.gt).to(dev)
    # jittered video: each frame is the base texture seen through the inverse of its
    # ground-truth frame->template map (one launch, outside the timed region; the PMC
    # summary skips this first warp dispatch)
    if bc.model == "projective":
        frames = stages.warp_perspective_u16(src, gt, inverse_map=True)
    else:
        frames = stages.warp_affine_u16(src, gt, inverse_map=True)
    del src
    inp = pipeline.SlabInputs(
        frames=frames,
        des_tpl=torch.from_numpy(ks.des_tpl).to(dev),
        kp_tpl=torch.from_numpy(ks.kp_tpl).to(dev),
        des_q=torch.from_numpy(ks.des_q).to(dev),
        kp_q=torch.from_numpy(ks.kp_q).to(dev),
        q_off=torch.from_numpy(ks.q_off).to(dev),
        q_off_host=ks.q_off,
    )
    torch.cuda.synchronize(dev)
    return inp, ks


class StageTimer:
    """HIP events on the stream the kernels run on (torch's current stream)."""

    def __init__(self):
        self.ev = {}

    def mark(self, name, ev=None):
        """ev: a timing event the pipeline already recorded at this position (shared marker
        packet); None: record one on the current stream."""
        if ev is None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
        self.ev.setdefault(name, []).append(ev)

    def elapsed(self, a, b):
        return [x.elapsed_time(y) for x, y in zip(self.ev[a], self.ev[b])]


def run_step(inp, cfg, out, timer=None, world=1, counts=None):
    """One pass of the hot path, strictly in order (--serial; single GPU or this rank's
    share of a sharded run through distributed.align_sharded).  Returns the SlabResult."""
    if world > 1:
        return kdist.align_sharded(inp, cfg, counts=counts)
    mark = timer.mark if timer else (lambda name, ev=None: None)
    n_tpl = inp.des_tpl.shape[0]
    mark("m0")
    m = pipeline.match_stage(inp, cfg)
    mark("m1")
    cons = pipeline.device_consensus(m, n_tpl, inp.q_off.numel() - 1, cfg)
    mark("r0")
    rr = pipeline.ransac_stage(m, inp.kp_tpl, cons, cfg)
    mark("r1")
    affines, skipped, interp, eu = pipeline.postprocess_affines(rr.params.cpu().numpy(), cfg)
    a_dev = torch.from_numpy(np.ascontiguousarray(affines[: inp.frames.shape[0]])).to(inp.frames.device)
    mark("w0")
    aligned = pipeline.warp_frames(inp.frames, a_dev, out=out)
    mark("w1")
    return pipeline.SlabResult(aligned, affines, eu, skipped, interp, match=m, consensus=cons, ransac=rr)


DUMP_SAMPLE_ELEMENTS = 4 << 20  # aligned-frame sample: 16 MB as float32
DUMP_SAMPLE_SEED = 20240607
DUMP_LIMIT_BYTES = 64 << 20


def sample_elements(t: torch.Tensor, n: int = DUMP_SAMPLE_ELEMENTS, seed: int = DUMP_SAMPLE_SEED) -> np.ndarray:
    """float32 copy of `t` (a uint16 frame stack on the device) when it has at most n elements,
    else of n of its elements: flat positions drawn once from `seed` (the same for every run
    of the same shape), sorted, so every frame is sampled at a few thousand pixels."""
    flat = t.reshape(-1).view(torch.int16)  # the bits; uint16 has no gather kernel
    if flat.numel() > n:
        pos = np.sort(np.random.default_rng(seed).integers(0, flat.numel(), n, dtype=np.int64))
        flat = flat[torch.from_numpy(pos).to(flat.device)]
    return flat.cpu().numpy().view(np.uint16).astype(np.float32)


def dump_outputs(dirpath: str, aligned, res, n_frames: int, suffix: str = "") -> None:
    """Write what the last timed step handed to its caller as <dirpath>/<name><suffix>.npy:
    `aligned_sample` (float32; sample_elements of every aligned stack in `aligned`, one after
    another) and, in float64, `affines` [F, 2, 3] / `euclidean` [F, 3] (after gap
    interpolation), `skipped` and `interpolated` ([F] 0/1 masks), and where the path returns
    them the consensus (`consensus_order`, `consensus_votes`, CSR point lists `pt_off` /
    `pt_idx`) and the RANSAC results (`ransac_params`, NaN where no model; `ransac_n_inliers`)."""
    os.makedirs(dirpath, exist_ok=True)
    stacks = aligned if isinstance(aligned, (list, tuple)) else [aligned]
    share = DUMP_SAMPLE_ELEMENTS // len(stacks)
    arrays = {"aligned_sample": np.concatenate([sample_elements(a, share) for a in stacks]),
              "affines": np.asarray(res.affines, dtype=np.float64),
              "euclidean": np.asarray(res.euclidean, dtype=np.float64)}
    f0 = getattr(res, "extras", {}).get("f0", 0)  # a rank's slab lists global frame indices
    for name in ("skipped", "interpolated"):
        mask = np.zeros(n_frames, np.float64)
        idx = np.asarray(getattr(res, name), dtype=np.int64) - f0
        mask[idx[(idx >= 0) & (idx < n_frames)]] = 1.0
        arrays[name] = mask
    cons = getattr(res, "consensus", None)
    if cons is not None:
        arrays.update(consensus_order=cons.order, consensus_votes=cons.votes, pt_off=cons.pt_off, pt_idx=cons.pt_idx)
    rr = getattr(res, "ransac", None)
    if rr is not None:
        arrays.update(ransac_params=rr.params.cpu().numpy(), ransac_n_inliers=rr.n_inliers.cpu().numpy())
    total = 0
    for name, a in arrays.items():
        a = np.ascontiguousarray(a, dtype=np.float32 if name == "aligned_sample" else np.float64)
        total += a.nbytes
        if total > DUMP_LIMIT_BYTES:
            raise SystemExit(f"bench.py: --dump-outputs would write more than {DUMP_LIMIT_BYTES >> 20} MB")
        np.save(os.path.join(dirpath, f"{name}{suffix}.npy"), a)
    log(f"dumped {len(arrays)} arrays ({total / 1e6:.1f} MB) to {dirpath}")


def isolated_stage_ms(inp, cfg, out, reps=7):
    """Each GPU stage alone on the current stream, after the timed region, one warm-up
    call first.  Match, the device consensus (vote + merge + lookup) and RANSAC: `reps`
    calls back to back between two HIP events, averaged, behind a spin kernel that keeps
    the device busy while the host queues them (no host launch time inside: a RANSAC launch
    chain once read 0.44 instead of 0.17 ms; the spin is short, 0.85 ms at 2.4 GHz).  The
    consensus includes its host merge (the device waits for it).  Warp: a HIP event pair
    around every launch and the MEDIAN launch (per-dispatch, like rocprofv3's kernel trace;
    the back-to-back average of round 2 read 7-10 % above the in-step launches)."""
    torch.cuda.synchronize()

    def timed(fn, head_start=True):
        r = fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if head_start:
            torch.cuda._sleep(ISOLATED_HEAD_START_CYCLES)
        e0.record()
        for _ in range(reps):
            r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps, r

    def per_dispatch_median(fn):
        fn()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in evs:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(b) for a, b in evs]))

    n_tpl = inp.des_tpl.shape[0]
    n_frames = inp.q_off.numel() - 1
    match_ms, m = timed(lambda: pipeline.match_stage(inp, cfg))
    cons_ms, cons = timed(lambda: pipeline.device_consensus(m, n_tpl, n_frames, cfg))
    ransac_ms, rr = timed(lambda: pipeline.ransac_stage(m, inp.kp_tpl, cons, cfg))
    affines = pipeline.postprocess_affines(rr.params.cpu().numpy(), cfg)[0]
    a_dev = torch.from_numpy(np.ascontiguousarray(affines[: inp.frames.shape[0]])).to(inp.frames.device)
    warp_ms = per_dispatch_median(lambda: pipeline.warp_frames(inp.frames, a_dev, out=out))
    return {"match": round(match_ms, 4), "consensus": round(cons_ms, 4), "ransac": round(ransac_ms, 4),
            "warp": round(warp_ms, 4)}, cons


def host_cpus():
    """(usable CPUs, os.cpu_count(), sched_getaffinity size, cgroup CPU quota or None) of
    this host.  The reference sizes its joblib pool with multiprocessing.cpu_count() (VA:21,
    VA:462); the processes it can actually run at once are the affinity set, bounded by the
    container's CPU quota (cgroup v2 cpu.max) when there is one."""
    import math

    total = os.cpu_count() or 1
    aff = len(os.sched_getaffinity(0))
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, period = f.read().split()[:2]
        if q != "max":
            quota = float(q) / float(period)
    except (OSError, ValueError):
        pass
    usable = aff if quota is None else max(1, min(aff, math.ceil(quota)))
    return usable, total, aff, quota


def _cpu_pool(procs: int, initargs):
    """`procs` spawned worker processes (oracle/cpu_baseline_workers.py).  The children
    must not re-run this script's imports (torch, the HIP library), so the main module's
    __file__ is hidden from multiprocessing while they start."""
    import multiprocessing as mp

    import cpu_baseline_workers as W  # noqa: F401  (oracle/, on sys.path)

    main = sys.modules["__main__"]
    saved = main.__dict__.pop("__file__", None)
    try:
        pool = mp.get_context("spawn").Pool(procs, initializer=W.init, initargs=initargs)
        pool.map(W.ping, range(procs), chunksize=1)
    finally:
        if saved is not None:
            main.__file__ = saved
    return pool


def cpu_baseline(bc: BenchConfig, ks, n_sample: int, procs: int):
    """The oracle restatement of the reference CPU path on a bounded sample, structured
    like the reference: the per-frame stages (C knnMatch + the reference's numpy filters;
    the numpy/LAPACK restatement of skimage 0.18.3 ransac with per-trial SVD; C warp) in
    `procs` single-threaded worker processes over frame chunks (the reference's joblib
    pool, VA:460-465), CPython consensus in the parent.  `procs` defaults to the host's
    usable CPUs (host_cpus): the reference's cpu_count()-sized pool as this host runs it."""
    import shutil
    import tempfile

    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import oracle  # cpu_baseline leg: the oracle is what is timed here
    import cpu_baseline_workers as W
    from threadpoolctl import threadpool_limits

    usable, total, aff, quota = host_cpus()
    base = make_texture(bc)
    procs = max(1, min(procs, n_sample))
    arrays = dict(des_tpl=ks.des_tpl, kp_tpl=ks.kp_tpl, des_q=ks.des_q, kp_q=ks.kp_q, q_off=ks.q_off, base=base)
    tmp = None
    chunks = [c.tolist() for c in np.array_split(np.arange(n_sample), procs)]
    with threadpool_limits(1):
        if procs == 1:
            W.init(arrays, bc.model, bc.descriptor)
            run = lambda fn, args: [fn(a) for a in args]  # noqa: E731
            pool = None
        else:
            tmp = tempfile.mkdtemp(prefix="kcmc_cpu_", dir="/tmp")
            for k, a in arrays.items():
                np.save(os.path.join(tmp, k + ".npy"), np.ascontiguousarray(a))
            pool = _cpu_pool(procs, (tmp, bc.model, bc.descriptor))
            run = lambda fn, args: pool.map(fn, args, chunksize=1)  # noqa: E731
        try:
            t0 = time.perf_counter()
            res = run(W.match_chunk, chunks)
            sets = [s for r in res for s, _ in r]
            kqs = [kq for r in res for _, kq in r]
            t1 = time.perf_counter()
            cons, _, _ = oracle.consensus(sets, bc.n_kp_global)
            lists = oracle.lookup(cons, sets)
            t2 = time.perf_counter()
            run(W.ransac_warp_chunk, [[(kqs[f], lists[f]) for f in c] for c in chunks])
            t3 = time.perf_counter()
        finally:
            if pool is not None:
                pool.close()
                pool.join()
            if tmp is not None:
                shutil.rmtree(tmp, ignore_errors=True)
    total_s = t3 - t0
    calib = ""
    try:  # the port against the reference's own code, measured in the build container
        with open(os.path.join(REPO, "profiles", "r03_cpu_reference_calibration.json")) as f:
            c = json.load(f)
        calib = (f"; calibration (profiles/r03_cpu_reference_calibration.json, {c['host']}): the port's RANSAC "
                 f"runs at {c['port_speed_over_reference']}x the speed of the reference's own "
                 f"_parallelize(_compute_euclidean_affine) with scikit-image 0.18.3 on the same {c['procs']} cores "
                 f"({c['port']['ms_per_frame_per_core']} vs {c['reference']['ms_per_frame_per_core']} ms/frame/core, "
                 f"N = 90, identical parameters)")
    except (OSError, ValueError, KeyError):
        pass
    return {
        "value": n_sample / total_s,
        "unit": "aligned frames/s",
        "cores": min(procs, usable),
        "kind": "port",
        "processes": procs,
        "host": {"usable_cpus": usable, "os_cpu_count": total, "sched_getaffinity": aff,
                 "cgroup_cpu_quota": quota},
        "sample": (f"{n_sample} frames of {bc.name} ({bc.H}x{bc.W}x{bc.C} u16, n_tpl={bc.n_tpl}, D={bc.D}, "
                   f"n_kp_global={bc.n_kp_global}, {bc.model}), {procs} single-threaded worker process(es) "
                   f"like the reference's joblib pool (VA:21 sizes it by multiprocessing.cpu_count() = "
                   f"{total} here; this host runs {usable} at once: sched_getaffinity {aff}, cgroup quota "
                   f"{'none' if quota is None else f'{quota:g} CPUs'}; {n_sample / procs:.1f} frames per process): "
                   f"match {1e3 * (t1 - t0):.0f} ms "
                   f"(C oracle knnMatch + reference numpy filters), consensus {1e3 * (t2 - t1):.1f} ms "
                   f"(CPython set/Counter, parent), RANSAC + warp {1e3 * (t3 - t2):.0f} ms "
                   f"(numpy/LAPACK restatement of skimage 0.18.3 with 1000 trials; C warp)" + calib),
        "seconds": total_s,
    }


def with_detection(inp, cfg, dev, world: int, reps: int = 3):
    """Device-resident frames -> aligned frames including the front end the hot path
    excludes: exact percentile normalisation (f2) and the build's ORB-style detector
    (f1, 500 keypoints per frame) on the synthetic video, then match / consensus /
    RANSAC / warp as in `value`."""
    out = torch.empty_like(inp.frames)
    res = pipeline.align_frames(inp.frames, cfg, out=out)
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        res = pipeline.align_frames(inp.frames, cfg, out=out)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / reps
    F = inp.frames.shape[0]
    return {"value": round(F * world / el, 1), "unit": "frames/s", "ms_per_pass": round(1e3 * el, 3),
            "template_keypoints": res.extras["n_template_keypoints"], "skipped_frames": len(res.skipped),
            "note": "normalisation + ORB-style detection + match + consensus + RANSAC + warp, frames on the device"}


def end_to_end(bc: BenchConfig, inp, cfg, dev, world: int, reps: int = 3):
    """PCIe-inclusive rate: the frames start and end in pinned host memory (analysis on
    the device-resident keypoints as in the hot path, then H2D / warp / D2H streamed in
    64-frame slabs).  Detection is excluded, as everywhere in this bench."""
    F = inp.frames.shape[0]
    host_in = inp.frames.cpu().pin_memory()
    host_out = torch.empty_like(host_in).pin_memory()
    pipeline.align_streamed(host_in, inp, cfg, out_host=host_out)
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        pipeline.align_streamed(host_in, inp, cfg, out_host=host_out)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / reps
    frame_bytes = host_in[0].numel() * host_in.element_size()
    return {"value": round(F * world / el, 1), "unit": "frames/s", "ms_per_pass": round(1e3 * el, 3),
            "pcie_GBps_each_way": round(F * frame_bytes / el / 1e9, 2),
            "note": "frames in pinned host memory, H2D + analysis + warp + D2H; detection excluded"}


def load_traffic(config: str):
    """HBM bytes per warp launch from the committed rocprofv3 PMC pass of this config
    (tools/pmc_warp.sh + tools/pmc_summary.py --sha), if present, with its source: the
    profiles/ file and the commit of the code it was measured on."""
    name = "warp_pmc_traffic.json" if config == "c2" else f"warp_pmc_traffic_{config}.json"
    p = os.path.join(REPO, "profiles", name)
    try:
        with open(p) as f:
            d = json.load(f)
        return d.get("hbm_bytes_per_launch"), {"file": f"profiles/{name}", "commit": d.get("commit"),
                                               "kernel_avg_ms_in_pmc_run": d.get("kernel_avg_ms")}
    except (OSError, ValueError):
        return None, None


def rank_envs(n: int, base_env: dict, port: int) -> list:
    """The environment of each rank process spawn_ranks starts (torchrun's variables)."""
    envs = []
    for r in range(n):
        e = dict(base_env)
        e.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                  "GROUP_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
        envs.append(e)
    return envs


def check_devices(n: int, visible: int, one_device: bool) -> None:
    """--gpus n needs n visible devices (unless every rank shares cuda:0, the rehearsal)."""
    if n > visible and not one_device:
        raise SystemExit(f"bench.py: --gpus {n} but only {visible} device(s) visible; refusing to report a "
                         f"{visible}-GPU number as {n} GPUs (set KCMC_BENCH_ONE_DEVICE=1 with "
                         f"KCMC_BENCH_BACKEND=gloo to rehearse {n} ranks on cuda:0)")


def spawn_ranks(n: int, argv: list) -> int:
    """Start `n` rank processes of this script (one per GPU) and wait for them; rank 0 prints
    the JSON line.  Runs before this process touches the GPU (device_count() does not
    initialise it on this image); the children are started, never exec'd into."""
    import signal
    import socket
    import subprocess

    with socket.socket() as sk:  # a free rendezvous port on the loopback
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=e)
             for e in rank_envs(n, os.environ, port)]
    rc = 0
    try:
        while procs:
            for p in list(procs):
                r = p.poll()
                if r is None:
                    continue
                procs.remove(p)
                if r != 0 and rc == 0:
                    rc = r
                    for q in procs:  # one rank failed: the others would wait in a collective
                        q.send_signal(signal.SIGTERM)
            time.sleep(0.05)
    finally:
        for p in procs:
            p.kill()
    return rc if rc >= 0 else 1


FP32_PEAK_TFLOPS = 157.3  # dense fp32 vector (packed) (MI355X_MICROARCH.md)
FP64_PEAK_TFLOPS = 78.6   # fp64 vector
# Algorithmic flops of one (trial, point) residual test: the map (X, Y) = A (x, y) + t
# (4 mul + 4 add), the residual (2 sub), q = ex^2 + ey^2 (2 mul + 1 add); the projective
# map adds w (2 mul + 2 add) and two divisions (counted as 1 each).
RANSAC_FLOPS_PER_TEST = {"euclidean": 13, "affine": 13, "projective": 19}


def ransac_roofline(model: str, cons, cfg, ransac_ms: float) -> dict:
    """The RANSAC stage against its VALU peak: every trial of every fitted frame tests all N
    of the frame's points (phase A), at RANSAC_FLOPS_PER_TEST flops each, over the isolated
    stage time.  The rigid scorer's phase A runs in fp32 (ransac_common.h score32; priced
    against the fp32 vector peak), the affine / projective ones in fp64."""
    n = np.diff(cons.pt_off)
    fitted = n[n >= cfg.effective_frame_skip]
    tests = float(fitted.sum()) * TRIALS
    fl = RANSAC_FLOPS_PER_TEST[model]
    achieved = tests * fl / (ransac_ms * 1e-3) / 1e12
    peak = FP32_PEAK_TFLOPS if model == "euclidean" else FP64_PEAK_TFLOPS
    return {"kernel": "ransac_rigid_kernel (fp32 phase A)" if model == "euclidean"
            else f"ransac_model_score_kernel<{model}> (fp64 phase A) + refit",
            "bound": "valu", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": None, "avg_launch_ms": ransac_ms,
            "trial_point_tests": tests, "flops_per_test": fl,
            "note": "achieved = trials x points x flops per residual test / isolated stage time (fit, "
                    "selection, exact re-scoring of tied trials and the refit are overhead, not counted)"}


def single_process(args, bc: BenchConfig) -> dict:
    """The drop-in VideoAligner's multi-GPU path (kcmc_amd.multidevice.align_split): one
    process, one contiguous frame slab per device of ``devices`` (a device may repeat), the
    consensus merge and the gap interpolation once on the host per step.  Steps are not
    pipelined across each other (each align_split call returns the aligned frames), which is
    what a caller of VideoAligner.align_keypoints with device-resident frames gets."""
    devices = [int(d) for d in args.devices.replace("+", ",").split(",")] if args.devices else list(range(args.gpus))
    cfg = pipeline.AlignConfig(n_kp_global=bc.n_kp_global, ransac_model=bc.model)
    slabs, ranges = [], []
    for k, d in enumerate(devices):
        dev = torch.device("cuda", d)
        inp, _ = make_inputs(bc, args.frames, k, dev)  # same template (seed 3), own frames per slab
        slabs.append(inp)
        f0 = k * args.frames
        ranges.append(md.SlabRange(f0, f0 + args.frames, f0, f0 + args.frames))
    log(f"single process: {len(devices)} slab(s) of {args.frames} frames on devices {devices}")

    def sync():
        for d in sorted(set(devices)):
            torch.cuda.synchronize(d)

    for _ in range(args.warmup):
        md.align_split(slabs, ranges, cfg)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = md.align_split(slabs, ranges, cfg)
    sync()
    elapsed = time.perf_counter() - t0
    total = args.frames * len(devices)
    ms_step = 1e3 * elapsed / args.steps
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, res.aligned, res, total)
    result = {
        "metric": METRIC, "value": round(total * args.steps / elapsed, 1), "unit": "frames/s",
        "n_gpus": len(set(devices)), "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "u16 frames; u8/f32 descriptors, f64 RANSAC, f32 warp weights",
        "data": "synthetic (seeded jittered texture + detector-shaped keypoints; no detector in image)",
        "config": {"workload": bc.workload, "frames_per_slab": args.frames, "devices": devices,
                   "parallelism": f"single-process split x{len(devices)} (VideoAligner drop-in path)"},
        "skipped_frames": len(res.skipped),
    }
    if args.full:  # slab 0's stages alone: runs of their own after the timed region
        out0 =torch.empty_like(slabs[0].frames)
        torch.cuda.set_device(slabs[0].frames.device)
        iso, _ = isolated_stage_ms(slabs[0], cfg, out0)
        warp_bytes = 2 * slabs[0].frames.numel() * slabs[0].frames.element_size()
        achieved = warp_bytes / (iso["warp"] * 1e-3) / 1e9
        result["stage_ms_isolated_slab0"] = iso
        result["roofline"] = {"kernel": (f"warp_perspective_u16_kernel<{bc.C}>" if bc.model == "projective"
                                         else f"warp_affine_u16_kernel<{bc.C}>"), "bound": "hbm",
                              "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None,
                              "algorithmic_bytes_per_launch": warp_bytes, "avg_launch_ms": iso["warp"],
                              "note": "slab 0's warp alone (median of per-dispatch HIP events)"}
    return result


def full_figures(result: dict, bc: BenchConfig, inp, cfg, out, warp_bytes: int) -> None:
    """--full: every GPU stage alone after the timed region (isolated_stage_ms) and the
    figures priced on those times, added to the result line."""
    iso, iso_cons = isolated_stage_ms(inp, cfg, out)
    iso_pts = np.diff(iso_cons.pt_off)
    iso_ransac = int((iso_pts >= cfg.effective_frame_skip).sum())
    # RANSAC kernel alone; the overlapped figure shares the CUs with the previous step's warp
    result["ransac_hypotheses_per_s_per_gpu"] = round(iso_ransac * TRIALS / (iso["ransac"] * 1e-3), 1)
    result["roofline_ransac"] = ransac_roofline(bc.model, iso_cons, cfg, iso["ransac"])
    result["stage_ms_isolated"] = iso
    # the warp's own roofline: the same launch alone, median of per-dispatch HIP event
    # pairs (the timed steps run RANSAC beside it, which `roofline` includes)
    result["roofline_isolated"] = {"kernel": "warp_plan_kernel + " + ("warp_perspective_u16_kernel"
                                                                     if cfg.ransac_model == "projective" else
                                                                     "warp_affine_u16_kernel"),
                                   "achieved": round(warp_bytes / (iso["warp"] * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                                   "unit": "GB/s",
                                   "frac": round(warp_bytes / (iso["warp"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                   "median_launch_ms": iso["warp"]}
    # the matcher against its rooflines (the dominant kernel of c5): algorithmic work
    # 2 * n_tpl * n_q * D per frame.  The float matcher issues one fp16 product per fp32
    # product (a certified candidate search; exact fp64 re-rank of 2-3 candidates), priced
    # against fp16 dense (= bf16 dense); its bound is the top-8 selection on VALU, reported
    # beside it against 8 integer VALU per distance (round 3's reference count, kept so the
    # fraction compares across rounds)
    n_q_total = float(inp.q_off_host[-1])
    match_ops = 2.0 * bc.n_tpl * n_q_total * bc.D
    iso_match_s = iso["match"] * 1e-3
    if bc.descriptor == "f32":
        issued = match_ops / iso_match_s / 1e12
        dists = match_ops / (2.0 * bc.D) / iso_match_s / 1e12
        valu_peak = VALU_INSTR_PER_S_PER_GPU * 64 / 8.0 / 1e12
        result["roofline_match"] = {
            "kernel": "tpl_stats + frame_images + knn2_l2f32_kernel (fp16 MFMA, top-8, exact re-rank) + fallback "
                      "+ match_filter (whole match stage)",
            "bound": "valu", "achieved": round(issued, 1), "peak": BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(issued / BF16_PEAK_TFLOPS, 4), "traffic": None,
            "algorithmic_tflops_fp32_equiv": round(issued, 1),
            "avg_launch_ms": iso["match"],
            "valu_bound": {"distances_per_s_T": round(dists, 3), "peak_distances_per_s_T": round(valu_peak, 3),
                           "frac": round(dists / valu_peak, 4),
                           "note": "peak = 1024 SIMDs x 0.25 wave64 VALU instr/cycle x 2.4 GHz x 64 lanes / 8 VALU "
                                   "per distance (the reference count; the top-8 costs 1 compare per distance "
                                   "plus 9 VALU when some lane of the wave inserts)"},
            "note": "achieved = issued fp16 MFMA work (= algorithmic) / isolated stage time; frac against dense fp16"}
    else:
        tops = match_ops / iso_match_s / 1e12
        # knn2_l2u8 is bound by its integer VALU top-2 epilogue (~2.5 VALU per distance), not
        # by the i8 MFMA: the MFMA fraction is reported beside the VALU-issue one
        valu_per_dist = 2.5
        valu_peak = VALU_INSTR_PER_S_PER_GPU * 64 / valu_per_dist / 1e12  # distances/s (T)
        dists = match_ops / (2.0 * bc.D) / iso_match_s / 1e12
        result["roofline_match"] = {
            "kernel": "knn2_l2u8_kernel + match_filter_kernel (whole match stage)", "bound": "valu",
            "achieved": round(tops, 1), "peak": I8_PEAK_TOPS, "unit": "TOP/s", "frac": round(tops / I8_PEAK_TOPS, 4),
            "traffic": None, "avg_launch_ms": iso["match"],
            "valu_bound": {"distances_per_s_T": round(dists, 3), "peak_distances_per_s_T": round(valu_peak, 3),
                           "frac": round(dists / valu_peak, 4),
                           "note": "peak = 1024 SIMDs x 0.25 wave64 VALU instr/cycle x 2.4 GHz x 64 lanes / "
                                   "2.5 VALU per distance (the top-2 epilogue); frac/peak above = i8 MFMA"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c2",
                    help="BASELINE workload (c2 = configs[1], the headline line)")
    ap.add_argument("--frames", type=int, default=None, help="frames per GPU (default: the config's)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run what takes runs of its own: every GPU stage alone "
                         "(stage_ms_isolated, the RANSAC / match / isolated-warp rooflines) and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one returned (a seeded sample of the aligned "
                         "frames, the affines, the consensus and RANSAC results) as DIR/<name>.npy")
    ap.add_argument("--cpu-sample", type=int, default=None,
                    help="with --full: frames in the CPU-baseline sample (0: skip)")
    ap.add_argument("--cpu-procs", type=int, default=None,
                    help="worker processes of the CPU baseline (default: the host's usable CPUs, the "
                         "reference's cpu_count()-sized pool as this host runs it)")
    ap.add_argument("--cpu-procs-secondary", type=int, default=8,
                    help="also time the CPU baseline at this many processes (the round-1..3 figure; 0: skip)")
    ap.add_argument("--e2e", action="store_true",
                    help="also time the PCIe-inclusive path: frames in pinned host memory, streamed through "
                         "the warp in slabs (pipeline.align_streamed); reported as `end_to_end`, not `value`")
    ap.add_argument("--detect", action="store_true",
                    help="also time align from raw uint16 frames on the device: normalisation + ORB-style "
                         "detection + the hot path (pipeline.align_frames); reported as `with_detection`")
    ap.add_argument("--single-process", action="store_true",
                    help="one process over --gpus devices (or --devices): the drop-in VideoAligner's split path "
                         "(kcmc_amd.multidevice), not the torchrun one-process-per-GPU path")
    ap.add_argument("--devices", default=None,
                    help="with --single-process: device list separated by , or +, a device may repeat (e.g. 0+0)")
    ap.add_argument("--serial", action="store_true",
                    help="run steps back to back on one stream (no warp/analysis overlap between steps)")
    args = ap.parse_args()
    bc = CONFIGS[args.config]
    if args.frames is None:
        args.frames = bc.frames_per_gpu
    if args.cpu_procs is None:
        args.cpu_procs = host_cpus()[0]
    if args.cpu_sample is None:
        # at least 4 frames per process, within the frames the config makes
        args.cpu_sample = min(max(bc.cpu_sample * max(1, args.cpu_procs) // 2, 4 * args.cpu_procs),
                              args.frames if args.frames else bc.frames_per_gpu)

    if args.single_process:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--single-process runs in one process (not under torchrun)")
        if not args.devices:
            check_devices(args.gpus, torch.cuda.device_count(), False)
        print(json.dumps(single_process(args, bc)), flush=True)
        return

    # KCMC_BENCH_BACKEND=gloo + KCMC_BENCH_ONE_DEVICE=1: rehearsal of the multi-rank
    # path with every rank on cuda:0 (a 1-GPU box cannot host two RCCL ranks)
    one_device = os.environ.get("KCMC_BENCH_ONE_DEVICE") == "1"
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        check_devices(args.gpus, torch.cuda.device_count(), one_device)
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))
    backend = os.environ.get("KCMC_BENCH_BACKEND", "nccl")
    rank, world, local = kdist.init_from_env(backend)
    if world != args.gpus:
        if args.gpus != 1:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
        log(f"note: WORLD_SIZE={world} without --gpus; using WORLD_SIZE")
    if not one_device:
        check_devices(world, torch.cuda.device_count(), False)
    if one_device:
        local = 0
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    t_setup = time.perf_counter()
    inp, ks = make_inputs(bc, args.frames, rank, dev)
    if world > 1:
        # the template descriptors/keypoints come from rank 0 (the reference pickles them
        # to every worker, VA:117-123 / VA:460-465): the other ranks' copies are discarded
        if rank != 0:
            inp.des_tpl.zero_()
            inp.kp_tpl.zero_()
        kdist.broadcast_template(inp.des_tpl, inp.kp_tpl)
    out = torch.empty_like(inp.frames)
    cfg = pipeline.AlignConfig(n_kp_global=bc.n_kp_global, ransac_model=bc.model)
    counts = [args.frames] * world
    log(f"[rank {rank}] setup {time.perf_counter() - t_setup:.1f}s; {args.frames} frames {bc.H}x{bc.W}x{bc.C} on {dev}")

    ov = None if args.serial else pipeline.OverlappedSlabs(dev, cfg, counts=counts if world > 1 else None,
                                                            match_beside=bc.match_beside)

    def step(timer):
        if ov is None:
            return run_step(inp, cfg, out, timer, world, counts)
        return ov.submit(inp, out=out, mark=timer.mark if timer else None)

    def drain(timer):  # the pipelined schedule: finish the slabs still in flight
        if ov is None:
            return None
        res = ov.flush(mark=timer.mark if timer else None)
        return res[-1] if res else None

    for _ in range(args.warmup):
        step(None)
    drain(None)
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    timer = StageTimer()
    if ov is not None:
        ov.stats = {k: 0.0 for k in ov.stats}
    t0 = time.perf_counter()
    # K steps = K passes of match -> consensus -> RANSAC -> post-processing -> warp; the
    # pipelined schedule starts empty and is drained inside the timed region
    last = None
    for _ in range(args.steps):
        last = step(timer) or last
    last = drain(timer) or last
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    cons = last.consensus  # `last`: the SlabResult of the last timed step
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last.aligned, last, args.frames, suffix=f"_rank{rank}" if world > 1 else "")
    ms_step = 1e3 * elapsed / args.steps
    total_frames = args.frames * world
    fps = total_frames * args.steps / elapsed
    warp_ms = float(np.mean(timer.elapsed("w0", "w1")))
    match_ms = float(np.mean(timer.elapsed("m0", "m1")))
    ransac_ms = float(np.mean(timer.elapsed("r0", "r1")))
    n_pts = np.diff(cons.pt_off)
    n_ransac = int((n_pts >= cfg.effective_frame_skip).sum())
    warp_bytes = 2 * inp.frames.numel() * inp.frames.element_size()  # read + write, algorithmic
    achieved = warp_bytes / (warp_ms * 1e-3) / 1e9
    # the committed PMC pass was taken at the config's own frame count: quote it only there
    traffic, traffic_src = load_traffic(bc.name) if args.frames == bc.frames_per_gpu else (None, None)
    stage_ms = {"match": round(match_ms, 3), "ransac": round(ransac_ms, 3), "warp": round(warp_ms, 3)}
    if ov is None:
        stage_ms["host_and_transfers"] = round(ms_step - match_ms - ransac_ms - warp_ms, 3)
    else:  # step k+1's match/consensus/RANSAC/post-processing overlap step k's warp
        if bc.match_beside:
            stage_ms["schedule"] = ("pipelined: kernel stream warp(k-1); analysis stream match+vote(k) -> "
                                    "lookup+RANSAC(k) beside it; host consensus merge under the warp")
        else:
            stage_ms["schedule"] = ("pipelined: match+vote(k) -> warp(k-1) on the kernel stream, lookup+RANSAC(k) "
                                    "on a second stream beside the warp; host consensus merge under the warp")
        stage_ms["step_minus_warp"] = round(ms_step - warp_ms, 3)
        # rank 0's host seconds per step blocked in event waits / inside the all-gathers, and
        # its consensus merge / post-processing (OverlappedSlabs.stats)
        stage_ms["host_ms_per_step_rank0"] = {k: round(1e3 * v / args.steps, 4) for k, v in ov.stats.items()}
    result = {
        "metric": METRIC,
        "value": round(fps, 1),
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_step, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": ("u16 frames; " + ("f32 descriptors: fp16 MFMA candidate search (certified bound) + exact f64 re-rank"
                                    if bc.descriptor == "f32" else "u8 descriptors: i8 MFMA exact integer distances")
                  + ", f64 RANSAC, f32 warp weights"),
        "data": (f"synthetic (seeded jittered {bc.W}x{bc.H}{'x%d' % bc.C if bc.C > 1 else ''} u16 texture + "
                 f"{'SIFT' if bc.descriptor == 'f32' else 'ORB/AKAZE'}-shaped keypoints; no detector in image)"),
        "config": {
            "workload": bc.workload,
            "frames_per_gpu": args.frames, "height": bc.H, "width": bc.W, "channels": bc.C, "n_tpl": bc.n_tpl,
            "descriptor_len": bc.D, "descriptor_dtype": "float32" if bc.descriptor == "f32" else "uint8", "n_kp_global": bc.n_kp_global, "ransac_model": bc.model,
            "ransac_trials": TRIALS, "parallelism": f"frame-sharded x{world}",
        },
        # RANSAC beside the previous step's warp, sharing the CUs with it (the kernel alone:
        # `ransac_hypotheses_per_s_per_gpu` of a --full run)
        "ransac_hypotheses_per_s_per_gpu_overlapped": round(n_ransac * TRIALS / (ransac_ms * 1e-3), 1),
        "ransac_mean_points": round(float(n_pts.mean()), 2),
        "stage_ms": stage_ms,
        "roofline": {
            "kernel": (f"warp_perspective_u16_kernel<{bc.C}>" if bc.model == "projective"
                       else f"warp_affine_u16_kernel<{bc.C}>"),
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": traffic,
            "traffic_source": traffic_src,
            "algorithmic_bytes_per_launch": warp_bytes,
            "avg_launch_ms": round(warp_ms, 4),
        },
    }
    if args.full:
        full_figures(result, bc, inp, cfg, out, warp_bytes)
    if args.e2e:
        result["end_to_end"] = end_to_end(bc, inp, cfg, dev, world)
    if args.detect and bc.C == 1:
        result["with_detection"] = with_detection(inp, cfg, dev, world)
    if args.full and rank == 0 and world == 1 and args.cpu_sample > 0:
        result["cpu_baseline"] = cpu_baseline(bc, ks, args.cpu_sample, args.cpu_procs)
        p2 = args.cpu_procs_secondary
        if p2 and p2 != args.cpu_procs:
            sec = cpu_baseline(bc, ks, min(args.cpu_sample, max(4 * p2, bc.cpu_sample * p2 // 2)), p2)
            result["cpu_baseline"]["secondary"] = {k: sec[k] for k in ("value", "cores", "processes", "seconds")}
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

"""The quality-metric kernels (csrc/quality.hip) timed with HIP events beside the warp, the
registration error of a refined template on a synthetic stack, and align_images with the
new switches off against another build of the library.

    python tools/quality_rates.py [--shapes c2,c3] [--reps 10] [--inner 10]
    python tools/quality_rates.py --accuracy [--frames 41] [--noise 6000] [--template-noise 20000]
    python tools/quality_rates.py --align-ab ab/parent.so [--rounds 3]

Rates: kcmc_stack_sum_u16, kcmc_frame_stats_u16 and kcmc_warp_affine_u16 on the same
device-resident stack in one process, alternating, at config 2's shape (2000 x 1080 x 1920)
and config 3's (16000 x 512 x 512).  The C entry points are called directly into
preallocated outputs; every timed window is `inner` calls between two events after a
warm-up of the same shape.  Bytes are what the algorithm needs: the two reductions read the
stack (frame stats: the rectangle) once, the warp reads and writes it.  Each reduction is
expected to take no longer than the warp of the same run, which moves twice the bytes.

--accuracy: crops of one scene at known integer shifts with independent noise per frame and
more noise on the template frame; RMS error of the estimated translations against the
shifts after the first pass and after one template refinement (a record, not a test).

--align-ab: align_images with QUALITY_METRICS / TEMPLATE_REFINE_ITERS off, timed in fresh
child processes that alternate between the in-tree library and another build
(tools/ab_build.py parent <rev>), because a process loads one library.

Each mode prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from kcmc_amd import VideoAligner, _lib, stages, synthetic  # noqa: E402

SHAPES = {"c2": (2000, 1080, 1920), "c3": (16000, 512, 512)}


def _i64(t):
    """uint16 -> int64 on the device through the int16 view (torch indexes and converts
    int16 everywhere)."""
    return t.view(torch.int16).to(torch.int64) & 0xFFFF


def make_stack(F, H, W, dev, distinct=16, shift=lambda k: (37 * k, 53 * k)):
    """[F, H, W] uint16 on the device: `distinct` rolled copies of one texture, repeated
    (neither reduction has a data-dependent path; the warp's dark-tile path sees what the
    bench texture gives it)."""
    base = synthetic.make_texture((H, W), seed=7)
    stack = torch.empty((F, H, W), dtype=torch.int16, device=dev)
    for k in range(distinct):
        fr = np.ascontiguousarray(np.roll(base, shift(k), axis=(0, 1)))
        stack[k::distinct] = torch.from_numpy(fr.view(np.int16)).to(dev)
    return stack.view(torch.uint16)


def rates(shape_name, reps, inner, dev):
    F, H, W = SHAPES[shape_name]
    stack = make_stack(F, H, W, dev)
    out = torch.empty_like(stack)
    rng = np.random.default_rng(5)
    maps = np.tile(np.eye(2, 3), (F, 1, 1))
    maps[:, :, 2] = rng.uniform(-4, 4, (F, 2))
    maps_d = torch.from_numpy(maps).to(dev)
    ref = stack.view(torch.int16)[0].clone().view(torch.uint16)
    m = 6  # ceil(4) + 1 and one more: the rectangle a pass with these maps would use, odd x0
    region = (m, H - m, m + 1, W - m)
    sums = torch.empty(H * W, dtype=torch.int64, device=dev)
    stats = torch.empty((F, 5), dtype=torch.int64, device=dev)
    sel = torch.from_numpy((np.arange(F) % 2 == 0).view(np.uint8)).to(dev)
    L = _lib.load()
    ctx, st, ptr = stages._ctx(dev).handle, stages._stream(dev), stages._ptr
    calls = {
        "warp_affine": lambda: L.kcmc_warp_affine_u16(ctx, ptr(stack), ptr(out), ptr(maps_d), F, H, W, 1, 0, st),
        "stack_sum": lambda: L.kcmc_stack_sum_u16(ctx, ptr(stack), F, H * W, None, ptr(sums), st),
        "stack_sum_half": lambda: L.kcmc_stack_sum_u16(ctx, ptr(stack), F, H * W, ptr(sel), ptr(sums), st),
        "frame_stats": lambda: L.kcmc_frame_stats_u16(ctx, ptr(stack), F, H, W, ptr(ref), *region, ptr(stats), st),
    }
    px = F * H * W
    nbytes = {"warp_affine": 4 * px, "stack_sum": 2 * px, "stack_sum_half": px,
              "frame_stats": 2 * F * (region[1] - region[0]) * (region[3] - region[2])}
    ts = {k: [] for k in calls}
    for k, c in calls.items():  # warm-up: code objects, the warp's workspace
        for _ in range(2):
            _lib.check(c())
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, c in calls.items():  # alternating, so drift hits all alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                _lib.check(c())
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) / inner)
    res = {"shape": [F, H, W], "region": list(region)}
    for k in calls:
        med = float(np.median(ts[k]))
        res[k] = {"ms_median": round(med, 4), "ms_best": round(min(ts[k]), 4),
                  "ms_p90": round(float(np.percentile(ts[k], 90)), 4), "gbytes": round(nbytes[k] / 1e9, 3),
                  "tb_per_s": round(nbytes[k] / med / 1e9, 3)}
    for k in ("stack_sum", "stack_sum_half", "frame_stats"):
        res[k]["over_warp"] = round(res[k]["ms_median"] / res["warp_affine"]["ms_median"], 4)
    res["reductions_within_warp_time"] = all(res[k]["over_warp"] <= 1.0 for k in ("stack_sum", "frame_stats"))
    # the sums of the last calls against torch on a few frames / pixels
    torch.cuda.synchronize()
    _lib.check(calls["stack_sum"]())
    cols = torch.arange(0, H * W, 4099, device=dev)
    want = (stack.view(torch.int16).reshape(F, -1)[:, cols].to(torch.int64) & 0xFFFF).sum(0)
    res["stack_sum_spot_check"] = bool(torch.equal(sums[cols], want))
    a = _i64(stack[F - 1, region[0]:region[1], region[2]:region[3]])
    b = _i64(ref[region[0]:region[1], region[2]:region[3]])
    want = torch.stack([a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()])
    res["frame_stats_spot_check"] = bool(torch.equal(stats[F - 1], want))
    return res


def noisy_scene(frames, noise, template_noise, seed=31):
    """The scene construction of tests/test_gpu_quality.py (crops of one scene at integer
    shifts <= 6, the middle frame unshifted) plus independent Gaussian noise per frame and
    more of it on the template frame."""
    rng = np.random.default_rng(seed)
    H, W = 200, 260
    lo = rng.integers(0, 60000, (H // 4 + 8, W // 4 + 8)).astype(np.float64)
    scene = np.clip(np.kron(lo, np.ones((4, 4))) + rng.normal(0, 800, (H + 32, W + 32)), 0, 65535)
    shifts = [(int(a), int(b)) for a, b in rng.integers(-6, 7, (frames, 2))]
    shifts[frames // 2] = (0, 0)
    imgs = np.stack([scene[16 + dy:16 + dy + H, 16 + dx:16 + dx + W] for dy, dx in shifts])
    sigma = np.full(frames, float(noise))
    sigma[frames // 2] = float(template_noise)
    imgs = imgs + rng.normal(0, 1, imgs.shape) * sigma[:, None, None]
    return np.clip(imgs, 0, 65535).astype(np.uint16), np.array(shifts, np.float64)


def accuracy(a):
    imgs, shifts = noisy_scene(a.frames, a.noise, a.template_noise)
    truth = shifts[:, ::-1]  # (tx, ty) = (dx, dy)

    def run(iters):
        class VA(VideoAligner):
            DEVICES = [0]
            QUALITY_METRICS = True
            TEMPLATE_REFINE_ITERS = iters

        va = VA()
        try:
            _, eu, skipped = va.align_images(imgs, n_kp_global=60, detector_algorithm="orb", frame_rate=30)
        except (VideoAligner.AlignmentError, ValueError) as e:  # a result of the measurement too
            return {"error": f"{type(e).__name__}: {e}"}
        err = eu[:, :2] - truth
        return {"rms_translation_error_px": round(float(np.sqrt((err ** 2).sum(1).mean())), 4),
                "max_translation_error_px": round(float(np.abs(err).max()), 4),
                "skipped": [int(i) for i in skipped], "template_keypoints": int(len(va._kp_template)),
                "mean_correlation": [round(float(np.nanmean(c)), 6) for c in va.correlation_history],
                "valid_region": list(va.valid_region)}

    return {"frames": a.frames, "size": list(imgs.shape[1:]), "noise_sigma": a.noise,
            "template_noise_sigma": a.template_noise, "pass_1": run(0), "refined_1": run(1), "refined_2": run(2)}


def align_child(a):
    """ms per align_images call (switches off) on a device-resident stack, in this process."""
    dev = torch.device("cuda", 0)
    F, H, W = 500, 512, 512
    stack = make_stack(F, H, W, dev, distinct=F, shift=lambda k: (k % 7 - 3, k % 5 - 2))

    class VA(VideoAligner):
        DEVICES = [0]

    va = VA()
    ts = []
    for i in range(a.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = va.align_images(stack, n_kp_global=60, detector_algorithm="orb", frame_rate=30)
        torch.cuda.synchronize()
        if i >= 2:  # two warm-up calls
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"lib": os.environ.get("KCMC_LIB_PATH", "in-tree"), "shape": [F, H, W],
            "ms_median": round(float(np.median(ts)), 3), "ms_best": round(min(ts), 3),
            "digest": int(_i64(out[0]).sum().item()), "skipped": len(out[2])}


def align_ab(a):
    runs = {"in-tree": [], a.align_ab: []}
    for rnd in range(a.rounds):
        for lib in (list(runs) if rnd % 2 == 0 else list(runs)[::-1]):  # alternating fresh processes, A B B A ...
            env = dict(os.environ)
            if lib != "in-tree":
                env.update(KCMC_LIB_PATH=os.path.abspath(lib), KCMC_TEST_ONLY_ALT_LIB="1")
            r = subprocess.run([sys.executable, "-W", "ignore", os.path.abspath(__file__), "--align-child", "--reps",
                                str(a.reps)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"child failed ({lib}):\n{r.stdout}\n{r.stderr}")
            runs[lib].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"shape": runs["in-tree"][0]["shape"], "rounds": a.rounds, "reps": a.reps}
    for lib, rs in runs.items():
        out[lib] = {"ms_median_per_round": [r["ms_median"] for r in rs], "ms_best": min(r["ms_best"] for r in rs),
                    "digest": rs[0]["digest"]}
    out["same_output"] = out["in-tree"]["digest"] == out[a.align_ab]["digest"]
    out["in_tree_over_other"] = round(float(np.median(out["in-tree"]["ms_median_per_round"]) /
                                            np.median(out[a.align_ab]["ms_median_per_round"])), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--noise", type=float, default=6000.0)
    ap.add_argument("--template-noise", type=float, default=20000.0)
    ap.add_argument("--align-ab", default=None)
    ap.add_argument("--align-child", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    if a.align_child:
        print(json.dumps(align_child(a)))
    elif a.align_ab:
        print(json.dumps(align_ab(a)))
    elif a.accuracy:
        print(json.dumps(accuracy(a)))
    else:
        dev = torch.device("cuda", 0)
        out = {"lib": os.environ.get("KCMC_LIB_PATH", "in-tree"), "reps": a.reps, "inner": a.inner}
        for name in a.shapes.split(","):
            out[name] = rates(name, a.reps, a.inner, dev)
            torch.cuda.empty_cache()
        print(json.dumps(out))


if __name__ == "__main__":
    main()

"""A campaign of tests/sweep_cases.py's seeded cases on one device: the generator-and-compare
code of tests/test_gpu_sweeps.py over any seed range.

    python tools/kernel_sweeps.py --kernel shift_search --seeds 1000:1300

Prints one line per case and a JSON summary line.  Stops at the first mismatch, exception or
HIP error and prints the failing case (exit status 1); it never retries a case and never goes
on after an error.  A failing seed is evidence for a fix and a candidate for
sweep_cases.PINNED; nothing in the suite depends on this tool."""
import argparse
import json
import os
import sys
import time
import traceback

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import kcmc_amd  # noqa: E402,F401  (registers the package name)
import sweep_cases as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernel", required=True, choices=sc.KERNELS)
    ap.add_argument("--seeds", required=True, help="A:B, the seeds A .. B - 1")
    args = ap.parse_args()
    a, b = (int(v) for v in args.seeds.split(":"))
    import torch

    dev = torch.device("cuda", 0)
    t0, done = time.time(), 0
    for seed in range(a, b):
        t1 = time.time()
        try:
            case = sc.check(args.kernel, seed, dev)
            torch.cuda.synchronize(dev)
        except BaseException:
            traceback.print_exc()
            print(f"FAILED {args.kernel} seed {seed}: {sc.describe(sc.GENERATORS[args.kernel](seed))}", flush=True)
            print(json.dumps({"kernel": args.kernel, "seeds": args.seeds, "passed": done, "failed_seed": seed}))
            return 1
        done += 1
        shape = {k: case[k] for k in ("F", "H", "W")}
        print(f"ok {args.kernel} seed {seed} {shape} {time.time() - t1:.2f} s", flush=True)
    print(json.dumps({"kernel": args.kernel, "seeds": args.seeds, "passed": done, "failed_seed": None,
                      "seconds": round(time.time() - t0, 1)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Print the device timeline (kernels + memory copies, with the idle gaps between them)
of a window of a rocprofv3 --kernel-trace --memory-copy-trace CSV run.

    python tools/timeline.py gpurun_out/<prof_dir> [--around warp_affine --index 10 --count 2]
    python tools/timeline.py <prof_dir> --intervals   (RANSAC against the tile kernels, medians)
"""
import csv
import glob
import os
import re
import sys


def intervals(d, tile="warp_affine_u16_kernel", ransac="ransac_rigid_kernel", plan="warp_plan_kernel"):
    """--intervals: how RANSAC(k) sits against tile kernel k - 1 (profiles/ransac_slot_ab.md).
    RANSAC(k) is the last RANSAC kernel that ends before tile kernel k starts (warp k waits for
    its parameters).  Medians over every consecutive pair of tile kernels, in microseconds."""
    import statistics

    ev = {tile: [], ransac: [], plan: []}
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(p)):
            for key in ev:
                if key in r["Kernel_Name"]:
                    ev[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for v in ev.values():
        v.sort()
    r_end, gap, r_dur = [], [], []
    for (ps, pe), (s, e) in zip(ev[tile], ev[tile][1:]):
        rk = [x for x in ev[ransac] if x[1] <= s and x[0] >= ps]  # launched since tile k - 1 began
        if not rk:
            continue
        r_end.append((rk[-1][1] - pe) / 1e3)
        r_dur.append((rk[-1][1] - rk[-1][0]) / 1e3)
        gap.append((s - pe) / 1e3)
    med = statistics.median
    print(f"pairs {len(gap)}: tile kernels {len(ev[tile])}, ransac kernels {len(ev[ransac])}, plan kernels {len(ev[plan])}")
    print(f"median end(RANSAC k) - end(tile k-1): {med(r_end):9.1f} us   (min {min(r_end):.1f}, max {max(r_end):.1f})")
    print(f"median start(tile k) - end(tile k-1): {med(gap):9.1f} us   (min {min(gap):.1f}, max {max(gap):.1f})")
    print(f"median plan kernel duration:          {med([e - s for s, e in ev[plan]]) / 1e3:9.1f} us")
    print(f"median RANSAC(k) duration:            {med(r_dur):9.1f} us")
    print(f"median tile kernel duration:          {med([e - s for s, e in ev[tile]]) / 1e3:9.1f} us")


def main():
    a = sys.argv[1:]
    d = a[0]
    if "--intervals" in a:
        return intervals(d)
    key = a[a.index("--around") + 1] if "--around" in a else "warp_affine"
    idx = int(a[a.index("--index") + 1]) if "--index" in a else 10
    cnt = int(a[a.index("--count") + 1]) if "--count" in a else 2
    ev = []

    def nm(s):
        s = s.replace("void ", "").replace("kcmc::", "").replace("(anonymous namespace)::", "")
        return re.split(r"[<(]", s)[0][:30]

    for p in glob.glob(os.path.join(d, "*kernel_trace.csv")):
        for r in csv.DictReader(open(p)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), nm(r["Kernel_Name"])))
    for p in glob.glob(os.path.join(d, "*memory_copy_trace.csv")):
        for r in csv.DictReader(open(p)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy " + r["Direction"].split("_")[-3:][0]
                       + "->" + r["Direction"].split("_")[-1]))
    ev.sort()
    t0 = ev[0][0]
    marks = [e for e in ev if e[2].startswith(key)]
    lo, hi = marks[idx][0], marks[min(idx + cnt, len(marks) - 1)][0]
    busy_end = None
    for s, e, n in ev:
        if lo <= s <= hi:
            gap = (s - busy_end) / 1e3 if busy_end is not None and s > busy_end else 0.0
            print(f"{n:32s} start {(s - t0) / 1e6:10.3f} ms  dur {(e - s) / 1e3:9.1f} us  idle before {gap:7.1f} us")
            busy_end = e if busy_end is None else max(busy_end, e)
    print(f"period ({key} start to start): {(marks[idx + 1][0] - marks[idx][0]) / 1e6:.4f} ms")


if __name__ == "__main__":
    main()

"""The object report (pft_report): GPU time of one pft_report at 2 048 and 25 000 points in both
summation orders (HIP events on the handle's stream around each launch, median of --reps after --warmup), and the host
path it replaces (tools/report_host_bench.cpp: objectPosition + viz_cb's box steps on one CPU thread).

    python tools/report_bench.py [--reps 50] [--warmup 5] [--json out.json]   # device (needs the GPU)
    python tools/report_bench.py --host [--reps 50]                           # host path, CPU only
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (2048, 25000)


def host(reps):
    from pcl_tracking_amd import build

    lib = build.build()
    exe = os.path.join(build.OUT_DIR, "report_host_bench")
    src = os.path.join(ROOT, "tools", "report_host_bench.cpp")
    cmd = [build.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "pcl_tracking_amd", "include"), src, "-o", exe, "-L", os.path.dirname(lib), "-lpft_hip",
           "-Wl,-rpath," + os.path.dirname(lib)]
    subprocess.run(cmd, check=True)
    out = []
    for n in SIZES:
        r = subprocess.run([exe, str(n), str(reps)], capture_output=True, text=True, check=True)
        out.append(json.loads(r.stdout))
    return out


def device(reps, warmup):
    import torch

    torch.cuda.init()
    from pcl_tracking_amd import scene, tracker

    frame = scene.make_scene(50000)
    out = []
    for order in ("tree", "pcl"):
        for n in SIZES:
            stream = torch.cuda.Stream()
            t = tracker.make_reference_tracker(sum_order=order, stream=stream.cuda_stream)
            t.setReferenceCloud(scene.make_model(2048))
            t.setTrans(scene.initial_trans())
            t.setReportCloud(scene.make_model(n, seed=scene.MODEL_SEED + 1))
            t.setInputCloud(frame)
            t.compute()
            t.synchronize()
            ms = []
            for i in range(warmup + reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                t.computeReport()
                b.record(stream)
                b.synchronize()
                if i >= warmup:
                    ms.append(a.elapsed_time(b))
            rep = t.getReport()
            assert rep.info == 0 and rep.n_points == n
            out.append({"side": "device", "order": order, "points": n, "reps": reps,
                        "us_median": round(1000 * float(np.median(ms)), 2), "us_min": round(1000 * float(np.min(ms)), 2),
                        "us_max": round(1000 * float(np.max(ms)), 2)})
            t.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="time the host path instead (no GPU needed)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = host(a.reps) if a.host else device(a.reps, a.warmup)
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    if a.json:
        with open(a.json, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

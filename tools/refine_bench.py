#!/usr/bin/env python3
"""What a pose refinement (pft_refine) costs, beside a re-acquisition call with K = 8 on the same
frame -- the call whose result it polishes.

Call time (default): wall time of one synchronous call, `--calls` calls per repetition, median / min / max over `--reps`
repetitions, the two variants alternating inside every repetition, for
    refine         tracker.refine(start = the ground truth with its yaw off by 22.5 degrees), the defaults: at most 16
                   iterations, pairs within the tracker's 0.1 m
    reacquire      tracker.reacquire(centres = the object's position, n = (1, 1, 8), apply=False)
on the 50 000-point synthetic frame with models of M = 300, 2 048 and 8 192 points.

Kernel time: `--M N --only refine` under `rocprofv3 --kernel-trace --stats`, in a run of its own (the rows of k_refine_pairs
and k_refine_step are the figures; both also count the launches that return at once behind a loop that ended early):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/refine_bench.py --M 2048 --only refine --reps 1

    python tools/refine_bench.py [--M 300|2048|8192] [--only refine|reacquire] [--reps 7] [--calls 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (300, 2048, 8192)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, choices=SIZES, default=None, help="default: all three")
    ap.add_argument("--only", choices=("refine", "reacquire"), default=None, help="default: both")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from pcl_tracking_amd import _lib, scene, tracker

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/refine_bench.py: %d repetitions of %d calls, warm-up %d calls" % (a.reps, a.calls, a.warmup))
    emit("# device: %s; library: %s" % (torch.cuda.get_device_name(0), os.path.relpath(_lib.LIB_PATH, ROOT)))
    emit("# ms per synchronous call; median [min .. max] over the repetitions")
    cloud = scene.make_scene(50000)
    for M in ([a.M] if a.M else SIZES):
        model = scene.make_model(M)
        gtp = scene.model_gt_pose(M=M)
        off = list(gtp)
        off[5] += np.pi / 8.0
        start = scene.pose_matrix(*off).astype(np.float32)
        centre = np.array([gtp[:3]], np.float32)
        t = tracker.make_reference_tracker(particle_num=400, seed=21)
        t.setReferenceCloud(model)
        t.setTrans(scene.pose_matrix(*gtp).astype(np.float32))
        t.setInputCloud(cloud)
        last = {}

        def call_refine():
            last["refine"] = t.refine(start=start)

        def call_reacquire():
            last["reacquire"] = t.reacquire(centres=centre, n=(1, 1, 8), base_rpy=gtp[3:], apply=False)

        variants = [(n, f) for n, f in (("refine", call_refine), ("reacquire", call_reacquire)) if a.only in (None, n)]
        for _, fn in variants:
            for _ in range(a.warmup):
                fn()
        times = [[] for _ in variants]
        for _ in range(a.reps):  # the variants alternate inside every repetition
            for k, (_, fn) in enumerate(variants):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                times[k].append((time.perf_counter() - t0) * 1e3 / a.calls)
        for (name, _), v in zip(variants, times):
            emit("M %-5d %-10s %.4f [%.4f .. %.4f]" % (M, name, statistics.median(v), min(v), max(v)))
            r = last[name]
            if name == "refine":
                emit("#   frame %d points, crop %d points, %s after %d iterations, inliers %d -> %d of %d, improved %d" % (
                    len(cloud), r.n_crop, r.status_name, r.iterations, r.n_inliers_before, r.n_inliers_after, M, r.improved))
            else:
                emit("#   K %d, crop %d points, inliers %d, accepted %d" % (r.n_candidates, r.n_crop, r.n_inliers, r.accepted))
        t.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What a scene subtraction (pft_subtract_apply_device) adds to a frame.

Wall time of one apply from the enqueue to pft_subtract_counts (the host's wait included), the frame already in HBM, with
1 and with 4 bound trackers of 2 048 model points, on
    bench     the 50 000-point frame of scene.make_scene
    frontend  the 518 400-point input of the front end (scene.make_depth_frame(960, 540), invalid pixels included)
and beside it the per-frame wall time of the same trackers' compute() (enqueue to synchronize, all trackers in flight
together), on the 50 000-point frame.  Every figure is the median of `--reps` repetitions of `--calls` calls with min and
max.  Before every apply the trackers have computed a frame, as --discover runs it.

Kernel time: one shape and tracker count under `rocprofv3 --kernel-trace --stats`, in a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/subtract_bench.py --shape bench --trackers 4 --reps 1

    python tools/subtract_bench.py [--shape bench|frontend] [--trackers 1|4] [--reps 7] [--calls 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("bench", "frontend"), default=None, help="default: both")
    ap.add_argument("--trackers", type=int, choices=(1, 4), default=None, help="default: both")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from pcl_tracking_amd import _lib, scene, subtract, tracker

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def on_device(cloud):
        return torch.from_numpy(cloud.view(np.uint8).copy()).cuda()

    def stats(v):
        return "%.4f [%.4f .. %.4f]" % (statistics.median(v), min(v), max(v))

    emit("# tools/subtract_bench.py: %d repetitions of %d calls, warm-up %d calls, models of %d points, radius 0.02" % (
        a.reps, a.calls, a.warmup, M))
    emit("# device: %s; library: %s" % (torch.cuda.get_device_name(0), os.path.relpath(_lib.LIB_PATH, ROOT)))
    emit("# ms per call, wall time, enqueue to the host's wait; median [min .. max] over the repetitions")
    track_frame = scene.make_scene(50000)
    d_track = on_device(track_frame)
    frames = {"bench": track_frame, "frontend": scene.make_depth_frame(960, 540)}
    gtp = scene.model_gt_pose(M=M)
    for nt in ([a.trackers] if a.trackers else [1, 4]):
        ts = []
        for k in range(nt):
            t = tracker.make_reference_tracker(particle_num=400, seed=21 + k)
            t.setReferenceCloud(scene.make_model(M))
            T = scene.pose_matrix(*gtp).astype(np.float32)
            T[0, 3] += np.float32(0.002 * k)
            t.setTrans(T)
            ts.append(t)

        def compute_all():
            for t in ts:
                t.setInputCloudDevice(d_track.data_ptr(), len(track_frame), keepalive=d_track)
                t.compute()
            for t in ts:
                t.synchronize()

        for _ in range(a.warmup):
            compute_all()
        v = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                compute_all()
            v.append((time.perf_counter() - t0) * 1e3 / a.calls)
        emit("%-9s %d tracker(s)  compute    %s" % ("bench", nt, stats(v)))
        for shape in ([a.shape] if a.shape else ["bench", "frontend"]):
            frame = frames[shape]
            d_frame = on_device(frame)
            sub = subtract.SceneSubtraction()
            for k, t in enumerate(ts):
                sub.bindTracker(k, t)

            def apply_once():
                sub.applyDevice(d_frame.data_ptr(), len(frame), keepalive=d_frame)
                return sub.counts()

            for _ in range(a.warmup):
                apply_once()
            v, gpu_ms = [], []
            for _ in range(a.reps):
                el = 0.0
                for _ in range(a.calls):
                    compute_all()  # (not timed: the pose the apply takes is a fresh one, as in the driver)
                    t0 = time.perf_counter()
                    counts = apply_once()
                    el += time.perf_counter() - t0
                    gpu_ms.append(sub.lastMilliseconds())
                v.append(el * 1e3 / a.calls)
            emit("%-9s %d tracker(s)  subtract   %s" % (shape, nt, stats(v)))
            emit("#   frame %d points, explained %d, residual %d, support %s; on the stream %s ms" % (
                counts[0], counts[1], counts[2], list(sub.support()[:nt]), stats(gpu_ms)))
            sub.close()
        for t in ts:
            t.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

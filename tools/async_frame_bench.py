#!/usr/bin/env python3
"""Wall time per frame from "frame resident in HBM" to "all poses on the host": the synchronous call sequence
(filterDevice, setInputCloudDevice, compute, getResult) against the asynchronous one (filterAsync,
setInputCloudFromFilter, compute, getResult) in one process.

Workload: the reference's operating point -- the qhd sensor frame (960 x 540 = 518 400 points), PassThrough +
ApproximateVoxelGrid, 1 and 4 objects at 400 particles and with the KLD-adaptive tracker, and one run at 8 192
particles.  Every variant has its own filter and trackers (same seeds); after a warm-up the variants alternate,
each repetition timing `--frames` frames, and the median / min / max over `--reps` repetitions is printed.  The
asynchronous path runs twice: with max_points = 0 (grids sized by the frame's 518 400 input points) and with
max_points = 2 x the frame's real output.

    python tools/async_frame_bench.py [--reps 7] [--frames 200] [--warmup 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 7 or a.frames < 200:
        print("note: fewer than 7 repetitions of 200 frames: not a figure to quote", file=sys.stderr)

    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from pcl_tracking_amd import filters, scene, tracker

    frame = scene.make_depth_frame(a.width, a.height)
    model = scene.make_model(2048)
    d_frame = torch.from_numpy(frame.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/async_frame_bench.py: %d x %d frame (%d points), model %d points, %d repetitions of %d frames, "
         "warm-up %d frames" % (a.width, a.height, len(frame), len(model), a.reps, a.frames, a.warmup))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    emit("# ms per frame, frame resident in HBM -> all poses on the host; median [min .. max] over the repetitions")

    def make_set(n_obj, particles, kld):
        f = filters.make_reference_input_filter()
        f.setInputCloudDevice(d_frame.data_ptr(), len(frame), keepalive=d_frame)
        objs = []
        for o in range(n_obj):
            t = tracker.make_reference_tracker(particle_num=particles, seed=21 + o, kld=kld)
            t.setReferenceCloud(model)
            t.setTrans(scene.initial_trans())
            objs.append(t)
        return f, objs

    def frame_sync(f, objs, _mp):
        p, n = f.filterDevice()
        for t in objs:
            t.setInputCloudDevice(p, n, keepalive=f)
            t.compute()
        for t in objs:
            t.getResult()

    def frame_async(f, objs, mp):
        f.filterAsync()
        for t in objs:
            t.setInputCloudFromFilter(f, mp)
            t.compute()
        for t in objs:
            t.getResult()

    probe = filters.make_reference_input_filter()
    probe.setInputCloudDevice(d_frame.data_ptr(), len(frame), keepalive=d_frame)
    probe.filterDevice()
    probe.filterDevice()  # (the first run of a process pays the kernels' loading)
    n_pass, n_out = probe.counts()
    emit("# front end: %d -> %d (PassThrough) -> %d points, %.3f ms on the device" % (len(frame), n_pass, n_out,
                                                                                   probe.lastMilliseconds()))

    for n_obj, particles, kld in ((1, 400, False), (4, 400, False), (1, 400, True), (4, 400, True), (1, 8192, False)):
        variants = [("sync", frame_sync, 0), ("async max_points=0", frame_async, 0),
                    ("async max_points=2*out", frame_async, 2 * n_out)]
        sets = [make_set(n_obj, particles, kld) for _ in variants]
        for (name, fn, mp), (f, objs) in zip(variants, sets):
            for _ in range(a.warmup):
                fn(f, objs, mp)
        times = [[] for _ in variants]
        for _ in range(a.reps):
            for k, ((name, fn, mp), (f, objs)) in enumerate(zip(variants, sets)):
                t0 = time.perf_counter()
                for _ in range(a.frames):
                    fn(f, objs, mp)
                times[k].append((time.perf_counter() - t0) * 1e3 / a.frames)
        label = "%d object%s, %s" % (n_obj, "s" if n_obj > 1 else "", "KLD (<= 500 particles)" if kld else
                                     "%d particles" % particles)
        base = statistics.median(times[0])
        for (name, _, _), ts in zip(variants, times):
            med = statistics.median(ts)
            emit("%-34s %-24s %.4f [%.4f .. %.4f]  %+.1f %% vs sync" % (label, name, med, min(ts), max(ts),
                                                                     100.0 * (med - base) / base))
        for f, objs in sets:
            for t in objs:
                t.close()
            f.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

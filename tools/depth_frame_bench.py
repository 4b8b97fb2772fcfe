#!/usr/bin/env python3
"""Wall time per frame from "frame in HOST memory" to "all poses on the host": what crosses the bus is either the
organised cloud of 32-byte records (the entrance every earlier number starts behind) or the depth + colour images the
sensor delivers, with the cloud formed on the device (InputFilter.setInputDepth, k_depth_deproject).

Variants, each with its own filter and trackers (same seeds), alternating in one process after a warm-up:
  (a) records, pageable   pft_filter_apply_async on the W x H x 32 B cloud in pageable memory: the baseline
  (b) records, pinned     the same from pinned (hipHostMalloc) memory
  (c) images, pageable    depth u16 + BGR8 from pageable memory
  (d) images, slots       depth u16 + BGR8 from the handle's two pinned slots, alternating
The frame behind the entrance is the same in all four: the records of (a) / (b) are the specification's cloud of the
images of (c) / (d).  The host buffers are filled once; no variant pays for producing its frame.

    python tools/depth_frame_bench.py [--reps 7] [--frames 200] [--warmup 20] [--out FILE]
    python tools/depth_frame_bench.py --kernel-only 50      # depth applies alone, for rocprofv3 --kernel-trace --stats
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--kernel-only", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not a.kernel_only and (a.reps < 7 or a.frames < 200):
        print("note: fewer than 7 repetitions of 200 frames: not a figure to quote", file=sys.stderr)

    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    import depth_model
    from pcl_tracking_amd import filters, scene, tracker

    depth, bgr, camera = scene.make_depth_images(a.width, a.height)
    records = depth_model.deproject(depth, bgr, camera)
    model = scene.make_model(2048)
    pinned = torch.empty(records.nbytes, dtype=torch.uint8, pin_memory=True)
    records_pinned = pinned.numpy().view(records.dtype)
    records_pinned[:] = records

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if a.kernel_only:
        f = filters.make_reference_input_filter()
        f.setInputDepth(depth, bgr, camera)
        for _ in range(a.kernel_only):
            f.filter()
        print("kernel-only: %d depth applies, %d -> %d points" % ((a.kernel_only, len(records)) + f.counts()[1:]))
        return

    emit("# tools/depth_frame_bench.py: %d x %d frame, model %d points, %d repetitions of %d frames, warm-up %d frames"
         % (a.width, a.height, len(model), a.reps, a.frames, a.warmup))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    emit("# bytes over the bus per frame: records %d (32 B per pixel), images %d (2 + 3 B per pixel): %.1f times less"
         % (records.nbytes, depth.nbytes + bgr.nbytes, records.nbytes / (depth.nbytes + bgr.nbytes)))
    emit("# ms per frame, frame in host memory -> all poses on the host; median [min .. max] over the repetitions")

    def make_set(kind, n_obj, particles, kld):
        f = filters.make_reference_input_filter()
        state = {"k": 0}
        if kind == "records_pageable":
            f.setInputCloud(records)
        elif kind == "records_pinned":
            f.setInputCloud(records_pinned)
            assert f._cloud.ctypes.data == records_pinned.ctypes.data  # the pinned bytes themselves, no copy
        elif kind == "images_pageable":
            f.setInputDepth(depth, bgr, camera)
        else:
            state["slots"] = []
            for s in range(2):
                d, c = f.depthHostBuffers(s, depth.shape, depth.dtype, "bgr8")
                d[...] = depth
                c[...] = bgr
                state["slots"].append((d, c))
        objs = []
        for o in range(n_obj):
            t = tracker.make_reference_tracker(particle_num=particles, seed=21 + o, kld=kld)
            t.setReferenceCloud(model)
            t.setTrans(scene.initial_trans())
            objs.append(t)
        return f, objs, state

    def one_frame(f, objs, state):
        if "slots" in state:
            s = state["k"] & 1
            state["k"] += 1
            f.depthSlotDone(s, wait=True)  # where the producer of the next frame would wait before it writes
            f.setInputDepth(state["slots"][s][0], state["slots"][s][1], camera)
        f.filterAsync()
        for t in objs:
            t.setInputCloudFromFilter(f)
            t.compute()
        for t in objs:
            t.getResult()

    kinds = [("(a) records, pageable", "records_pageable"), ("(b) records, pinned", "records_pinned"),
             ("(c) images, pageable", "images_pageable"), ("(d) images, pinned slots", "images_slots")]
    for n_obj, particles, kld in ((1, 400, False), (4, 400, False), (1, 400, True), (4, 400, True)):
        sets = [make_set(kind, n_obj, particles, kld) for _, kind in kinds]
        results = []
        for f, objs, state in sets:
            for _ in range(a.warmup):
                one_frame(f, objs, state)
            results.append((f.counts(), [t.getResult().tobytes() for t in objs]))
        assert all(r[0] == results[0][0] for r in results), "the four entrances disagree on the front end's counts"
        times = [[] for _ in kinds]
        for _ in range(a.reps):
            for k, (f, objs, state) in enumerate(sets):
                t0 = time.perf_counter()
                for _ in range(a.frames):
                    one_frame(f, objs, state)
                times[k].append((time.perf_counter() - t0) * 1e3 / a.frames)
        label = "%d object%s, %s" % (n_obj, "s" if n_obj > 1 else "", "KLD (<= 500 particles)" if kld else
                                     "%d particles" % particles)
        base = statistics.median(times[0])
        emit("%s: front end %d -> %d points; spread of (a): %.4f ms" % ((label,) + results[0][0] + (max(times[0]) - min(times[0]),)))
        for (name, _), ts in zip(kinds, times):
            med = statistics.median(ts)
            emit("  %-26s %.4f [%.4f .. %.4f]  %+.4f ms (%+.1f %%) vs (a)" % (name, med, min(ts), max(ts), med - base,
                                                                           100.0 * (med - base) / base))
        for f, objs, _ in sets:
            for t in objs:
                t.close()
            f.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

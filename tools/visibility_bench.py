#!/usr/bin/env python3
"""What the visibility (pft_visibility) costs.

Frame time (default): wall time per frame of `compute(); getResult()` against `compute(); computeMatch(); getResult();
getMatch()` and `compute(); computeMatch(); computeVisibility(); getResult(); getVisibility()` -- trackers with the same
seed alternating in one process, each repetition timing `--frames` frames; the median / min / max over `--reps`
repetitions is printed (the method of tools/match_bench.py).  Workloads: the reference's operating point (2 048-point
model, 50 000-point cloud, 400 particles) and BASELINE configs[1] (8 192 particles).

Kernel time: `--shape NAME` runs `--frames` frames with computeVisibility() on one workload and nothing else, to be
started under `rocprofv3 --kernel-trace --stats` in a run of its own per shape (the k_vis_* rows are the figures):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/visibility_bench.py --shape voxel50k --frames 200

shapes: voxel50k (M = 2 048, the 50 000-point voxel frame), organised (M = 2 048, the 518 400-point organised frame).

    python tools/visibility_bench.py [--reps 7] [--frames 200] [--warmup 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("voxel50k", "organised")
WORKLOADS = [("400 particles", 2048, 400), ("configs[1]: 8192 particles", 2048, 8192)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shape", choices=SHAPES, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from pcl_tracking_amd import scene, tracker

    def make(M, particles, cloud):
        t = tracker.make_reference_tracker(particle_num=particles, seed=21)
        t.setReferenceCloud(scene.make_model(M))
        t.setTrans(scene.initial_trans())
        t.setInputCloud(cloud)
        return t

    def frame_plain(t):
        t.compute()
        t.getResult()

    def frame_match(t):
        t.compute()
        t.computeMatch()
        t.getResult()
        return t.getMatch()

    def frame_visibility(t):
        t.compute()
        t.computeMatch()
        t.computeVisibility()
        t.getResult()
        return t.getVisibility()

    if a.shape:
        cloud = scene.make_scene(50000) if a.shape == "voxel50k" else scene.make_depth_frame(960, 540)
        t = make(2048, 400, cloud)
        for _ in range(a.warmup + a.frames):
            st = frame_visibility(t)
        print("shape %s: M 2048, %d frame points, visible %d occluded %d self %d out %d, %d frames with computeVisibility()" % (
            a.shape, st.n_frame, st.n_visible, st.n_occluded, st.n_self, st.n_out, a.warmup + a.frames), flush=True)
        t.close()
        return

    if a.reps < 7 or a.frames < 200:
        print("note: fewer than 7 repetitions of 200 frames: not a figure to quote", file=sys.stderr)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    cloud = scene.make_scene(50000)
    emit("# tools/visibility_bench.py: 50 000-point cloud, %d repetitions of %d frames, warm-up %d frames" % (
        a.reps, a.frames, a.warmup))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    emit("# ms per frame, compute() -> result (and statistics) on the host; median [min .. max] over the repetitions")
    for label, M, particles in WORKLOADS:
        variants = [("compute", frame_plain), ("compute + match", frame_match),
                    ("compute + match + visibility", frame_visibility)]
        ts = [make(M, particles, cloud) for _ in variants]
        for (_, fn), t in zip(variants, ts):
            for _ in range(a.warmup):
                fn(t)
        times = [[] for _ in variants]
        for _ in range(a.reps):
            for k, ((_, fn), t) in enumerate(zip(variants, ts)):
                t0 = time.perf_counter()
                for _ in range(a.frames):
                    fn(t)
                times[k].append((time.perf_counter() - t0) * 1e3 / a.frames)
        base = statistics.median(times[0])
        st = ts[2].getVisibility()
        for (name, _), v in zip(variants, times):
            med = statistics.median(v)
            emit("%-28s %-30s %.4f [%.4f .. %.4f]  %+.1f %% (%+.1f us)" % (label, name, med, min(v), max(v),
                                                                          100.0 * (med - base) / base, 1e3 * (med - base)))
        emit("#   M %d, visible %d occluded %d self %d out %d, visible and matched %d" % (
            M, st.n_visible, st.n_occluded, st.n_self, st.n_out, st.n_visible_matched))
        for t in ts:
            t.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

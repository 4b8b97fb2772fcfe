#!/usr/bin/env python3
"""What the match statistics (pft_match) cost.

Frame time (default): wall time per frame of `compute(); getResult()` against `compute(); computeMatch(); getResult();
getMatch()` -- two trackers with the same seed alternating in one process, each repetition timing `--frames` frames; the
median / min / max over `--reps` repetitions is printed (the method of tools/async_frame_bench.py).  Workloads: BASELINE
configs[1] (2 048-point model, 50 000-point cloud, 8 192 particles), the reference's operating point (400 particles) and its
KLD-adaptive tracker.

Kernel time: `--shape NAME` runs `--frames` frames with computeMatch() on one workload and nothing else, to be started
under `rocprofv3 --kernel-trace --stats` in a run of its own per shape (k_match's row of the statistics is the figure):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/match_bench.py --shape configs1 --frames 200

shapes: configs1 (M = 2 048, 8 192 particles), p400 (M = 2 048, 400 particles), m8192 (M = 8 192, 8 192 particles).

    python tools/match_bench.py [--reps 7] [--frames 200] [--warmup 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"configs1": (2048, 8192, False), "p400": (2048, 400, False), "m8192": (8192, 8192, False)}
WORKLOADS = [("configs[1]: 8192 particles", 2048, 8192, False), ("400 particles", 2048, 400, False),
             ("KLD (<= 500 particles)", 2048, 400, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from pcl_tracking_amd import scene, tracker

    cloud = scene.make_scene(50000)

    def make(M, particles, kld):
        t = tracker.make_reference_tracker(particle_num=particles, seed=21, kld=kld)
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

    if a.shape:
        M, particles, kld = SHAPES[a.shape]
        t = make(M, particles, kld)
        for _ in range(a.warmup + a.frames):
            st = frame_match(t)
        print("shape %s: M %d, %d particles, crop %d points, matched %d, %d frames with computeMatch()" % (
            a.shape, M, particles, st.n_crop, st.n_matched, a.warmup + a.frames), flush=True)
        t.close()
        return

    if a.reps < 7 or a.frames < 200:
        print("note: fewer than 7 repetitions of 200 frames: not a figure to quote", file=sys.stderr)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/match_bench.py: 50 000-point cloud, %d repetitions of %d frames, warm-up %d frames" % (a.reps, a.frames,
                                                                                                      a.warmup))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    emit("# ms per frame, compute() -> result (and match) on the host; median [min .. max] over the repetitions")
    for label, M, particles, kld in WORKLOADS:
        variants = [("compute", frame_plain), ("compute + computeMatch", frame_match)]
        ts = [make(M, particles, kld) for _ in variants]
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
        st = ts[1].getMatch()
        for (name, _), v in zip(variants, times):
            med = statistics.median(v)
            emit("%-28s %-24s %.4f [%.4f .. %.4f]  %+.1f %% (%+.1f us)" % (label, name, med, min(v), max(v),
                                                                          100.0 * (med - base) / base, 1e3 * (med - base)))
        emit("#   M %d, crop %d points, matched %d" % (M, st.n_crop, st.n_matched))
        for t in ts:
            t.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

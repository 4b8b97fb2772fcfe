#!/usr/bin/env python3
"""What a re-acquisition call (pft_reacquire) costs, against the only way to score candidate poses
that existed before it: the test hook pft_eval_weights on the same candidates, on a handle created with particle_num >= K.

Call time (default): wall time of one synchronous call, `--calls` calls per repetition, median / min / max over `--reps`
repetitions, for
    reacquire      tracker.reacquire(centres, n = (1, 1, n_yaw), apply=False) on a handle of 400 particles
    eval_weights   pft_eval_weights(candidates, K, raw_w) on a handle of max(K, 400) particles; the candidates are the same
                   lattice, formed on the host
`--only eval_weights` runs the yardstick alone: it needs nothing of this feature, so PFT_LIB_PATH may point at the library of
an earlier commit.

shapes: bench (M = 2 048, the 50 000-point synthetic frame), reference (M = 500, the synthetic 960 x 540 sensor frame through
the reference's front end: PassThrough z + ApproximateVoxelGrid 0.01).  8 centres -- the object's position and 7 points
of the frame -- x 36 yaw steps over the full circle: K = 288.

Kernel time: `--shape NAME --only reacquire` under `rocprofv3 --kernel-trace --stats`, in a run of its own
(k_reacquire_score's row of the statistics is the figure):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/reacquire_bench.py --shape bench --only reacquire --reps 1

    python tools/reacquire_bench.py [--shape bench|reference] [--only reacquire|eval_weights] [--reps 7] [--calls 50] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CENTRES, N_YAW = 8, 36


def lattice(centres, base_rpy, n_yaw, dtype):
    """the candidates of pft_reacquire for n = (1, 1, n_yaw), span (0, 0, 2 pi), formed on the host"""
    i = np.arange(n_yaw, dtype=np.float64)
    yaw = (np.float64(np.float32(base_rpy[2])) + np.float64(np.float32(2.0 * np.pi)) * ((i + 0.5) / n_yaw - 0.5)).astype(np.float32)
    out = np.zeros(len(centres) * n_yaw, dtype)
    for c, cen in enumerate(centres):
        for k in range(n_yaw):
            out[c * n_yaw + k] = (cen[0], cen[1], cen[2], 1.0, base_rpy[0], base_rpy[1], yaw[k], 0.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("bench", "reference"), default=None, help="default: both")
    ap.add_argument("--only", choices=("reacquire", "eval_weights"), default=None, help="default: both")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from pcl_tracking_amd import _lib, filters, scene, tracker

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def frame_of(shape):
        if shape == "bench":
            return 2048, scene.make_scene(50000)
        f = filters.make_reference_input_filter()
        f.setInputCloud(scene.make_depth_frame(960, 540))
        return 500, f.filter()

    emit("# tools/reacquire_bench.py: %d centres x %d yaw steps, %d repetitions of %d calls, warm-up %d calls" % (
        N_CENTRES, N_YAW, a.reps, a.calls, a.warmup))
    emit("# device: %s; library: %s" % (torch.cuda.get_device_name(0), os.path.relpath(_lib.LIB_PATH, ROOT)))
    emit("# ms per synchronous call; median [min .. max] over the repetitions")
    for shape in ([a.shape] if a.shape else ["bench", "reference"]):
        M, cloud = frame_of(shape)
        model = scene.make_model(M)
        gtp = scene.model_gt_pose(M=M)
        xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
        pick = np.random.default_rng(5).choice(len(cloud), N_CENTRES - 1, replace=False)
        centres = np.concatenate([np.array([gtp[:3]], np.float32), xyz[pick]]).astype(np.float32)
        K = N_CENTRES * N_YAW
        variants = []
        if a.only in (None, "reacquire"):
            t = tracker.make_reference_tracker(particle_num=400, seed=21)
            t.setReferenceCloud(model)
            t.setTrans(scene.pose_matrix(*gtp).astype(np.float32))
            t.setInputCloud(cloud)
            last = {}

            def call_new(t=t, last=last):
                last["res"] = t.reacquire(centres=centres, n=(1, 1, N_YAW), base_rpy=gtp[3:], apply=False)

            variants.append(("reacquire", call_new, t, last))
        if a.only in (None, "eval_weights"):
            e = tracker.make_reference_tracker(particle_num=max(K, 400), seed=21)
            e.setReferenceCloud(model)
            e.setTrans(scene.pose_matrix(*gtp).astype(np.float32))
            e.setInputCloud(cloud)
            cand = lattice(centres, gtp[3:], N_YAW, scene.PARTICLE_DTYPE)
            raw = np.zeros(K, np.float32)

            def call_old(e=e):
                e._check(e._L.pft_eval_weights(e._h, cand.ctypes.data_as(C.c_void_p), K, raw.ctypes.data_as(C.c_void_p), None, None))

            variants.append(("eval_weights", call_old, e, None))
        for _, fn, _, _ in variants:
            for _ in range(a.warmup):
                fn()
        times = [[] for _ in variants]
        for _ in range(a.reps):  # the variants alternate inside every repetition
            for k, (_, fn, _, _) in enumerate(variants):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                times[k].append((time.perf_counter() - t0) * 1e3 / a.calls)
        for (name, _, t, last), v in zip(variants, times):
            emit("%-10s %-13s %.4f [%.4f .. %.4f]" % (shape, name, statistics.median(v), min(v), max(v)))
            if last:
                r = last["res"]
                emit("#   M %d, frame %d points, K %d, crop %d points, best centre %d, inliers %d, accepted %d" % (
                    M, len(cloud), r.n_candidates, r.n_crop, r.best_centre, r.n_inliers, r.accepted))
            t.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

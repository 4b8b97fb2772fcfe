#!/usr/bin/env python3
"""What the view-dependent reference (pft_view_select / pft_set_reference_from_view) costs.

Per model size (random points on the surface of the scene's box at the ground-truth pose, in HBM):
  select          GPU time of one selectView() of the device cloud, events on the tracker's stream, median of --reps
  set reference   wall time of setReferenceFromView() behind it (the view cloud crosses to the host: Morton order, hull)
  new route       wall time of selectView() + setReferenceFromView()
  old route       wall time of what a caller did for the same reference cloud before: setReferenceCloud(full model),
                  computeVisibility(T), getVisibilityPoints(), a host compaction of the points that are neither
                  self-occluded nor out of view, setReferenceCloud(subset)
Both routes end with the same records as the reference cloud (checked).

    python tools/view_reference_bench.py [--reps 7] [--sizes 4096,65536,1048576] [--out FILE]
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
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from pcl_tracking_amd import scene, tracker

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def surface(n, rng):
        """n random points on the six faces of the scene's box, object frame"""
        h = np.asarray(scene.MODEL_DIMS) / 2
        p = rng.uniform(-1, 1, (n, 3)) * h
        area = np.array([h[1] * h[2], h[0] * h[2], h[0] * h[1]])
        axis = rng.choice(3, n, p=area / area.sum())
        p[np.arange(n), axis] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * h[axis]
        return scene.make_points(p.astype(np.float32), rng.integers(0, 255, (n, 3)))

    T = scene.pose_matrix(*scene.GT_POSE)[:3].astype(np.float32)
    stream = torch.cuda.Stream()
    far = scene.make_points(np.array([[0, 0, 9.0]], np.float32), np.full((1, 3), 128))
    emit("# tools/view_reference_bench.py: %d repetitions, the default 160 x 90 camera, 64 particles" % a.reps)
    emit("# device: %s" % torch.cuda.get_device_name(0))
    emit("# %9s %9s %9s | %12s %16s %14s | %14s" % ("model", "visible", "kept", "select (ms)", "set ref (ms)", "new route (ms)", "old route (ms)"))
    for n in (int(s) for s in a.sizes.split(",")):
        model = surface(n, np.random.default_rng(n))
        dev = torch.from_numpy(np.frombuffer(model.tobytes(), np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        t = tracker.make_reference_tracker(particle_num=64, seed=1, stream=stream.cuda_stream)
        src = (dev.data_ptr(), n)
        for _ in range(2):  # warm-up: the buffers grow here
            t.selectView(src, T)
            t.setReferenceFromView()
        ev, ref_ms, new_ms = [], [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t.selectView(src, T)
            e1.record(stream)
            t0 = time.perf_counter()
            t.setReferenceFromView()
            ref_ms.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            t.selectView(src, T)
            t.setReferenceFromView()
            new_ms.append((time.perf_counter() - t0) * 1e3)
        st = t.getView()
        new_cloud = t.getViewCloud()
        old_ms = []
        o = tracker.make_reference_tracker(particle_num=64, seed=1)
        o.setInputCloud(far)
        for _ in range(min(a.reps, 3) + 1):  # (the first is the warm-up)
            t0 = time.perf_counter()
            o.setReferenceCloud(model)
            o.computeVisibility(T)
            state = o.getVisibilityPoints()[0]
            subset = model[(state == 0) | (state == 1)]  # visible, or occluded by the scene only
            o.setReferenceCloud(subset)
            old_ms.append((time.perf_counter() - t0) * 1e3)
        assert subset.tobytes() == new_cloud.tobytes(), "the two routes disagree"
        med = statistics.median
        emit("  %9d %9d %9d | %12.4f %16.3f %14.3f | %14.3f" % (n, st.n_visible, st.n_kept, med(ev), med(ref_ms), med(new_ms), med(old_ms[1:])))
        t.close()
        o.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""GPU time of one model-growth apply (pft_grow_last_ms) beside the scene subtraction that feeds it (pft_subtract_last_ms),
on the 50 000-point synthetic frame: the residual behind one and behind four subtracted objects, and the whole frame.

    python tools/grow_bench.py [--repeat 20]

Every figure is the median of `repeat` consecutive applies on one handle in the default configuration (the model grows
while they run, as it does in use).  The text under profiles/grow.txt is this tool's output."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pcl_tracking_amd import grow, scene, subtract  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    a = ap.parse_args()
    frame = scene.make_scene(50000)
    model = scene.make_model()
    T = scene.pose_matrix(*scene.model_gt_pose())[:3].astype(np.float32)
    shifts = [(0.0, 0.0, 0.0), (-0.5, 0.1, 0.3), (0.45, 0.15, 0.2), (0.0, 0.3, 0.5)]  # the same model set down elsewhere
    for n_obj in (1, 4):
        sub = subtract.SceneSubtraction()
        for k in range(n_obj):
            Tk = T.copy()
            Tk[:, 3] += np.array(shifts[k], np.float32)
            sub.setObject(k, model, Tk)
        g = grow.ModelGrowth()
        g.setModel(model)
        sub_ms, grow_ms = [], []
        for _ in range(a.repeat):
            sub.apply(frame)
            sub_ms.append(sub.lastMilliseconds())
            g.applyResidual(sub, T)
            grow_ms.append(g.lastMilliseconds())
        n_in, _, n_res = sub.counts()
        s = g.stats()
        print("objects %d: frame %d residual %d  subtract %.3f ms  grow on the residual %.3f ms  (model %d -> %d points)" % (
            n_obj, n_in, n_res, statistics.median(sub_ms), statistics.median(grow_ms), len(model), s["n_model_points"]))
    g = grow.ModelGrowth()
    g.setModel(model)
    whole = []
    for _ in range(a.repeat):
        g.apply(frame, T)
        whole.append(g.lastMilliseconds())
    print("whole frame %d: grow %.3f ms  (model %d -> %d points; the time includes the frame's upload)" % (
        len(frame), statistics.median(whole), len(model), g.stats()["n_model_points"]))


if __name__ == "__main__":
    main()

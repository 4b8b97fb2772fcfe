"""Model creation on the device (include/pft_segment.h): median GPU time of apply_device on the qhd frame
(scene.make_depth_frame(), 960 x 540 = 518 400 points), the per-stage split, hypotheses and iterations, clusters.

    python tools/segment_bench.py [--reps 20] [--warmup 3] [--no-plane] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-plane", action="store_true")
    ap.add_argument("--box", default="-0.4,0.6,-0.45,0.35,0.4,1.4", help="xmin,xmax,ymin,ymax,zmin,zmax or 'off'")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch

    torch.cuda.init()
    from pcl_tracking_amd import _lib, scene, segment

    cloud = scene.make_depth_frame()
    dev = torch.from_numpy(cloud.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    s = segment.ModelSegmenter()
    if a.box == "off":
        s.configure(plane=not a.no_plane, box_enable=(0, 0, 0))
    else:
        s.configure(plane=not a.no_plane, box=[float(v) for v in a.box.split(",")], box_enable=(1, 1, 1))
    s.setInputCloudDevice(dev.data_ptr(), len(cloud), dev)
    tot, stages = [], {k: [] for k in _lib.SEGMENT_STAGES}
    for i in range(a.warmup + a.reps):
        s.apply()
        ms, st = s.lastMilliseconds()
        if i >= a.warmup:
            tot.append(ms)
            for k, v in st.items():
                stages[k].append(v)
    pl = s.plane()
    out = {
        "points": len(cloud), "plane": not a.no_plane, "box": a.box, "reps": a.reps,
        "ms_median": float(np.median(tot)), "ms_min": float(np.min(tot)), "ms_max": float(np.max(tot)),
        "stage_ms_median": {k: round(float(np.median(v)), 4) for k, v in stages.items()},
        "n_valid": pl["n_valid"], "hypotheses_scored": pl["hypotheses_scored"], "iterations": pl["iterations"],
        "plane_inliers": pl["inliers"], "survivors": pl["n_survivors"], "clusters": [int(v) for v in s.clusterSizes()],
    }
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

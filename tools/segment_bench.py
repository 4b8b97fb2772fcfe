"""Model creation on the device (include/pft_segment.h): median GPU time of apply_device on the qhd frame
(scene.make_depth_frame(), 960 x 540 = 518 400 points), the per-stage split, hypotheses and iterations, clusters.

    python tools/segment_bench.py [--reps 20] [--warmup 3] [--no-plane] [--json out.json]
                                  [--planes MAX,FRACTION] [--sac ITER,THRESHOLD] [--refit-order pcl|tree]

--planes runs the plane rounds (cluster_euclid.cpp:59-85); the host reads the header once for the cloud size and once
per round, on top of the reads of the single-plane pipeline (`host_reads_rounds` in the output).
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
    ap.add_argument("--planes", default=None, help="MAX,FRACTION: plane rounds")
    ap.add_argument("--sac", default=None, help="ITER,THRESHOLD")
    ap.add_argument("--refit-order", default="pcl", choices=["pcl", "tree"])
    ap.add_argument("--max-size", type=int, default=None)
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
    if a.planes:
        mx, fr = a.planes.split(",")
        s.configure(plane_rounds=(int(mx), float(fr)))
    if a.sac:
        it, thr = a.sac.split(",")
        s.configure(max_iterations=int(it), distance_threshold=float(thr))
    if a.max_size is not None:
        s.configure(max_size=a.max_size)
    s.configure(refit_order=a.refit_order)
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
    out["refit_order"] = a.refit_order
    if a.planes:
        rounds = [s.plane(k) for k in range(max(s.planeCount(), 1))]
        out.update(planes=s.planeCount(), stopped_by=s.stoppedBy(), round_inliers=[p["inliers"] for p in rounds],
                   round_iterations=[p["iterations"] for p in rounds], round_ransac_inliers=[p["ransac_inliers"] for p in rounds])
        ran = s.planeCount() + (1 if s.stoppedBy() == _lib.ROUNDS_STOP_NO_PLANE else 0)
        out["host_reads_rounds"] = 1 + ran
    else:
        out["ransac_inliers"] = pl["ransac_inliers"]
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Frame time with PCL's change detector off and on, on a moving and on a static scene (one handle, host timer around
compute() + synchronize, the input already in HBM).

  python tools/change_detector_bench.py [--frames 200] [--warmup 20] [--out profiles/change_detector_frames.json]

Configurations: configs[1] (8 192 fixed particles, 2 048-point model, 50 000-point cloud), the reference's 400 fixed
particles and its KLD tracker.  Detector on, interval 0 (a test every iteration): on the static scene 5 points at 0.05 m,
where every iteration after the first tests skips (what is left of a skipped iteration); on the moving scene 1 point at
0.01 m, where nearly every test finds a change (the detector's cost on top of a full iteration; the loop of eight frames jumps back
to the first, and the column skipped_of_last_32_iterations says how many tests found none)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="", help="the build's commit, recorded in --out (default: git rev-parse HEAD)")
    args = ap.parse_args()
    import torch

    from pcl_tracking_amd import scene, tracker

    torch.zeros(1, device="cuda")  # torch initialises HIP first
    moving = [scene.make_scene(50000, obj_pose=scene.advance_pose(scene.GT_POSE, f)) for f in range(8)]
    dev = [torch.from_numpy(c.view(np.uint8).copy()).cuda() for c in moving]
    model = scene.make_model(2048)
    rows = []
    for name, P, kld in (("configs[1] 8192 fixed", 8192, False), ("400 fixed", 400, False), ("400 KLD", 400, True)):
        for scn in ("moving", "static"):
            for cd in (None, (0, 5, 0.05) if scn == "static" else (0, 1, 0.01)):
                t = tracker.make_reference_tracker(particle_num=P, seed=1, kld=kld, change_detector=cd)
                t.setReferenceCloud(model)
                t.setTrans(scene.initial_trans())
                times = []
                for f in range(args.warmup + args.frames):
                    c = dev[f % len(dev)] if scn == "moving" else dev[0]
                    t.setInputCloudDevice(c.data_ptr(), len(moving[0]), keepalive=c)
                    t.synchronize()
                    t0 = time.perf_counter()
                    t.compute()
                    t.synchronize()
                    if f >= args.warmup:
                        times.append((time.perf_counter() - t0) * 1e6)
                ring = t.debugChangeState()["ring"] if cd else None
                skipped = int((ring[:, 0] == 1).sum() - ring[:, 1].sum()) if cd else 0
                row = dict(config=name, scene=scn, detector="on %s" % (cd,) if cd else "off",
                           median_us=float(np.median(times)), p10_us=float(np.percentile(times, 10)),
                           p90_us=float(np.percentile(times, 90)), frames=args.frames,
                           skipped_of_last_32_iterations=skipped if cd else None)
                rows.append(row)
                print(json.dumps(row), flush=True)
                t.close()
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(commit=commit or "unknown", rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()

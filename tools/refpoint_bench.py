"""The reference's own operating point (auto_tracking.cpp:201-254): 400 fixed particles / KLD-adaptive <= 500, same model
and cloud as bench.py; prints per-stage event timings.
Usage: python tools/refpoint_bench.py [fixed|kld] [frames] [--sum-order tree|pcl] [--particles N]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcl_tracking_amd import scene, tracker  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("mode", nargs="?", default="kld", choices=("fixed", "kld"))
ap.add_argument("frames", nargs="?", type=int, default=300)
ap.add_argument("--sum-order", default="tree", choices=("tree", "pcl"),
                help="order of the population sums (pft_config::sum_order)")
ap.add_argument("--particles", type=int, default=400, help="particle_num (the KLD tracker's initial count)")
args = ap.parse_args()
kld, frames = args.mode == "kld", args.frames
model, cloud = scene.make_model(2048), scene.make_scene(50000)
t = tracker.make_reference_tracker(particle_num=args.particles, seed=1, kld=kld, sum_order=args.sum_order)
t.setReferenceCloud(model)
t.setTrans(scene.initial_trans())
t.setInputCloud(cloud)
for _ in range(20):
    t.compute()
t.synchronize()
t0 = time.perf_counter()
for _ in range(frames):
    t.compute()
t.synchronize()
print("%s, %s sums: %.3f ms per frame, %d particles" % ("kld" if kld else "fixed", args.sum_order,
                                                        (time.perf_counter() - t0) / frames * 1e3, len(t.getParticles())))
t.profileEnable(True)
for _ in range(50):
    t.compute()
t.synchronize()
pr = t.profileGet()
print({k: round(v[0] / max(v[1], 1) * 1e3, 1) for k, v in pr.items()}, "us per launch (events add ~7 us each)")

#!/usr/bin/env python3
"""Does a view-dependent reference follow an object that turns?  (an experiment, not a test: its
outcome is not derivable.)

The scene's box rolls by --step rad per frame for --frames frames (scene.make_scene(20000) at every pose, the same frames
for every run).  --seeds trackers per mode, --particles particles, every tracker started at the true pose of frame 0 with
the translation 1 cm off on every axis:
  one view        scene.make_model(2048): the faces the camera sees at frame 0 (the tracker's usual model)
  full lattice    the 1.2 cm lattice of all six faces as the reference cloud
  view A          the same lattice through selectView() / setReferenceFromView(): selected at the start pose, and again
                  whenever the result has turned more than A rad from the pose of the last selection
Per mode: mean and worst translation error of the box centre and rotation error over the last 10 frames of all seeds.

    python tools/view_reference_track.py [--seeds 8] [--particles 400] [--step 0.02] [--frames 50] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--particles", type=int, default=400)
    ap.add_argument("--step", type=float, default=0.02)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--angles", default="0.15,0.2")
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

    def pose(f):
        p = list(scene.GT_POSE)
        p[3] += a.step * f
        return tuple(p)

    frames = [scene.make_scene(20000, obj_pose=pose(f)) for f in range(a.frames)]
    truth = [scene.pose_matrix(*pose(f)) for f in range(a.frames)]
    one_view, offset = scene.make_model(2048, return_offset=True)  # box frame minus `offset`
    xyz, fid = scene._box_surface_lattice(scene.MODEL_DIMS, 0.012)
    lattice = scene.make_points(xyz.astype(np.float32), scene.FACE_RGB[fid])

    def angle_between(Ra, Rb):
        return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))

    def run(mode, seed):
        """(translation errors, rotation errors) of the last 10 frames, and the number of selections"""
        t = tracker.make_reference_tracker(particle_num=a.particles, seed=seed)
        start = truth[0].copy()
        centre = offset if mode == "one view" else np.zeros(3)  # the model's origin in the box frame
        start[:3, 3] += start[:3, :3] @ centre + 0.01
        t.setTrans(start.astype(np.float32))
        selections, last = 0, None
        if mode == "one view":
            t.setReferenceCloud(one_view)
        elif mode == "full lattice":
            t.setReferenceCloud(lattice)
        else:
            t.selectView(lattice, start[:3])
            t.setReferenceFromView()
            selections, last = 1, start[:3, :3]
        te, re = [], []
        for f in range(a.frames):
            t.setInputCloud(frames[f])
            t.compute()
            T = np.asarray(t.toEigenMatrix(t.getResult()), np.float64).reshape(4, 4)
            if last is not None and angle_between(last, T[:3, :3]) > mode:
                t.selectView(lattice)
                try:
                    t.setReferenceFromView(min_points=100)
                    selections, last = selections + 1, T[:3, :3]
                except tracker.PftError as e:
                    emit("#   seed %d frame %d: %s" % (seed, f, e))
            if f >= a.frames - 10:
                te.append(float(np.linalg.norm(T[:3, :3] @ (-centre) + T[:3, 3] - truth[f][:3, 3])))
                re.append(angle_between(truth[f][:3, :3], T[:3, :3]))
        t.close()
        return te, re, selections

    emit("# tools/view_reference_track.py: the box rolls %.3f rad per frame for %d frames; %d seeds, %d particles" % (
        a.step, a.frames, a.seeds, a.particles))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    emit("# errors over the last 10 frames of all seeds: translation of the box centre (cm), rotation (rad)")
    emit("# %-14s %10s %10s %10s %10s %12s" % ("reference", "mean cm", "worst cm", "mean rad", "worst rad", "selections"))
    modes = ["one view", "full lattice"] + [float(s) for s in a.angles.split(",")]
    for mode in modes:
        te, re, sel = [], [], []
        for seed in range(1, a.seeds + 1):
            x, y, s = run(mode, seed)
            te += x
            re += y
            sel.append(s)
        name = mode if isinstance(mode, str) else "view %.2f" % mode
        emit("  %-14s %10.2f %10.2f %10.3f %10.3f %12s" % (name, 100 * np.mean(te), 100 * np.max(te), np.mean(re), np.max(re),
                                                           "%d..%d" % (min(sel), max(sel)) if max(sel) else "-"))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

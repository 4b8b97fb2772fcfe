#!/usr/bin/env python3
"""What the population statistics (pft_spread) cost, and what they replace.

Frame time (default): wall time per frame of three loops on trackers with the same seed, alternating in one process, each
repetition timing `--frames` frames; the median / min / max over `--reps` repetitions is printed (the method of
tools/match_bench.py):

    compute(); getResult()                                           the frame without the statistics
    compute(); computeSpread(); getResult(); getSpread()             the statistics on the device
    compute(); getResult(); getParticles(); spread_model.stats()     the same numbers on the host: the copy of P x 32 bytes
                                                                     and the NumPy restatement the tests use

at 400 and 8 192 particles (2 048-point model, 50 000-point cloud).

Kernel time: `--shape p400|p8192` runs `--frames` frames with computeSpread() on one workload and nothing else, to be
started under `rocprofv3 --kernel-trace --stats` in a run of its own per shape (the rows of k_spread_partial and
k_spread_final are the figures):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/spread_bench.py --shape p8192 --frames 200

`--check N` puts an explicit population of N particles on a handle, compares every field of the block with the model bit
for bit and prints the time of the two launches (sizes the suite does not afford, up to 1 048 576).

    python tools/spread_bench.py [--reps 7] [--frames 200] [--warmup 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"p400": 400, "p8192": 8192}
M = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    ap.add_argument("--check", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    import spread_model as sm
    from pcl_tracking_amd import scene, tracker

    if a.check:
        n = a.check
        rng = np.random.default_rng(n)
        p = np.zeros(n, scene.PARTICLE_DTYPE)
        for k, c, s in zip(sm.POSE, (0.3, -0.2, 1.1, 0.1, -0.4, 2.0), (0.02, 0.03, 0.01, 0.1, 0.05, 0.2)):
            p[k] = (rng.normal(0.0, s, n) + c).astype(np.float32)
        w = rng.uniform(0.0, 1.0, n)
        w[rng.uniform(size=n) < 0.2] = 0.0
        p["weight"] = (w / w.sum()).astype(np.float32)
        p["w"] = 1.0
        t = tracker.make_reference_tracker(particle_num=n)
        t.setParticles(p)
        t.computeSpread()
        t.getSpread()
        t0 = time.perf_counter()
        for _ in range(20):
            t.computeSpread()
        got = t.getSpread()
        dt = (time.perf_counter() - t0) / 20
        bad = sm.compare(got, sm.stats(t.getParticles(), t.getResult()), "n=%d" % n)
        print("check %d particles: %s; n_eff %.6g, zero %d, i_max %d, pos_sigma %s; %.1f us per computeSpread() (20 enqueued, "
              "one read-back)" % (n, "every field equals the model" if not bad else "DIFFERS: %s" % [b[1] for b in bad],
                                  got.n_eff, got.n_zero, got.i_max, got.pos_sigma.tolist(), dt * 1e6), flush=True)
        t.close()
        sys.exit(1 if bad else 0)

    cloud = scene.make_scene(50000)

    def make(particles):
        t = tracker.make_reference_tracker(particle_num=particles, seed=21)
        t.setReferenceCloud(scene.make_model(M))
        t.setTrans(scene.initial_trans())
        t.setInputCloud(cloud)
        return t

    def frame_plain(t):
        t.compute()
        return t.getResult()

    def frame_device(t):
        t.compute()
        t.computeSpread()
        t.getResult()
        return t.getSpread()

    def frame_host(t):
        t.compute()
        r = t.getResult()
        return sm.stats(t.getParticles(), r)

    if a.shape:
        t = make(SHAPES[a.shape])
        for _ in range(a.warmup + a.frames):
            st = frame_device(t)
        print("shape %s: %d particles, n_eff %.6g, pos_sigma %s, %d frames with computeSpread()" % (
            a.shape, SHAPES[a.shape], st.n_eff, st.pos_sigma.tolist(), a.warmup + a.frames), flush=True)
        t.close()
        return

    if a.reps < 7 or a.frames < 200:
        print("note: fewer than 7 repetitions of 200 frames: not a figure to quote", file=sys.stderr)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/spread_bench.py: %d-point model, 50 000-point cloud, %d repetitions of %d frames, warm-up %d frames" % (
        M, a.reps, a.frames, a.warmup))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    emit("# ms per frame on the host; median [min .. max] over the repetitions")
    for particles in (400, 8192):
        variants = [("compute", frame_plain), ("+ computeSpread + getSpread", frame_device),
                    ("+ getParticles + NumPy model", frame_host)]
        ts = [make(particles) for _ in variants]
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
        for (name, _), v in zip(variants, times):
            med = statistics.median(v)
            emit("%5d particles  %-30s %.4f [%.4f .. %.4f]  %+.1f us" % (particles, name, med, min(v), max(v),
                                                                         1e3 * (med - base)))
        dev, host = frame_device(ts[1]), frame_host(ts[2])
        emit("#   device: n_eff %.6g, pos_sigma[2] %.6g;  host: n_eff %.6g, pos_sigma[2] %.6g (same seed, same frames)" % (
            dev.n_eff, float(dev.pos_sigma[2]), host["n_eff"], float(host["pos_sigma"][2])))
        for t in ts:
            t.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

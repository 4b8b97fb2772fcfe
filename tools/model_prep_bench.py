"""Model preparation: the host path of setObjectsToTrack against the device path, each from an
object cluster that lies in HBM to a tracker that is ready to compute (tools/model_prep_bench.cpp explains the two),
at 500, 5 000 and 25 000 points, with and without the report cloud; wall-clock median of --reps alternating runs, and the
GPU time of the device pipeline's four stages (HIP events on the handle's stream).

    python tools/model_prep_bench.py [--reps 20] [--out profiles/model_prep_bench.txt]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (500, 5000, 25000)


def build_bench(force=False):
    from pcl_tracking_amd import build

    lib = build.build()
    exe = os.path.join(build.OUT_DIR, "model_prep_bench")
    src = os.path.join(ROOT, "tools", "model_prep_bench.cpp")
    deps = [src, lib, os.path.join(build.EXAMPLES_DIR, "tracking_app.hpp")]
    if not force and os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    cmd = [build.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "pcl_tracking_amd", "include"), src, "-o", exe, "-L", os.path.dirname(lib), "-lpft_hip",
           "-Wl,-rpath," + os.path.dirname(lib)]
    subprocess.run(cmd, check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    exe = build_bench()
    if a.build_only:
        print(exe)
        return
    lines = []
    for report in (0, 1):
        for n in SIZES:
            r = subprocess.run([exe, str(n), str(a.reps), str(report)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit("model_prep_bench %d failed (%d)" % (n, r.returncode))
            lines.append(r.stdout.strip())
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

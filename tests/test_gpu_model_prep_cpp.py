"""The C++ drivers with the model preparation on the device: `auto_tracking_amd --segment <scene>` (model creation,
model preparation and tracking in one process, the clusters never leaving HBM) and `--device-models` (models from files,
prepared on the device) print the same `frame ... object ...` lines as the file-based flow through create_model_amd and
the host-side setObjectsToTrack().  Binary PCD keeps every bit, so the bar is line-for-line equality."""
import os
import subprocess

import pytest

from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu
# the plane-after-plane loop of test/cluster_euclid.cpp on the synthetic scene: no box, clusters from 50 points
SEGMENT_FLAGS = ["--planes", "16,0.3", "--sac", "100,0.02", "--min-size", "50", "--box", "-10,10,-10,10,-10,10"]
TRACK_FLAGS = ["--particles", "64", "--seed", "1"]


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def frame_lines(r):
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("frame ")]
    assert lines
    return lines


@pytest.fixture(scope="module")
def flow(tmp_path_factory):
    """the scene, two frames, and the model files create_model_amd writes from the scene"""
    from pcl_tracking_amd import build

    d = tmp_path_factory.mktemp("model_prep_cpp")
    scene_path = str(d / "scene.bin")
    scene.make_scene(50000).tofile(scene_path)
    frames = []
    for f in range(2):
        p = str(d / ("frame%d.bin" % f))
        scene.make_scene(20000, obj_pose=scene.advance_pose(scene.GT_POSE, f)).tofile(p)
        frames.append(p)
    out = d / "models"
    out.mkdir()
    create, track = build.build_create_model_example(), build.build_example()
    r = run(create, [scene_path, "--out", out] + SEGMENT_FLAGS)
    n = int([ln for ln in r.stdout.splitlines() if ln.startswith("clusters ")][0].split()[1])
    assert n >= 2
    models = [str(out / ("%d.pcd" % j)) for j in range(n)]
    assert all(os.path.exists(m) for m in models)
    return dict(track=track, scene=scene_path, frames=frames, models=models)


@pytest.mark.parametrize("report", [[], ["--device-report"]], ids=["host-report", "device-report"])
def test_segment_and_device_models_print_the_file_flows_lines(flow, report):
    tail = ["--frames"] + flow["frames"] + TRACK_FLAGS + report
    files = frame_lines(run(flow["track"], flow["models"] + tail))
    assert len(files) == len(flow["models"]) * 2 * (2 if report else 1)  # objects x frames (x the box line)
    device_models = frame_lines(run(flow["track"], flow["models"] + ["--device-models"] + tail))
    assert device_models == files
    segment = frame_lines(run(flow["track"], ["--segment", flow["scene"]] + SEGMENT_FLAGS + tail))
    assert segment == files

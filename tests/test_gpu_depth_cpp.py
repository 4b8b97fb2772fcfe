"""The C++ path of the depth entrance: `auto_tracking_amd --depth-frames` over pft/filters.hpp and pft/pnm_io.hpp.  Three
frames of the moving object (scene.make_depth_images, 320 x 180) are written twice: as PGM / PPM image pairs, and as binary
PCD files of the cloud the specification's model (tests/depth_model.py) forms from those images.  The driver must print the
same lines for both, with and without --async: the depth entrance forms the same records and everything behind it is the
same code."""
import subprocess

import numpy as np
import pytest

import depth_cases as dc
import depth_model as dm
import subtract_cases as sc
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu
TRACK = ["--particles", "200", "--seed", "3"]


@pytest.fixture(scope="module")
def exe():
    from pcl_tracking_amd import build

    return build.build_example()


@pytest.fixture(scope="module")
def runs(exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_cpp")
    model = scene.make_model(512).copy()
    off = np.array(scene.model_gt_pose()[:3], np.float32)
    for k, name in enumerate(("x", "y", "z")):  # a model file is the object's cluster in the camera frame
        model[name] = model[name] + off[k]
    sc.write_pcd(str(d / "model.pcd"), model)
    pcd, pairs, bare = [], [], []
    for f in range(3):
        depth, bgr, camera = scene.make_depth_images(320, 180, obj_pose=scene.advance_pose(scene.GT_POSE, f))
        dc.write_pgm(str(d / ("depth%d.pgm" % f)), depth)
        dc.write_ppm(str(d / ("colour%d.ppm" % f)), bgr)
        sc.write_pcd(str(d / ("frame%d.pcd" % f)), dm.deproject(depth, bgr, camera))
        pcd.append(str(d / ("frame%d.pcd" % f)))
        pairs.append("%s:%s" % (d / ("depth%d.pgm" % f), d / ("colour%d.ppm" % f)))
        bare.append(str(d / ("depth%d.pgm" % f)))
    cam = "%r,%r,%r,%r" % camera
    out = {}
    for name, frames, extra in (("pcd", pcd, ["--raw"]), ("pcd_async", pcd, ["--raw", "--async"]),
                                ("depth", pairs, ["--depth-frames", cam]),
                                ("depth_async", pairs, ["--depth-frames", cam + ",1000", "--async"]),
                                ("bare", bare, ["--depth-frames", cam])):
        r = subprocess.run([exe, str(d / "model.pcd"), "--frames"] + frames + TRACK + extra, capture_output=True, text=True,
                           timeout=300)
        print(name, r.stdout[-1500:], r.stderr[-1500:])
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = (r.stdout.splitlines(), r.stderr.splitlines())
    return out


def test_depth_frames_print_the_lines_of_the_raw_flow(runs):
    out, err = runs["pcd"]
    assert len([ln for ln in out if ln.startswith("frame ")]) == 3
    down = [ln for ln in err if ln.startswith("PointCloud")]
    assert len(down) == 6 and int(down[1].split()[3]) > 1000  # the front end ran, and kept a cloud to track in
    assert runs["depth"] == runs["pcd"]


def test_depth_frames_async_through_the_pinned_slots(runs):
    assert runs["depth_async"] == runs["pcd_async"]
    assert runs["depth_async"][0] == runs["pcd"][0]  # and the poses are those of the synchronous flow


def test_a_bare_depth_image_has_no_colour(runs):
    """the same geometry, every valid point black: the front end's counts are the coloured run's, the run completes"""
    out, err = runs["bare"]
    assert len([ln for ln in out if ln.startswith("frame ")]) == 3
    assert [ln for ln in err if ln.startswith("PointCloud")] == [ln for ln in runs["pcd"][1] if ln.startswith("PointCloud")]

"""The C++ driver with scene subtraction: `auto_tracking_amd --discover` finds an object that has no model and tracks it
from the next frame on, without disturbing the object it was given; `--reacquire --reacquire-residual` looks for a lost
object only among the clusters that no tracked object explains.  Two small objects of the same shape half a metre apart
(tests/subtract_cases.py::two_object_frame), frames written as binary PCD files."""
import subprocess

import numpy as np
import pytest

import subtract_cases as sc

pytestmark = pytest.mark.gpu
TRACK = ["--particles", "64", "--seed", "1", "--model-leaf", "0"]
SEGMENT = ["--no-plane", "--box", "-10,10,-10,10,-10,10", "--tolerance", "0.02", "--min-size", "100"]


@pytest.fixture(scope="module")
def exe():
    from pcl_tracking_amd import build

    return build.build_example()


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def object_lines(out, obj):
    """{frame: the centroid of the object's line}"""
    res = {}
    for ln in out:
        w = ln.split()
        if len(w) > 4 and w[0] == "frame" and w[2] == "object" and int(w[3]) == obj and w[4] == "pose":
            res[int(w[1])] = np.array([float(v) for v in w[w.index("centroid") + 1:][:3]])
    return res


def write_frames(d, jumped_from=None, n=4):
    paths = []
    for f in range(n):
        paths.append(str(d / ("frame%d.pcd" % f)))
        sc.write_pcd(paths[-1], sc.two_object_frame(f, jumped=jumped_from is not None and f >= jumped_from))
    return paths


def test_discover_finds_the_object_without_a_model(exe, tmp_path):
    """400 particles and a subtraction radius of 0.04 m: with 64 particles the pose of the (static) object moves by 2 cm and
    more from frame to frame, and a model that is 2 cm off leaves a strip of its object unexplained at the default radius
    of 0.02 m -- which --discover then rightly reports as an object of its own (known limits)"""
    sc.write_pcd(str(tmp_path / "a.pcd"), sc.object_cluster())
    frames = write_frames(tmp_path)
    base = [str(tmp_path / "a.pcd"), "--frames"] + frames + ["--particles", "400", "--seed", "1", "--model-leaf", "0"]
    plain = run(exe, base)
    found = run(exe, base + ["--discover=1,0.04"] + SEGMENT)
    disc = [ln for ln in found if ln.startswith("discover ")]
    first = [ln for ln in disc if ln.startswith("discover frame 1:")]
    assert len(first) == 1 and first[0].startswith("discover frame 1: cluster 0 -> obj 1 (")
    assert disc == first, "the new object is subtracted from the frames after it: nothing else turns up"
    n_points = int(first[0].split("(")[1].split()[0])
    assert 500 <= n_points <= 700  # object B has 600 points in a frame
    # the new object has pose lines from the next frame on, where object B stands
    gt_b = sc.small_world()["gt"] + np.array([sc.SECOND_OFFSET, 0.0, 0.0])
    new = object_lines(found, 1)
    assert sorted(new) == [2, 3, 4]
    for c in new.values():
        assert np.linalg.norm(c - gt_b) < 0.05, c
    # the object that came with a model is tracked as without --discover, line for line
    mine = [ln for ln in found if ln.startswith("frame ") and " object 0 " in ln]
    assert mine == [ln for ln in plain if ln.startswith("frame ")] and len(mine) == 4


def test_discover_prints_the_support_with_match(exe, tmp_path):
    sc.write_pcd(str(tmp_path / "a.pcd"), sc.object_cluster())
    frames = write_frames(tmp_path, n=2)
    out = run(exe, [str(tmp_path / "a.pcd"), "--frames"] + frames + TRACK + ["--match", "--discover=2,0.02"] + SEGMENT)
    sup = [ln.split() for ln in out if ln.startswith("support obj ")]
    assert len(sup) == 1 and sup[0][2] == "0" and 1200 <= int(sup[0][3]) <= 1500  # every=2: frame 1 only; A has 1 500 points
    assert len([ln for ln in out if ln.startswith("discover ")]) == 1


def test_reacquire_residual_never_lands_on_the_live_object(exe, tmp_path):
    """object A jumps half a metre at the fourth frame and is lost at the fifth; object B, of the same shape, stays and is
    tracked.  The residual of the frame has no cluster on B, so A can only be found where it went"""
    sc.write_pcd(str(tmp_path / "a.pcd"), sc.object_cluster())
    sc.write_pcd(str(tmp_path / "b.pcd"), sc.object_cluster(shift_x=sc.SECOND_OFFSET))
    frames = write_frames(tmp_path, jumped_from=3, n=8)
    out = run(exe, [str(tmp_path / "a.pcd"), str(tmp_path / "b.pcd"), "--frames"] + frames + TRACK +
              ["--match=0.5,2", "--reacquire=9", "--reacquire-residual", "--no-plane", "--box", "-10,10,-10,10,-10,10",
               "--tolerance", "0.04", "--min-size", "100"])
    rq = [ln.split() for ln in out if ln.startswith("reacquire obj ")]
    assert len(rq) == 1 and rq[0][2] == "0:" and rq[0][-2:] == ["accepted", "1"] and int(rq[0][4]) >= 0
    gt = sc.small_world()["gt"]
    gt_b, gt_a_new = gt + np.array([sc.SECOND_OFFSET, 0.0, 0.0]), gt + np.array([0.0, sc.JUMP, 0.0])
    a, b = object_lines(out, 0), object_lines(out, 1)
    assert sorted(a) == sorted(b) == list(range(1, 9))
    for f in (6, 7, 8):  # after the restart: where A went, not where B stands
        assert np.linalg.norm(a[f] - gt_a_new) < 0.05 and np.linalg.norm(a[f] - gt_b) > 0.3, (f, a[f])
    for c in b.values():
        assert np.linalg.norm(c - gt_b) < 0.05

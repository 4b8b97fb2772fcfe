"""The C++ path of the visibility: `auto_tracking_amd --visibility` over pft/particle_filter_tracker.hpp.  A patch that a
plate hides for three frames (tests/visibility_cases.py), frames written as binary PCD files: with --match alone the lost
rule fires on the hidden frames; with --visibility the object is reported occluded and never lost, and the `visibility`
lines show what the camera sees."""
import subprocess

import numpy as np
import pytest

import subtract_cases as sc
import visibility_cases as vc

pytestmark = pytest.mark.gpu
KINDS = ["full", "hidden", "hidden", "hidden", "full"]
TRACK = ["--particles", "64", "--seed", "1", "--model-leaf", "0", "--match=0.5,2"]


@pytest.fixture(scope="module")
def exe():
    from pcl_tracking_amd import build

    return build.build_example()


@pytest.fixture(scope="module")
def runs(exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("visibility_cpp")
    model = vc.patch_model().copy()
    moved = vc._move(vc.cloud_xyz(model), vc.patch_trans())
    model["x"], model["y"], model["z"] = moved[:, 0], moved[:, 1], moved[:, 2]
    sc.write_pcd(str(d / "patch.pcd"), model)
    frames = []
    for f, kind in enumerate(KINDS):
        frames.append(str(d / ("frame%d.pcd" % f)))
        sc.write_pcd(frames[-1], vc.patch_frame(kind, f))
    out = {}
    for name, extra in (("match", []), ("visibility", ["--visibility"]), ("own_values", ["--visibility=0.9,0.5"])):
        r = subprocess.run([exe, str(d / "patch.pcd"), "--frames"] + frames + TRACK + extra, capture_output=True, text=True,
                           timeout=300)
        print(name, r.stdout[-3000:], r.stderr[-2000:])
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = (r.stdout.splitlines(), r.stderr.splitlines())
    return out


def test_match_alone_loses_the_hidden_object(runs):
    _, err = runs["match"]
    assert [ln for ln in err if "Object not recognized" in ln] == ["frame %d object 0: Object not recognized" % f for f in (3, 4)]
    assert not any("occluded" in ln for ln in err)


def test_visibility_reports_occluded_and_never_lost(runs):
    out, err = runs["visibility"]
    assert not any("Object not recognized" in ln for ln in err)
    assert [ln for ln in err if "Object occluded" in ln] == ["frame %d object 0: Object occluded" % f for f in (2, 3, 4)]
    vis = [ln.split() for ln in out if ln.startswith("visibility obj 0 ")]
    assert len(vis) == len(KINDS)
    for w, kind in zip(vis, KINDS):
        assert w[3] == "visible" and w[5] == "occluded" and w[7] == "self" and w[9] == "out"
        n, M = (int(v) for v in w[4].split("/"))
        occluded, n_self, n_out = int(w[6]), int(w[8]), int(w[10])
        assert M == 300 and n + occluded + n_self + n_out == M
        assert (n >= 240 and occluded == 0) if kind == "full" else (n < 75 and occluded > 225), (kind, w)
    # the frames' pose and match lines are those of the run without the flag as long as the two runs did the same
    plain = [ln for ln in runs["match"][0] if ln.startswith("frame 1 ")]
    assert plain and plain == [ln for ln in out if ln.startswith("frame 1 ")]


def test_visibility_takes_its_own_values(runs):
    """min_visible_ratio 0.9 with an occlusion margin of 0.5 m: the plate, 0.2 m in front, occludes nothing"""
    out, err = runs["own_values"]
    vis = [ln.split() for ln in out if ln.startswith("visibility obj 0 ")]
    assert len(vis) == len(KINDS) and all(int(w[6]) == 0 for w in vis)
    assert not any("Object occluded" in ln for ln in err)
    assert any("Object not recognized" in ln for ln in err)  # visible but unmatched: the rule counts it

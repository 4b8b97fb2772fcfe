"""The C++ path of the view-dependent reference: `auto_tracking_amd --view-reference --view-model` over
pft/particle_filter_tracker.hpp.  A static object of two parallel plates (tests/view_cases.py), the front plate as the
object's model and both plates as its full model, three frames written as binary PCD files: the `view obj` lines are
well formed, the reference cloud of the next frame is the view that was kept, and a refused hand-off leaves the run going."""
import subprocess

import numpy as np
import pytest

import subtract_cases as sc
import view_cases as wc

pytestmark = pytest.mark.gpu
TRACK = ["--particles", "64", "--seed", "1", "--model-leaf", "0", "--match"]
N_FRAMES = 3


@pytest.fixture(scope="module")
def exe():
    from pcl_tracking_amd import build

    return build.build_example()


@pytest.fixture(scope="module")
def runs(exe, tmp_path_factory):
    from pcl_tracking_amd import scene

    d = tmp_path_factory.mktemp("view_cpp")
    xyz = wc.two_plates()["xyz"]  # the camera frame: the front plate at 1 m, the back plate 10 cm behind it
    n = len(xyz) // 2
    full = scene.make_points(xyz, np.where(np.arange(2 * n)[:, None] < n, (150, 90, 60), (60, 90, 150)))
    sc.write_pcd(str(d / "front.pcd"), full[:n])
    sc.write_pcd(str(d / "full.pcd"), full)
    u, v = np.meshgrid(np.arange(25) * 0.03 - 0.36, np.arange(20) * 0.03 - 0.3, indexing="ij")
    wall = scene.make_points(np.stack([u.ravel(), v.ravel(), np.full(u.size, 1.6)], 1).astype(np.float32), np.full((u.size, 3), 80))
    frames = []
    for f in range(N_FRAMES):
        frames.append(str(d / ("frame%d.pcd" % f)))
        sc.write_pcd(frames[-1], np.concatenate([full[:n], wall]))
    out = {}
    for name, flag in (("view", "--view-reference=0,50"), ("refused", "--view-reference=0,%d" % (2 * n + 1))):
        r = subprocess.run([exe, str(d / "front.pcd"), "--frames"] + frames + TRACK + [flag, "--view-model", str(d / "full.pcd")],
                           capture_output=True, text=True, timeout=300)
        print(name, r.stdout[-3000:], r.stderr[-2000:])
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = (r.stdout.splitlines(), r.stderr.splitlines())
    return out, n


def view_lines(out):
    """frame -> (model, visible, kept) of `view obj 0 frame <f>: model <n> visible <n> kept <n>`"""
    got = {}
    for ln in out:
        if not ln.startswith("view obj 0 "):
            continue
        w = ln.split()
        assert len(w) == 11 and w[3] == "frame" and w[4].endswith(":") and (w[5], w[7], w[9]) == ("model", "visible", "kept"), ln
        got[int(w[4][:-1])] = (int(w[6]), int(w[8]), int(w[10]))
    return got


def match_m(out):
    """frame -> n_reference of the `match` line"""
    return {int(w[1]): int(w[7]) for w in (ln.split() for ln in out) if len(w) > 7 and w[0] == "frame" and w[4] == "match"}


def test_view_lines_and_the_next_frames_reference(runs):
    (out, err), n = runs[0]["view"], runs[1]
    views, M = view_lines(out), match_m(out)
    assert 1 in views and len(M) == N_FRAMES  # the first result always selects
    assert M[1] == n  # the model file
    kept_now = n
    for f in range(1, N_FRAMES + 1):
        assert M[f] == kept_now, (f, M, views)
        if f in views:
            model, visible, kept = views[f]
            assert model == 2 * n and kept <= visible <= model and kept >= 50
            kept_now = kept
    assert not any("setReferenceFromView" in ln for ln in err)


def test_a_refused_hand_off_keeps_the_old_reference(runs):
    (out, err), n = runs[0]["refused"], runs[1]
    views, M = view_lines(out), match_m(out)
    assert sorted(views) == list(range(1, N_FRAMES + 1))  # never consumed: every frame selects again
    assert all(M[f] == n for f in range(1, N_FRAMES + 1))
    refusals = [ln for ln in err if "setReferenceFromView" in ln]
    assert len(refusals) == N_FRAMES and all("fewer than the %d" % (2 * n + 1) in ln for ln in refusals)

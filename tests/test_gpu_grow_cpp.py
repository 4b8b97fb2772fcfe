"""Model growth from C++: a small program over pft::ModelGrowth (tests/cpp/grow_frontier_tool.cpp) whose printed counts for
the frontier case equal the restatement's, and the driver's --grow-models flag over a short sequence in which the object
rolls (tests/grow_cases.py::rolling_sequence)."""
import os
import subprocess

import numpy as np
import pytest

import grow_cases as gc
import grow_model as gm
import subtract_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("reach,confirm,applies", [(2, 3, 7), (1, 1, 5)])
def test_frontier_counts_from_cpp(tmp_path, reach, confirm, applies):
    from pcl_tracking_amd import build

    case = gc.frontier_case(reach=reach, confirm=confirm, applies=applies)
    model, frame = case["ops"][0][1], case["ops"][1][1]
    model.tofile(str(tmp_path / "model.bin"))
    frame.tofile(str(tmp_path / "frame.bin"))
    exe = build.build_host_program(os.path.join(ROOT, "tests", "cpp", "grow_frontier_tool.cpp"), str(tmp_path / "grow_frontier_tool"))
    env = dict(os.environ, LD_LIBRARY_PATH=build.OUT_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, str(reach), str(confirm), str(applies), str(tmp_path / "model.bin"), str(tmp_path / "frame.bin")],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    g, _, stats = gc.run(case)
    want = ["apply %d known %d unreached %d candidate %d added %d voxels %d model %d pending %d" % (
        a + 1, s["n_state"]["KNOWN"], s["n_state"]["UNREACHED"], s["n_state"]["CANDIDATE"], s["n_added"], s["n_model_voxels"],
        s["n_model_points"], s["n_pending_live"]) for a, s in enumerate(stats)]
    want.append("table %d" % len(g.debug_table()["kind"]))
    want.append("model_bytes %d" % int(np.frombuffer(g.cloud.tobytes(), np.uint8).sum(dtype=np.uint64)))
    assert r.stdout.splitlines() == want


@pytest.fixture(scope="module")
def exe():
    from pcl_tracking_amd import build

    return build.build_example()


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_driver_grows_the_model_of_a_rolling_object(exe, tmp_path):
    """it asserts that `grow obj` lines are printed and that some frame adds points, and that without the flag the lines
    are those of the driver before the flag existed (tests/golden/grow_driver_plain.txt, recorded from that driver).  It
    makes no claim about tracking quality"""
    seq = gc.rolling_sequence()
    sc.write_pcd(str(tmp_path / "scene.pcd"), seq[0])
    frames = []
    for f, cloud in enumerate(seq[1:]):
        frames.append(str(tmp_path / ("frame%d.pcd" % f)))
        sc.write_pcd(frames[-1], cloud)
    base = ["--segment", str(tmp_path / "scene.pcd")] + gc.ROLLING_FLAGS + ["--frames"] + frames + \
           ["--particles", "400", "--seed", "1", "--model-leaf", "0", "--discover"]
    plain = run(exe, base)
    assert not any(ln.startswith("grow ") for ln in plain)
    golden = open(os.path.join(ROOT, "tests", "golden", "grow_driver_plain.txt")).read().splitlines()
    assert plain == golden
    grown = run(exe, base + ["--grow-models=1"])
    lines = [ln.split() for ln in grown if ln.startswith("grow obj ")]
    assert len(lines) >= len(frames)  # one per bound object and frame
    assert all(ln[2] == "0:" or ln[2][:-1].isdigit() for ln in lines)
    added = [int(ln[ln.index("added") + 1]) for ln in lines]
    assert max(added) > 0
    models = [int(ln[ln.index("model") + 1]) for ln in lines if ln[2] == "0:"]
    assert models == sorted(models) and models[-1] > models[0]

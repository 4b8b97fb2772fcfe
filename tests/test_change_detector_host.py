"""CPU checks of the change detector: hand-worked answers of the NumPy model (tests/change_detector_model.py) the GPU tests
compare the device against, the counter schedule of weight(), the C++ mirror's and the Python binding's new setters, and
the unchanged configuration ABI (the detector is configured through entry points of its own; pft_config did not grow)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from change_detector_model import ChangeDetectorModel, CounterModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pft.h")
RES = 0.05


def cloud(xyz):
    from pcl_tracking_amd import scene

    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return scene.make_points(xyz, np.full((len(xyz), 3), 128, np.uint8))


def in_voxel(x, y, z, n):
    """n points in one detector voxel: copies of (x, y, z) (the box is centred on the first point ever inserted, so
    the voxel faces are not at multiples of the resolution)"""
    return np.tile(np.array([[x, y, z]]), (n, 1))


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_first_call_finds_everything_new(orc):
    m = ChangeDetectorModel(orc, RES)
    pts = np.vstack([in_voxel(0.02, 0.02, 0.02, 3), in_voxel(0.32, 0.02, 0.02, 2), in_voxel(0.02, 0.52, 0.02, 1)])
    idx, nv, box, depth = m.test(cloud(pts), 1)
    assert nv == 3 and idx.tolist() == list(range(6))
    assert depth >= 1 and np.all(box[:3] <= pts.min(0)) and np.all(box[3:] > pts.max(0))


def test_same_cloud_twice_finds_nothing_new(orc):
    m = ChangeDetectorModel(orc, RES)
    c = cloud(np.vstack([in_voxel(0.02, 0.02, 0.02, 4), in_voxel(0.42, 0.12, 0.02, 4)]))
    assert m.test(c, 1)[1] == 2
    idx, nv, _, _ = m.test(c, 1)
    assert nv == 0 and len(idx) == 0


@pytest.mark.parametrize("min_points", [5, 10])
def test_min_points_threshold(orc, min_points):
    base = in_voxel(0.02, 0.02, 0.02, 3)
    for n, want in ((min_points - 1, 0), (min_points, 1)):
        m = ChangeDetectorModel(orc, RES)
        m.test(cloud(base), 1)
        extra = in_voxel(0.22, 0.02, 0.02, n)
        idx, nv, _, _ = m.test(cloud(np.vstack([base, extra])), min_points)
        assert nv == want
        assert idx.tolist() == (list(range(3, 3 + n)) if want else [])


def test_min_points_zero_and_one_agree(orc):
    a, b = ChangeDetectorModel(orc, RES), ChangeDetectorModel(orc, RES)
    c1, c2 = cloud(in_voxel(0.02, 0.02, 0.02, 2)), cloud(np.vstack([in_voxel(0.02, 0.02, 0.02, 2), in_voxel(0.3, 0, 0, 1)]))
    a.test(c1, 0)
    b.test(c1, 1)
    assert a.test(c2, 0)[0].tolist() == b.test(c2, 1)[0].tolist() == [2]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_growth_towards_negative_keeps_old_voxels_known(orc, axis):
    m = ChangeDetectorModel(orc, RES)
    base = np.vstack([in_voxel(0.02, 0.02, 0.02, 3), in_voxel(0.12, 0.07, 0.17, 3)])
    _, _, box0, d0 = m.test(cloud(base), 1)
    far = np.array([[0.03, 0.03, 0.03]])
    far[0, axis] = -2.0  # several root doublings with the minimum lowered on this axis
    idx, nv, box1, d1 = m.test(cloud(np.vstack([base, far])), 1)
    assert d1 > d0 and box1[axis] < box0[axis]
    assert nv == 1 and idx.tolist() == [len(base)]


def test_empty_crop_switches_the_buffers(orc):
    m = ChangeDetectorModel(orc, RES)
    c = cloud(in_voxel(0.02, 0.02, 0.02, 4))
    m.test(c, 1)
    idx, nv, _, _ = m.test(cloud(np.zeros((0, 3))), 1)
    assert nv == 0 and len(idx) == 0
    assert m.test(c, 1)[1] == 1  # the previous test held nothing: everything is new again


# ---- the counter schedule ----------------------------------------------------------------------------------------------
def run_schedule(interval, outcomes, n, use=True):
    cm, it = CounterModel(), iter(outcomes)
    return [cm.step(use, interval, lambda: next(it)) for _ in range(n)]


def test_counter_interval_zero_tests_every_iteration():
    got = run_schedule(0, [True, False, False, True], 4)
    assert got == [(True, True, 0), (True, False, 0), (True, False, 0), (True, True, 0)]


def test_counter_interval_one():
    got = run_schedule(1, [True, False, True], 5)
    assert got == [(True, True, 1), (False, True, 0), (True, False, 0), (True, True, 1), (False, True, 0)]


def test_counter_interval_ten():
    got = run_schedule(10, [True, True], 12)
    assert [g[0] for g in got] == [True] + [False] * 10 + [True]
    assert [g[2] for g in got] == [10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 10]
    assert all(g[1] for g in got)


def test_counter_off_and_on_again():
    cm = CounterModel()
    seq = [cm.step(False, 3, lambda: pytest.fail("no test while off")) for _ in range(5)]
    assert seq == [(False, True, 3), (False, True, 2), (False, True, 1), (False, True, 0), (False, True, 3)]
    # turned on with the counter at 3: three more evaluations, then the first test
    on = [cm.step(True, 3, lambda: False) for _ in range(5)]
    assert on == [(False, True, 2), (False, True, 1), (False, True, 0), (True, False, 0), (True, False, 0)]


# ---- interfaces ----------------------------------------------------------------------------------------------------------
def _header_define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, open(HEADER).read(), re.M)
    assert m, name
    return int(m.group(1))


def test_config_abi_is_untouched():
    from pcl_tracking_amd import _lib

    assert _header_define("PFT_ABI_VERSION") == _lib.PFT_ABI_VERSION == 5
    assert _header_define("PFT_CD_RING") == _lib.PFT_CD_RING
    fields = [f[0] for f in _lib.Config._fields_]
    assert fields[-1] == "sum_order" and not any("change" in f for f in fields)
    L = _lib.load()
    cfg = _lib.Config()
    L.pft_config_default(C.byref(cfg))
    assert cfg.abi_version == 5 and C.sizeof(cfg) == C.sizeof(_lib.Config)
    src = "#include <stdio.h>\n#include \"pft.h\"\nint main(void){printf(\"%zu\\n\", sizeof(pft_config));return 0;}\n"
    exe = os.path.join(os.environ.get("TMPDIR", "/tmp"), "pft_cd_sizeof_%d" % os.getpid())
    r = subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True,
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    try:
        assert int(subprocess.run([exe], capture_output=True, text=True).stdout) == C.sizeof(_lib.Config)
    finally:
        os.unlink(exe)


def test_new_symbols_are_declared_and_bound():
    from pcl_tracking_amd import _lib

    names = {s[0] for s in _lib.SYMBOLS}
    hdr = open(HEADER).read()
    for n in ("pft_set_change_detector", "pft_get_change_detector", "pft_debug_change_state", "pft_debug_change_detect"):
        assert n in names and re.search(r"\b%s\(" % n, hdr)
        assert hasattr(_lib.load(), n)


def test_cpp_mirror_setters_compile():
    src = r'''
#include "pft/particle_filter_tracker.hpp"
int main() {
  pft::tracking::ParticleFilterOMPTracker<pft::PointXYZRGBA, pft::ParticleXYZRPY> t(8);
  t.setUseChangeDetector(true);
  t.setIntervalOfChangeDetection(10);
  t.setMinPointsOfChangeDetection(5);
  t.setResolutionOfChangeDetection(0.05);
  pft::tracking::KLDAdaptiveParticleFilterOMPTracker<pft::PointXYZRGBA, pft::ParticleXYZRPY> k(8);
  k.setUseChangeDetector(false);
  bool ok = t.getUseChangeDetector() && t.getIntervalOfChangeDetection() == 10u && t.getMinPointsOfChangeDetection() == 5u &&
            t.getResolutionOfChangeDetection() == 0.05 && !k.getUseChangeDetector();
  return ok ? 0 : 1;
}
'''
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", "-", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "pcl_tracking_amd", "include")], input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("kld", [False, True])
def test_python_setters_round_trip(kld):
    from pcl_tracking_amd import tracker

    t = tracker.make_reference_tracker(kld=kld)
    assert (t.getUseChangeDetector(), t.getIntervalOfChangeDetection(), t.getMinPointsOfChangeDetection(),
            t.getResolutionOfChangeDetection()) == (False, 10, 10, 0.01)
    t.setUseChangeDetector(True)
    t.setIntervalOfChangeDetection(3)
    t.setMinPointsOfChangeDetection(5)
    t.setResolutionOfChangeDetection(0.05)
    assert (t.getUseChangeDetector(), t.getIntervalOfChangeDetection(), t.getMinPointsOfChangeDetection(),
            t.getResolutionOfChangeDetection()) == (True, 3, 5, 0.05)
    t2 = tracker.make_reference_tracker(kld=kld, change_detector=(7, 2, 0.02))
    assert (t2.getUseChangeDetector(), t2.getIntervalOfChangeDetection(), t2.getMinPointsOfChangeDetection(),
            t2.getResolutionOfChangeDetection()) == (True, 7, 2, 0.02)

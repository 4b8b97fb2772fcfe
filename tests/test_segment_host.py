"""Model creation, CPU side (no GPU): the NumPy restatement of the recalled PCL 1.8.0 rules (tests/segment_model.py)
against known answers and hand cases, the C ABI's config defaults, the PCD writer and the create_model_amd build.
The device is compared with the same restatement in tests/test_gpu_segment.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import segment_model as M
from pcl_tracking_amd import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _compile(src, out, extra=()):
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "pcl_tracking_amd", "include"), src, "-o", str(out)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


# ---- RULE rng ----
def test_mt19937_known_answer():
    e = M.MT19937(5489)
    for _ in range(9999):
        e()
    assert e() == 4123659995  # the C++ standard's required 10 000th output of default-seeded mt19937


def test_mt19937_matches_std_mt19937_seed_12345(tmp_path):
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "mt19937_tool.cpp"), tmp_path / "mt")
    want = [int(v) for v in subprocess.run([exe, "12345", "2000"], capture_output=True, text=True,
                                           check=True).stdout.split()]
    e = M.MT19937(12345)
    assert [e() for _ in range(2000)] == want


def test_uniform_int_reduces_to_shift():
    e1, e2 = M.MT19937(12345), M.MT19937(12345)
    for _ in range(3000):
        assert M.uniform_int_0_intmax(e1) == e2() >> 1


# ---- RULE draw ----
class _Fixed:
    def __init__(self, vals):
        self.vals = list(vals)

    def __call__(self):
        return self.vals.pop(0)


def test_draw_index_sample_by_hand():
    s = M.Sampler(5)
    s.eng = _Fixed([2 * r for r in (3, 0, 7, 1, 1, 1)])  # rnd() = engine() >> 1
    # [0 1 2 3 4] -> i0: swap 0,3 -> [3 1 2 0 4]; i1: 1 + 0 % 4 = 1; i2: 2 + 7 % 3 = 3 -> [3 1 0 2 4]
    assert s.draw() == [3, 1, 0]
    # not reset: i0: 0 + 1 % 5 -> [1 3 0 2 4]; i1: 1 + 1 % 4 = 2 -> [1 0 3 2 4]; i2: 2 + 1 % 3 = 3 -> [1 0 2 3 4]
    assert s.draw() == [1, 0, 2]


# ---- RULE good / coef ----
def test_sample_good_hand_cases():
    z = np.zeros(3, F)
    assert M.sample_good(z, F([1, 0, 0]), F([0, 1, 0]))
    assert not M.sample_good(z, F([1, 2, 4]), F([2, 4, 8]))  # exact multiples: every ratio 0.5
    # ratios NaN, NaN, 0.5: NaN != NaN, so PCL's test calls the collinear triple good
    assert M.sample_good(z, F([0, 0, 1]), F([0, 0, 2]))


def test_plane_coefficients_hand_cases():
    c = M.plane_of(F([0, 0, 2]), F([1, 0, 2]), F([0, 1, 2]))
    assert c.tolist() == [0.0, 0.0, 1.0, -2.0]
    c = M.plane_of(F([0, 0, 0]), F([0, 1, 0]), F([1, 0, 0]))
    assert c.tolist() == [0.0, 0.0, -1.0, 0.0]
    c = M.plane_of(F([1, 0, 0]), F([0, 1, 0]), F([0, 0, 1]))
    s = F(1) / F(np.sqrt(F(3)))
    assert np.allclose(c, [s, s, s, -s], atol=1e-7)
    xyz = np.array([[0, 0, 2], [0, 0, 2.015], [0, 0, 2.0149999], [5, 5, 1.99]], F)
    assert M.within([0, 0, 1, -2], xyz, 0.015).tolist() == [True, False, True, True]


# ---- RULE loop ----
def test_stop_rule_dominant_plane():
    it, best = M.ransac_stop([50] * 100, 100)
    k = math.log(0.01) / math.log(1 - 0.125)  # 34.48
    assert it == math.ceil(k) == 35 and best == 0


def test_stop_rule_max_plus_one_edge():
    assert M.ransac_stop([0] * 2000, 100, max_iterations=1000) == (1001, 0)  # w = 0: k ~ 4e16
    assert M.ransac_stop([1] * 10, 1000, max_iterations=5) == (6, 0)
    assert M.ransac_stop([0] * 10, 100, max_iterations=0) == (1, 0)


def test_stop_rule_better_model_and_empty_sample():
    it, best = M.ransac_stop([10, 20, 60, 5] + [1] * 50, 100)
    k = math.log(0.01) / math.log(1 - 0.6 ** 3)
    assert best == 2 and it == math.ceil(k)
    assert M.ransac_stop([10, 20, None, 30], 100) == (2, 1)
    assert M.ransac_stop([None], 100) == (0, -1)


# ---- RULE link / size / order ----
def test_pair_exactly_at_tolerance_is_not_connected():
    xyz = np.array([[0, 0, 0], [0.25, 0, 0], [1, 0, 0], [1.25 - 2 ** -12, 0, 0]], F)
    cl = M.clusters(xyz, 0.25, 1, 10)
    assert [c.tolist() for c in cl] == [[2, 3], [0], [1]]


def test_cluster_sizes_min_and_max_inclusive():
    rows = []
    for k, n in enumerate((3, 5, 2, 6)):
        rows += [[10.0 * k + 0.01 * j, 0, 0] for j in range(n)]
    cl = M.clusters(np.array(rows, F), 0.02, 3, 5)
    assert [len(c) for c in cl] == [5, 3]


def test_cluster_tie_order_by_smallest_index():
    rows = [[0, 0, 0], [5, 0, 0], [0.01, 0, 0], [5.01, 0, 0], [9, 0, 0], [9.01, 0, 0], [9.02, 0, 0]]
    cl = M.clusters(np.array(rows, F), 0.02, 1, 10)
    assert [c.tolist() for c in cl] == [[4, 5, 6], [0, 2], [1, 3]]


def test_refit_recovers_a_plane():
    rng = np.random.default_rng(3)
    xy = rng.uniform(-1, 1, (500, 2)).astype(F)
    xyz = np.concatenate([xy, (F(0.5) + F(0.1) * xy[:, :1]).astype(F)], 1).astype(F)
    c = M.refit(xyz, [0, 0, 1, -0.5])
    n = np.array([-0.1, 0, 1]) / np.linalg.norm([-0.1, 0, 1])
    assert abs(abs(float(np.dot(c[:3], n))) - 1) < 1e-5
    assert abs(float(c[3]) / float(np.sign(np.dot(c[:3], n))) + 0.5 * n[2]) < 1e-5


def test_model_pipeline_small_frame():
    fr = scene.make_depth_frame(96, 54)
    r = M.pipeline(fr, box_enable=(0, 0, 0), min_size=5)
    assert r["found"] and r["iterations"] >= 1 and len(r["samples"]) == r["iterations"]
    assert not np.isin(r["inliers"], np.concatenate(r["clusters"])).any()


# ---- the C ABI, the writer, the driver ----
def test_segment_config_defaults_are_the_reference_values():
    from pcl_tracking_amd import _lib

    L = _lib.load()
    c = _lib.SegmentConfig()
    L.pft_segment_default_config(C.byref(c))
    assert c.abi_version == _lib.PFT_ABI_VERSION and c.transform_enable == 0
    assert list(c.transform) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    # create_model_planar_segmentation.cpp:161-167, PCL defaults
    assert (c.plane_enable, c.max_iterations, c.distance_threshold) == (1, 1000, 0.015)
    assert (c.probability, c.seed, c.optimize_coefficients) == (0.99, 12345, 1)
    # params.yaml segm_limits ("normal table"); the planar node filters y and x
    assert list(c.box_enable) == [1, 1, 0]
    assert [round(v, 6) for v in c.box_min] == [0.45, -0.6, -0.17]
    assert [round(v, 6) for v in c.box_max] == [1.1, 0.6, 0.2]
    # :186-188
    assert (c.cluster_tolerance, c.min_cluster_size, c.max_cluster_size) == (0.02, 500, 25000)


def test_segment_create_refuses_bad_configs():
    from pcl_tracking_amd import _lib

    L = _lib.load()
    for field, bad in (("max_iterations", 1920), ("max_iterations", -1), ("cluster_tolerance", 0.0),
                       ("probability", 1.0), ("abi_version", 1)):
        c = _lib.SegmentConfig()
        L.pft_segment_default_config(C.byref(c))
        setattr(c, field, bad)
        h = C.c_void_p()
        assert L.pft_segment_create(C.byref(c), C.byref(h)) == 1 and not h.value


@pytest.mark.parametrize("mode", ["binary", "ascii"])
def test_pcd_writer_round_trips_through_the_reader(tmp_path, mode):
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "pcd_roundtrip_tool.cpp"), tmp_path / "rt")
    pts = scene.make_depth_frame(64, 36)
    pts["rgba"][:5] = [0, 1, 0xFFFFFFFF, 0x80000000, 12345]
    raw = tmp_path / "in.bin"
    pts.tofile(raw)
    r = subprocess.run([exe, str(raw), str(tmp_path / "out.pcd"), mode], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(len(pts))], (r.returncode, r.stdout, r.stderr)
    head = open(tmp_path / "out.pcd", "rb").read(400).decode("latin-1")
    assert "FIELDS x y z rgba" in head and "TYPE F F F U" in head and ("DATA %s" % mode) in head


def test_create_model_amd_compiles():
    from pcl_tracking_amd import build

    exe = build.build_create_model_example()
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr

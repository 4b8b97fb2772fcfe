"""Plane rounds and the tree-order refit, CPU side (no GPU): the library exports and binds the new symbols, the iterated
NumPy restatement (tests/segment_rounds_model.py) against its known answers on scene.make_scene(50000), the compare rule
at its boundary, the stop without a plane, and what the Python layer refuses.  The device is compared with the same
restatement in tests/test_gpu_segment_rounds.py."""
import numpy as np
import pytest

import segment_model as M
import segment_rounds_model as R
from report_model import tree_sum
from pcl_tracking_amd import scene

F = np.float32
NEW_SYMBOLS = ["pft_segment_set_plane_rounds", "pft_segment_get_plane_rounds", "pft_segment_plane_count",
               "pft_segment_get_plane_round", "pft_segment_get_plane_round_inliers", "pft_segment_set_refit_order",
               "pft_debug_segment_round_hypotheses"]


def test_library_exports_and_binds_the_new_symbols():
    from pcl_tracking_amd import build

    build.build()
    from pcl_tracking_amd import _lib

    L = _lib.load()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), "library does not export %s" % n
        assert n in bound, "ctypes binding missing for %s" % n
        assert getattr(L, n).argtypes == bound[n][1]
    assert _lib.SEGMENT_MAX_PLANES == 16
    assert (_lib.ROUNDS_STOP_FRACTION, _lib.ROUNDS_STOP_NO_PLANE, _lib.ROUNDS_STOP_MAX_PLANES) == (0, 1, 2)
    assert len(_lib.SEGMENT_STAGES) == 7  # the rounds add into the same stages


@pytest.mark.parametrize("order", ["pcl", "tree"])
def test_known_answers_on_the_50000_point_scene(order):
    """cluster_euclid.cpp's values: 100 iterations, 0.02 m, 30 %, clusters at 0.02 m with 10 .. 2 500 points"""
    r = R.pipeline(scene.make_scene(50000), max_planes=16, fraction=0.3, order=order, max_iterations=100,
                   threshold=0.02, tol=0.02, min_size=10, max_size=2500)
    assert r["n_valid"] == 50000
    assert [len(x["inliers"]) for x in r["rounds"]] == [31856, 17080]  # the wall, then the table
    assert r["n_planes"] == 2 and r["stopped_by"] == R.STOP_FRACTION
    assert r["remaining"] == 1064 and len(r["survivors"]) == 1064
    assert [len(c) for c in r["clusters"]] == [411, 328, 196, 58, 58]
    assert r["rounds"][0]["n_valid"] == 50000 and r["rounds"][1]["n_valid"] == 50000 - 31856
    for x in r["rounds"]:
        assert np.all(np.diff(x["inliers"]) > 0) and len(x["near"]) == 0


def test_one_plane_only_leaves_the_table_in_the_cloud():
    r = R.pipeline(scene.make_scene(50000), max_planes=1, fraction=0.3)
    assert r["n_planes"] == 1 and r["stopped_by"] == R.STOP_MAX_PLANES and r["remaining"] == 18144


def test_the_two_orders_are_two_specifications():
    """same inliers on this scene, coefficients that differ in the fourth digit: each order has its own model"""
    c = scene.make_scene(50000)
    a = R.pipeline(c, order="pcl")["rounds"]
    b = R.pipeline(c, order="tree")["rounds"]
    d = max(np.abs(x["coefficients"] - y["coefficients"]).max() for x, y in zip(a, b))
    assert 1e-6 < d < 1e-3
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x["ransac_coefficients"], y["ransac_coefficients"])
        np.testing.assert_array_equal(x["inliers"], y["inliers"])


def test_tree_refit_sums_are_tree_sums():
    rng = np.random.default_rng(3)
    xyz = (rng.normal(0, 1, (1000, 3)) * [1, 1, 0.001] + [0.3, -0.2, 1.5]).astype(F)
    c = R.refit(xyz, np.array([0, 0, 1, -1.5], F), "tree")
    ref = np.linalg.eigh(np.cov(xyz.astype(np.float64).T))[1][:, 0]
    assert abs(abs(float(np.dot(c[:3], ref))) - 1.0) < 1e-5
    # -0.0 padding: the padding length does not change a bit
    v = rng.normal(0, 1, 777).astype(F)
    assert tree_sum(v) == tree_sum(np.r_[v, np.full(247 + 1024, F(-0.0))])
    np.testing.assert_array_equal(R.refit(xyz[:3], np.array([1, 2, 3, 4], F), "tree"), [1, 2, 3, 4])  # fewer than 4


def _plane_and_strays(n_plane, n_stray):
    g = np.arange(n_plane)
    plane = np.c_[(g % 4) * 0.25, (g // 4) * 0.25, np.ones(n_plane)]  # exact floats on z = 1
    rng = np.random.default_rng(1)
    stray = rng.uniform(-1, 1, (n_stray, 3)) * [1, 1, 0.3] + [0, 0, 3.0]
    xyz = np.r_[plane, stray].astype(F)
    return scene.make_points(xyz, np.zeros((len(xyz), 3)))


def test_compare_rule_at_the_boundary():
    """remaining == fraction * nr exactly: `>` is false, no further round runs (0.5 * 20 == 10.0 in double)"""
    assert not R.another_round(10, 20, 0.5) and R.another_round(11, 20, 0.5)
    assert not R.another_round(3, 10, 0.3) and R.another_round(4, 10, 0.3)  # the double product 0.3 * 10 is 3.0
    assert not R.another_round(15000, 50000, 0.3) and R.another_round(15001, 50000, 0.3)
    assert not R.another_round(0, 0, 0.0) and R.another_round(1, 50000, 0.0)
    cloud = _plane_and_strays(10, 10)
    r = R.pipeline(cloud, fraction=0.5, threshold=0.015)
    assert [len(x["inliers"]) for x in r["rounds"]] == [10]
    assert r["remaining"] == 10 and r["n_planes"] == 1 and r["stopped_by"] == R.STOP_FRACTION
    r = R.pipeline(cloud, fraction=0.49, threshold=0.015)  # just below the boundary: another round runs
    assert len(r["rounds"]) >= 2


def test_stop_without_a_plane_with_fewer_than_three_points_left():
    cloud = _plane_and_strays(12, 2)
    r = R.pipeline(cloud, fraction=0.0, threshold=0.015)
    assert [len(x.get("inliers", [])) for x in r["rounds"]] == [12, 0]
    assert not r["rounds"][1]["found"] and r["rounds"][1]["iterations"] == 0 and r["rounds"][1]["n_valid"] == 2
    assert r["n_planes"] == 1 and r["stopped_by"] == R.STOP_NO_PLANE and r["remaining"] == 2
    np.testing.assert_array_equal(r["survivors"], [12, 13])  # the remaining cloud is unchanged


def test_max_planes_is_reported():
    r = R.pipeline(scene.make_scene(50000), max_planes=2, fraction=0.01)
    assert r["n_planes"] == 2 and r["stopped_by"] == R.STOP_MAX_PLANES and r["remaining"] == 1064


def test_single_round_equals_the_single_plane_model():
    cloud = scene.make_depth_frame(160, 90)
    a = M.pipeline(cloud, box_enable=(0, 0, 0), min_size=50)
    b = R.pipeline(cloud, max_planes=1, fraction=0.0, max_iterations=1000, threshold=0.015, min_size=50, max_size=25000)
    assert a["samples"] == b["rounds"][0]["samples"] and a["counts"] == b["rounds"][0]["counts"]
    np.testing.assert_array_equal(a["inliers"], b["rounds"][0]["inliers"])
    np.testing.assert_array_equal(a["coefficients"], b["rounds"][0]["coefficients"])
    assert len(a["clusters"]) == len(b["clusters"])
    for x, y in zip(a["clusters"], b["clusters"]):
        np.testing.assert_array_equal(x, y)


def test_python_layer_refuses_bad_rounds_and_orders():
    from pcl_tracking_amd import build

    build.build()
    from pcl_tracking_amd import _lib, segment

    s = segment.ModelSegmenter()
    for bad in ((0, 0.3), (17, 0.3), (2, -0.1), (2, 1.5), (2, float("nan"))):
        with pytest.raises(_lib.PftError):
            s.configure(plane_rounds=bad)
    with pytest.raises(_lib.PftError):
        s.configure(refit_order="double")
    m = segment.make_scene_segmenter()
    c = m.config
    assert (c.max_iterations, c.distance_threshold, list(c.box_enable)) == (100, 0.02, [0, 0, 0])
    assert (c.cluster_tolerance, c.min_cluster_size, c.max_cluster_size) == (0.02, 10, 2500)
    assert m._rounds == (16, 0.3)

"""Plane rounds and the tree-order refit on the device (include/pft_segment.h) against the iterated NumPy restatement
(tests/segment_rounds_model.py), each refit order against the model of the SAME order.  Per round the bounds are those
of tests/test_gpu_segment.py::_check_against_model: sample stream and every scored count exact, pre-refit inliers exact,
coefficients within 1e-5 on the normal and 1e-6 on d, final inliers exact except for points within 1e-6 of the
threshold.  A near-threshold point in round k would change round k + 1 wholesale, so the round tests first assert that
the model reports no such point in any round but (where stated) the last, and then demand every round and every cluster
exactly.  PARITY UNPINNED: PCL is not available, the model restates it.

Tree sums at 1 inlier: a hypothesis always holds its own three sample points, so the smallest inlier list an apply can
produce has 3 entries (below 4: the coefficients stay, as at 1); the sizes run are 3, 4, 8 191, 8 192, 8 193, 300 000."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import segment_rounds_model as R
from pcl_tracking_amd import _lib, scene, segment

pytestmark = pytest.mark.gpu
F = np.float32
# seeds of _planes_scene whose model has no point within 1e-5 of the threshold in any round, in either order
# (0, 2, 28 and 30 have one or two and are left out)
SMALL_SEEDS = [1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21]
SMALL_KW = dict(max_iterations=300, threshold=0.015, tol=0.03, min_size=10, max_size=500)


def _seg(order="pcl", rounds=(16, 0.3), max_iterations=100, threshold=0.02, tol=0.02, min_size=10, max_size=2500):
    s = segment.make_scene_segmenter()
    s.configure(plane_rounds=rounds, refit_order=order, max_iterations=max_iterations, distance_threshold=threshold,
                tolerance=tol, min_size=min_size, max_size=max_size)
    return s


def _model(cloud, order="pcl", rounds=(16, 0.3), **kw):
    return R.pipeline(cloud, max_planes=rounds[0], fraction=rounds[1], order=order, **kw)


@functools.lru_cache(maxsize=None)
def _scene_model(order, max_iterations, threshold, rounds=(16, 0.3)):
    return _model(scene.make_scene(50000), order, rounds, max_iterations=max_iterations, threshold=threshold,
                  near_eps=1e-5)


def _check_rounds(s, r, allow_near_in_last=False):
    """every round against the model's; -> the number of near-threshold points of the last round"""
    assert s.planeCount() == r["n_planes"] and s.stoppedBy() == r["stopped_by"]
    assert s.plane()["n_valid"] == r["n_valid"] or not r["rounds"]
    n_near = 0
    for k, m in enumerate(r["rounds"]):
        last = k == len(r["rounds"]) - 1
        if not (allow_near_in_last and last):
            assert len(m["near"]) == 0, "condition of the test: no point near the threshold in round %d" % k
        pl = s.plane(k)
        assert pl["n_valid"] == m["n_valid"]
        smp, cnt = s.hypotheses(k)
        assert pl["iterations"] == m["iterations"] == len(smp)
        assert smp.tolist() == [list(v) for v in m["samples"]]  # the round's sample stream, in draw order
        assert cnt.tolist() == m["counts"]                     # every scored count
        assert (pl["status"] == _lib.PLANE_FOUND) == m["found"]
        if not m["found"]:
            assert len(s.planeInliers(0, k)) == 0
            continue
        assert pl["sample"] == list(m["sample"])
        np.testing.assert_array_equal(pl["ransac_coefficients"], m["ransac_coefficients"])
        np.testing.assert_array_equal(s.planeInliers(1, k), m["ransac_inliers"])  # pre-refit inliers, exactly
        assert np.abs(pl["coefficients"][:3] - m["coefficients"][:3]).max() <= 1e-5
        assert abs(float(pl["coefficients"][3]) - float(m["coefficients"][3])) <= 1e-6
        got = s.planeInliers(0, k)
        assert np.all(np.diff(got) > 0)
        diff = np.setxor1d(got, m["inliers"])
        assert np.isin(diff, m["near"]).all(), (k, len(diff), len(m["near"]))
        assert pl["inliers"] == len(got)
        n_near = len(m["near"])
    return n_near


def _check_clusters(s, r, cloud):
    assert s.plane()["n_survivors"] == len(r["survivors"])
    got = s.clusters()
    assert len(got) == len(r["clusters"])
    for (idx, pts), want in zip(got, r["clusters"]):
        np.testing.assert_array_equal(idx, want)
        assert pts.tobytes() == cloud[idx].tobytes()  # the sensor's own bits


@pytest.mark.parametrize("order", ["pcl", "tree"])
@pytest.mark.parametrize("max_iterations,threshold", [(100, 0.02), (1000, 0.015)])
def test_scene_50000(order, max_iterations, threshold):
    cloud = scene.make_scene(50000)
    r = _scene_model(order, max_iterations, threshold)
    s = _seg(order, max_iterations=max_iterations, threshold=threshold)
    s.setInputCloud(cloud)
    s.apply()
    _check_rounds(s, r)
    _check_clusters(s, r, cloud)
    assert s.planeCount() == 2 and s.stoppedBy() == _lib.ROUNDS_STOP_FRACTION
    if (max_iterations, threshold) == (100, 0.02):
        assert [s.plane(k)["inliers"] for k in range(2)] == [31856, 17080]
        assert s.plane()["n_survivors"] == 1064 and s.clusterSizes().tolist() == [411, 328, 196, 58, 58]


@pytest.mark.parametrize("order,rounds", [("pcl", (16, 0.3)), ("tree", (1, 0.3))])
def test_qhd_frame(order, rounds):
    """PCL order: the model has 6 points within 1e-6 of the threshold in round 2, its last, and none in round 1: the
    existing allowance applies to the last round only.  Tree order: the model has one such point in round 1, so that
    order is run with one round, which is then the last."""
    cloud = scene.make_depth_frame()
    r = _model(cloud, order, rounds, max_size=10 ** 6)
    s = _seg(order, rounds, max_size=10 ** 6)
    s.setInputCloud(cloud)
    s.apply()
    n_near = _check_rounds(s, r, allow_near_in_last=True)
    print("qhd %s: %d rounds, %d points within 1e-6 of the threshold in the last" % (order, len(r["rounds"]), n_near))
    if not n_near:
        _check_clusters(s, r, cloud)
    if order == "pcl":
        assert s.planeCount() == 2 and s.stoppedBy() == _lib.ROUNDS_STOP_FRACTION
    else:
        assert s.planeCount() == 1 and s.stoppedBy() == _lib.ROUNDS_STOP_MAX_PLANES


def _planes_scene(seed):
    """two or three tilted planes 0.45 m apart, blobs and scattered points, shuffled, 2 % NaN: built like
    test_gpu_segment._blob_scene"""
    rng = np.random.default_rng(1000 + seed)
    parts = []
    for k in range(int(rng.integers(2, 4))):
        n0 = int(rng.integers(600, 2500))
        xy = rng.uniform(-1, 1, (n0, 2))
        tilt = rng.uniform(-0.3, 0.3, 2)
        parts.append(np.c_[xy, 1.0 + 0.45 * k + xy @ tilt + rng.normal(0, 0.003, n0)])
    for _ in range(int(rng.integers(1, 5))):
        cc = rng.uniform(-0.8, 0.8, 3) + [0, 0, 0.6]
        m = int(rng.integers(20, 300))
        parts.append(cc + rng.normal(0, 0.02, (m, 3)))
    parts.append(rng.uniform(-1, 1, (int(rng.integers(0, 150)), 3)) + [0, 0, 1.5])
    xyz = np.concatenate(parts).astype(F)
    xyz = xyz[rng.permutation(len(xyz))]
    pts = scene.make_points(xyz, rng.integers(0, 255, (len(xyz), 3)))
    pts["x"][rng.random(len(pts)) < 0.02] = np.nan
    return pts


@pytest.mark.parametrize("seed", SMALL_SEEDS)
def test_small_seeded_scenes(seed):
    cloud = _planes_scene(seed)
    for order in ("pcl", "tree"):
        r = _model(cloud, order, (16, 0.1), near_eps=1e-5, **SMALL_KW)
        assert 2 <= r["n_planes"] <= 5
        s = _seg(order, (16, 0.1), **SMALL_KW)
        s.setInputCloud(cloud)
        s.apply()
        _check_rounds(s, r)
        _check_clusters(s, r, cloud)


def test_max_planes_reached_is_reported():
    cloud = scene.make_scene(50000)
    for rounds in ((1, 0.3), (2, 0.01)):
        r = _scene_model("pcl", 100, 0.02, rounds)
        assert r["stopped_by"] == R.STOP_MAX_PLANES
        s = _seg("pcl", rounds)
        s.setInputCloud(cloud)
        s.apply()
        _check_rounds(s, r)
        _check_clusters(s, r, cloud)
        assert s.stoppedBy() == _lib.ROUNDS_STOP_MAX_PLANES and s.planeCount() == rounds[0]
    assert s.plane()["n_survivors"] == 1064  # (2, 0.01): both planes gone, 2 % left > 1 %


def test_stop_without_a_plane():
    g = np.arange(12)
    xyz = np.r_[np.c_[(g % 4) * 0.25, (g // 4) * 0.25, np.ones(12)], [[0.3, 0.1, 3.0], [-0.4, 0.2, 2.7]]].astype(F)
    cloud = scene.make_points(xyz, np.zeros((len(xyz), 3)))
    r = _model(cloud, "pcl", (16, 0.0), threshold=0.015, min_size=1)
    assert r["stopped_by"] == R.STOP_NO_PLANE and len(r["rounds"]) == 2
    s = _seg("pcl", (16, 0.0), threshold=0.015, min_size=1)
    s.setInputCloud(cloud)
    s.apply()
    _check_rounds(s, r)
    _check_clusters(s, r, cloud)
    assert s.plane(1)["status"] == _lib.PLANE_NONE and s.plane(1)["n_valid"] == 2 and s.plane()["n_survivors"] == 2
    # the boundary of the compare rule: 10 of 20 left at fraction 0.5 is not "more than"
    xyz = np.r_[xyz[:10], np.random.default_rng(1).uniform(-1, 1, (10, 3)) * [1, 1, 0.3] + [0, 0, 3.0]].astype(F)
    cloud = scene.make_points(xyz, np.zeros((len(xyz), 3)))
    r = _model(cloud, "pcl", (16, 0.5), threshold=0.015, min_size=1)
    assert len(r["rounds"]) == 1 and r["remaining"] == 10 and r["stopped_by"] == R.STOP_FRACTION
    s = _seg("pcl", (16, 0.5), threshold=0.015, min_size=1)
    s.setInputCloud(cloud)
    s.apply()
    _check_rounds(s, r)
    assert s.planeCount() == 1 and s.stoppedBy() == _lib.ROUNDS_STOP_FRACTION


def _raw_results(L, h, cloud):
    """everything a handle reports after one apply, through the C ABI alone"""
    assert L.pft_segment_apply(h, cloud.ctypes.data_as(C.c_void_p), len(cloud)) == 0
    pl = _lib.SegmentPlane()
    assert L.pft_segment_get_plane(h, C.byref(pl)) == 0
    out = [bytes(pl)]
    n = C.c_size_t()
    for which, cnt in ((0, pl.inliers), (1, pl.ransac_inliers)):
        idx = np.zeros(cnt, np.int32)
        assert L.pft_segment_get_plane_inliers(h, which, idx.ctypes.data_as(C.c_void_p), cnt, C.byref(n)) == 0
        out.append(idx[: n.value].tobytes())
    assert L.pft_segment_cluster_count(h, C.byref(n)) == 0
    sizes = np.zeros(n.value, np.uint32)
    assert L.pft_segment_cluster_sizes(h, sizes.ctypes.data_as(C.c_void_p), n.value) == 0
    total = int(sizes.sum())
    idx, pts = np.zeros(total, np.int32), np.zeros(total, scene.POINT_DTYPE)
    assert L.pft_segment_get_cluster_indices(h, idx.ctypes.data_as(C.c_void_p), total, C.byref(n)) == 0
    assert L.pft_segment_get_cluster_points(h, pts.ctypes.data_as(C.c_void_p), total, C.byref(n)) == 0
    smp, cnt = np.zeros((pl.iterations, 3), np.int32), np.zeros(pl.iterations, np.uint32)
    assert L.pft_debug_segment_hypotheses(h, smp.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
                                          pl.iterations, C.byref(n)) == 0
    return out + [sizes.tobytes(), idx.tobytes(), pts.tobytes(), smp.tobytes(), cnt.tobytes()]


def test_defaults_are_byte_identical_to_a_handle_that_never_called_the_setters():
    L = _lib.load()
    cloud = scene.make_depth_frame(480, 270)
    cfg = _lib.SegmentConfig()
    L.pft_segment_default_config(C.byref(cfg))
    cfg.box_min = (C.c_float * 3)(-0.4, -0.45, 0.4)
    cfg.box_max = (C.c_float * 3)(0.6, 0.35, 1.4)
    cfg.box_enable = (C.c_int32 * 3)(1, 1, 1)
    res = []
    for setters in (False, True, "rounds_of_one"):
        h = C.c_void_p()
        assert L.pft_segment_create(C.byref(cfg), C.byref(h)) == 0
        mx, fr = C.c_int(-1), C.c_double(-1.0)
        assert L.pft_segment_get_plane_rounds(h, C.byref(mx), C.byref(fr)) == 0 and (mx.value, fr.value) == (1, 0.0)
        if setters is True:
            assert L.pft_segment_set_plane_rounds(h, 1, 0.0) == 0
            assert L.pft_segment_set_refit_order(h, _lib.PFT_SUM_PCL) == 0
        elif setters:  # the round loop with one round: the same results by the other path
            assert L.pft_segment_set_plane_rounds(h, 1, 2.0 ** -40) == 0
        res.append(_raw_results(L, h, cloud))
        np_, why = C.c_size_t(), C.c_int()
        assert L.pft_segment_plane_count(h, C.byref(np_), C.byref(why)) == 0
        assert (np_.value, why.value) == (1, _lib.ROUNDS_STOP_MAX_PLANES)
        L.pft_segment_destroy(h)
    assert len(res[0][4]) > 0 and len(res[0][1]) > 0
    assert res[0] == res[1]
    assert res[0] == res[2]


def _flat_cloud(m, seed=0):
    """m points on z = 1 exactly (every good sample of them gives the same plane and all m as inliers) plus strays"""
    rng = np.random.default_rng(seed)
    xyz = np.r_[np.c_[rng.uniform(-1, 1, (m, 2)), np.ones(m)], rng.uniform(-1, 1, (40 if m > 4 else 0, 3)) * 0.2 +
                [0, 0, 2.0]].astype(F)
    return scene.make_points(xyz[rng.permutation(len(xyz))], np.zeros((len(xyz), 3)))


@pytest.mark.parametrize("m", [3, 4, 8191, 8192, 8193, 300000])
def test_tree_order_sums(m, monkeypatch):
    """inlier lists around the tile size of the tile launch (2 048), its multiple 8 192, and qhd scale; the coefficients
    are bit-identical under three grid sizes of the tile launch (every level is an aligned subtree)"""
    cloud = _flat_cloud(m)
    r = _model(cloud, "tree", (1, 0.0), max_iterations=50, threshold=0.02, min_size=1)
    assert len(r["rounds"][0]["ransac_inliers"]) == m
    got = []
    for grid in (None, "1", "7"):
        if grid is None:
            monkeypatch.delenv("PFT_SEGMENT_REFIT_GRID", raising=False)
        else:
            monkeypatch.setenv("PFT_SEGMENT_REFIT_GRID", grid)
        for rounds in ((1, 0.0), (2, 0.0)):  # the single plane and the round loop launch the same refit
            s = _seg("tree", rounds, max_iterations=50, min_size=1)
            s.setInputCloud(cloud)
            s.apply()
            pl = s.plane()
            assert pl["ransac_inliers"] == m
            got.append(pl["coefficients"].tobytes())
            if grid is None and rounds == (1, 0.0):
                _check_rounds(s, r)
    assert len(set(got)) == 1
    if m < 4:
        np.testing.assert_array_equal(s.plane()["coefficients"], s.plane()["ransac_coefficients"])


def test_apply_device_equals_apply_and_no_stale_round():
    import torch

    a = scene.make_scene(50000)
    b = _planes_scene(11)  # two rounds at (16, 0.1); one at (1, 0.1)
    s = _seg("tree", (16, 0.3))
    s.setInputCloud(a)
    s.apply()

    def snap(s):
        n = max(s.planeCount(), 1)
        return ([s.plane(k) for k in range(n)], [s.planeInliers(w, k).tobytes() for k in range(n) for w in (0, 1)],
                [h.tobytes() for k in range(n) for h in s.hypotheses(k)], [i.tobytes() for i, _ in s.clusters()],
                s.planeCount(), s.stoppedBy())

    def same(x, y):
        assert x[1:] == y[1:]
        for p, q in zip(x[0], y[0]):
            assert all(np.array_equal(p[k], q[k]) for k in p)

    ref = snap(s)
    assert ref[4] == 2
    dev = torch.from_numpy(a.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    s.setInputCloudDevice(dev.data_ptr(), len(a), dev)
    s.apply()
    same(snap(s), ref)
    # a second apply with fewer rounds: no round of the first is left behind
    L = _lib.load()
    assert L.pft_segment_set_plane_rounds(s._h, 1, 0.3) == 0
    s.setInputCloud(b)
    s.apply()
    fresh = _seg("tree", (1, 0.3))
    fresh.setInputCloud(b)
    fresh.apply()
    same(snap(s), snap(fresh))
    assert s.planeCount() == 1
    pl = _lib.SegmentPlane()
    n = C.c_size_t()
    assert L.pft_segment_get_plane_round(s._h, 1, C.byref(pl)) == 1
    assert b"round" in L.pft_segment_last_error_string(s._h)
    assert L.pft_segment_get_plane_round_inliers(s._h, 1, 0, None, 0, C.byref(n)) == 1
    assert L.pft_debug_segment_round_hypotheses(s._h, 1, None, None, 0, C.byref(n)) == 1
    assert L.pft_segment_set_plane_rounds(s._h, 16, 0.3) == 0
    s.setInputCloud(a)
    s.apply()
    same(snap(s), ref)


def test_refusals():
    L = _lib.load()
    s = segment.ModelSegmenter()
    s._ensure()
    h = s._h
    for mx, fr, word in ((0, 0.3, b"max_planes"), (17, 0.3, b"max_planes"), (-1, 0.3, b"max_planes"),
                         (2, -0.01, b"min_remaining_fraction"), (2, 1.01, b"min_remaining_fraction"),
                         (2, float("nan"), b"min_remaining_fraction")):
        assert L.pft_segment_set_plane_rounds(h, mx, fr) == 1  # PFT_ERR_INVALID_ARG
        assert word in L.pft_segment_last_error_string(h)
    mx, fr = C.c_int(), C.c_double()
    assert L.pft_segment_get_plane_rounds(h, C.byref(mx), C.byref(fr)) == 0 and (mx.value, fr.value) == (1, 0.0)
    for order in (-1, 2, 7):
        assert L.pft_segment_set_refit_order(h, order) == 1
        assert b"order" in L.pft_segment_last_error_string(h)
    n, why = C.c_size_t(), C.c_int()
    assert L.pft_segment_plane_count(h, C.byref(n), C.byref(why)) == 7  # PFT_ERR_STATE: no apply yet
    assert L.pft_segment_get_plane_round(h, 0, C.byref(_lib.SegmentPlane())) == 7
    assert L.pft_segment_set_plane_rounds(None, 2, 0.3) == 1 and L.pft_segment_set_refit_order(None, 0) == 1
    assert L.pft_segment_set_plane_rounds(h, 16, 1.0) == 0 and L.pft_segment_set_plane_rounds(h, 1, 0.0) == 0
    # plane_enable = 0: no round runs
    s = _seg("pcl", (16, 0.3))
    s.configure(plane=False)
    cloud = _planes_scene(11)
    s.setInputCloud(cloud)
    s.apply()
    assert s.planeCount() == 0 and s.plane()["status"] == _lib.PLANE_DISABLED
    assert s.plane()["n_survivors"] == s.plane()["n_valid"]


def _read_pcd_binary(path):
    data = open(path, "rb").read()
    end = data.index(b"DATA binary\n") + len(b"DATA binary\n")
    return np.frombuffer(data[end:], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])


def test_create_model_voxel_planes_then_track(tmp_path):
    """cluster_euclid.cpp end to end through the driver: --voxel 0.01 (VoxelGrid on the device, its output handed over
    on the device), --planes 16,0.3 --sac 100,0.02, no box; the object's cluster then feeds auto_tracking_amd.  The
    bound on the tracked centroid is test_gpu_segment.py::test_create_model_then_track's 4 cm."""
    from pcl_tracking_amd import build

    exe = build.build_create_model_example()
    trk = build.build_example()
    frame0 = scene.make_depth_frame(480, 270)
    raw = tmp_path / "scene.bin"
    frame0.tofile(raw)
    out = tmp_path / "models"
    out.mkdir()
    r = subprocess.run([exe, str(raw), "--out", str(out), "--voxel", "0.01", "--planes", "16,0.3", "--sac", "100,0.02",
                        "--box", "-100,100,-100,100,-100,100", "--tolerance", "0.02", "--min-size", "100",
                        "--max-size", "25000", "--tree-refit"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    planes = [l.split() for l in lines if l.startswith("plane ")]
    summary = [l.split() for l in lines if l.startswith("planes ")]
    assert len(planes) >= 2 and summary == [["planes", str(len(planes)), "stopped-by", "fraction"]]
    assert all(int(p[8]) > 1000 for p in planes)  # inliers of every removed plane
    sizes = [int(l.split()[3]) for l in lines if l.startswith("cluster ")]
    assert sizes and all(100 <= v <= 25000 for v in sizes)
    T = scene.pose_matrix(*scene.GT_POSE)
    h = np.asarray(scene.MODEL_DIMS) / 2 + 0.015
    best, best_frac, best_pts = None, 0.0, None
    for j in range(len(sizes)):
        pts = _read_pcd_binary(out / ("%d.pcd" % j))
        xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(np.float64)
        loc = (xyz - T[:3, 3]) @ T[:3, :3]
        frac = float(np.mean(np.all(np.abs(loc) <= h, axis=1)))
        if frac > best_frac:
            best, best_frac, best_pts = j, frac, xyz
    assert best_frac >= 0.95, best_frac  # the object is a cluster of its own: both planes are gone without a box
    frames = []
    for f in range(1, 4):
        pose = scene.advance_pose(scene.GT_POSE, f)
        p = tmp_path / ("f%d.bin" % f)
        scene.make_depth_frame(480, 270, obj_pose=pose).tofile(p)
        frames.append((p, pose))
    r = subprocess.run([trk, str(out / ("%d.pcd" % best)), "--frames"] + [str(p) for p, _ in frames] + ["--raw"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cents = [np.array(list(map(float, l.split()[12:15]))) for l in r.stdout.splitlines() if l.startswith("frame")]
    assert len(cents) == len(frames)
    loc = np.linalg.solve(T[:3, :3], best_pts.mean(axis=0) - T[:3, 3])
    errs = []
    for c, (_, pose) in zip(cents, frames):
        Tf = scene.pose_matrix(*pose)
        errs.append(float(np.linalg.norm(c - (Tf[:3, :3] @ loc + Tf[:3, 3] + np.array([0.0, 0.0, -0.005])))))
    print("centroid errors (m):", [round(e, 4) for e in errs])
    assert max(errs) < 0.04, errs

"""Model creation on the device (include/pft_segment.h) against the NumPy restatement of the recalled PCL 1.8.0 rules
(tests/segment_model.py): the RANSAC sample stream, every scored count, the stop, the refit, the compactions and the
clusters; degenerate inputs; handle state; and create_model_amd feeding auto_tracking_amd.  PARITY UNPINNED: PCL is not
available, the model restates it."""
import os
import subprocess

import numpy as np
import pytest

import segment_model as M
from pcl_tracking_amd import _lib, scene, segment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
OBJ_BOX = (-0.4, 0.6, -0.45, 0.35, 0.4, 1.4)  # camera frame: the object, part of the table and clutter


def _seg(plane=True, box=OBJ_BOX, box_enable=(1, 1, 1), **kw):
    s = segment.ModelSegmenter()
    s.configure(plane=plane, box=box, box_enable=box_enable, **kw)
    return s


def _model(cloud, plane=True, box=OBJ_BOX, box_enable=(1, 1, 1), tol=0.02, min_size=500, max_size=25000, **kw):
    return M.pipeline(cloud, plane=plane, box_enable=box_enable, box_lo=box[0::2], box_hi=box[1::2], tol=tol,
                      min_size=min_size, max_size=max_size, **kw)


def _near(cloud, r, thr=0.015, eps=1e-6):
    """input indices of points within eps of the distance threshold of the final plane"""
    if not r["found"]:
        return np.zeros(0, np.int64)
    valid = np.flatnonzero(M.keep_nonzero(r["xyz"]))
    d = r["dist_final"].astype(np.float64)
    return valid[np.abs(d - thr) < eps]


def _check_against_model(s, cloud, r, exact_clusters=True):
    pl = s.plane()
    assert pl["n_valid"] == r["n_valid"]
    if pl["status"] == _lib.PLANE_DISABLED:
        assert not r["samples"]
    else:
        smp, cnt = s.hypotheses()
        assert pl["iterations"] == r["iterations"] == len(smp)
        assert smp.tolist() == [list(v) for v in r["samples"]]  # the sample stream, in draw order
        assert cnt.tolist() == r["counts"]                     # every scored count
        assert (pl["status"] == _lib.PLANE_FOUND) == r["found"]
    near = _near(cloud, r)
    if r["found"]:
        assert pl["sample"] == list(r["sample"])
        np.testing.assert_array_equal(pl["ransac_coefficients"], r["ransac_coefficients"])
        np.testing.assert_array_equal(s.planeInliers(1), r["ransac_inliers"])  # pre-refit inliers, exactly
        assert np.abs(pl["coefficients"][:3] - r["coefficients"][:3]).max() <= 1e-5
        assert abs(float(pl["coefficients"][3]) - float(r["coefficients"][3])) <= 1e-6
        got = s.planeInliers(0)
        diff = np.setxor1d(got, r["inliers"])
        assert np.isin(diff, near).all(), (len(diff), len(near))
    got_cl = [idx for idx, _ in s.clusters()]
    if exact_clusters or not len(near):
        assert len(got_cl) == len(r["clusters"])
        for a, b in zip(got_cl, r["clusters"]):
            np.testing.assert_array_equal(a, b)
    return len(near)


def _points_equal_input(s, cloud):
    for idx, pts in s.clusters():
        assert np.all(np.diff(idx) > 0)
        assert pts.tobytes() == cloud[idx].tobytes()  # the sensor's own bits


@pytest.mark.parametrize("plane", [True, False])
def test_qhd_frame_whole_pipeline(plane):
    cloud = scene.make_depth_frame()  # 960 x 540 = 518 400 points, NaN holes
    s = _seg(plane=plane, max_size=10 ** 6)
    s.setInputCloud(cloud)
    s.apply()
    r = _model(cloud, plane=plane, max_size=10 ** 6)
    n_near = _check_against_model(s, cloud, r)
    print("qhd plane=%s: %d points within 1e-6 of the threshold (expected 0)" % (plane, n_near))
    _points_equal_input(s, cloud)
    if plane:
        assert s.plane()["iterations"] < 200  # a dominant plane stops early


def _blob_scene(seed):
    rng = np.random.default_rng(seed)
    parts = []
    n0 = int(rng.integers(800, 3000))
    xy = rng.uniform(-1, 1, (n0, 2))
    tilt = rng.uniform(-0.3, 0.3, 2)
    parts.append(np.c_[xy, 1.0 + xy @ tilt + rng.normal(0, 0.003, n0)])
    for _ in range(int(rng.integers(1, 5))):
        c = rng.uniform(-0.8, 0.8, 3) + [0, 0, 1.3]
        m = int(rng.integers(20, 400))
        parts.append(c + rng.normal(0, 0.02, (m, 3)))
    parts.append(rng.uniform(-1, 1, (int(rng.integers(0, 200)), 3)) + [0, 0, 1])
    xyz = np.concatenate(parts).astype(F)
    xyz = xyz[rng.permutation(len(xyz))]
    pts = scene.make_points(xyz, rng.integers(0, 255, (len(xyz), 3)))
    pts["x"][rng.random(len(pts)) < 0.02] = np.nan
    return pts


@pytest.mark.parametrize("seed", range(20))
def test_small_seeded_scenes(seed):
    cloud = _blob_scene(seed)
    kw = dict(tol=0.03, min_size=10, max_size=500, max_iterations=300 + 50 * seed)
    s = _seg(box_enable=(0, 0, 0), tolerance=kw["tol"], min_size=kw["min_size"], max_size=kw["max_size"],
             max_iterations=kw["max_iterations"])
    s.setInputCloud(cloud)
    s.apply()
    r = _model(cloud, box_enable=(0, 0, 0), **kw)
    _check_against_model(s, cloud, r, exact_clusters=False)
    _points_equal_input(s, cloud)


def test_clusters_at_exact_tolerance_spacing():
    # tolerance 0.25 and coordinates that are multiples of 2^-4: squared distances are exact in float
    rows = []
    for k in range(4):
        for j in range(8):
            step = 0.25 if k % 2 else 0.25 - 2 ** -6  # at the tolerance: no link; just below: one chain
            rows.append([3.0 * k + step * j, 1.0, 2.0])
    cloud = scene.make_points(np.array(rows, F), np.zeros((len(rows), 3)))
    s = _seg(plane=False, box_enable=(0, 0, 0), tolerance=0.25, min_size=1, max_size=100)
    s.setInputCloud(cloud)
    s.apply()
    r = _model(cloud, plane=False, box_enable=(0, 0, 0), tol=0.25, min_size=1, max_size=100)
    got = [idx.tolist() for idx, _ in s.clusters()]
    assert got == [c.tolist() for c in r["clusters"]]
    assert [len(c) for c in got] == [8, 8] + [1] * 16


@pytest.mark.parametrize("case", ["empty", "all_nan", "two_points", "collinear", "box_removes_all"])
def test_degenerate_inputs(case):
    s = _seg(box_enable=(0, 0, 0), min_size=1)
    if case == "empty":
        cloud = np.zeros(0, scene.POINT_DTYPE)
    elif case == "all_nan":
        cloud = scene.make_depth_frame(32, 18)
        cloud["z"] = np.nan
    elif case == "two_points":
        cloud = scene.make_points(np.array([[1, 0, 1], [1, 0, 1.01]], F), np.zeros((2, 3)))
    elif case == "collinear":  # (t, 2t, 4t): every ratio of the collinearity test is equal -> no good sample
        t = (np.arange(1, 301) * 2.0 ** -7).astype(F)
        cloud = scene.make_points(np.c_[t, 2 * t, 4 * t].astype(F), np.zeros((300, 3)))
    else:
        cloud = scene.make_depth_frame(64, 36)
        s = _seg(box=(50, 51, 50, 51, 50, 51), min_size=1)
    s.setInputCloud(cloud)
    s.apply()
    pl = s.plane()
    if case in ("empty", "all_nan", "two_points", "collinear"):
        assert pl["status"] == _lib.PLANE_NONE and pl["inliers"] == 0 and len(s.planeInliers(0)) == 0
        assert pl["n_survivors"] == pl["n_valid"]  # no plane: nothing removed
    if case == "collinear":
        assert pl["iterations"] == 0 and pl["n_valid"] == 300
        assert len(s.clusterSizes()) == 300  # spacing 0.036 > 0.02: single points
    if case == "box_removes_all":
        assert pl["n_survivors"] == 0 and len(s.clusters()) == 0
    if case != "collinear" and case != "box_removes_all":
        assert len(s.clusterSizes()) == (1 if case == "two_points" else 0)


def _cube_cloud(case, rng):
    xyz = rng.uniform(0.0, 1.0, (4000, 3)) + [0.0, 0.0, 1.0]
    if case == "low_w":  # a plane with a quarter of the points: the loop decides in a later batch
        xyz[:1000, 2] = 1.5 + 0.3 * xyz[:1000, 0] + rng.normal(0, 0.002, 1000)
    if case == "redraws":  # 20 % copies of one point: samples with two of them are degenerate and redrawn
        xyz[:800] = [0.5, 0.5, 1.5]
    xyz = xyz[rng.permutation(len(xyz))].astype(F)
    return scene.make_points(xyz, rng.integers(0, 255, (len(xyz), 3)))


@pytest.mark.parametrize("case,max_iterations", [("noise", 300), ("noise", 1000), ("noise", 1919), ("low_w", 1000),
                                                 ("redraws", 1000)])
def test_ransac_spans_batches(case, max_iterations):
    """Low inlier fractions: the loop runs over several batches of 128 (mt19937 state and sparse map carried in HBM,
    twist refills in the middle of the stream, k and the best count carried between replay launches, the decided gate),
    and in uniform noise it ends at max + 1 hypotheses"""
    cloud = _cube_cloud(case, np.random.default_rng(11))
    s = _seg(box_enable=(0, 0, 0), max_iterations=max_iterations, min_size=10, max_size=500)
    s.setInputCloud(cloud)
    s.apply()
    r = _model(cloud, box_enable=(0, 0, 0), max_iterations=max_iterations, min_size=10, max_size=500)
    _check_against_model(s, cloud, r, exact_clusters=False)
    pl = s.plane()
    assert pl["hypotheses_scored"] > 128
    if case == "noise":
        assert pl["iterations"] == max_iterations + 1
    if case == "low_w":
        assert 128 < pl["iterations"] < max_iterations + 1  # decided by k in a later batch
        assert pl["hypotheses_scored"] < 1024  # the batches after the decision did not run


def test_clustering_skipped_when_no_cluster_can_be_kept():
    """min > max (the plane-only wrappers): the clustering is not run, so a survivor box beyond the cell grid's extent
    (2^17 cells of tol / 2 per axis) does not matter; with clustering the same cloud is PFT_ERR_CAPACITY"""
    rng = np.random.default_rng(5)
    xy = rng.uniform(-1, 1, (3000, 2))
    xyz = np.r_[np.c_[xy, 1.0 + 0.001 * rng.normal(size=3000)], [[5000.0, 0, 1], [-5000.0, 0, 1]]].astype(F)
    cloud = scene.make_points(xyz, np.zeros((len(xyz), 3)))
    seg = segment.SACSegmentation()
    seg.setInputCloud(cloud)
    inl, coef = seg.segment()
    assert len(coef) == 4 and len(inl) == 3000
    s = _seg(box_enable=(0, 0, 0), min_size=1)
    s.setInputCloud(cloud)
    with pytest.raises(_lib.PftError) as e:
        s.apply()
    assert e.value.status == 6


def test_apply_device_equals_apply_and_no_stale_state():
    import torch

    a = scene.make_depth_frame(480, 270)
    b = _blob_scene(7)
    s = _seg()
    s.setInputCloud(a)
    s.apply()
    ref = ([i.copy() for i, _ in s.clusters()], s.plane(), s.hypotheses())
    dev = torch.from_numpy(a.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    s.setInputCloudDevice(dev.data_ptr(), len(a), dev)
    s.apply()
    got = [i for i, _ in s.clusters()]
    assert len(got) == len(ref[0]) and all(np.array_equal(x, y) for x, y in zip(got, ref[0]))
    for cloud in (b, a):  # A, B, A on one handle
        s.setInputCloud(cloud)
        s.apply()
    got = [i for i, _ in s.clusters()]
    assert len(got) == len(ref[0]) and all(np.array_equal(x, y) for x, y in zip(got, ref[0]))
    pl = s.plane()
    for k, v in ref[1].items():
        assert np.array_equal(pl[k], v), k
    smp, cnt = s.hypotheses()
    assert np.array_equal(smp, ref[2][0]) and np.array_equal(cnt, ref[2][1])


def test_handle_grows_on_demand():
    s = segment.ModelSegmenter(max_size=10 ** 6)
    s.configure(box=OBJ_BOX, box_enable=(1, 1, 1))
    s._cfg.max_points = 1024
    small = scene.make_depth_frame(32, 18)
    big = scene.make_depth_frame(320, 180)
    for cloud in (small, big):
        s.setInputCloud(cloud)
        s.apply()
        r = _model(cloud, max_size=10 ** 6)
        _check_against_model(s, cloud, r)


def test_transform_runs_before_remove_zero_points():
    cloud = scene.make_depth_frame(320, 180)
    T = scene.pose_matrix(0.05, -0.4, 0.3, 0.3, -0.2, 0.5).astype(F)
    s = _seg(transform=T, box=(-1, 1, -1, 1, -1, 2))
    s.setInputCloud(cloud)
    s.apply()
    r = _model(cloud, transform_matrix=T, box=(-1, 1, -1, 1, -1, 2))
    _check_against_model(s, cloud, r)


def test_python_pcl_classes():
    cloud = scene.make_depth_frame(320, 180)
    seg = segment.SACSegmentation()
    seg.setMaxIterations(1000)
    seg.setDistanceThreshold(0.015)
    seg.setInputCloud(cloud)
    inl, coef = seg.segment()
    r = _model(cloud, box_enable=(0, 0, 0))
    assert len(coef) == 4 and len(np.setxor1d(inl, r["inliers"])) == 0
    ec = segment.EuclideanClusterExtraction()
    ec.setClusterTolerance(0.02)
    ec.setMinClusterSize(100)
    ec.setMaxClusterSize(25000)
    ec.setInputCloud(cloud)
    got = ec.extract()
    want = _model(cloud, plane=False, box_enable=(0, 0, 0), min_size=100)["clusters"]
    assert len(got) == len(want) and all(np.array_equal(x, y) for x, y in zip(got, want))


def test_create_model_then_track(tmp_path):
    """create_model_amd segments a 480 x 270 frame (the object, ~9 000 points, falls inside [500, 25 000] at this size;
    at qhd it has ~36 000); auto_tracking_amd then tracks the written model over advance_pose frames (frame f: the
    object at GT_POSE + f mm in x and f * 0.5 deg in yaw).  The same run tracks a reference model that did not come from
    the segmentation -- scene.make_model's visible faces at the true pose of frame 0, in the camera frame -- so that what
    the tracker itself does over these frames (the weighted mean sits millimetres to centimetres off)
    is measured next to it.
    Measured on an MI355X (frames 1..8): segmented model 3, 11, 17, 22, 23, 24, 24, 28 mm; reference model 14, 15, 20,
    25, 23, 23, 30, 32 mm.  Both drift the same way, so the drift is the tracker's on these frames, not the segmentation's,
    and the issue's first-guess absolute bound of 2 cm does not hold for the tracker even with the reference model.  The
    bounds are therefore: the segmented model is never worse than the reference model by more than 5 mm, and stays
    within 4 cm (the reference model's worst frame plus a margin)."""
    from pcl_tracking_amd import build

    exe = build.build_create_model_example()
    trk = build.build_example()
    frame0 = scene.make_depth_frame(480, 270)
    raw = tmp_path / "scene.bin"
    frame0.tofile(raw)
    out = tmp_path / "models"
    out.mkdir()
    box = ",".join(str(v) for v in OBJ_BOX)
    r = subprocess.run([exe, str(raw), "--out", str(out), "--box", box], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    sizes = [int(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("cluster ")]
    assert sizes and all(500 <= v <= 25000 for v in sizes)
    # the object's cluster: the one whose points lie inside the object's box
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
    assert best_frac >= 0.95, best_frac  # >= 95 % of the cluster within 1.5 cm of the object box
    # the reference model: make_model's visible faces at the true pose, camera frame
    mdl, off = scene.make_model(4000, return_offset=True)
    mxyz = np.stack([mdl["x"], mdl["y"], mdl["z"]], 1).astype(np.float64) + off
    ref = mdl.copy()
    cam = mxyz @ T[:3, :3].T + T[:3, 3]
    ref["x"], ref["y"], ref["z"] = cam[:, 0], cam[:, 1], cam[:, 2]
    ref_path = tmp_path / "reference_model.bin"
    ref.tofile(ref_path)
    frames = []
    for f in range(1, 9):
        pose = scene.advance_pose(scene.GT_POSE, f)
        fr = scene.make_depth_frame(480, 270, obj_pose=pose)
        p = tmp_path / ("f%d.bin" % f)
        fr.tofile(p)
        frames.append((p, pose))
    r = subprocess.run([trk, str(out / ("%d.pcd" % best)), str(ref_path), "--frames"] + [str(p) for p, _ in frames] +
                       ["--raw"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cents = {0: {}, 1: {}}
    for line in r.stdout.splitlines():
        if line.startswith("frame"):
            t = line.split()
            cents[int(t[3])][int(t[1])] = np.array(list(map(float, t[12:15])))
    assert len(cents[0]) == len(cents[1]) == len(frames)
    # each model's centroid in the object frame; the driver publishes the moved model 5 mm towards the camera
    locs = [np.linalg.solve(T[:3, :3], best_pts.mean(axis=0) - T[:3, 3]), off]
    errs = {0: [], 1: []}
    for k in (0, 1):
        got = [cents[k][f] for f in sorted(cents[k])]
        for f, (_, pose) in enumerate(frames):
            Tf = scene.pose_matrix(*pose)
            want = Tf[:3, :3] @ locs[k] + Tf[:3, 3] + np.array([0.0, 0.0, -0.005])
            errs[k].append(float(np.linalg.norm(got[f] - want)))
    print("centroid errors (m), segmented model:", [round(e, 4) for e in errs[0]])
    print("centroid errors (m), reference model:", [round(e, 4) for e in errs[1]])
    for a, b in zip(errs[0], errs[1]):
        assert a <= b + 0.005, (errs[0], errs[1])
    assert max(errs[0]) < 0.04, errs[0]


def _read_pcd_binary(path):
    data = open(path, "rb").read()
    end = data.index(b"DATA binary\n") + len(b"DATA binary\n")
    rec = np.frombuffer(data[end:], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
    return rec

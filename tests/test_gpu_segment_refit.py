"""The plane refit on the device (csrc/pft_segment.hip k_sg_refit / k_sg_refit_tiles / k_sg_refit_top and the one-lane
tail csrc/pft_segment_solve.h) against the NumPy model, bit for bit: the nine means of either summation order at every
stage, wave, tile and chunk edge (tests/refit_cases.py, proved on the CPU in tests/test_refit_cases_host.py), and, with
the device's own atan2f / cosf / sinf values substituted into the model, every other field of pft_debug_segment_refit's
record and the four coefficients -- the branch bitmap and the all-NaN plane of the cube included.  The three trig values
are held to the OpenCL full-profile bounds of float64 on the device's own arguments.  The final inliers are the exact set
the model's distance rule gives at the device's coefficients: no allowance near the threshold."""
import numpy as np
import pytest

import refit_cases as RC
import segment_model as M
import segment_rounds_model as R
from pcl_tracking_amd import _lib, segment

pytestmark = pytest.mark.gpu
F = np.float32
_worst = [0.0, 0.0, 0.0]  # largest device trig error seen, ulps: atan2f, cosf, sinf


def _seg(order, rounds, max_iterations, threshold, tol, min_size, max_size, optimize=True):
    s = segment.make_scene_segmenter()
    s.configure(plane_rounds=rounds, refit_order=order, max_iterations=max_iterations, distance_threshold=threshold,
                tolerance=tol, min_size=min_size, max_size=max_size, optimize=optimize)
    return s


def _check_round(s, r, order, k, threshold, label):
    """round k of the device against round k of the model result r; -> (record, branch bitmap or None)"""
    rd, pl = r["rounds"][k], s.plane(k)
    assert (pl["status"] == _lib.PLANE_FOUND) == rd["found"], label
    if not rd["found"]:
        return None, None
    assert pl["sample"] == list(rd["sample"]), label
    assert pl["ransac_coefficients"].tobytes() == rd["ransac_coefficients"].tobytes(), label
    np.testing.assert_array_equal(s.planeInliers(1, k), rd["ransac_inliers"])
    p = r["xyz"][rd["ransac_inliers"]]
    assert pl["ransac_inliers"] == len(p), label
    # the cloud of the round: what the model's earlier rounds left
    left = np.flatnonzero(M.keep_nonzero(r["xyz"]))
    for j in range(k):
        left = np.setdiff1d(left, r["rounds"][j]["inliers"])
    assert pl["n_valid"] == len(left), label
    d = None
    if len(p) < 4:
        with pytest.raises(_lib.PftError) as e:
            s.refitDebug(k)
        assert e.value.status == 7  # no refit ran: the coefficients stay
        assert pl["coefficients"].tobytes() == pl["ransac_coefficients"].tobytes(), label
    else:
        d = s.refitDebug(k)
        err = RC.check_record(d, M.moment_means(p, order), len(p), label)  # m, the nine means, every non-trig field
        assert RC.same_bits(pl["coefficients"], d["coef"]), label
        if err is not None:
            for i in range(3):
                _worst[i] = max(_worst[i], err[i])
    # the final inliers: the model's distance rule at the device's own coefficients, exactly
    dist = M.distances(pl["coefficients"], r["xyz"][left])
    with np.errstate(invalid="ignore"):
        want = left[dist < M.float_bound_below(threshold)]
    got = s.planeInliers(0, k)
    np.testing.assert_array_equal(got, want)
    assert pl["inliers"] == len(want), label
    return d, (None if d is None else d["branches"])


def _run_single(cloud, r, order, kw, label, rounds=(1, 0.0)):
    s = _seg(order, rounds, **kw)
    s.setInputCloud(cloud)
    s.apply()
    d, bits = _check_round(s, r, order, 0, kw["threshold"], label)
    return s, d, bits


def _record_bytes(d):
    return b"".join(np.asarray(d[k]).tobytes() for k in ("m", "branches") + RC.FIELDS + ("trig",))


@pytest.mark.parametrize("m", RC.PCL_M)
def test_pcl_order_sums(m):
    """k_sg_refit: 4 096 points per stage, 1 024 threads, nine serial chains"""
    r = RC.model("sum", m, "pcl")
    cloud = RC.sum_cloud(m, RC.SUM_SEEDS.get(m, 0))
    for rounds in ((1, 0.0), (2, 0.0)):  # the single plane and the round loop launch the same refit
        s, d, _ = _run_single(cloud, r, "pcl", RC.SUM_KW, "pcl m = %d" % m, rounds)
        assert s.plane()["ransac_inliers"] == m
        s.close()
    print("device trig errors so far, ulps (atan2f, cosf, sinf): %.3f %.3f %.3f" % tuple(_worst))


@pytest.mark.parametrize("m", RC.TREE_M)
def test_tree_order_sums(m, monkeypatch):
    """k_sg_refit_tiles + k_sg_refit_top: 8 points per thread, 512 per wave, 2 048 per tile, 1 024 tiles per chunk; 2 097 153
    inliers are 1 025 tiles, so the chunk loop runs twice and the chunk sums go through the second tree.  Up to 4 097 the
    record's bytes are the same under three grid sizes of the tile launch"""
    r = RC.model("sum", m, "tree")
    cloud = RC.sum_cloud(m, RC.SUM_SEEDS.get(m, 0))
    got = []
    for grid in ((None, "1", "7") if m in RC.TREE_GRID_M else (None,)):
        if grid is None:
            monkeypatch.delenv("PFT_SEGMENT_REFIT_GRID", raising=False)
        else:
            monkeypatch.setenv("PFT_SEGMENT_REFIT_GRID", grid)
        s, d, _ = _run_single(cloud, r, "tree", RC.SUM_KW, "tree m = %d grid %s" % (m, grid))
        assert s.plane()["ransac_inliers"] == m
        got.append(s.plane()["coefficients"].tobytes() + (_record_bytes(d) if d is not None else b""))
        s.close()
    assert len(set(got)) == 1
    print("device trig errors so far, ulps (atan2f, cosf, sinf): %.3f %.3f %.3f" % tuple(_worst))


@pytest.mark.parametrize("order", RC.ORDERS)
def test_rounds_scene(order):
    """three planes, plane rounds: rounds 2 and 3 sum over the compacted ping-pong buffers"""
    r = RC.model("rounds", None, order)
    s = _seg(order, RC.ROUNDS, **RC.ROUNDS_KW)
    s.setInputCloud(RC.rounds_scene())
    s.apply()
    assert s.planeCount() == r["n_planes"] == 3 and s.stoppedBy() == r["stopped_by"]
    for k in range(3):
        assert len(r["rounds"][k]["near"]) == 0  # so the device's final inliers are the model's, and the rounds stay in step
        _check_round(s, r, order, k, RC.ROUNDS_KW["threshold"], "rounds scene %s round %d" % (order, k))
        np.testing.assert_array_equal(s.planeInliers(0, k), r["rounds"][k]["inliers"])
    with pytest.raises(_lib.PftError) as e:
        s.refitDebug(3)
    assert e.value.status == 1  # no such round
    assert s.plane()["n_survivors"] == len(r["survivors"])
    s.close()


def test_solve_cases_and_branch_coverage():
    """every solve case in both orders; at the end the union of the device's branch bitmaps is the set
    tests/test_refit_cases_host.py proved reachable: every bit of the record"""
    union = 0
    for name in RC.SOLVE_CASES:
        cloud, kw = RC.SOLVE_CASES[name][0](), RC.solve_kw(name)
        for o, order in enumerate(RC.ORDERS):
            r = RC.model("solve", name, order)
            s, d, bits = _run_single(cloud, r, order, kw, "%s %s" % (name, order))
            assert bits == RC.EXPECTED[name][o], (name, order, M.branch_names(bits))
            union |= bits
            s.close()
    print("device branches:", M.branch_names(union))
    print("device trig errors, ulps (atan2f, cosf, sinf): %.3f %.3f %.3f" % tuple(_worst))
    assert union == RC.REACHABLE


@pytest.mark.parametrize("name,order", RC.NAN_PLANES)
def test_nan_planes(name, order):
    """the cube (covariance 2^-16 I exactly: all roots 1, M - r0 I the zero matrix) and the far specks (every entry of
    accu - mean * mean cancels to 0: scale = 1, the zero matrix): the normal is 0 / 0.  Plane found with every point a
    pre-refit inlier, coefficients all NaN, no final inlier, nothing removed, one cluster of all points; with rounds, one
    round and stop NO_PLANE"""
    kw = RC.solve_kw(name)
    cloud = RC.SOLVE_CASES[name][0]()
    n = len(cloud)
    for rounds in ((1, 0.0), (16, 0.0)):
        r = R.pipeline(cloud, max_planes=rounds[0], fraction=rounds[1], order=order, **kw)
        s, d, bits = _run_single(cloud, r, order, kw, "%s %s" % (name, order), rounds)
        pl = s.plane()
        assert pl["status"] == _lib.PLANE_FOUND and pl["ransac_inliers"] == n and pl["inliers"] == 0
        assert np.isnan(pl["coefficients"]).all() and np.isnan(d["coef"]).all()
        assert d["len"].tolist() == [0, 0, 0] and bits & M.ZERO_LENGTH
        if name == "cube":
            assert d["cov"].tolist() == [2.0 ** -16, 0, 0, 2.0 ** -16, 0, 2.0 ** -16] and d["roots"].tolist() == [1, 1, 1]
        else:
            assert d["cov"].tolist() == [0] * 6 and d["scale"] == 1 and bits & M.SCALE_TINY
        assert len(s.planeInliers(0)) == 0 and pl["n_survivors"] == pl["n_valid"] == n
        assert s.clusterSizes().tolist() == [n] and [len(c) for c in r["clusters"]] == [n]
        assert s.planeCount() == 0 and s.stoppedBy() == _lib.ROUNDS_STOP_NO_PLANE == r["stopped_by"]
        if rounds[0] > 1:
            with pytest.raises(_lib.PftError):
                s.plane(1)  # one round
        s.close()


def test_refit_debug_refusals():
    kw = dict(RC.SOLVE_KW)
    s = _seg("pcl", (1, 0.0), **kw)
    with pytest.raises(_lib.PftError):
        s.refitDebug()  # no handle yet, no apply
    s.close()
    s = _seg("pcl", (1, 0.0), optimize=False, **kw)
    s.setInputCloud(RC.SOLVE_CASES["normal z"][0]())
    s.apply()
    assert s.plane()["status"] == _lib.PLANE_FOUND
    assert s.plane()["coefficients"].tobytes() == s.plane()["ransac_coefficients"].tobytes()
    with pytest.raises(_lib.PftError) as e:
        s.refitDebug()
    assert e.value.status == 7 and "no refit" in str(e.value)
    s.close()
    two = RC.cube()[:2]  # fewer than three points: no plane
    s = _seg("tree", (1, 0.0), **kw)
    s.setInputCloud(two)
    s.apply()
    assert s.plane()["status"] == _lib.PLANE_NONE
    with pytest.raises(_lib.PftError) as e:
        s.refitDebug()
    assert e.value.status == 7 and "no plane" in str(e.value)
    with pytest.raises(_lib.PftError) as e:
        s.refitDebug(1)
    assert e.value.status == 1
    s.close()

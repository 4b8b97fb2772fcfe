"""The refit cases (tests/refit_cases.py) are what they claim -- proved on the CPU with the NumPy model alone, no GPU and no
library: every sum case has exactly m pre-refit inliers gathered from between strays, nothing near the threshold, and
sums whose bits depend on the order of the adds; every solve case takes the branches it is listed for, and together they
set every branch bit a cloud can reach.  The device runs the same cases in tests/test_gpu_segment_refit.py."""
import numpy as np
import pytest

import refit_cases as RC
import segment_model as M
import segment_rounds_model as R

F = np.float32


def _near(coef, xyz, thr, eps=1e-4):
    return int((np.abs(M.distances(coef, xyz).astype(np.float64) - thr) < eps).sum())


@pytest.mark.parametrize("m", sorted(set(RC.PCL_M + RC.TREE_M)))
def test_sum_case(m):
    orders = [o for o, lst in (("pcl", RC.PCL_M), ("tree", RC.TREE_M)) if m in lst]
    thr = RC.SUM_KW["threshold"]
    for order in orders:
        r = RC.model("sum", m, order)
        rd, xyz = r["rounds"][0], r["xyz"]
        assert rd["found"] and len(rd["ransac_inliers"]) == m  # RANSAC stops on the plane
        inl = rd["ransac_inliers"]
        assert _near(rd["ransac_coefficients"], xyz, thr) == 0 and _near(rd["coefficients"], xyz, thr) == 0
        assert len(rd["near"]) == 0
        out = np.setdiff1d(np.arange(len(xyz)), inl)
        assert len(out) >= 2 and inl.tolist() != list(range(m)), "a gather, not a prefix"
        if m >= 4:
            # the strays are at least 0.3 m off the plane the inliers span, and stay out of the final plane
            assert M.distances(rd["coefficients"], xyz[out]).min() >= 0.3
            np.testing.assert_array_equal(rd["inliers"], inl)
    if m < 4:
        np.testing.assert_array_equal(rd["coefficients"], rd["ransac_coefficients"])  # the coefficients stay
        return
    # order-sensitive: the two orders' means differ, and so do the PCL chain's when a term at a stage edge is dropped or
    # two are swapped
    p = xyz[inl]
    a, b = M.moment_means(p, "pcl"), M.moment_means(p, "tree")
    assert a.tobytes() != b.tobytes()
    if m > 4096 and "pcl" in orders:
        assert M.moment_sums(np.delete(p, 4096, 0), "pcl").tobytes() != M.moment_sums(p, "pcl").tobytes()
        q = p.copy()
        q[[4095, 4096]] = q[[4096, 4095]]
        assert M.moment_means(q, "pcl").tobytes() != a.tobytes()
    if m in (2049, 4097):
        q = p.copy()
        q[[2047, 2048]] = q[[2048, 2047]]  # across a tile edge: another pairing
        assert M.moment_means(q, "tree").tobytes() != b.tobytes()


@pytest.mark.parametrize("order", RC.ORDERS)
def test_rounds_scene_has_three_planes(order):
    r = RC.model("rounds", None, order)
    assert r["n_planes"] == 3 and len(r["rounds"]) == 3 and r["stopped_by"] == R.STOP_FRACTION
    assert [len(x["ransac_inliers"]) for x in r["rounds"]] == [5053, 3049, 1900]
    for k, x in enumerate(r["rounds"]):
        assert len(x["near"]) == 0
        t = RC.model_trace(r, k, order)
        assert t["m"] == len(x["ransac_inliers"]) and t["coef"].tobytes() == x["coefficients"].tobytes()


def test_solve_cases_take_their_branches_and_cover_every_reachable_bit():
    union = 0
    for name in RC.SOLVE_CASES:
        for o, order in enumerate(RC.ORDERS):
            r = RC.model("solve", name, order)
            rd = r["rounds"][0]
            assert rd["found"] and len(rd["ransac_inliers"]) == r["n_valid"], name  # the whole cloud is the inlier list
            kw = RC.solve_kw(name)
            assert _near(rd["ransac_coefficients"], r["xyz"], kw["threshold"]) == 0 and len(rd["near"]) == 0, name
            t = RC.model_trace(r, 0, order)
            print("%-62s %-4s %s" % (name, order, " ".join(M.branch_names(t["branches"]))))
            assert t["branches"] == RC.EXPECTED[name][o], (name, order, M.branch_names(t["branches"]))
            assert t["coef"].tobytes() == rd["coefficients"].tobytes()
            union |= t["branches"]
    print("covered:", M.branch_names(union), "| not reached by any cloud:", M.branch_names(((1 << 13) - 1) & ~union))
    assert union == RC.REACHABLE


def test_solve_cases_are_the_geometry_they_name():
    tr = {n: RC.model_trace(RC.model("solve", n, "pcl"), 0, "pcl") for n in RC.SOLVE_CASES}
    for n, axis in (("normal z", 2), ("normal y", 1), ("normal x", 0)):
        assert abs(tr[n]["coef"][axis]) > 0.99
    for n in ("flat axis-aligned", "found: flat four-fold, seed 1 (d < 0, PCL order)"):
        assert tr[n]["cov"][[2, 4, 5]].tolist() == [0, 0, 0] and np.abs(tr[n]["coef"]).tolist() == [0, 0, 1, 1]
    c = tr["lattice slab"]["cov"]
    assert c.tolist() == [0.08203125, 0, 0, 0.08203125, 0, 2.0 ** -16]  # a double root, exactly, in both orders
    assert RC.model_trace(RC.model("solve", "lattice slab", "tree"), 0, "tree")["cov"].tobytes() == c.tobytes()
    c = tr["cube"]["cov"]
    assert c.tolist() == [2.0 ** -16, 0, 0, 2.0 ** -16, 0, 2.0 ** -16] and tr["cube"]["roots"].tolist() == [1, 1, 1]
    assert tr["cube"]["len"].tolist() == [0, 0, 0] and np.isnan(tr["cube"]["coef"]).all()
    r = RC.model_trace(RC.model("solve", "thin strip", "pcl"), 0, "pcl")
    lam = np.linalg.eigvalsh(_cov3(r["cov"]))
    assert 2e-4 < (lam[1] - lam[0]) / lam[2] < 8e-4
    kw = RC.solve_kw("blob")
    xyz = RC.model("solve", "blob", "pcl")["xyz"]
    assert np.linalg.norm(xyz.max(0) - xyz.min(0)) < kw["threshold"]  # smaller than the threshold
    for n in ("plane at z = 8", "plane at z = 30"):  # cancellation: accu_zz and mean_z^2 agree to 4 .. 5 digits
        assert tr[n]["cov"][5] < 1e-2 and tr[n]["accu"][5] > 60


def _cov3(c):
    c = np.asarray(c, np.float64)
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])


@pytest.mark.parametrize("name,order", RC.NAN_PLANES)
def test_nan_planes_remove_nothing(name, order):
    """the NaN cases (the cube's zero-length cross product; the far specks' covariance that cancels to the zero matrix):
    plane found with every point a pre-refit inlier, coefficients all NaN, 0 final inliers, stop NO_PLANE, nothing
    removed, one cluster of all points"""
    cloud = RC.SOLVE_CASES[name][0]()
    n = len(cloud)
    r = R.pipeline(cloud, max_planes=16, fraction=0.0, order=order, **RC.solve_kw(name))
    assert len(r["rounds"]) == 1 and r["n_planes"] == 0 and r["stopped_by"] == R.STOP_NO_PLANE
    rd = r["rounds"][0]
    assert rd["found"] and len(rd["ransac_inliers"]) == n and len(rd["inliers"]) == 0
    assert np.isnan(rd["coefficients"]).all()
    assert r["remaining"] == n == r["n_valid"] and [len(c) for c in r["clusters"]] == [n]
    t = RC.model_trace(r, 0, order)
    assert t["branches"] & M.ZERO_LENGTH and t["len"].tolist() == [0, 0, 0]
    if "speck" in name:
        assert t["cov"].tolist() == [0] * 6 and t["scale"] == 1 and t["branches"] & M.SCALE_TINY


def test_the_search_finds_the_found_cases():
    """the seeds in the names of the "found:" cases are the first the search meets"""
    rng = range(20)
    assert RC.search(RC._iso_blob, M.A_CLAMPED, rng, "tree") == 0 and RC.search(RC._iso_blob, M.A_CLAMPED, rng, "pcl") == 3
    assert RC.search(RC._flat_iso, M.D_NEGATIVE, rng, "pcl") == 1 and RC.search(RC._flat_iso, M.D_NEGATIVE, rng, "tree") == 6
    assert RC.search(RC._flat_sloped, M.R0_FALLBACK, rng, "pcl") == 1
    assert RC.search(RC._flat_sloped, M.R0_FALLBACK, rng, "tree") == 3
    both = [s for s in range(200) if all(RC.direct_trace(RC._far_speck(s), o)["branches"] & M.SCALE_TINY for o in RC.ORDERS)]
    assert both[0] == 109


def test_trig_substitution_and_wrappers():
    """eigen33 / refit stay wrappers of the traced forms; the model's own trig values substituted back change nothing, and
    a 2 ulp nudge of all three moves the normal of a typical plane by about an ulp of a coefficient (the slack the
    1e-5 bound of the older tests has)"""
    r = RC.model("solve", "normal z", "pcl")
    rd = r["rounds"][0]
    p = r["xyz"][rd["ransac_inliers"]]
    t = M.refit_trace(p, rd["ransac_coefficients"], "pcl")
    assert M.refit(p, rd["ransac_coefficients"]).tobytes() == t["coef"].tobytes() == R.refit(p, None, "pcl").tobytes()
    assert M.eigen33(_cov3(t["cov"])).tobytes() == t["coef"][:3].tobytes()
    t2 = M.refit_trace(p, None, "pcl", trig=t["trig"])
    for k in t:
        assert np.asarray(t[k]).tobytes() == np.asarray(t2[k]).tobytes(), k
    worst = 0.0
    for sa in (-2, 2):
        for sc in (-2, 2):
            for ss in (-2, 2):
                g = t["trig"].copy()
                for i, n in enumerate((sa, sc, ss)):
                    for _ in range(abs(n)):
                        g[i] = np.nextafter(g[i], F(np.inf if n > 0 else -np.inf))
                worst = max(worst, np.abs(M.refit_trace(p, None, "pcl", trig=g)["coef"][:3] - t["coef"][:3]).max())
    print("largest move of the normal under a 2 ulp nudge of the three trig values: %.3g" % worst)
    assert worst <= 2.4e-7
    assert M.refit_trace(p[:3], None) is None and R.refit(p[:3], np.array([1, 2, 3, 4], F), "tree").tolist() == [1, 2, 3, 4]

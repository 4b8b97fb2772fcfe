"""The shared result-pose search (mt_min_child / mt_search / mt_load_tree, pcl_tracking_amd/csrc/pft_match_search.h) on the
constructions of tests/search_cases.py, through each of its three callers -- k_match (compute() + computeMatch()),
k_reacquire_score (reacquire()) and k_refine_pairs (refine()) --, in both leaf-record forms and with both builders.  Every
comparison is bit for bit: against the oracle's search at the device's own matrices and crop box, against what the
construction itself predicts (at an exact tie between children the lower child, inside a leaf the earliest record, a gate
pair on either side of its g*g), and, for the match, against the likelihood kernel's own search on a fresh handle.
tests/test_search_cases_host.py proves on the CPU that the constructions are what they claim.

The poses are pure x translations.  The match is driven at an exactly known transform through the normal compute(): with
all step and initial covariances zero and 64 particles (weights that are powers of two) the result pose is `trans` itself,
which every test asserts before it compares anything.

Sizes: models of 64 to 256 points, clouds of at most 5 001 points, 64 particles, at most 7 candidates or start matrices."""
import numpy as np
import pytest

import match_model as mm
import reacquire_model as rm
import refine_model as rfm
import search_cases as sc
import test_gpu_match as tgm
from test_gpu_reacquire import centres_of, check_result_is_the_selection, gt_rpy
from test_gpu_refine import check_every_pass, neighbour

pytestmark = pytest.mark.gpu
F = np.float32
P = 64
LEAF_FORMS = {"copied": "0", "followed": "1"}
BUILDERS = ("single", "sorted")


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sc.all_cases()}


@pytest.fixture
def switches(monkeypatch, leaf, builder):
    monkeypatch.setenv("PFT_LEAF_INDIRECT", LEAF_FORMS[leaf])  # latched at pft_create
    monkeypatch.setenv("PFT_FORCE_BUILDER", builder)
    return leaf, builder


def make(gpu, reference, trans, resolution, exact_pose=True, seed=3):
    """the reference tracker at another octree resolution; exact_pose: no noise at all, so that compute() returns `trans`"""
    t = gpu.make_reference_tracker(particle_num=P, seed=seed)
    coh = gpu.ApproxNearestPairPointCloudCoherence()
    coh.addPointCoherence(gpu.DistanceCoherence())
    hc = gpu.HSVColorCoherence()
    hc.setWeight(0.1)
    coh.addPointCoherence(hc)
    coh.setSearchMethod(gpu.OctreeSearch(resolution))
    coh.setMaximumDistance(0.1)
    t.setCloudCoherence(coh)
    if exact_pose:
        t.setStepNoiseCovariance([0.0] * 6)
        t.setInitialNoiseCovariance([0.0] * 6)
    t.setIterationNum(2)
    t.setReferenceCloud(reference)
    t.setTrans(trans)
    return t


def check_route(t, switches, n_crop):
    """proof of the route: the tree's own record of its leaf form and of the builder that wrote it"""
    if switches is None or n_crop == 0:
        return
    leaf, builder = switches
    tree = t.debugGetTree()
    assert tree["n_crop"] == n_crop
    assert (tree["build_path"] == 2) == (builder == "sorted"), tree["build_path"]
    # (the sorted builder always writes the leaf records itself: behind it the search reads the copied form whatever is asked)
    assert tree["leaf_indirect"] == int(leaf == "followed" and builder == "single"), tree["leaf_indirect"]


def with_resolution(monkeypatch, resolution):
    """test_gpu_refine.check_every_pass takes the oracle's configuration from test_gpu_match.oracle_cfg: hand it the case's
    octree resolution (the helper itself is imported, not edited)"""
    plain = tgm.oracle_cfg
    monkeypatch.setattr(tgm, "oracle_cfg", lambda orc, coherence=None: plain(orc, dict(coherence or {}, octree_resolution=resolution)))


def check_match_against_oracle(orc, t, reference, cloud, label, resolution):
    """test_gpu_match.check_against_oracle at an octree resolution (its `coherence` values go into the oracle's config)"""
    return tgm.check_against_oracle(orc, t, reference, cloud, label, coherence=dict(octree_resolution=resolution))


def check_reacquire_against_oracle(orc, t, reference, cloud, resolution, label, inlier_distance=0.02, **call):
    """test_gpu_reacquire.check_against_oracle with the oracle at an octree resolution: counts equal, sums bit for bit, the
    selection rule"""
    res = t.reacquire(inlier_distance=inlier_distance, apply=False, **call)
    s = t.getReacquireScores()
    K = len(s["candidates"])
    assert res.n_candidates == K and not res.applied, label
    assert s["mats"].tobytes() == t.debugPoseToMatrix(s["candidates"]).tobytes(), label
    cfg = orc.default_config(particle_num=max(K, P), threads=0, emulate_pcl_alloc=0, octree_resolution=resolution)
    o = orc.Tracker(cfg)
    o.set_reference(reference)
    o.set_input(cloud)
    E = o.eval_weights(s["candidates"], want_nn=True, mats=s["mats"], bbox=tgm.get_bbox(t))
    want = rm.scores(orc, cfg, reference, s["mats"], cloud, E["nn_idx"], E["nn_d2"], E["crop_idx"], inlier_distance)
    print("%s: K %d crop %d depth %d inliers %s matched %s" % (label, K, res.n_crop, E["octree_depth"], s["n_inliers"].tolist(),
                                                                 s["n_matched"].tolist()))
    assert res.n_crop == len(E["crop_idx"]), label
    assert s["n_inliers"].tolist() == want["n_inliers"].tolist(), label
    assert s["n_matched"].tolist() == want["n_matched"].tolist(), label
    for f in ("coherence", "sum_sq_dist", "inlier_sq_dist"):  # adjacent-pair trees over the stored order: bit for bit
        assert s[f].tobytes() == want[f].tobytes(), (label, f)
    check_result_is_the_selection(res, s, len(reference), 0.5, K // max(res.n_centres, 1))
    return res, s, E


def is_the_translation(m, x):
    """a 3x4 that is the pure translation by x (a -0.0 among the zeros of the rotation counts as zero)"""
    return np.array_equal(np.asarray(m, F).reshape(3, 4), sc.translation(x)[:3])


# ---- k_match --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("leaf", sorted(LEAF_FORMS))
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_match_on_the_constructed_cases(gpu, orc, cases, switches, name, leaf, builder):
    c = cases[name]
    n_crop = len(c.cloud) if c.whole_crop else 0
    for pose in (c.expect_pose, len(c.poses) - 1):  # the pose of the construction's answers, and another: the oracle's alone
        x = c.poses[pose]
        label = "%s %s %s pose %d" % (name, leaf, builder, pose)
        t = make(gpu, c.model, sc.translation(x), c.resolution)
        tgm.step(t, c.cloud)
        st = t.getMatch()
        idx, d2 = t.getMatchPairs()
        # preconditions: the result is the translation itself, the crop is the whole cloud
        r = t.getResult()
        assert r["x"] == F(x) and all(r[k] == 0.0 for k in ("y", "z", "roll", "pitch", "yaw")), (label, r)
        assert st.transform.tobytes() == t.debugPoseToMatrix(sc.particles_of([x]))[0].tobytes(), label
        assert is_the_translation(st.transform, x), (label, st.transform)
        assert st.evaluated and st.n_crop == n_crop, (label, st.n_crop)
        check_route(t, switches, n_crop)
        # 1. the oracle
        _, want, E = check_match_against_oracle(orc, t, c.model, c.cloud, label, c.resolution)
        if not c.whole_crop:
            assert st.n_matched == 0 and (idx == -1).all() and np.isinf(d2).all(), label
            t.close()
            continue
        # 2. the construction
        gate2 = mm.gate(0.1)
        if pose == c.expect_pose:
            assert c.expect
            for qi, rec, dd in c.expect:
                assert d2[qi].tobytes() == F(dd).tobytes(), (label, qi, d2[qi], dd)
                assert idx[qi] == (rec if np.float64(F(dd)) < gate2 else -1), (label, qi, idx[qi], rec)
            for qi, tie in c.leaf_ties:
                assert idx[qi] == min(tie), (label, qi)
            for tie in c.ties:
                assert idx[tie["query"]] == tie["winner"] == min(tie["tied"]) and idx[tie["up"]] == tie["winner_up"], (label, tie["name"])
            for qi, rec, gname, g, inside in c.gate:
                if gname == "max_distance":
                    assert idx[qi] == (rec if inside else -1), (label, qi)
        # 3. the likelihood kernel's own search of the same pose on a fresh handle: the other device restatement
        g = make(gpu, c.model, np.eye(4, dtype=F), c.resolution)
        g.setInputCloud(c.cloud)
        one = sc.particles_of([x] * 4)  # (four copies of the pose: row 0 is read)
        assert g.debugPoseToMatrix(one)[0].tobytes() == st.transform.tobytes(), label
        g.evalWeights(one)  # (the builder's mode follows the previous build's size: the compared call runs its own)
        G = g.evalWeights(one, want_nn=True)
        np.testing.assert_array_equal(G["crop_idx"], np.arange(len(c.cloud)))
        assert G["nn_d2"][0].tobytes() == d2.tobytes(), label
        near = (G["nn_idx"][0] >= 0) & (G["nn_d2"][0].astype(np.float64) < gate2)
        assert np.where(near, G["crop_idx"][np.maximum(G["nn_idx"][0], 0)], -1).tolist() == idx.tolist(), label
        g.close()
        t.close()


# ---- k_reacquire_score ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("leaf", sorted(LEAF_FORMS))
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_reacquire_on_the_constructed_cases(gpu, orc, cases, switches, name, leaf, builder):
    c = cases[name]
    label = "%s %s %s" % (name, leaf, builder)
    t = make(gpu, c.model, np.eye(4, dtype=F), c.resolution)
    t.setInputCloud(c.cloud)
    centres = np.array([[x, 0.0, 0.0] for x in c.poses], F)
    res, s, E = check_reacquire_against_oracle(orc, t, c.model, c.cloud, c.resolution, label, centres=centres, n=(1, 1, 1),
                                               span=(0.0, 0.0, 0.0), base_rpy=(0.0, 0.0, 0.0))
    # precondition: the candidates are the pure translations
    assert len(s["mats"]) == len(c.poses)
    for k, x in enumerate(c.poses):
        assert is_the_translation(s["mats"][k], x), (label, k, s["mats"][k])
    n_crop = len(c.cloud) if c.whole_crop else 0
    assert res.n_crop == n_crop, label
    check_route(t, switches, n_crop)
    # the counts from the oracle's distances at both gates, stated here once more
    for k in range(len(c.poses)):
        found, dd = E["nn_idx"][k] >= 0, E["nn_d2"][k].astype(np.float64)
        assert int(s["n_matched"][k]) == int((found & (dd < np.float64(0.1) * np.float64(0.1))).sum()), (label, k)
        assert int(s["n_inliers"][k]) == int((found & (dd < np.float64(0.02) * np.float64(0.02))).sum()), (label, k)
    if c.whole_crop and c.expect:  # the construction's distances at its pose, through the oracle's arrays the sums were built on
        k = c.expect_pose
        for qi, rec, dd in c.expect:
            assert E["nn_idx"][k, qi] == rec and E["nn_d2"][k, qi].tobytes() == F(dd).tobytes(), (label, qi)
        for qi, _, gname, g, inside in c.gate:  # the pair of the inlier gate lies on either side of it
            if gname == "inlier_distance":
                assert (np.float64(E["nn_d2"][k, qi]) < np.float64(g) * np.float64(g)) == inside, (label, qi)
    # more inliers, then the smaller inlier_sq_dist, then the lower index
    best, _ = rm.select(s["n_inliers"], s["inlier_sq_dist"], len(c.model), 0.5)
    assert res.best == best, label
    order = sorted(range(len(c.poses)), key=lambda k: (-int(s["n_inliers"][k]), float(s["inlier_sq_dist"][k]), k))
    assert res.best == order[0], (label, order)
    t.close()


# ---- k_refine_pairs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("leaf", sorted(LEAF_FORMS))
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_refine_on_the_constructed_cases(gpu, orc, cases, switches, monkeypatch, name, leaf, builder):
    c = cases[name]
    with_resolution(monkeypatch, c.resolution)
    t = make(gpu, c.model, np.eye(4, dtype=F), c.resolution)
    t.setInputCloud(c.cloud)
    n_crop = len(c.cloud) if c.whole_crop else 0
    kw = dict(max_iterations=2)
    if any(g[2] == "pair_distance" for g in c.gate):
        kw["pair_distance"] = 0.05
    for k, x in enumerate(c.poses):
        label = "%s %s %s start %d" % (name, leaf, builder, k)
        res, tr, want = check_every_pass(orc, t, c.model, c.cloud, sc.translation(x)[:3], label, **kw)
        assert res.n_crop == n_crop, (label, res.n_crop)
        if not c.whole_crop:
            assert res.n_pairs_before == 0 and res.status == rfm.TOO_FEW_PAIRS and res.iterations == 0, label
            continue
        if k == c.expect_pose:  # pass 0 pairs the construction's queries: its records, its distances, its gates
            o = orc.Tracker(tgm.oracle_cfg(orc))
            o.set_reference(c.model)
            o.set_input(c.cloud)
            E = o.eval_weights(sc.particles_of([x]), want_nn=True, mats=tr["transform"][:1], bbox=res.bbox)
            for qi, rec, dd in c.expect:
                assert E["nn_idx"][0, qi] == rec and E["nn_d2"][0, qi].tobytes() == F(dd).tobytes(), (label, qi)
            found, dd = E["nn_idx"][0] >= 0, E["nn_d2"][0].astype(np.float64)
            pair2 = np.float64(kw.get("pair_distance", 0.1)) * np.float64(kw.get("pair_distance", 0.1))
            assert int(tr["n_pairs"][0]) == int((found & (dd < pair2)).sum()), label
            assert int(tr["n_inliers"][0]) == int((found & (dd < np.float64(0.02) * np.float64(0.02))).sum()), label
    check_route(t, switches, n_crop)
    t.close()


# ---- other resolutions, the realistic frame -------------------------------------------------------------------------------
def realistic(gpu, resolution):
    t = make(gpu, tgm.model(300), tgm._world()["trans"], resolution, exact_pose=False)
    return t, tgm.model(300), tgm.frame(0)


@pytest.mark.parametrize("resolution", sc.RESOLUTIONS)
def test_match_at_other_resolutions(gpu, orc, resolution):
    t, ref, cloud = realistic(gpu, resolution)
    for f in range(2):
        tgm.step(t, cloud)
        st, want, E = check_match_against_oracle(orc, t, ref, cloud, "res %g frame %d" % (resolution, f), resolution)
        print("res %g: depth %d matched %d" % (resolution, E["octree_depth"], st.n_matched))
        assert st.n_matched > 0
    t.close()


@pytest.mark.parametrize("resolution", sc.RESOLUTIONS)
def test_reacquire_at_other_resolutions(gpu, orc, resolution):
    t, ref, cloud = realistic(gpu, resolution)
    tgm.step(t, cloud, match=False)
    res, s, _ = check_reacquire_against_oracle(orc, t, ref, cloud, resolution, "res %g" % resolution, centres=centres_of(cloud),
                                               n=(1, 1, 4), span=(0.0, 0.0, 2.0 * np.pi), base_rpy=gt_rpy())
    assert res.n_candidates == 12 and s["n_matched"].max() > 0
    t.close()


@pytest.mark.parametrize("resolution", sc.RESOLUTIONS)
def test_refine_at_other_resolutions(gpu, orc, monkeypatch, resolution):
    with_resolution(monkeypatch, resolution)
    t, ref, cloud = realistic(gpu, resolution)
    t.setInputCloud(cloud)
    res, _, want = check_every_pass(orc, t, ref, cloud, neighbour(orc), "res %g" % resolution, max_iterations=4)
    assert res.iterations >= 1 and res.n_pairs_before >= 3
    t.close()

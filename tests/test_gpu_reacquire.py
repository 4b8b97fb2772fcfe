"""GPU checks of the re-acquisition step (pft_reacquire; pcl_tracking_amd/csrc/pft_reacquire.hip): every candidate's scores
against the CPU oracle's search at the device's own matrices and crop box, through tests/reacquire_model.py, counts equal and
sums bit for bit; the same bits as pft_match for the same pose and tree; the selection; recovery of a lost object end to end
against a fresh handle; apply=False leaving the tracker alone; the segmenter form; the refusals; and the C++ driver's
--reacquire.

Sizes: a model of 300 points unless a case says otherwise, frames of about 4 000 points (test_gpu_match's), at most 81
candidates."""
import os
import subprocess

import numpy as np
import pytest

import match_model as mm
import reacquire_model as rm
import test_gpu_match as tgm
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu
TWO_PI = 2.0 * np.pi


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


def gt_rpy():
    return tuple(scene.model_gt_pose()[3:])


def centres_of(cloud, shift=0.0):
    """a background point, the object's position, another background point"""
    gt = tgm._world()["gt"] + np.array([shift, 0.0, 0.0])
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
    far = np.flatnonzero(np.linalg.norm(xyz - gt, axis=1) >= 0.6)
    return np.stack([xyz[far[0]], gt.astype(np.float32), xyz[far[len(far) // 2]]]).astype(np.float32)


def model_scores(orc, t, reference, cloud, sc, inlier_distance=0.02):
    """one oracle evaluation of all the device's candidates at the device's matrices and crop box -> the model's scores"""
    K = len(sc["candidates"])
    cfg = orc.default_config(particle_num=max(K, tgm.P), threads=0, emulate_pcl_alloc=0)
    o = orc.Tracker(cfg)
    o.set_reference(reference)
    o.set_input(cloud)
    E = o.eval_weights(sc["candidates"], want_nn=True, mats=sc["mats"], bbox=tgm.get_bbox(t))
    return E, rm.scores(orc, cfg, reference, sc["mats"], cloud, E["nn_idx"], E["nn_d2"], E["crop_idx"], inlier_distance)


def check_result_is_the_selection(res, sc, M, accept_ratio, per_centre):
    best, accepted = rm.select(sc["n_inliers"], sc["inlier_sq_dist"], M, accept_ratio)
    assert (res.best, res.accepted) == (best, accepted)
    assert res.n_candidates == len(sc["n_inliers"]) and res.n_reference == M
    if best < 0:
        assert res.best_centre == -1
        return
    assert res.best_centre == best // per_centre
    assert res.pose.tobytes() == sc["candidates"][best].tobytes()
    assert res.transform.tobytes() == sc["mats"][best].tobytes()
    assert (res.n_inliers, res.n_matched) == (int(sc["n_inliers"][best]), int(sc["n_matched"][best]))
    assert (res.coherence, res.sum_sq_dist, res.inlier_sq_dist) == (sc["coherence"][best], sc["sum_sq_dist"][best],
                                                                   sc["inlier_sq_dist"][best])


def check_against_oracle(orc, t, reference, cloud, centres, n, base, span, label, inlier_distance=0.02):
    res = t.reacquire(centres=centres, n=n, span=span, base_rpy=base, inlier_distance=inlier_distance, apply=False)
    sc = t.getReacquireScores()
    per = n[0] * n[1] * n[2]
    K = len(centres) * per
    assert res.n_centres == len(centres) and res.n_candidates == K and len(sc["candidates"]) == K, label
    assert not res.applied
    assert sc["centres"].tobytes() == np.ascontiguousarray(centres, np.float32).tobytes(), label
    assert sc["candidates"].tobytes() == rm.candidates(centres, n, base, span).tobytes(), label
    assert sc["mats"].tobytes() == t.debugPoseToMatrix(sc["candidates"]).tobytes(), label
    E, want = model_scores(orc, t, reference, cloud, sc, inlier_distance)
    print("%s: K %d crop %d depth %d inliers %s matched %s" % (label, K, res.n_crop, E["octree_depth"],
                                                                 sc["n_inliers"].tolist(), sc["n_matched"].tolist()))
    assert res.n_crop == len(E["crop_idx"]), label
    assert sc["n_inliers"].tolist() == want["n_inliers"].tolist(), label
    assert sc["n_matched"].tolist() == want["n_matched"].tolist(), label
    for f in ("coherence", "sum_sq_dist", "inlier_sq_dist"):  # adjacent-pair trees over the stored order: bit for bit
        assert sc[f].tobytes() == want[f].tobytes(), (label, f)
    check_result_is_the_selection(res, sc, len(reference), 0.5, per)
    return res, sc, E


# ---- 1. every candidate against the oracle ------------------------------------------------------------------------------
VARIANTS = {
    "builder_single": dict(env={"PFT_FORCE_BUILDER": "single"}),
    "builder_sorted": dict(env={"PFT_FORCE_BUILDER": "sorted"}),
    "leaf_direct": dict(env={"PFT_LEAF_INDIRECT": "0"}),
    "leaf_indirect": dict(env={"PFT_LEAF_INDIRECT": "1"}),
    "M1": dict(M=1),
    "M513": dict(M=513),  # two tiles of the 256-thread workgroup and a one-point third
    "M769": dict(M=769),  # four 256-position tiles: the push at tile 3 merges two levels
    "M1153": dict(M=1153),  # five tiles: the fold joins levels 2 and 0 across the empty level 1
    "M1281": dict(M=1281),  # six tiles (five and a one-point sixth): the fold joins levels 2 and 1
    "K1": dict(one=True),
    "kld": dict(kld=True),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_every_candidate_against_the_oracle(gpu, orc, monkeypatch, name):
    v = VARIANTS[name]
    for k, val in v.get("env", {}).items():  # the switches are latched at pft_create
        monkeypatch.setenv(k, val)
    M = v.get("M", 300)
    t = tgm.make(gpu, M=M, kld=v.get("kld", False))
    cloud = tgm.frame(0)
    cen = centres_of(cloud)
    if v.get("one"):  # a handle that has never computed: one candidate, the ground-truth pose
        t.setInputCloud(cloud)
        res, sc, _ = check_against_oracle(orc, t, tgm.model(M), cloud, cen[1:2], (1, 1, 1), gt_rpy(), (0.0, 0.0, 0.0), name)
        assert res.best == 0 and res.accepted and res.n_inliers > 0.8 * M
    else:
        tgm.step(t, cloud, match=False)
        res, sc, _ = check_against_oracle(orc, t, tgm.model(M), cloud, cen, (1, 1, 4), gt_rpy(), (0.0, 0.0, TWO_PI), name)
        if M > 1:  # (one model point can lie within 2 cm of the frame at a decoy as well)
            assert res.best_centre == 1
            assert sc["n_inliers"][4:8].max() > 2 * max(sc["n_inliers"][:4].max(), sc["n_inliers"][8:].max(), 1)
    t.close()


def test_more_candidates_than_the_handle_has_particles(gpu, orc):
    """K = 81 (3 centres x 3 x 3 x 3) on a handle of 16 particles: nothing of the call lives in particle_num-sized buffers"""
    t = gpu.make_reference_tracker(particle_num=16, seed=3)
    t.setReferenceCloud(tgm.model())
    t.setTrans(tgm._world()["trans"])
    cloud = tgm.frame(1)
    tgm.step(t, cloud, match=False)
    before = tgm.snapshot(t)
    res, sc, _ = check_against_oracle(orc, t, tgm.model(), cloud, centres_of(cloud), (3, 3, 3), gt_rpy(), (0.4, 0.4, 0.8), "K81")
    assert res.n_candidates == 81 and res.best_centre == 1
    assert tgm.snapshot(t) == before
    # a smaller call afterwards reuses the buffers
    check_against_oracle(orc, t, tgm.model(), cloud, centres_of(cloud)[:2], (1, 1, 2), gt_rpy(), (0.0, 0.0, 0.5), "K4 after K81")
    t.close()


def test_on_a_tree_deeper_than_ten_levels(gpu, orc):
    ref, cloud = tgm.scattered(1200, 10.0, 1)
    t = tgm.make(gpu, reference=ref, trans=np.eye(4, dtype=np.float32))
    tgm.step(t, cloud, match=False)
    cen = np.array([[0.0, 0.0, 0.0], [0.004, -0.003, 0.002]], np.float32)
    res, sc, E = check_against_oracle(orc, t, ref, cloud, cen, (1, 1, 3), (0.0, 0.0, 0.0), (0.0, 0.0, 0.02), "deep")
    assert E["octree_depth"] > 10 and res.n_crop == len(cloud)
    assert sc["n_matched"].max() > 200
    t.close()


# ---- 2. the same bits as pft_match ---------------------------------------------------------------------------------------
def test_same_bits_as_the_match_of_the_same_pose(gpu):
    """the scattered scene: the model holds the corners of the cloud's box grown by 0.3 m, so the crop of the frame's
    particles and the crop of the single candidate are both the whole cloud -- the same points in the same order, the same
    tree -- and the result pose as the only candidate gives pft_match's statistics bit for bit"""
    ref, cloud = tgm.scattered(1200, 10.0, 1)
    t = tgm.make(gpu, reference=ref, trans=np.eye(4, dtype=np.float32))
    tgm.step(t, cloud)
    st = t.getMatch()
    r = t.getResult()
    res = t.reacquire(centres=[[r["x"], r["y"], r["z"]]], n=(1, 1, 1), span=(0.0, 0.0, 0.0),
                      base_rpy=(r["roll"], r["pitch"], r["yaw"]), apply=False)
    print("match %d / %.17g / %.17g, reacquire %d / %.17g / %.17g" % (st.n_matched, st.coherence, st.sum_sq_dist, res.n_matched,
                                                                        res.coherence, res.sum_sq_dist))
    assert st.evaluated and st.n_crop == len(cloud) == res.n_crop, "precondition: both crops are the whole cloud"
    assert res.transform.tobytes() == st.transform.tobytes()
    assert res.n_matched == st.n_matched and st.n_matched > 200
    assert res.coherence == st.coherence and res.sum_sq_dist == st.sum_sq_dist
    t.close()


# ---- 3. selection and ties ----------------------------------------------------------------------------------------------
def test_selection_and_the_lower_index_on_a_tie(gpu):
    t = tgm.make(gpu)
    cloud = tgm.frame(2)
    t.setInputCloud(cloud)
    cen = centres_of(cloud)
    twice = np.stack([cen[0], cen[1], cen[2], cen[1]])  # the object's centre at 1 and again at 3
    res = t.reacquire(centres=twice, n=(1, 1, 8), span=(0.0, 0.0, TWO_PI), base_rpy=gt_rpy(), apply=False)
    sc = t.getReacquireScores()
    check_result_is_the_selection(res, sc, 300, 0.5, 8)
    assert sc["n_inliers"][8:16].tolist() == sc["n_inliers"][24:32].tolist()
    assert sc["inlier_sq_dist"][8:16].tobytes() == sc["inlier_sq_dist"][24:32].tobytes()
    assert res.best_centre == 1 and res.accepted
    strict = t.reacquire(centres=twice, n=(1, 1, 8), span=(0.0, 0.0, TWO_PI), base_rpy=gt_rpy(), accept_ratio=1.0, apply=True)
    assert strict.best == res.best and not strict.accepted and not strict.applied
    t.close()


# ---- 4. recovery end to end ---------------------------------------------------------------------------------------------
def test_recovery_end_to_end(gpu):
    """the tracker's seed is one with which the jump is lost with room to spare: half a metre leaves the object's near edge
    at the 10 cm gate's reach, the particles crawl after it, and with some seeds (3, the default of these tests, among them:
    107 and then exactly 150 of 300 matched) the second frame is not below one half.  With seed 10 the device matches 58, 102
    and 111 points in the three frames after the jump (the CPU oracle, searching the result's own crop: 40, 93, 102)"""
    t = tgm.make(gpu, seed=10)
    t.setMatchThreshold(0.5, 2)
    for f in range(3):
        tgm.step(t, tgm.frame(f))
        assert not t.isLost()
    for f in (3, 4):  # the object, and everything else, half a metre further
        tgm.step(t, tgm.frame(f, shift=0.5))
    assert t.isLost()
    cloud = tgm.frame(4, shift=0.5)
    res = t.reacquire(centres=centres_of(cloud, shift=0.5))  # the defaults: 8 yaw steps around the current trans, apply
    print("recovery: best %d centre %d inliers %d matched %d" % (res.best, res.best_centre, res.n_inliers, res.n_matched))
    assert res.accepted and res.applied and res.best_centre == 1
    assert not t.getMatch().lost, "the streak is cleared with the restart"
    fresh = tgm.make(gpu, seed=10, trans=res.trans)
    for f in range(5, 10):
        c = tgm.frame(f, shift=0.5)
        tgm.step(t, c)
        tgm.step(fresh, c, match=False)
        assert tgm.snapshot(t) == tgm.snapshot(fresh), f
        assert not t.isLost(), f
    assert t.getMatch().n_matched >= 150
    t.close()
    fresh.close()


# ---- 5. apply=False leaves the tracker alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("kld", [False, True])
def test_without_apply_the_tracker_is_left_alone(gpu, kld):
    a, b = tgm.make(gpu, kld=kld), tgm.make(gpu, kld=kld)
    a.setMatchThreshold(1.0, 1)
    b.setMatchThreshold(1.0, 1)
    for f in range(2):
        tgm.step(a, tgm.frame(f))
        tgm.step(b, tgm.frame(f))
    streak = a.getMatch().streak
    res = a.reacquire(centres=centres_of(tgm.frame(1)), base_rpy=gt_rpy(), apply=False)
    assert res.accepted and not res.applied
    with pytest.raises(gpu.PftError) as e:
        a.computeMatch()
    assert e.value.status == 7 and "not the last pft_compute's" in str(e.value)
    assert a.getMatch().streak == streak == b.getMatch().streak
    assert tgm.snapshot(a) == tgm.snapshot(b)
    for f in range(2, 5):
        tgm.step(a, tgm.frame(f))
        tgm.step(b, tgm.frame(f))
        assert tgm.snapshot(a) == tgm.snapshot(b), f
        ma, mb = a.getMatch(), b.getMatch()
        assert (ma.n_matched, ma.coherence, ma.streak, ma.calls) == (mb.n_matched, mb.coherence, mb.streak, mb.calls), f
    a.close()
    b.close()


# ---- 6. from a segmenter ------------------------------------------------------------------------------------------------
def test_from_a_segmenter(gpu, orc):
    from pcl_tracking_amd import segment

    seg = segment.make_scene_segmenter()
    seg.setInputCloud(scene.make_scene(50000))
    seg.apply()
    clusters = seg.clusters()
    assert len(clusters) >= 2
    want = np.stack([orc.compute_3d_centroid(pts)[0][:3] for _, pts in clusters]).astype(np.float32)
    t = tgm.make(gpu)
    t.setInputCloud(tgm.frame(0))
    kw = dict(n=(1, 1, 2), span=(0.0, 0.0, 0.6), base_rpy=gt_rpy(), apply=False)
    a = t.reacquire(segmenter=seg, **kw)
    sa = t.getReacquireScores()
    print("segmenter: %d clusters, K %d, best centre %d inliers %d" % (len(clusters), a.n_candidates, a.best_centre, a.n_inliers))
    assert a.n_centres == len(clusters) and a.n_candidates == 2 * len(clusters)
    assert sa["centres"].tobytes() == want.tobytes(), "compute3DCentroid of every cluster, bit for bit"
    b = t.reacquire(centres=want, **kw)
    sb = t.getReacquireScores()
    for f in sa:
        assert sa[f].tobytes() == sb[f].tobytes(), f
    assert (a.best, a.best_centre, a.n_inliers, a.n_matched, a.accepted, a.n_crop) == (b.best, b.best_centre, b.n_inliers,
                                                                                        b.n_matched, b.accepted, b.n_crop)
    assert a.pose.tobytes() == b.pose.tobytes() and a.transform.tobytes() == b.transform.tobytes()
    assert (a.coherence, a.sum_sq_dist, a.inlier_sq_dist) == (b.coherence, b.sum_sq_dist, b.inlier_sq_dist)
    # a segmenter without clusters
    none = segment.ModelSegmenter()
    none.configure(plane=False, box_enable=(0, 0, 0), tolerance=0.02, min_size=100000, max_size=200000)
    none.setInputCloud(tgm.frame(0))
    none.apply()
    assert len(none.clusterSizes()) == 0
    r = t.reacquire(segmenter=none, **kw)
    assert (r.n_centres, r.n_candidates, r.best, r.best_centre, r.accepted, r.applied) == (0, 0, -1, -1, False, False)
    assert len(t.getReacquireScores()["candidates"]) == 0
    t.close()
    seg.close()
    none.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def refused(gpu, call, status, text):
    with pytest.raises(gpu.PftError) as e:
        call()
    assert e.value.status == status and text in str(e.value), (status, text, str(e.value))


def test_refusals(gpu):
    from pcl_tracking_amd import segment

    one = np.zeros((1, 3), np.float32)
    s = gpu.ParticleFilterTracker(world_size=2)
    s.setParticleNum(tgm.P)
    s.setReferenceCloud(tgm.model())
    s.setInputCloud(tgm.frame(0))
    refused(gpu, lambda: s.reacquire(centres=one), 1, "sharded")
    s.close()

    x = gpu.make_reference_tracker(particle_num=tgm.P)
    x.setCloudCoherence(tgm._exact_coherence(gpu))
    x.setReferenceCloud(tgm.model())
    x.setInputCloud(tgm.frame(0))
    refused(gpu, lambda: x.reacquire(centres=one), 1, "exact")
    x.close()

    t = tgm.make(gpu)
    refused(gpu, lambda: t.reacquire(centres=one), 2, "")  # no input cloud yet
    t.setInputCloud(tgm.frame(0))
    for kw in (dict(n=(0, 1, 8)), dict(n=(1, 1, -1)), dict(span=(0.0, 0.0, -1.0)), dict(span=(0.0, np.inf, 1.0)),
               dict(base_rpy=(np.nan, 0.0, 0.0)), dict(inlier_distance=0.0), dict(inlier_distance=0.2),
               dict(accept_ratio=1.5), dict(accept_ratio=-0.1)):
        refused(gpu, lambda: t.reacquire(centres=one, **kw), 1, "bad configuration value")
    refused(gpu, lambda: t.reacquire(centres=[[0.0, np.nan, 0.0]]), 1, "non-finite")
    refused(gpu, lambda: t.reacquire(centres=[[0.0, 0.0, 0.0], [np.inf, 0.0, 0.0]]), 1, "centre 1")
    refused(gpu, lambda: t.reacquire(centres=np.zeros((2, 3), np.float32), n=(1, 256, 256)), 6, "PFT_REACQUIRE_MAX_CANDIDATES")
    never = segment.ModelSegmenter()
    never._ensure()  # a handle that has not been applied
    refused(gpu, lambda: t.reacquire(segmenter=never), 7, "not been applied")
    never.close()
    # after every refusal the handle still works
    assert t.reacquire(centres=centres_of(tgm.frame(0)), base_rpy=gt_rpy(), apply=False).accepted

    import torch

    other = segment.ModelSegmenter(device_id=1)
    other.configure(plane=False, box_enable=(0, 0, 0), min_size=100)
    other.setInputCloud(tgm.frame(0))
    if torch.cuda.device_count() < 2:
        # one device: a segmenter on another device cannot come into being (pft_segment_create refuses the ordinal), which
        # is all there is to check of that refusal here; with two devices the call itself is refused below
        with pytest.raises(gpu.PftError):
            other.apply()
    else:
        other.apply()
        refused(gpu, lambda: t.reacquire(segmenter=other), 1, "lives on device 1")
        other.close()
    t.close()

    n = gpu.make_reference_tracker(particle_num=tgm.P)
    n.setInputCloud(tgm.frame(0))
    refused(gpu, lambda: n.reacquire(centres=one), 3, "")  # no reference cloud
    n.close()


# ---- 8. the C++ path ----------------------------------------------------------------------------------------------------
def test_cpp_driver_reacquires_an_object_that_jumped(gpu, tmp_path):
    """three frames with the object where its model was cut out, then seven with everything half a metre further: the match
    rule (0.5, 2) reports the loss at frame 5, the frame's clusters (0.04 m, at least 100 points: the object and a piece of
    background) are scored at 9 yaw steps -- an odd number, so that the object's own orientation is among them --, the object
    is found at the object's cluster, and no later frame reports a loss"""
    from pcl_tracking_amd import build

    w = tgm._world()
    cluster = w["obj"][np.random.default_rng(7).choice(2000, 300, replace=False)]
    tgm.write_pcd(str(tmp_path / "model.pcd"), cluster)
    paths = []
    for f in range(10):
        paths.append(str(tmp_path / ("frame%d.pcd" % f)))
        tgm.write_pcd(paths[-1], tgm.frame(f, shift=0.0 if f < 3 else 0.5))
    r = subprocess.run([build.build_example(), str(tmp_path / "model.pcd"), "--frames"] + paths +
                       ["--particles", str(tgm.P), "--seed", "1", "--model-leaf", "0", "--match=0.5,2", "--reacquire=9",
                        "--no-plane", "--box", "-10,10,-10,10,-10,10", "--tolerance", "0.04", "--min-size", "100"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    at = [i for i, ln in enumerate(out) if ln.startswith("reacquire obj 0:")]
    assert len(at) == 1
    words = out[at[0]].split()
    assert words[-2:] == ["accepted", "1"] and words[3] == "centre" and int(words[4]) >= 0
    n, M = (int(v) for v in words[8].split("/"))
    assert M == 300 and n >= 150
    said = [int(ln.split()[1]) for ln in r.stderr.splitlines() if ln.endswith("Object not recognized")]
    assert said == [5], "lost once, at the second shifted frame; never again after the restart"
    later = [ln.split() for ln in out[at[0]:] if " match " in ln]
    assert len(later) == 5 and all(ln[-1] == "0" for ln in later)

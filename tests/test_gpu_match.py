"""GPU checks of the match statistics of the result pose (pft_match; k_match in pcl_tracking_amd/csrc/pft_match.hip), the
lost rule and resetTracking: the device against the CPU oracle's search at the device's own transform and crop box, pair
by pair and bit by bit; the sums against tests/match_model.py; the lost rule against the model driven by the device's own
counts; frames that are not evaluated; no side effects on the tracker; resetTracking against a fresh handle; the refusals;
and the C++ path (the driver's --match and compute() throwing PFT_ERR_LOST).

Sizes: a model of 300 points, frames of about 4 000 points, 64 particles (KLD: at most 100), 2 iterations.  The frames
hold the object as a denser sample of the model's own surface at the ground-truth pose plus background of the synthetic
scene, so that the matched share is near 1 with the object and 0 without it whatever the particles do."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import match_model as mm
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("x", "y", "z", "roll", "pitch", "yaw")
P = 64
SEQUENCE = [1, 1, 1, 0, 0, 0, 0, 1, 1, 1]  # object present, absent for four frames, back


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


@functools.lru_cache(maxsize=None)
def _world():
    full = scene.make_scene(50000)
    gtp = scene.model_gt_pose()
    gt = np.array(gtp[:3])
    xyz = np.stack([full["x"], full["y"], full["z"]], 1)
    far = np.flatnonzero(np.linalg.norm(xyz - gt, axis=1) >= 0.6)
    dense = scene.make_model(2000)
    T = scene.pose_matrix(*gtp)
    moved = (np.stack([dense["x"], dense["y"], dense["z"]], 1).astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    obj = dense.copy()
    obj["x"], obj["y"], obj["z"] = moved[:, 0], moved[:, 1], moved[:, 2]
    return dict(full=full, far=far, obj=obj, gt=gt, trans=T.astype(np.float32))


@functools.lru_cache(maxsize=None)
def frame(f, present=True, half=False, shift=0.0):
    """1 500 points of the object (none when absent; the x <= centre half when half) and 2 500 of the background"""
    w = _world()
    rng = np.random.default_rng(100 + f)
    o = w["obj"][rng.choice(2000, 1500, replace=False)]
    if not present:
        o = o[:0]
    if half:
        o = o[o["x"] <= w["gt"][0]]
    c = np.concatenate([o, w["full"][rng.choice(w["far"], 2500, replace=False)]])
    c = c[rng.permutation(len(c))]
    c["x"] += np.float32(shift)
    return c


@functools.lru_cache(maxsize=None)
def model(M=300):
    return scene.make_model(M)


def other_trans():
    t = _world()["trans"].copy()
    t[:3, 3] += np.array([0.02, -0.015, 0.01], np.float32)
    return t


def make(gpu, M=300, kld=False, seed=3, iterations=2, trans=None, reference=None, cd=None, coherence=None):
    """coherence: dict(hsv_weight, h_weight, s_weight, v_weight) in place of the reference's 0.1, 1, 1, 0"""
    t = gpu.make_reference_tracker(particle_num=P, seed=seed, kld=kld, change_detector=cd)
    if coherence:
        coh = gpu.ApproxNearestPairPointCloudCoherence()
        coh.addPointCoherence(gpu.DistanceCoherence())
        hc = gpu.HSVColorCoherence()
        hc.setWeight(coherence.get("hsv_weight", 0.1))
        hc.setHWeight(coherence.get("h_weight", 1.0))
        hc.setSWeight(coherence.get("s_weight", 1.0))
        hc.setVWeight(coherence.get("v_weight", 0.0))
        coh.addPointCoherence(hc)
        coh.setSearchMethod(gpu.OctreeSearch(0.01))
        coh.setMaximumDistance(0.1)
        t.setCloudCoherence(coh)
    if kld:
        t.setMaximumParticleNum(100)
    t.setIterationNum(iterations)
    t.setReferenceCloud(model(M) if reference is None else reference)
    t.setTrans(_world()["trans"] if trans is None else trans)
    return t


def oracle_cfg(orc, coherence=None):
    return orc.default_config(particle_num=P, threads=0, emulate_pcl_alloc=0, **(coherence or {}))


def get_bbox(t):
    b = np.zeros(6, np.float32)
    t._check(t._L.pft_debug_get_bbox(t._h, b.ctypes.data))
    return b


def step(t, cloud, match=True):
    t.setInputCloud(cloud)
    t.compute()
    if match:
        t.computeMatch()


def oracle_stats(orc, t, reference, cloud, st, coherence=None):
    """the oracle's search for the device's own transform and crop box, turned into pft_match's outputs by the model"""
    cfg = oracle_cfg(orc, coherence)
    o = orc.Tracker(cfg)
    o.set_reference(reference)
    o.set_input(cloud)
    E = o.eval_weights(np.array([t.getResult()]), want_nn=True, mats=st.transform[None], bbox=get_bbox(t))
    return E, mm.stats(orc, cfg, reference, st.transform, cloud, E["nn_idx"][0], E["nn_d2"][0], E["crop_idx"])


def check_against_oracle(orc, t, reference, cloud, label, coherence=None):
    st = t.getMatch()
    idx, d2 = t.getMatchPairs()
    E, want = oracle_stats(orc, t, reference, cloud, st, coherence)
    M = len(reference)
    assert st.evaluated and st.n_reference == M and len(idx) == M and len(d2) == M, label
    assert st.n_crop == want["n_crop"], label
    assert d2.tobytes() == want["sq_dist"].tobytes(), label
    assert idx.tolist() == want["input_idx"].tolist(), label
    assert st.n_matched == want["n_matched"], label
    # the terms are the same bits and non-negative: a chain of M adds and a tree each err by at most M * 2^-53 of the
    # sum; 64 is slack for the padding levels
    bound = (M + 64) * 2.0 ** -53
    for got, ref in ((st.coherence, want["coherence"]), (st.sum_sq_dist, want["sum_sq_dist"])):
        rel = abs(got - ref) / ref if ref else abs(got)
        print("%s: device %.17g model %.17g rel %.3g bound %.3g" % (label, got, ref, rel, bound))
        assert rel <= bound, label
    # the device's own order: adjacent-pair trees over the handle's stored positions, bit for bit
    assert st.coherence == want["coherence_tree"], label
    assert st.sum_sq_dist == want["sum_sq_dist_tree"], label
    return st, want, E


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------
VARIANTS = {
    "builder_single": dict(env={"PFT_FORCE_BUILDER": "single"}),
    "builder_sorted": dict(env={"PFT_FORCE_BUILDER": "sorted"}),
    "leaf_direct": dict(env={"PFT_LEAF_INDIRECT": "0"}),
    "leaf_indirect": dict(env={"PFT_LEAF_INDIRECT": "1"}),
    "kld": dict(kld=True),
    "M1": dict(M=1),
    "M1025": dict(M=1025),  # a one-point tail round
    "M2049": dict(M=2049),  # three 1024-position tiles: the fold joins two pending subtrees (levels 1 and 0)
    "M3073": dict(M=3073),  # four tiles: the push at tile 3 merges two levels
    "half_object": dict(half=True),  # some pairs outside the gate
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_match_against_the_oracle(gpu, orc, monkeypatch, name):
    v = VARIANTS[name]
    for k, val in v.get("env", {}).items():  # the switches are latched at pft_create
        monkeypatch.setenv(k, val)
    M = v.get("M", 300)
    t = make(gpu, M=M, kld=v.get("kld", False))
    matched = []
    for f in range(3):
        cloud = frame(f, half=v.get("half", False))
        step(t, cloud)
        st, want, _ = check_against_oracle(orc, t, model(M), cloud, "%s frame %d" % (name, f))
        assert st.calls == f + 1
        matched.append(st.n_matched)
    if name == "half_object":
        assert any(0 < n < M for n in matched), "the case holds pairs on both sides of the gate"
    elif M > 1:
        assert min(matched) > 0.8 * M
    t.close()


def scattered(n_loc, span, seed):
    """points on random locations of a span^3 box and a 256-point model of some of them plus the corners of the box grown
    by 0.3 m: particles near the identity crop the whole cloud (the `u16_no_table` inputs of the likelihood's layout cases)"""
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(0, span, (n_loc, 3)) + np.array([-span / 2, -span / 2, 1.0])).astype(np.float32)
    cloud = scene.make_points(xyz, rng.integers(0, 256, (n_loc, 3)))
    lo, hi = xyz.min(0) - 0.3, xyz.max(0) + 0.3
    corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], np.float32)
    mxyz = np.concatenate([xyz[rng.choice(n_loc, 248, replace=False)], corners])
    return scene.make_points(mxyz, rng.integers(0, 256, (256, 3))), cloud


def test_match_on_a_tree_deeper_than_ten_levels(gpu, orc):
    """1 200 points over 10 m at 1 cm leaves: 11 levels, no centre tables in the likelihood"""
    ref, cloud = scattered(1200, 10.0, 1)
    t = make(gpu, reference=ref, trans=np.eye(4, dtype=np.float32))
    for f in range(3):
        step(t, cloud)
        st, want, E = check_against_oracle(orc, t, ref, cloud, "deep frame %d" % f)
        assert E["octree_depth"] > 10
        assert st.n_crop == len(cloud)
    t.close()


@pytest.mark.parametrize("coherence", [dict(hsv_weight=4.0, v_weight=1.0),
                                       dict(hsv_weight=4.0, h_weight=0.5, s_weight=2.0, v_weight=1.0)], ids=["hsv111", "hsv0.5_2_1"])
def test_match_pair_values_on_edge_colours(gpu, orc, coherence):
    """mt_pair_value (k_match; k_reacquire_score calls the same function) on the colours of tests/colour_cases.py: the
    reference cycles REFS, the frame holds the same locations coloured by TARGETS, permuted; hsv_weight 4 and v_weight 1
    make every channel count, and three different channel weights tell the channels apart.  The sums are compared in
    double, so one wrong term shows"""
    import colour_cases as cc

    ref, cloud = scattered(256, 2.0, 5)  # (248 of the frame's locations and the corners of their box)
    rrgba, trgba = cc.refs()[1], cc.targets()[1]
    ref["rgba"] = rrgba[np.arange(256) % len(rrgba)]
    cloud["rgba"] = trgba[np.random.default_rng(7).permutation(256)]
    t = make(gpu, reference=ref, trans=np.eye(4, dtype=np.float32), coherence=coherence)
    for f in range(2):
        step(t, cloud)
        st, want, E = check_against_oracle(orc, t, ref, cloud, "colours frame %d" % f, coherence)
        print("colours frame %d: %d of 256 matched, coherence %.6f" % (f, st.n_matched, st.coherence))
        assert st.n_crop == len(cloud) and st.n_matched >= 128
        # colours that matter: the sum is well below the count of matched pairs
        assert st.coherence < 0.9 * st.n_matched
    t.close()


# ---- 2. empty crop ------------------------------------------------------------------------------------------------------
def test_empty_crop_is_evaluated_with_nothing_matched(gpu):
    t = make(gpu)
    step(t, frame(0))
    assert t.getMatch().n_matched > 0
    step(t, frame(1, shift=5.0))  # the frame moved metres away
    st = t.getMatch()
    idx, d2 = t.getMatchPairs()
    assert st.evaluated and st.n_crop == 0 and st.n_matched == 0 and st.calls == 2
    assert st.coherence == 0.0 and st.sum_sq_dist == 0.0
    assert (idx == -1).all() and np.isinf(d2).all() and len(idx) == 300
    t.synchronize()  # no error
    t.close()


# ---- 3. the lost rule ---------------------------------------------------------------------------------------------------
def run_sequence(gpu, orc, thr):
    t = make(gpu)
    t.setMatchThreshold(*thr)
    rule = mm.LostRule(*thr)
    out = []
    for f, present in enumerate(SEQUENCE):
        cloud = frame(f, present=bool(present))
        step(t, cloud)
        st = t.getMatch()
        if orc is not None:  # the scene does what the test needs, by the oracle's count
            _, want = oracle_stats(orc, t, model(), cloud, st)
            ratio = want["n_matched"] / 300.0
            assert ratio > 0.8 if present else ratio < 0.2, (f, ratio)
        assert (st.below, st.streak, st.lost) == rule.step(st.n_matched, 300), f
        assert st.evaluated and st.calls == f + 1
        out.append(st.lost)
    assert t.isLost() == out[-1]
    t.close()
    return out


@pytest.mark.parametrize("thr", [(0.5, 1), (0.5, 3)])
def test_lost_rule_follows_the_model(gpu, orc, thr):
    lost = run_sequence(gpu, orc, thr)
    absent = [not p for p in SEQUENCE]
    if thr[1] == 1:
        assert lost == absent
    else:
        assert lost == [False] * 5 + [True, True] + [False] * 3  # the third absent frame on


# ---- 4. skipped and failed iterations -----------------------------------------------------------------------------------
def same_but(a, b, calls):
    """b is a's statistics kept: evaluated 0, calls advanced, everything else the last evaluated frame's"""
    assert not b.evaluated and b.calls == calls
    assert b.transform.tobytes() == a.transform.tobytes()
    assert (b.coherence, b.sum_sq_dist, b.n_reference, b.n_matched, b.n_crop) == (a.coherence, a.sum_sq_dist, a.n_reference,
                                                                               a.n_matched, a.n_crop)
    assert (b.below, b.streak, b.lost) == (a.below, a.streak, a.lost)


def test_skipped_last_iteration_is_not_evaluated(gpu):
    t = make(gpu)
    # every iteration would be tested (interval 0), and no voxel ever holds 100 000 new points: once the detector is in
    # use the iterations are skipped.  Set before the first frame, so that no count-down is pending when it is turned on
    t.setMinPointsOfChangeDetection(100000)
    t.setIntervalOfChangeDetection(0)
    t.setMatchThreshold(1.0, 1)
    step(t, frame(0))
    step(t, frame(1, present=False))  # below: a streak to keep
    a = t.getMatch()
    pairs = [x.copy() for x in t.getMatchPairs()]
    assert a.evaluated and a.calls == 2 and a.streak >= 1
    t.setUseChangeDetector(True)
    for k in range(2):
        step(t, frame(2 + k))
        ring = t.debugChangeState()["ring"]
        assert ring[-1][0] == 1 and ring[-1][1] == 0, "precondition: the last iteration was tested and skipped"
        same_but(a, t.getMatch(), 3 + k)
        got = t.getMatchPairs()
        assert got[0].tobytes() == pairs[0].tobytes() and got[1].tobytes() == pairs[1].tobytes()
    t.setUseChangeDetector(False)
    step(t, frame(4))
    b = t.getMatch()
    assert b.evaluated and b.calls == 5
    t.close()


def test_failed_last_iteration_is_not_evaluated_and_reported_once(gpu):
    t = make(gpu, iterations=1)  # the injection lands behind the NEXT crop: with one iteration that is the frame's last
    t.setMatchThreshold(0.5, 1)
    step(t, frame(0))
    a = t.getMatch()
    assert a.evaluated and a.calls == 1
    t.debugInjectError(4)
    step(t, frame(1))
    with pytest.raises(gpu.PftError) as e:
        t.getMatch()
    assert e.value.status == 5 and "bit2" in str(e.value)
    same_but(a, t.getMatch(), 2)  # reported once
    step(t, frame(2))  # per iteration, not sticky
    b = t.getMatch()
    assert b.evaluated and b.calls == 3
    t.close()


def test_new_reference_forgets_the_pairs_until_a_match_is_evaluated(gpu):
    t = make(gpu, iterations=1)
    step(t, frame(0))
    assert t.getMatch().n_matched > 0 and len(t.getMatchPairs()[0]) == 300
    t.setReferenceCloud(model(1025))  # larger: the pair arrays are allocated anew
    with pytest.raises(gpu.PftError) as e:
        t.getMatchPairs()
    assert e.value.status == 7
    t.debugInjectError(4)
    step(t, frame(1))  # this match is not evaluated
    with pytest.raises(gpu.PftError):
        t.getMatch()
    st = t.getMatch()
    idx, d2 = t.getMatchPairs()
    assert not st.evaluated and st.calls == 2 and (st.n_reference, st.n_matched, st.n_crop) == (1025, 0, 0)
    assert st.coherence == 0.0 and st.sum_sq_dist == 0.0
    assert len(idx) == 1025 and (idx == -1).all() and np.isinf(d2).all()
    step(t, frame(2))
    st = t.getMatch()
    assert st.evaluated and st.n_reference == 1025 and st.n_matched > 0.8 * 1025
    assert (t.getMatchPairs()[0] >= 0).sum() == st.n_matched
    t.close()


# ---- 5. no side effects -------------------------------------------------------------------------------------------------
def snapshot(t):
    return t.getResult().tobytes(), t.getParticles().tobytes(), t.getFitRatio()


@pytest.mark.parametrize("kld", [False, True])
def test_match_leaves_the_tracker_alone(gpu, kld):
    a, b = make(gpu, kld=kld), make(gpu, kld=kld)
    for f in range(8):
        step(a, frame(f % 4), match=True)
        step(b, frame(f % 4), match=False)
        assert snapshot(a) == snapshot(b), f
    assert a.getMatch().calls == 8
    a.close()
    b.close()


def test_four_handles_in_flight_equal_each_alone(gpu):
    def outputs(t):
        st = t.getMatch()
        idx, d2 = t.getMatchPairs()
        return (snapshot(t), st.transform.tobytes(), st.coherence, st.sum_sq_dist, st.n_matched, st.n_crop, st.calls,
                idx.tobytes(), d2.tobytes())

    alone = []
    for k in range(4):
        t = make(gpu, seed=10 + k)
        per_frame = []
        for f in range(3):
            step(t, frame(f))
            per_frame.append(outputs(t))
        alone.append(per_frame)
        t.close()
    ts = [make(gpu, seed=10 + k) for k in range(4)]
    for f in range(3):
        for t in ts:  # compute and match of all four enqueued before anyone synchronises
            step(t, frame(f))
        for k, t in enumerate(ts):
            assert outputs(t) == alone[k][f], (k, f)
    for t in ts:
        t.close()


# ---- 6. resetTracking ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kld", [False, True])
def test_reset_tracking_equals_a_fresh_handle(gpu, kld):
    t = make(gpu, kld=kld)
    t.setMatchThreshold(0.5, 2)
    for f in range(3):
        step(t, frame(f, present=False))
    st = t.getMatch()
    assert (st.below, st.streak, st.lost) == (True, 3, True)
    t.setTrans(other_trans())
    t.resetTracking()
    st = t.getMatch()
    assert (st.below, st.streak, st.lost) == (False, 0, False), "the streak is cleared"
    fresh = make(gpu, kld=kld, trans=other_trans())
    for f in range(3, 6):
        step(t, frame(f))
        step(fresh, frame(f), match=False)
        assert snapshot(t) == snapshot(fresh), f
    st = t.getMatch()
    assert st.evaluated and st.calls == 6 and st.n_matched > 240 and not st.lost
    t.close()
    fresh.close()


def test_reset_tracking_keeps_the_change_detector(gpu):
    t = make(gpu, cd=(1, 1, 0.01))
    for f in range(3):
        step(t, frame(f))
    before = t.debugChangeState()
    assert before["n_calls"] == 6
    t.resetTracking()
    kept = t.debugChangeState()
    assert kept["n_calls"] == 6 and kept["ring"].tolist() == before["ring"].tolist()
    assert kept["box"].tobytes() == before["box"].tobytes() and kept["counter"] == before["counter"]
    for f in range(3, 6):
        step(t, frame(f))
    after = t.debugChangeState()
    assert after["n_calls"] == 12 and after["ring"][:6].tolist() == before["ring"].tolist()
    r = t.getResult()
    assert all(np.isfinite(r[k]) for k in KEYS)
    assert t.getMatch().evaluated or after["ring"][-1][1] == 0
    t.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def _exact_coherence(gpu):
    c = gpu.NearestPairPointCloudCoherence()
    c.addPointCoherence(gpu.DistanceCoherence())
    h = gpu.HSVColorCoherence()
    h.setWeight(0.1)
    c.addPointCoherence(h)
    c.setSearchMethod(gpu.OctreeSearch(0.01))
    c.setMaximumDistance(0.1)
    return c


def test_refusals(gpu):
    s = gpu.ParticleFilterTracker(world_size=2)
    s.setParticleNum(P)
    s.setReferenceCloud(model())
    s.setInputCloud(frame(0))
    with pytest.raises(gpu.PftError) as e:
        s.computeMatch()
    assert e.value.status == 1 and "sharded" in str(e.value)
    s.resetTracking()  # host state only: works on a sharded handle
    s.close()

    x = gpu.make_reference_tracker(particle_num=P)
    x.setCloudCoherence(_exact_coherence(gpu))
    x.setReferenceCloud(model())
    x.setTrans(_world()["trans"])
    x.setInputCloud(frame(0))
    x.compute()
    with pytest.raises(gpu.PftError) as e:
        x.computeMatch()
    assert e.value.status == 1 and "exact" in str(e.value)
    x.close()

    t = make(gpu)
    t.setInputCloud(frame(0))
    with pytest.raises(gpu.PftError) as e:
        t.computeMatch()
    assert e.value.status == 7 and "before the first pft_compute" in str(e.value)
    with pytest.raises(gpu.PftError) as e:
        t.getMatch()
    assert e.value.status == 7
    t.compute()
    t.computeMatch()
    assert t.getMatch().evaluated
    hooks = {
        "evalWeights": lambda: t.evalWeights(t.getParticles()[:8]),
        "setParticles": lambda: t.setParticles(t.getParticles()),
        "setReferenceCloud": lambda: t.setReferenceCloud(model()),
    }
    for name, hook in hooks.items():  # whatever rebuilt the tree, or replaced what it was built for
        hook()
        with pytest.raises(gpu.PftError) as e:
            t.computeMatch()
        assert e.value.status == 7 and "not the last pft_compute's" in str(e.value), name
        t.compute()
        t.computeMatch()
        assert t.getMatch().evaluated, name
    t.debugStateSave()
    t.compute()
    t.debugStateRestore()
    with pytest.raises(gpu.PftError) as e:
        t.computeMatch()
    assert e.value.status == 7
    with pytest.raises(gpu.PftError) as e:
        t.setMatchThreshold(1.5, 1)
    assert e.value.status == 1
    t.close()


# ---- 8. the C++ path ----------------------------------------------------------------------------------------------------
def write_pcd(path, cloud):
    """PCD v0.7 binary with FIELDS x y z rgba, as pcl::PCDWriter lays it out"""
    n = len(cloud)
    hdr = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgba\nSIZE 4 4 4 4\nTYPE F F F U\n"
           "COUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (n, n))
    rec = np.zeros(n, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")]))
    for k in ("x", "y", "z", "rgba"):
        rec[k] = cloud[k]
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(rec.tobytes())


@pytest.fixture(scope="module")
def cpp_case(gpu, orc, tmp_path_factory):
    """a 300-point object cluster in the camera frame, the sequence of test 3, and the frames the Python path -- with the
    reference and trans the driver's "set object to track" step forms -- reports lost at --match=0.5,2"""
    w = _world()
    cluster = w["obj"][np.random.default_rng(7).choice(2000, 300, replace=False)]
    frames = [frame(f, present=bool(p)) for f, p in enumerate(SEQUENCE)]
    c, _ = orc.compute_3d_centroid(cluster)
    ref, trans = orc.recentre_model(cluster, c)
    t = make(gpu, seed=1, reference=ref, trans=trans)
    t.setMatchThreshold(0.5, 2)
    lost = []
    for cloud in frames:
        step(t, cloud)
        lost.append(t.isLost())
    t.close()
    assert lost == [False] * 4 + [True] * 3 + [False] * 3
    d = tmp_path_factory.mktemp("match_cpp")
    return dict(dir=d, cluster=cluster, frames=frames, lost=[f + 1 for f, v in enumerate(lost) if v])


def test_cpp_driver_prints_object_not_recognized_at_the_lost_frames(cpp_case):
    from pcl_tracking_amd import build

    d = cpp_case["dir"]
    write_pcd(str(d / "model.pcd"), cpp_case["cluster"])
    paths = []
    for f, cloud in enumerate(cpp_case["frames"]):
        paths.append(str(d / ("frame%d.pcd" % f)))
        write_pcd(paths[-1], cloud)
    r = subprocess.run([build.build_example(), str(d / "model.pcd"), "--frames"] + paths +
                       ["--particles", str(P), "--seed", "1", "--model-leaf", "0", "--match=0.5,2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    said = [int(ln.split()[1]) for ln in r.stderr.splitlines() if ln.endswith("Object not recognized")]
    assert said == cpp_case["lost"]
    lines = [ln.split() for ln in r.stdout.splitlines() if " match " in ln]
    assert len(lines) == len(SEQUENCE)
    assert [int(ln[1]) for ln in lines if ln[-1] == "1"] == cpp_case["lost"]


def test_cpp_compute_throws_lost_with_throw_on_failure(cpp_case, tmp_path):
    from pcl_tracking_amd import build

    d = cpp_case["dir"]
    cpp_case["cluster"].tofile(str(d / "model.bin"))
    paths = []
    for f, cloud in enumerate(cpp_case["frames"]):
        paths.append(str(d / ("frame%d.bin" % f)))
        cloud.tofile(paths[-1])
    exe = build.build_host_program(os.path.join(ROOT, "tests", "cpp", "match_throw_tool.cpp"), str(tmp_path / "match_throw_tool"))
    env = dict(os.environ, LD_LIBRARY_PATH=build.OUT_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, "0.5", "2", str(P), str(d / "model.bin")] + paths, capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("frame ")]
    assert len(got) == len(SEQUENCE)
    assert [int(g[1]) for g in got if g[2] == "threw"] == cpp_case["lost"]
    assert all(g[3] == "8" for g in got if g[2] == "threw")  # PFT_ERR_LOST

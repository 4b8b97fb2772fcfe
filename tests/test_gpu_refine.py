"""GPU checks of the pose refinement (pft_refine; pcl_tracking_amd/csrc/pft_refine.hip): every pass of the loop against
tests/refine_model.py driven by the CPU oracle's search at the device's own matrices and crop box -- the integers, all 17
sums, every T, the step sizes, the status and the scores bit for bit --; a fixed point; the default start; apply=False leaving
the tracker alone; apply=True equal to a fresh handle; reacquire(refine=True) end to end; the refusals; and the C++ driver's
--refine.

Sizes: models of at most 1 025 points, frames of about 4 000 points (test_gpu_match's), the default 16 iterations."""
import subprocess

import numpy as np
import pytest

import refine_model as rfm
import test_gpu_match as tgm
from pcl_tracking_amd import scene
from test_gpu_reacquire import centres_of, refused

pytestmark = pytest.mark.gpu
SCORES = ("n_pairs_before", "n_inliers_before", "sum_sq_dist_before", "inlier_sq_dist_before", "n_pairs_after",
          "n_inliers_after", "sum_sq_dist_after", "inlier_sq_dist_after")


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


def neighbour(orc, dyaw=np.pi / 8.0, shift=(0.0, 0.0, 0.0)):
    """the ground-truth pose with its yaw off by one half lattice step (22.5 degrees), as a 3x4"""
    p = list(scene.model_gt_pose())
    p[5] += dyaw
    for a in range(3):
        p[a] += shift[a]
    return np.asarray(orc.get_transformation(*p), np.float32).reshape(4, 4)[:3].copy()


def check_every_pass(orc, t, reference, cloud, start, label, **kw):
    """one device call against the model's loop: returns (device result, device trace, model result)"""
    res = t.refine(start=start, **kw)
    tr = t.getRefineTrace()
    ocfg = tgm.oracle_cfg(orc)
    o = orc.Tracker(ocfg)
    o.set_reference(reference)
    o.set_input(cloud)
    cfg = rfm.config(max_iterations=kw.get("max_iterations", 16), min_pairs=kw.get("min_pairs", 3),
                     pair_distance=kw.get("pair_distance") or ocfg.max_distance,
                     inlier_distance=kw.get("inlier_distance", 0.02), trans_eps=kw.get("trans_eps", 1e-4),
                     rot_eps=kw.get("rot_eps", 1e-3))
    want_tr, want = rfm.run(orc, o, reference, cloud, res.start, cfg, res.bbox)
    print("%s: M %d crop %d depth %d status %s iterations %d pairs %d -> %d inliers %d -> %d improved %d" % (
        label, len(reference), res.n_crop, want["octree_depth"], res.status_name, res.iterations, res.n_pairs_before,
        res.n_pairs_after, res.n_inliers_before, res.n_inliers_after, res.improved))
    if start is not None:
        assert res.start.tobytes() == np.ascontiguousarray(start, np.float32).reshape(-1)[:12].tobytes(), label
    assert res.n_reference == len(reference) and res.n_crop == want["n_crop"], label
    assert len(tr["n_pairs"]) == res.iterations + 1 == len(want_tr), (label, len(tr["n_pairs"]), len(want_tr))
    for k, w in enumerate(want_tr):
        assert tr["transform"][k].tobytes() == w["transform"].tobytes(), (label, k, "T")
        assert (int(tr["n_pairs"][k]), int(tr["n_inliers"][k])) == (w["n_pairs"], w["n_inliers"]), (label, k)
        assert rfm.bits(tr["sums"][k]).tolist() == rfm.bits(w["sums"]).tolist(), (label, k, "sums")
        assert rfm.bits(np.array([tr["step_t2"][k], tr["step_r2"][k]])).tolist() == \
            rfm.bits(np.array([w["step_t2"], w["step_r2"]], np.float64)).tolist(), (label, k, "steps")
    assert (res.status, res.iterations, res.improved) == (want["status"], want["iterations"], want["improved"]), label
    assert res.transform.tobytes() == want["transform"].tobytes(), label
    for f in SCORES:
        g, w = getattr(res, f), want[f]
        assert (rfm.bits(np.float64(g)) == rfm.bits(np.float64(w))) if isinstance(w, float) else g == w, (label, f, g, w)
    assert not res.applied
    pose = np.atleast_1d(orc.to_state(res.trans))
    for f in tgm.KEYS:  # toState: the angles to that function's float tolerance, the position exactly
        assert abs(float(res.pose[f]) - float(pose[0][f])) <= (0.0 if f in "xyz" else 1e-5), (label, f)
    return res, tr, want


# ---- 1. every pass against the model -------------------------------------------------------------------------------------
def model_of(M):
    return tgm.model(M) if M >= 300 else tgm.model(300)[:M].copy()


@pytest.mark.parametrize("M", [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 300, 1025])
def test_every_pass_against_the_model(gpu, orc, M):
    ref = model_of(M)
    t = tgm.make(gpu, reference=ref)
    cloud = tgm.frame(0)
    t.setInputCloud(cloud)
    start = neighbour(orc)
    res, tr, _ = check_every_pass(orc, t, ref, cloud, start, "M%d" % M)
    if M < 3:
        assert res.status == rfm.TOO_FEW_PAIRS and res.iterations == 0 and res.transform.tobytes() == start.tobytes()
        assert not res.improved
    else:
        assert res.iterations >= 1 and res.n_pairs_before >= 3
    if M >= 255:
        assert res.improved and res.n_inliers_after > res.n_inliers_before
    # a second call on the same handle reuses the buffers and gives the same bits
    again = t.refine(start=start)
    assert again.transform.tobytes() == res.transform.tobytes() and again.iterations == res.iterations
    assert t.getRefineTrace()["sums"].tobytes() == tr["sums"].tobytes()
    t.close()


VARIANTS = {
    "builder_single": {"PFT_FORCE_BUILDER": "single"},
    "builder_sorted": {"PFT_FORCE_BUILDER": "sorted"},
    "leaf_direct": {"PFT_LEAF_INDIRECT": "0"},
    "leaf_indirect": {"PFT_LEAF_INDIRECT": "1"},
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_every_pass_with_the_path_switches(gpu, orc, monkeypatch, name):
    for k, val in VARIANTS[name].items():  # the switches are latched at pft_create
        monkeypatch.setenv(k, val)
    cloud = tgm.frame(0)
    for M in (300, 1025):
        ref = model_of(M)
        t = tgm.make(gpu, reference=ref)
        tgm.step(t, cloud, match=False)
        res, _, _ = check_every_pass(orc, t, ref, cloud, neighbour(orc, -np.pi / 8.0, (0.01, 0.0, -0.01)), "%s M%d" % (name, M),
                                     max_iterations=8, pair_distance=0.05, inlier_distance=0.015, margin=0.07)
        assert res.iterations >= 1
        t.close()


def test_on_a_tree_deeper_than_ten_levels(gpu, orc):
    ref, cloud = tgm.scattered(1200, 10.0, 1)
    t = tgm.make(gpu, reference=ref, trans=np.eye(4, dtype=np.float32))
    tgm.step(t, cloud, match=False)
    start = np.asarray(orc.get_transformation(0.004, -0.003, 0.002, 0.0, 0.0, 0.01), np.float32).reshape(4, 4)[:3]
    res, _, want = check_every_pass(orc, t, ref, cloud, start, "deep")
    assert want["octree_depth"] > 10 and res.n_crop == len(cloud)
    assert res.n_pairs_before > 200 and res.iterations >= 1
    t.close()


def test_pass_zero_has_the_bits_of_the_match_of_the_same_pose(gpu):
    """the scattered scene of test_gpu_reacquire's test_same_bits_as_the_match_of_the_same_pose: both crops are the whole
    cloud, so pass 0 from the result pose pairs what pft_match matched -- one search -- and its gated tree over signed
    terms gives the bits of pft_match's ungated tree over the same non-negative terms at the same positions"""
    ref, cloud = tgm.scattered(1200, 10.0, 1)
    t = tgm.make(gpu, reference=ref, trans=np.eye(4, dtype=np.float32))
    tgm.step(t, cloud)
    st = t.getMatch()
    res = t.refine(start=None, pair_distance=float(t._cfg.max_distance), apply=False)
    tr = t.getRefineTrace()
    print("match %d / %.17g, refine pass 0 %d / %.17g" % (st.n_matched, st.sum_sq_dist, res.n_pairs_before, tr["sums"][0][15]))
    assert st.evaluated and st.n_crop == len(cloud) == res.n_crop, "precondition: both crops are the whole cloud"
    assert tr["transform"][0].tobytes() == st.transform.tobytes(), "precondition: the same pose"
    assert st.n_matched > 200, "precondition"
    assert res.n_pairs_before == st.n_matched
    assert rfm.bits(np.float64(tr["sums"][0][15])) == rfm.bits(np.float64(st.sum_sq_dist))
    t.close()


# ---- 2. a fixed point ----------------------------------------------------------------------------------------------------
def test_a_fixed_point(gpu, orc):
    """the frame is the model moved by T0 and the start is T0: every pair has distance 0, a == b, the step is exactly zero"""
    T0 = tgm._world()["trans"]
    ref = tgm.model(300)
    cloud = orc.transform_cloud(ref, T0)
    t = tgm.make(gpu)
    t.setInputCloud(cloud)
    res = t.refine(start=T0)
    tr = t.getRefineTrace()
    print("fixed point: status %s iterations %d pairs %d sum_sq_dist %.3g steps %s %s" % (
        res.status_name, res.iterations, res.n_pairs_before, res.sum_sq_dist_before, tr["step_t2"].tolist(), tr["step_r2"].tolist()))
    assert res.n_pairs_before == 300 == res.n_inliers_before and res.sum_sq_dist_before == 0.0
    assert (res.status, res.iterations) == (rfm.CONVERGED, 1)
    assert tr["step_t2"].tolist() == [0.0, 0.0] and tr["step_r2"].tolist() == [0.0, 0.0], "dq is exactly the identity"
    assert res.transform.tobytes() == np.ascontiguousarray(T0[:3], np.float32).tobytes() == res.start.tobytes()
    assert tr["transform"][1].tobytes() == tr["transform"][0].tobytes()
    assert not res.improved and not res.applied
    t.close()


# ---- 3. the default start ------------------------------------------------------------------------------------------------
def test_default_start_is_the_result_pose(gpu):
    t = tgm.make(gpu)
    tgm.step(t, tgm.frame(0))
    T = t.getMatch().transform
    a = t.refine()
    ta = t.getRefineTrace()
    b = t.refine(start=T)
    tb = t.getRefineTrace()
    assert a.start.tobytes() == np.ascontiguousarray(T, np.float32).tobytes()
    for f in ("start", "transform", "bbox", "pose"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert (a.status, a.iterations, a.n_crop, a.improved) == (b.status, b.iterations, b.n_crop, b.improved)
    assert [getattr(a, f) for f in SCORES] == [getattr(b, f) for f in SCORES]
    for f in ta:
        assert ta[f].tobytes() == tb[f].tobytes(), f
    t.close()


# ---- 4. apply=False leaves the tracker alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("kld", [False, True])
def test_without_apply_the_tracker_is_left_alone(gpu, kld):
    a, b = tgm.make(gpu, kld=kld), tgm.make(gpu, kld=kld)
    a.setMatchThreshold(1.0, 1)
    b.setMatchThreshold(1.0, 1)
    for f in range(2):
        tgm.step(a, tgm.frame(f))
        tgm.step(b, tgm.frame(f))
    streak = a.getMatch().streak
    res = a.refine()
    assert res.iterations >= 1 and not res.applied
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


# ---- 5. applied ----------------------------------------------------------------------------------------------------------
def test_applied_equals_a_fresh_handle_at_the_final_pose(gpu, orc):
    t = tgm.make(gpu)
    for f in range(2):
        tgm.step(t, tgm.frame(f))
    res = t.refine(start=neighbour(orc), apply=True)
    assert res.improved and res.applied
    fresh = tgm.make(gpu, trans=res.trans)
    for f in range(2, 5):
        tgm.step(t, tgm.frame(f), match=False)
        tgm.step(fresh, tgm.frame(f), match=False)
        assert tgm.snapshot(t) == tgm.snapshot(fresh), f
    # apply without an improvement applies nothing: from the fixed point of its own result
    keep = tgm.snapshot(t)
    again = t.refine(start=res.transform, max_iterations=1, trans_eps=0.0, rot_eps=0.0, inlier_distance=1e-6, apply=True)
    assert again.applied == again.improved
    if not again.applied:
        assert tgm.snapshot(t) == keep
    t.close()
    fresh.close()


def test_a_builder_failure_is_reported_and_nothing_is_applied(gpu, orc):
    """a crop that fails on the device (injected: the one-pass crop's flag) leaves the passes without a target: the call
    reports it as getResult() would, applies nothing, and the tracker goes on like a twin that never called"""
    a, b = tgm.make(gpu), tgm.make(gpu)
    for f in range(2):
        tgm.step(a, tgm.frame(f), match=False)
        tgm.step(b, tgm.frame(f), match=False)
    a.debugInjectError(4)
    with pytest.raises(gpu.PftError) as e:
        a.refine(start=neighbour(orc), apply=True)
    assert e.value.status == 5 and "bit2" in str(e.value)
    tr = a.getRefineTrace()
    assert len(tr["n_pairs"]) == 1 and int(tr["n_pairs"][0]) == 0, "one pass, nothing paired"
    assert tgm.snapshot(a) == tgm.snapshot(b)
    for f in range(2, 4):
        tgm.step(a, tgm.frame(f), match=False)
        tgm.step(b, tgm.frame(f), match=False)
        assert tgm.snapshot(a) == tgm.snapshot(b), f
    assert a.refine(start=neighbour(orc)).improved, "per call, not sticky"
    a.close()
    b.close()


# ---- 6. re-acquisition with refinement -----------------------------------------------------------------------------------
def test_reacquire_with_refinement(gpu):
    """the jump scenario of test_gpu_reacquire.test_recovery_end_to_end: the lattice's best candidate is refined, the
    refined pose is applied, and the next five frames keep the object under that test's lost rule"""
    t = tgm.make(gpu, seed=10)
    t.setMatchThreshold(0.5, 2)
    for f in range(3):
        tgm.step(t, tgm.frame(f))
        assert not t.isLost()
    for f in (3, 4):
        tgm.step(t, tgm.frame(f, shift=0.5))
    assert t.isLost()
    cloud = tgm.frame(4, shift=0.5)
    res = t.reacquire(centres=centres_of(cloud, shift=0.5), refine=True)
    rr = res.refined
    print("recovery: best %d centre %d inliers %d; refined %s after %d iterations, inliers %d -> %d improved %d applied %d" % (
        res.best, res.best_centre, res.n_inliers, rr.status_name, rr.iterations, rr.n_inliers_before, rr.n_inliers_after,
        rr.improved, rr.applied))
    assert res.accepted and res.applied and res.best_centre == 1
    assert rr.start.tobytes() == res.transform.tobytes()  # (its crop, and so its tree, is its own: the counts may differ)
    assert rr.improved and rr.applied and rr.n_inliers_after > rr.n_inliers_before
    assert not t.getMatch().lost, "the streak is cleared with the restart"
    fresh = tgm.make(gpu, seed=10, trans=rr.trans)
    for f in range(5, 10):
        c = tgm.frame(f, shift=0.5)
        tgm.step(t, c)
        tgm.step(fresh, c, match=False)
        assert tgm.snapshot(t) == tgm.snapshot(fresh), f
        assert not t.isLost(), f
    assert t.getMatch().n_matched >= 150
    t.close()
    fresh.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(gpu, orc):
    eye = np.eye(4, dtype=np.float32)[:3]
    s = gpu.ParticleFilterTracker(world_size=2)
    s.setParticleNum(tgm.P)
    s.setReferenceCloud(tgm.model())
    s.setInputCloud(tgm.frame(0))
    refused(gpu, lambda: s.refine(start=eye), 1, "sharded")
    s.close()

    x = gpu.make_reference_tracker(particle_num=tgm.P)
    x.setCloudCoherence(tgm._exact_coherence(gpu))
    x.setReferenceCloud(tgm.model())
    x.setInputCloud(tgm.frame(0))
    refused(gpu, lambda: x.refine(start=eye), 1, "exact")
    x.close()

    t = tgm.make(gpu)
    refused(gpu, lambda: t.refine(start=eye), 2, "")  # no input cloud yet
    t.setInputCloud(tgm.frame(0))
    refused(gpu, lambda: t.refine(), 7, "before the first pft_compute")
    for kw in (dict(max_iterations=0), dict(max_iterations=65), dict(min_pairs=2), dict(pair_distance=-0.1),
               dict(pair_distance=np.inf), dict(inlier_distance=0.0), dict(inlier_distance=np.nan), dict(margin=-1.0),
               dict(margin=np.inf), dict(trans_eps=-1e-4), dict(trans_eps=np.nan), dict(rot_eps=-1e-3), dict(rot_eps=np.inf)):
        refused(gpu, lambda: t.refine(start=eye, **kw), 1, "bad configuration value")
    for bad in (np.nan, np.inf):
        m = neighbour(orc)
        m[1, 2] = bad
        refused(gpu, lambda: t.refine(start=m), 1, "non-finite")
    with pytest.raises(gpu.PftError):
        t.refine(start=np.zeros((2, 3), np.float32))
    # after every refusal the handle still works
    assert t.refine(start=neighbour(orc)).improved
    t.close()

    n = gpu.make_reference_tracker(particle_num=tgm.P)
    n.setInputCloud(tgm.frame(0))
    refused(gpu, lambda: n.refine(start=eye), 3, "")  # no reference cloud
    n.close()


# ---- 8. the C++ path -----------------------------------------------------------------------------------------------------
def test_cpp_driver_refines_the_reacquired_pose(gpu, tmp_path):
    """the scenario of test_gpu_reacquire's driver test with --refine: one `refine obj` line right behind the `reacquire obj`
    line, and no later frame reports a loss"""
    from pcl_tracking_amd import build

    w = tgm._world()
    cluster = w["obj"][np.random.default_rng(7).choice(2000, 300, replace=False)]
    tgm.write_pcd(str(tmp_path / "model.pcd"), cluster)
    paths = []
    for f in range(10):
        paths.append(str(tmp_path / ("frame%d.pcd" % f)))
        tgm.write_pcd(paths[-1], tgm.frame(f, shift=0.0 if f < 3 else 0.5))
    r = subprocess.run([build.build_example(), str(tmp_path / "model.pcd"), "--frames"] + paths +
                       ["--particles", str(tgm.P), "--seed", "1", "--model-leaf", "0", "--match=0.5,2", "--reacquire=9", "--refine",
                        "--no-plane", "--box", "-10,10,-10,10,-10,10", "--tolerance", "0.04", "--min-size", "100"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    at = [i for i, ln in enumerate(out) if ln.startswith("reacquire obj 0:")]
    assert len(at) == 1 and out[at[0]].split()[-2:] == ["accepted", "1"]
    words = out[at[0] + 1].split()
    assert words[:4] == ["refine", "obj", "0:", "iterations"] and words[5] == "status" and words[7] == "inliers"
    assert words[6] in ("CONVERGED", "MAX_ITERATIONS") and 1 <= int(words[4]) <= 16
    before, after = int(words[8]), int(words[10].split("/")[0])
    assert words[9] == "->" and words[10].split("/")[1] == "300" and words[11] == "improved" and words[12] in ("0", "1")
    assert after >= before if words[12] == "1" else after <= before
    assert sum(ln.startswith("refine obj") for ln in out) == 1
    said = [int(ln.split()[1]) for ln in r.stderr.splitlines() if ln.endswith("Object not recognized")]
    assert said == [5], "lost once, at the second shifted frame; never again after the restart"
    later = [ln.split() for ln in out[at[0]:] if " match " in ln]
    assert len(later) == 5 and all(ln[-1] == "0" for ln in later)

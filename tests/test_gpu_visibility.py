"""GPU checks of the visibility (pft_visibility; pcl_tracking_amd/csrc/pft_visibility.hip): every array and every count of
the device equal to the NumPy model (tests/visibility_model.py), starting from the transform the result reports.  With an
explicit matrix: the hand-made and adversarial cases of tests/visibility_cases.py.  With the result pose: a patch half
covered by a plate, has_match with and without a pft_match, the occlusion-aware rule over a frame sequence, KLD and
exact-NN handles, a filter hand-off whose count lives on the device, and no side effect on pft_compute.  Then the refusals.

Sizes: models of 1 .. 300 points, frames of at most 2 000 points, 64 particles, 1 iteration, images 16 x 12 and 160 x 90."""
import numpy as np
import pytest

import visibility_cases as vc
import visibility_model as vm

pytestmark = pytest.mark.gpu
P = 64
COUNTS = ("n_reference", "n_visible", "n_occluded", "n_self", "n_out", "n_frame", "has_match", "n_visible_matched",
          "hidden", "below", "streak", "lost")


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


def cloud_of(xyz):
    from pcl_tracking_amd import scene

    return scene.make_points(np.asarray(xyz, np.float32), np.full((len(xyz), 3), 128))


def check(t, cam, ref_xyz, frame_xyz, label, match_idx=None, threshold=vm.DEFAULT_THRESHOLD, prev_streak=0, T=None):
    """the device's last call against the model at the transform the device reports"""
    st = t.getVisibility()
    state, sgap, mgap = t.getVisibilityPoints()
    assert st.evaluated, label
    if T is not None:
        np.testing.assert_array_equal(st.transform, np.asarray(T, np.float32).reshape(-1)[:12].reshape(3, 4), label)
    want = vm.visibility(cam, ref_xyz, st.transform, frame_xyz, match_idx=match_idx, threshold=threshold,
                         prev_streak=prev_streak)
    np.testing.assert_array_equal(state, want["state"], label)
    np.testing.assert_array_equal(sgap, want["scene_gap"], label)
    np.testing.assert_array_equal(mgap, want["self_gap"], label)
    for k in COUNTS:
        assert getattr(st, k) == want[k], (label, k, getattr(st, k), want[k])
    return st, want


def explicit_tracker(gpu, case):
    t = gpu.make_reference_tracker(particle_num=P, seed=3)
    t.setIterationNum(1)
    t.setVisibilityCamera(**case["cam"])
    t.setReferenceCloud(cloud_of(case["ref"]))
    t.setInputCloud(cloud_of(case["frame"]))
    return t


# ---- 1. an explicit matrix, right after setInputCloud (the 32-byte records are read) -----------------------------------
@pytest.mark.parametrize("name", sorted(vc.HAND_MADE) + sorted(vc.ADVERSARIAL))
def test_explicit_matrix_cases(gpu, name):
    case = (vc.HAND_MADE.get(name) or vc.ADVERSARIAL[name])()
    t = explicit_tracker(gpu, case)
    t.computeVisibility(case["T"])
    st, want = check(t, case["cam"], case["ref"], case["frame"], name, T=case["T"])
    if "state" in case:  # the answers worked out by hand
        assert t.getVisibilityPoints()[0].tolist() == case["state"]
    else:
        assert case["claim"](want)
    assert not st.has_match and st.calls == 1
    # again with a 4x4 matrix: the same result, one more call
    t.computeVisibility(np.vstack([case["T"], [[0, 0, 0, 1]]]))
    st2, _ = check(t, case["cam"], case["ref"], case["frame"], name + " again", T=case["T"])
    assert st2.calls == 2
    t.close()


def test_explicit_matrix_after_compute_reads_the_packed_records(gpu):
    """after a compute() the frame is the handle's 16-byte records; the camera may change between two calls"""
    case = vc.random_case(21, vm.camera())
    t = explicit_tracker(gpu, case)
    t.setTrans(np.vstack([case["T"], [[0, 0, 0, 1]]]))
    t.compute()
    for cam in (case["cam"], vc.small(), vm.camera(splat=4), vm.camera(width=320, height=180, fx=180.0, fy=180.0, cx=159.5, cy=89.5)):
        t.setVisibilityCamera(**cam)
        t.computeVisibility(case["T"])
        check(t, cam, case["ref"], case["frame"], "camera %dx%d splat %d" % (cam["width"], cam["height"], cam["splat"]),
              T=case["T"])
    assert t.getVisibilityCamera()["width"] == 320
    t.close()


# ---- 2. the result pose ----------------------------------------------------------------------------------------------------
def patch_tracker(gpu, kld=False, exact=False, seed=3):
    t = gpu.make_reference_tracker(particle_num=P, seed=seed, kld=kld)
    if kld:
        t.setMaximumParticleNum(100)
    if exact:
        c = gpu.NearestPairPointCloudCoherence()
        c.addPointCoherence(gpu.DistanceCoherence())
        h = gpu.HSVColorCoherence()
        h.setWeight(0.1)
        c.addPointCoherence(h)
        c.setSearchMethod(gpu.OctreeSearch(0.01))
        c.setMaximumDistance(0.1)
        t.setCloudCoherence(c)
    t.setIterationNum(1)
    t.setReferenceCloud(vc.patch_model())
    t.setTrans(vc.patch_trans())
    return t


REF = None


def ref_xyz():
    global REF
    if REF is None:
        REF = vc.cloud_xyz(vc.patch_model())
    return REF


def test_half_covered_patch(gpu):
    t = patch_tracker(gpu)
    cloud = vc.patch_frame("half")
    t.setInputCloud(cloud)
    t.compute()
    t.computeVisibility()
    st, want = check(t, vm.camera(), ref_xyz(), vc.cloud_xyz(cloud), "half")
    # exactly the T pft_match stores
    t.computeMatch()
    np.testing.assert_array_equal(st.transform, t.getMatch().transform)
    assert st.n_visible >= 60 and st.n_occluded >= 60 and not st.has_match
    t.close()


def test_has_match_with_and_without_a_preceding_match(gpu):
    t = patch_tracker(gpu)
    cloud = vc.patch_frame("half")
    xyz = vc.cloud_xyz(cloud)
    t.setInputCloud(cloud)
    t.compute()
    t.computeVisibility()
    assert not check(t, vm.camera(), ref_xyz(), xyz, "no match yet")[0].has_match
    t.computeMatch()
    t.computeVisibility()
    idx, _ = t.getMatchPairs()
    st, _ = check(t, vm.camera(), ref_xyz(), xyz, "after the match", match_idx=idx)
    assert st.has_match and 0 < st.n_visible_matched <= st.n_visible
    t.computeVisibility(st.transform)  # an explicit matrix never has a match
    assert not check(t, vm.camera(), ref_xyz(), xyz, "explicit")[0].has_match
    t.setInputCloud(cloud)
    t.compute()  # a new frame: the match of the last one does not count
    t.computeVisibility()
    assert not check(t, vm.camera(), ref_xyz(), xyz, "next frame")[0].has_match
    t.close()


def test_rule_over_a_frame_sequence(gpu):
    t = patch_tracker(gpu)
    t.setVisibilityThreshold(*vc.RULE_THRESHOLD)
    assert t.getVisibilityThreshold() == vc.RULE_THRESHOLD
    streak, seen = 0, []
    for f, kind in enumerate(vc.RULE_SEQUENCE):
        cloud = vc.patch_frame(kind)
        t.setInputCloud(cloud)
        t.compute()
        t.computeMatch()
        t.computeVisibility()
        idx, _ = t.getMatchPairs()
        st, _ = check(t, vm.camera(), ref_xyz(), vc.cloud_xyz(cloud), "frame %d %s" % (f, kind), match_idx=idx,
                      threshold=vc.RULE_THRESHOLD, prev_streak=streak)
        assert st.has_match and st.calls == f + 1
        streak = st.streak
        seen.append((st.hidden, st.below, st.streak, st.lost))
        assert t.isOccluded() == st.hidden and t.isLostVisible() == st.lost
    # visible then below: the streak counts; hidden: held; below again: lost; visible and matched: cleared; below
    assert seen == [(False, False, 0, False), (False, True, 1, False), (True, False, 1, False), (False, True, 2, True),
                    (False, False, 0, False), (False, True, 1, False)]
    assert not t.getMatch().lost  # the rule of pft_match has its own settings: untouched
    t.resetTracking()
    st = t.getVisibility()
    assert (st.below, st.streak, st.lost) == (False, 0, False) and st.calls == len(vc.RULE_SEQUENCE)
    t.close()


@pytest.mark.parametrize("kind", ["kld", "exact"])
def test_kld_and_exact_nn_handles(gpu, kind):
    t = patch_tracker(gpu, kld=kind == "kld", exact=kind == "exact")
    for f, frame_kind in enumerate(["full", "half"]):
        cloud = vc.patch_frame(frame_kind)
        t.setInputCloud(cloud)
        t.compute()
        t.computeVisibility()
        st, _ = check(t, vm.camera(), ref_xyz(), vc.cloud_xyz(cloud), "%s %s" % (kind, frame_kind))
        assert st.n_visible > 0 and (st.n_occluded > 0) == (frame_kind == "half")
    t.close()


def test_filter_hand_off_with_the_count_on_the_device(gpu):
    from pcl_tracking_amd import filters

    cloud = vc.patch_frame("half")
    f = filters.PassThrough()
    f.setFilterFieldName("z")
    f.setFilterLimits(0.0, 1.3)  # drops the wall: the count on the device is below the bound
    f.setInputCloud(cloud)
    f.filterAsync()
    t = patch_tracker(gpu)
    t.setInputCloudFromFilter(f)
    with pytest.raises(gpu.PftError) as e:
        t.computeVisibility(vc.patch_trans()[:3])
    assert e.value.status == 7 and "pft_set_input_from_filter" in str(e.value)
    t.compute()
    t.computeVisibility()
    out = f.output()
    assert 0 < len(out) < len(cloud)
    st, _ = check(t, vm.camera(), ref_xyz(), vc.cloud_xyz(out), "filter hand-off")
    assert st.n_frame == len(out) and st.n_occluded > 0
    t.computeVisibility(st.transform)
    check(t, vm.camera(), ref_xyz(), vc.cloud_xyz(out), "filter hand-off, explicit", T=st.transform)
    t.close()


def test_compute_results_do_not_change(gpu):
    """the same frames with and without the visibility calls: results and populations byte for byte"""
    runs = []
    for with_calls in (False, True):
        t = patch_tracker(gpu, seed=5)
        out = []
        for kind in ("full", "half", "full"):
            t.setInputCloud(vc.patch_frame(kind))
            if with_calls:
                t.computeVisibility(vc.patch_trans()[:3])  # before the frame's first crop
            t.compute()
            if with_calls:
                t.computeMatch()
                t.computeVisibility()
                t.getVisibility()
            out.append(t.getResult().tobytes() + t.getParticles().tobytes())
        runs.append(out)
        t.close()
    assert runs[0] == runs[1]


def test_unevaluated_after_a_failed_iteration(gpu):
    """PftHeader::error and a NULL matrix: evaluated = 0, everything but `calls` keeps its values; an explicit matrix is
    evaluated all the same"""
    t = patch_tracker(gpu)
    cloud = vc.patch_frame("half")
    t.setInputCloud(cloud)
    t.compute()
    t.computeVisibility()
    before = t.getVisibility()
    pts_before = t.getVisibilityPoints()
    t.debugInjectError(4)
    t.setInputCloud(vc.patch_frame("full"))
    t.compute()
    t.computeVisibility()
    with pytest.raises(gpu.PftError):
        t.getVisibility()  # the deferred device failure, as getResult reports it
    after = t.getVisibility()
    assert not after.evaluated and after.calls == before.calls + 1
    for k in COUNTS:
        assert getattr(after, k) == getattr(before, k), k
    np.testing.assert_array_equal(after.transform, before.transform)
    for a, b in zip(t.getVisibilityPoints(), pts_before):
        np.testing.assert_array_equal(a, b)
    t.computeVisibility(vc.patch_trans()[:3])
    check(t, vm.camera(), ref_xyz(), vc.cloud_xyz(vc.patch_frame("full")), "explicit after a failure", T=vc.patch_trans()[:3])
    t.close()


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    s = gpu.ParticleFilterTracker(world_size=2)
    s.setParticleNum(P)
    s.setReferenceCloud(vc.patch_model())
    s.setInputCloud(vc.patch_frame("full"))
    with pytest.raises(gpu.PftError) as e:
        s.computeVisibility(vc.patch_trans()[:3])
    assert e.value.status == 1 and "sharded" in str(e.value)
    s.close()

    t = patch_tracker(gpu)
    with pytest.raises(gpu.PftError) as e:
        t.computeVisibility(vc.patch_trans()[:3])
    assert e.value.status == 2  # no input cloud, as compute()
    t.setInputCloud(vc.patch_frame("full"))
    with pytest.raises(gpu.PftError) as e:
        t.computeVisibility()
    assert e.value.status == 7 and "before the first pft_compute" in str(e.value)
    with pytest.raises(gpu.PftError) as e:
        t.getVisibility()
    assert e.value.status == 7
    for k in (0, 5, 11):
        for bad in (np.nan, np.inf, -np.inf):
            m = vc.patch_trans()[:3].copy()
            m.reshape(-1)[k] = bad
            with pytest.raises(gpu.PftError) as e:
                t.computeVisibility(m)
            assert e.value.status == 1 and "not finite" in str(e.value)
    good = t.getVisibilityCamera()
    for bad in (dict(width=0), dict(width=1025), dict(height=0), dict(height=2000), dict(fx=0.0), dict(fy=-1.0),
                dict(fx=np.inf), dict(cx=np.nan), dict(cy=np.inf), dict(z_near=-0.1), dict(z_near=np.nan), dict(splat=-1),
                dict(splat=5), dict(occlusion_margin=-1e-3), dict(self_margin=np.nan), dict(self_margin=np.inf)):
        with pytest.raises(gpu.PftError) as e:
            t.setVisibilityCamera(**bad)
        assert e.value.status == 1 and "pft_set_visibility_camera" in str(e.value), bad
    assert t.getVisibilityCamera() == good
    for bad in ((-0.1, 0.0, 1), (0.25, 1.5, 1), (0.25, 0.0, 0), (np.nan, 0.0, 1)):
        with pytest.raises(gpu.PftError):
            t.setVisibilityThreshold(*bad)
    # nothing above reached the device: the handle works
    t.computeVisibility(vc.patch_trans()[:3])
    check(t, vm.camera(), ref_xyz(), vc.cloud_xyz(vc.patch_frame("full")), "after the refusals", T=vc.patch_trans()[:3])
    n = gpu.make_reference_tracker(particle_num=P)
    n.setInputCloud(vc.patch_frame("full"))
    with pytest.raises(gpu.PftError) as e:
        n.computeVisibility(vc.patch_trans()[:3])
    assert e.value.status == 3  # no reference cloud
    n.close()
    t.close()

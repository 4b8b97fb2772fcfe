"""GPU checks of the view-dependent reference (include/pft_view.h; pcl_tracking_amd/csrc/pft_view.hip): every array, index,
cloud byte and count of the device equal to the NumPy model (tests/view_model.py) at the transform the device reports --
there is no tolerance on a selection in this file.  With an explicit matrix: every case of tests/view_cases.py through the
host and the device entry and through grids of 1, 3 and the default.  With the result pose: fixed, KLD and exact-NN handles
and a ModelGrowth source.  Then the hand-off to the reference cloud bit for bit against setReferenceCloud, the refusals,
and no side effect on compute().

Sizes: 64 particles, 1 iteration, models of at most 700 points (view_cases.BIG apart), frames of at most 2 000 points,
images 16 x 12 and 160 x 90."""
import functools

import numpy as np
import pytest

import view_cases as wc
import view_model as wm
import visibility_model as vm

pytestmark = pytest.mark.gpu
P = 64
F = np.float32


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


def xyz_of(recs):
    return np.stack([recs["x"], recs["y"], recs["z"]], 1).astype(F)


def compare(t, recs, want, label, T=None):
    """the device's last select against the model's output `want` for the records `recs`"""
    st = t.getView()
    assert st.evaluated, label
    if T is not None:
        np.testing.assert_array_equal(st.transform, np.asarray(T, F).reshape(-1)[:12].reshape(3, 4), label)
    state, gap = t.getViewPoints()
    np.testing.assert_array_equal(state, want["state"], label)
    np.testing.assert_array_equal(gap.view(np.uint32), want["self_gap"].view(np.uint32), label)
    np.testing.assert_array_equal(t.getViewIndices(), want["kept_index"], label)
    assert t.getViewCloud().tobytes() == recs[want["kept_index"]].tobytes(), label
    assert (st.n_model, st.n_visible, st.n_kept, st.n_state) == (want["n_model"], want["n_visible"], want["n_kept"], want["n_state"]), label
    return st


def check(t, cam, recs, K, label):
    """... against the model at the transform the device reports"""
    tr = t.getView().transform
    return compare(t, recs, wm.select(cam, xyz_of(recs), tr, K), label)


def fresh(gpu, cam, **kw):
    t = gpu.make_reference_tracker(particle_num=P, seed=3, **kw)
    t.setIterationNum(1)
    t.setVisibilityCamera(**cam)
    return t


def on_device(recs):
    import torch

    d = torch.from_numpy(np.frombuffer(recs.tobytes(), np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return d


# ---- 1. an explicit matrix: needs neither a reference nor an input cloud -------------------------------------------------
@pytest.mark.parametrize("name", sorted(wc.all_cases()))
def test_explicit_matrix_cases(gpu, name):
    c, want = wc.expected(name)
    recs = wc.records(c["xyz"])
    t = fresh(gpu, c["cam"])
    calls = 0
    for grid in (0, 1, 3):
        t.debugSetViewGrid(grid)
        t.selectView(recs, c["T"], c["K"])
        calls += 1
        st = compare(t, recs, want, "%s host grid %d" % (name, grid), T=c["T"])
        assert st.calls == calls
        if "state" in c:  # the answers worked out by hand
            assert t.getViewPoints()[0].tolist() == c["state"]
    d = on_device(recs)
    t.debugSetViewGrid(0)
    t.selectView((d.data_ptr() if len(recs) else 0, len(recs)), np.vstack([c["T"], [[0, 0, 0, 1]]]), c["K"])
    compare(t, recs, want, name + " device", T=c["T"])
    p, n = t.viewCloudDevice()
    assert n == want["n_kept"] and (p != 0 or n == 0)
    t.close()


def test_big_model_ranks_cross_workgroups(gpu):
    """2^18 + 3 records, half of them visible, decimated to 50 001: the ranks and the kept positions span a thousand tiles"""
    c, want = wc.expected("big")
    recs = wc.records(c["xyz"])
    t = fresh(gpu, c["cam"])
    for grid in (0, 3):
        t.debugSetViewGrid(grid)
        t.selectView(recs, c["T"], c["K"])
        compare(t, recs, want, "big grid %d" % grid, T=c["T"])
    d = on_device(recs)
    t.debugSetViewGrid(0)
    t.selectView((d.data_ptr(), len(recs)), c["T"], c["K"])
    compare(t, recs, want, "big device", T=c["T"])
    t.close()


def test_buffers_are_reused_and_grown(gpu):
    """one handle: a model, a smaller one, a larger one, another camera"""
    t = fresh(gpu, vm.camera())
    for name in ("shell_257", "shell_63", "shell_1025", "alternating", "shell_1025_K333", "shell_0", "two_plates"):
        c, want = wc.expected(name)
        recs = wc.records(c["xyz"])
        t.setVisibilityCamera(**c["cam"])
        t.selectView(recs, c["T"], c["K"])
        compare(t, recs, want, "reuse " + name, T=c["T"])
    assert t.getView().calls == 7
    t.close()


# ---- 2. the box: a full-surface model, its one-view subset, frames of the visible side and a wall --------------------------
BOX_DIMS = (0.21, 0.15, 0.12)
POSE0 = (0.05, -0.03, 1.0, 0.3, -0.2, 0.5)


def pose(f):
    return (POSE0[0] + 0.002 * f,) + POSE0[1:]


def pose_matrix(f):
    from pcl_tracking_amd import scene

    return scene.pose_matrix(*pose(f)).astype(F)


@functools.lru_cache(maxsize=None)
def box_model():
    """the 1.5 cm lattice of all six faces: 664 records, one colour per face"""
    from pcl_tracking_amd import scene

    xyz, fid = scene._box_surface_lattice(BOX_DIMS, 0.015)
    assert len(xyz) == 664
    return scene.make_points(xyz.astype(F), scene.FACE_RGB[fid])


@functools.lru_cache(maxsize=None)
def one_view():
    """the records of the box the camera sees at pose(0), and three strays 60 cm to the side that no frame point matches"""
    from pcl_tracking_amd import scene

    full = box_model()
    o = wm.select(vm.camera(), xyz_of(full), pose_matrix(0)[:3])
    stray = scene.make_points(np.array([[0.6, 0, 0], [0.6, 0.02, 0], [0.6, 0, 0.02]], F), np.full((3, 3), 128))
    return np.concatenate([full[o["kept_index"]], stray])


@functools.lru_cache(maxsize=None)
def frame(f):
    """the visible side of the box at pose(f) and a wall 0.6 m behind it: under 1 000 points"""
    from pcl_tracking_amd import scene

    full = box_model()
    T = pose_matrix(f)[:3]
    o = wm.select(vm.camera(), xyz_of(full), T)
    surf = full[o["kept_index"]].copy()
    q = vm.xform(T, xyz_of(surf))
    surf["x"], surf["y"], surf["z"] = q[:, 0], q[:, 1], q[:, 2]
    u, v = np.meshgrid(np.arange(25) * 0.03 - 0.36, np.arange(20) * 0.03 - 0.3, indexing="ij")
    wall = scene.make_points(np.stack([u.ravel() + POSE0[0], v.ravel() + POSE0[1], np.full(u.size, 1.6)], 1).astype(F),
                             np.full((u.size, 3), 80))
    return np.concatenate([surf, wall])


def box_tracker(gpu, seed=5, kld=False, exact=False):
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
    t.setReferenceCloud(one_view())
    t.setTrans(pose_matrix(0))
    return t


@pytest.mark.parametrize("mode", ["fixed", "kld", "exact"])
def test_result_pose(gpu, mode):
    t = box_tracker(gpu, kld=mode == "kld", exact=mode == "exact")
    full = box_model()
    for f in range(2):
        t.setInputCloud(frame(f))
        t.compute()
        t.selectView(full, max_points=150 * f)
        st = check(t, vm.camera(), full, 150 * f, "%s frame %d" % (mode, f))
        # exactly pose_to_matrix of the result as reported: the T computeVisibility() stores for the same frame
        t.computeVisibility()
        np.testing.assert_array_equal(st.transform, t.getVisibility().transform)
        np.testing.assert_allclose(st.transform, t.toEigenMatrix(t.getResult())[:3], rtol=0, atol=1e-6)
        assert st.n_visible > 150 and st.n_kept == (150 if f else st.n_visible)
    t.close()


def test_model_growth_source(gpu):
    from pcl_tracking_amd import grow

    t = box_tracker(gpu)
    g = grow.ModelGrowth(confirm=1)
    g.setModel(one_view()[:-3])
    for f in range(2):
        t.setInputCloud(frame(f))
        t.compute()
        g.apply(frame(f), pose_matrix(f)[:3])
    model = g.model()
    assert len(model) >= len(one_view()) - 3
    t.selectView(g)
    st = check(t, vm.camera(), model, 0, "grown model")
    assert st.n_model == len(model)
    cloud = t.getViewCloud()
    t.selectView(model)  # the same records from the host: the same bytes
    check(t, vm.camera(), model, 0, "grown model, host copy")
    assert t.getViewCloud().tobytes() == cloud.tobytes()
    g.close()
    t.close()


# ---- 3. the hand-off ---------------------------------------------------------------------------------------------------------
def run_frames(t, frames, match=False):
    out = []
    for f in frames:
        t.setInputCloud(frame(f))
        t.compute()
        if match:
            t.computeMatch()
        out.append(t.getResult().tobytes() + t.getParticles().tobytes())
    return out


def test_hand_off_bit_for_bit(gpu):
    full = box_model()
    A, B = box_tracker(gpu), box_tracker(gpu)
    for t in (A, B):
        t.setMatchThreshold(1.0, 10)  # the strays are never matched: every evaluated match is below
    assert run_frames(A, (0, 1)) == run_frames(B, (0, 1))
    assert run_frames(A, (2,), match=True) == run_frames(B, (2,), match=True)
    assert A.getMatch().streak == 1 and B.getMatch().streak == 1
    epoch = A.getParticles().tobytes()
    A.selectView(full, max_points=300)
    st = check(A, vm.camera(), full, 300, "hand-off select")
    n_kept = st.n_kept
    assert n_kept == min(300, st.n_visible) and n_kept > 150
    A.setReferenceFromView()
    view, vi = A.getViewCloud(), A.getViewIndices()
    assert view.tobytes() == full[vi].tobytes()
    B.setReferenceCloud(view)
    assert A.getParticles().tobytes() == epoch  # the particles are untouched
    # the same object for A, a new one for B
    assert A.getMatch().streak == 1 and not A.getMatch().lost
    assert B.getMatch().streak == 0
    with pytest.raises(gpu.PftError) as e:
        A.getMatchPairs()  # the pairs belonged to the old reference
    assert e.value.status == 7
    a, b = run_frames(A, (3,), match=True), run_frames(B, (3,), match=True)
    assert a == b
    m = A.getMatch()
    assert m.evaluated and m.n_reference == n_kept
    assert m.streak == 0 and B.getMatch().streak == 0  # every record of the view finds a partner
    # the pairs, composed with the view's indices, point into the full model
    idx, d2 = A.getMatchPairs()
    assert len(idx) == n_kept and (idx >= 0).all()
    q = vm.xform(m.transform, xyz_of(full[vi]))
    fr = xyz_of(frame(3))[idx]
    np.testing.assert_allclose(((q - fr) ** 2).sum(1), d2, rtol=1e-4, atol=1e-9)
    assert run_frames(A, (4, 5)) == run_frames(B, (4, 5))
    A.close()
    B.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def test_too_few_points_keeps_the_old_reference(gpu):
    """min_points above n_kept: PFT_ERR_STATE, and the old reference tracks on with the bytes of a handle that never tried"""
    full = box_model()
    A, B = box_tracker(gpu), box_tracker(gpu)
    assert run_frames(A, (0, 1)) == run_frames(B, (0, 1))
    A.selectView(full, max_points=100)
    with pytest.raises(gpu.PftError) as e:
        A.setReferenceFromView(min_points=101)
    assert e.value.status == 7 and "fewer than the 101" in str(e.value)
    assert run_frames(A, (2, 3)) == run_frames(B, (2, 3))
    A.setReferenceFromView(min_points=100)  # the select is still there
    with pytest.raises(gpu.PftError) as e:
        A.setReferenceFromView()  # ... and now consumed
    assert e.value.status == 7 and "consumed" in str(e.value)
    A.setInputCloud(frame(4))
    A.compute()
    A.computeMatch()
    assert A.getMatch().n_reference == 100
    A.close()
    B.close()


def test_refusals(gpu):
    full = box_model()
    T = pose_matrix(0)[:3]
    s = gpu.ParticleFilterTracker(world_size=2)
    s.setParticleNum(P)
    s.setReferenceCloud(one_view())
    s.setInputCloud(frame(0))
    with pytest.raises(gpu.PftError) as e:
        s.selectView(full, T)
    assert e.value.status == 1 and "sharded" in str(e.value)
    s.close()

    t = box_tracker(gpu)
    with pytest.raises(gpu.PftError) as e:
        t.setReferenceFromView()  # no handle yet
    assert e.value.status == 7
    t.setInputCloud(frame(0))
    with pytest.raises(gpu.PftError) as e:
        t.setReferenceFromView()  # no select
    assert e.value.status == 7 and "no pft_view_select" in str(e.value)
    with pytest.raises(gpu.PftError) as e:
        t.getView()
    assert e.value.status == 7
    with pytest.raises(gpu.PftError) as e:
        t.selectView(full)  # NULL before compute
    assert e.value.status == 7 and "before the first pft_compute" in str(e.value)
    for k in (0, 6, 11):
        for bad in (np.nan, np.inf, -np.inf):
            m = T.copy()
            m.reshape(-1)[k] = bad
            with pytest.raises(gpu.PftError) as e:
                t.selectView(full, m)
            assert e.value.status == 1 and "not finite" in str(e.value)
    with pytest.raises(gpu.PftError) as e:
        t.selectView((256, wm_max() + 1), T)  # refused on the count: the pointer is never read
    assert e.value.status == 6
    with pytest.raises(gpu.PftError) as e:
        t.selectView((264, 10), T)  # a device cloud that is not 16-byte aligned
    assert e.value.status == 1 and "aligned" in str(e.value)
    # nothing above reached the device: the handle tracks and selects
    t.compute()
    t.selectView(full)
    check(t, vm.camera(), full, 0, "after the refusals")
    t.close()


def wm_max():
    from pcl_tracking_amd import _lib

    return _lib.VIEW_MAX_MODEL_POINTS


def test_unevaluated_after_a_failed_iteration(gpu):
    """PftHeader::error and no matrix: evaluated = 0, everything but `calls` keeps its values, setReferenceFromView refuses
    and the old reference stays; an explicit matrix is evaluated all the same"""
    full = box_model()
    t = box_tracker(gpu)
    t.setInputCloud(frame(0))
    t.compute()
    t.selectView(full, max_points=150)
    before = check(t, vm.camera(), full, 150, "before")
    arrays = t.getViewPoints() + (t.getViewIndices(), t.getViewCloud())
    t.debugInjectError(4)
    t.setInputCloud(frame(1))
    t.compute()
    t.selectView(full)
    with pytest.raises(gpu.PftError):
        t.getView()  # the deferred device failure, as getResult reports it
    after = t.getView()
    assert not after.evaluated and after.calls == before.calls + 1
    assert (after.n_model, after.n_state, after.n_visible, after.n_kept) == (before.n_model, before.n_state, before.n_visible, before.n_kept)
    np.testing.assert_array_equal(after.transform, before.transform)
    for a, b in zip(t.getViewPoints() + (t.getViewIndices(), t.getViewCloud()), arrays):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(gpu.PftError) as e:
        t.setReferenceFromView()
    assert e.value.status == 7 and "not evaluated" in str(e.value)
    t.selectView(full, pose_matrix(1)[:3])
    check(t, vm.camera(), full, 0, "explicit after a failure")
    t.setInputCloud(frame(2))
    t.compute()  # the old reference is still in force
    t.computeMatch()
    assert t.getMatch().n_reference == len(one_view())
    t.close()


# ---- 5. no side effect ---------------------------------------------------------------------------------------------------------
def test_selecting_changes_no_pose(gpu):
    full = box_model()
    runs = []
    for with_calls in (False, True):
        t = box_tracker(gpu)
        out = []
        for f in range(4):
            t.setInputCloud(frame(f))
            t.compute()
            if with_calls:
                t.selectView(full, max_points=123)
                t.getView()
            out.append(t.getResult().tobytes() + t.getParticles().tobytes())
        runs.append(out)
        t.close()
    assert runs[0] == runs[1]

"""GPU checks of model growth (include/pft_grow.h; pcl_tracking_amd/csrc/pft_grow.hip) against the NumPy restatement
(tests/grow_model.py).  Every case of tests/grow_cases.py runs through ModelGrowth and through the restatement, and after
EACH apply the states, every field of the statistics, the model's bytes, the inverse transform's bits and the voxel table
are compared, all with assert_array_equal or on bytes: there is no tolerance in this file.
tests/test_grow_host.py shows by the restatement alone that each case tests what it claims."""
import numpy as np
import pytest

import grow_cases as gc
import grow_model as gm
import subtract_cases as sc
import subtract_model as sm
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import grow, subtract, tracker

    class G:
        pass

    g = G()
    g.grow, g.subtract, g.tracker = grow, subtract, tracker
    g.PftError = grow.PftError
    return g


def compare(dev, ref, what=""):
    """everything a handle shows after an apply (or a set_model) against the restatement"""
    if ref.pending_error:  # the apply overflowed: the first synchronising call says so, once
        with pytest.raises(Exception) as e:
            dev.stats()
        assert e.value.status == 6 and "overflow" in str(e.value), what
        ref.pending_error = False
    assert dev.stats() == ref.stats(), what
    if ref.states is not None:
        np.testing.assert_array_equal(dev.states(), ref.states, err_msg=what)
        np.testing.assert_array_equal(dev.transform().view(np.uint32), ref.Ti.view(np.uint32), err_msg=what)
    assert dev.model().tobytes() == ref.cloud.tobytes(), what
    got, want = dev.debugTable(), ref.debug_table()
    for k in ("keys", "kind", "hits", "last_seen"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=what + " table " + k)


def play(gpu, case, device_input=False):
    """the case's ops on a fresh handle and a fresh restatement, compared after every step"""
    dev, ref = gpu.grow.ModelGrowth(**case["cfg"]), gm.Grow(**case["cfg"])
    held = []
    for j, op in enumerate(case["ops"]):
        if op[0] == "model":
            dev.setModel(op[1])
            ref.set_model(op[1])
        elif op[0] == "planes":
            dev.setPlanes(op[1])
            ref.set_planes(op[1])
        else:
            if device_input:
                import torch

                t = torch.from_numpy(np.frombuffer(op[1].tobytes(), np.uint8).copy()).cuda()
                torch.cuda.synchronize()
                held.append(t)
                dev.applyDevice(t.data_ptr() if len(op[1]) else 0, len(op[1]), op[2], keepalive=t)
            else:
                dev.apply(op[1], op[2])
            ref.apply(op[1], op[2])
        compare(dev, ref, "op %d (%s)" % (j, op[0]))
    return dev, ref


@pytest.mark.parametrize("name", list(gc.CASES))
def test_case(gpu, name):
    play(gpu, gc.CASES[name]())


def test_rebuilds_do_not_change_a_result(gpu):
    small, _ = play(gpu, gc.rebuild_case(64))
    large, _ = play(gpu, gc.rebuild_case(1 << 16))
    assert small.stats()["n_rebuilds"] >= 2 and large.stats()["n_rebuilds"] == 0
    assert small.model().tobytes() == large.model().tobytes()
    np.testing.assert_array_equal(small.states(), large.states())
    a, b = small.debugTable(), large.debugTable()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.parametrize("name", ["rules", "crowd_1000", "shape_one_view_4099", "forget_1"])
def test_host_and_device_input_give_the_same_bytes(gpu, name):
    a, _ = play(gpu, gc.CASES[name]())
    b, _ = play(gpu, gc.CASES[name](), device_input=True)
    assert a.stats() == b.stats()
    assert a.states().tobytes() == b.states().tobytes() and a.model().tobytes() == b.model().tobytes()


def test_set_model_device_and_model_device(gpu):
    import torch

    model = gc.shape_model("one_view")
    t = torch.from_numpy(np.frombuffer(model.tobytes(), np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    dev, ref = gpu.grow.ModelGrowth(), gm.Grow()
    dev.setModelDevice(t.data_ptr(), len(model))
    ref.set_model(model)
    compare(dev, ref)
    p, n = dev.modelDevice()
    assert n == len(model) and p != 0
    again = gpu.grow.ModelGrowth()
    again.setModelDevice(p, n)  # a handle's model in HBM is a model for another handle
    assert again.model().tobytes() == model.tobytes()


# ---- the ghost (ISSUE: the face that turns into view is a cluster of its own) ----
def object_points_left(gpu, model, w):
    sub = gpu.subtract.SceneSubtraction()
    sub.setObject(0, model, w["T"])
    sub.apply(w["frame"])
    return int(w["on_object"][sub.residualIndices()].sum()), sub


def test_ghost_end_to_end(gpu):
    w = gc.ghost_world()
    ref, _, stats = gc.ghost_run()
    dev = gpu.grow.ModelGrowth(confirm=1)
    dev.setModel(w["model"])
    twin = gm.Grow(confirm=1)
    twin.set_model(w["model"])
    before, sub = object_points_left(gpu, w["model"], w)
    assert before == gc.ghost_counts()["before"] >= 500
    # the first apply on the residual of a real subtraction, device to device, then the whole frame until nothing is added
    dev.applyResidual(sub, w["T"])
    twin.apply(w["frame"][sub.residualIndices()], w["T"])
    compare(dev, twin, "residual")
    dev.setModel(w["model"])
    for a, want in enumerate(stats):
        dev.apply(w["frame"], w["T"])
        assert dev.stats() == want, a
    assert dev.stats()["n_added"] == 0
    assert dev.model().tobytes() == ref.cloud.tobytes()
    np.testing.assert_array_equal(dev.states(), ref.states)
    after, _ = object_points_left(gpu, dev.model(), w)
    assert after == gc.ghost_counts()["after"] < 500


# ---- a tracker whose report cloud is replaced between frames ----
def test_report_cloud_replaced_between_frames(gpu):
    model = scene.make_model(300)

    def make():
        t = gpu.tracker.make_reference_tracker(particle_num=64, seed=3)
        t.setIterationNum(2)
        t.setReferenceCloud(model)
        t.setTrans(sc.small_world()["trans"])
        t.setReportCloud(model)
        return t

    a, b = make(), make()
    dev = gpu.grow.ModelGrowth(confirm=1)
    dev.setModel(model)
    for f in (0, 1, 2):
        frame = sc.small_frame(f)
        for t in (a, b):
            t.setInputCloud(frame)
            t.compute()
        dev.applyTracker(a, frame)
        ref = gm.Grow(confirm=1)  # the apply took the result pose
        ref.Ti = gm.inverse(a.toEigenMatrix(a.getResult()))
        np.testing.assert_array_equal(dev.transform().view(np.uint32), ref.Ti.view(np.uint32))
        a.setReportCloud(dev.model())
        assert a.getResult().tobytes() == b.getResult().tobytes(), f
    assert a.getParticles().tobytes() == b.getParticles().tobytes()


# ---- error paths ----
@pytest.mark.parametrize("field,value", [("leaf", 0.0), ("leaf", float("nan")), ("leaf", float("inf")), ("reach", 0), ("reach", 5),
                                         ("confirm", 0), ("confirm", 256), ("forget", 0), ("forget", (1 << 20) + 1),
                                         ("max_radius", 0.0), ("max_radius", float("inf")), ("max_voxels", 32),
                                         ("max_voxels", 96), ("max_voxels", 1 << 23), ("plane_margin", -0.001),
                                         ("plane_margin", float("nan"))])
def test_bad_config_values(gpu, field, value):
    with pytest.raises(gpu.PftError) as e:
        gpu.grow.ModelGrowth(**{field: value})
    assert e.value.status == 1 and field in str(e.value)


def test_config_limits_are_accepted(gpu):
    for kw in (dict(reach=1, confirm=1, forget=1, max_voxels=64, plane_margin=0.0), dict(reach=4, confirm=255, forget=1 << 20)):
        g = gpu.grow.ModelGrowth(**kw)
        g.setModel(gc.shape_model("one"))
        assert g.stats()["n_model_voxels"] == 1


def test_refusals(gpu):
    one = gc.shape_model("one")
    g = gpu.grow.ModelGrowth(max_voxels=64)
    with pytest.raises(gpu.PftError) as e:  # apply before set_model
        g.apply(one, gc.IDENT)
    assert e.value.status == 7 and "pft_grow_set_model" in str(e.value)
    with pytest.raises(gpu.PftError) as e:
        g.stats()
    assert e.value.status == 7
    with pytest.raises(gpu.PftError) as e:  # max_voxels / 2 + 1 voxels
        g.setModel(gc.too_many_voxels_model(33))
    assert e.value.status == 6 and "33 distinct voxels" in str(e.value)
    g.setModel(gc.too_many_voxels_model(32))
    assert g.stats()["n_model_voxels"] == g.stats()["occupied"] == 32
    for bad, text in ((np.nan, "non-finite"), (1e9, "no key")):
        pts = one.copy()
        pts["y"][0] = bad
        with pytest.raises(gpu.PftError) as e:
            g.setModel(pts)
        assert e.value.status == 1 and text in str(e.value)
    g.setModel(one)
    with pytest.raises(gpu.PftError) as e:  # states before the first apply
        g.states()
    assert e.value.status == 7
    for k in (0, 3, 11):
        m = gc.IDENT.copy().reshape(-1)
        m[k] = np.inf if k else np.nan
        with pytest.raises(gpu.PftError) as e:
            g.apply(one, m)
        assert e.value.status == 1 and "non-finite" in str(e.value)
    assert g.stats()["applies"] == 0  # a refused apply does not count
    with pytest.raises(gpu.PftError) as e:  # five planes
        g.setPlanes(np.ones((5, 4), F))
    assert e.value.status == 1 and "5 planes" in str(e.value)
    with pytest.raises(gpu.PftError) as e:
        g.setPlanes([[0, 0, np.nan, 1]])
    assert e.value.status == 1
    g.setPlanes(np.zeros((0, 4), F))
    g.apply(one, gc.IDENT)
    assert g.stats()["n_state"]["KNOWN"] == 1


def test_capacity_error_is_reported_exactly_once(gpu):
    g = gpu.grow.ModelGrowth(reach=4, max_voxels=64)
    g.setModel(gc.shape_model("one"))
    g.apply(gc.records(gc.centre(gc.near_cells(64)), 51), gc.IDENT)
    with pytest.raises(gpu.PftError) as e:
        g.model()  # any synchronising call
    assert e.value.status == 6
    s = g.stats()  # ... once
    assert s["overflow"] == 1 and s["n_pending_live"] == 0 and s["occupied"] == 1 and s["n_model_points"] == 1
    assert len(g.model()) == 1 and len(g.debugTable()["kind"]) == 1
    g.apply(gc.records(gc.centre(gc.near_cells(63)), 50), gc.IDENT)  # the handle stays usable
    s = g.stats()
    assert s["overflow"] == 0 and s["n_candidate_voxels"] == 63 and s["occupied"] == 64

"""The depth entrance on the device: InputFilter.setInputDepth (pft_filter_apply_depth*, k_depth_deproject).  The yardstick
of the cloud is tests/depth_model.py, the literal float32 restatement of the specification, and every comparison is of
bytes: the division is the correctly rounded one and nothing is fused, so there is no tolerance in this file.  Behind the
cloud the yardstick is the existing host path (setInputCloud + filter()) on the model's cloud: the pipeline is the same
code, so its outputs, counts and pass indices must be the same bytes too."""
import ctypes as C

import numpy as np
import pytest

import depth_cases as dc
import depth_model as dm
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu
QNAN = 0x7FC00000


@pytest.fixture(scope="module")
def F():
    from pcl_tracking_amd import filters

    return filters


def make_filter(F, kind):
    f = F.InputFilter()
    if kind == "approx":  # PassThrough z in [0, 10] + ApproximateVoxelGrid(0.01): the reference's front end
        pass
    elif kind == "exact":  # PassThrough + VoxelGrid
        f.setVoxelMode(F.VOXEL_EXACT)
        f.setLeafSize(0.01)
    else:  # no filter at all: the cloud goes through, NaN records included
        f.setPassThrough(enable=False)
        f.setVoxelMode(F.VOXEL_NONE)
    return f


KINDS = ["approx", "exact", "none"]


@pytest.fixture(scope="module")
def handles(F):
    """one depth handle and one record handle per configuration, shared by the cases (handles are reusable)"""
    return {k: (make_filter(F, k), make_filter(F, k)) for k in KINDS}


@pytest.fixture(scope="module")
def models():
    return {name: dm.deproject(**dc.kwargs(c)) for name, c in dc.CASES.items()}


@pytest.fixture(scope="module")
def qhd():
    depth, bgr, camera = scene.make_depth_images()
    return dict(depth=depth, color=bgr, camera=camera), dm.deproject(depth, bgr, camera)


def check_nan_records(cloud):
    bad = cloud["rgba"] == 0
    for k in ("x", "y", "z"):
        bits = cloud[k].view(np.uint32)
        assert (bits[bad] == QNAN).all() and np.isfinite(cloud[k][~bad]).all()
    assert (cloud["w"] == 1.0).all()


# ---- 1. the cloud --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.CASES))
def test_input_cloud_equals_the_model(handles, models, name):
    f = handles["none"][0]
    f.setInputDepth(**dc.kwargs(dc.CASES[name]))
    f.filter()
    got = f.inputCloud()
    want = models[name]
    assert len(got) == dc.CASES[name]["depth"].size
    assert got.tobytes() == want.tobytes()
    check_nan_records(got)


def test_padding_never_reaches_a_result(handles):
    f = handles["none"][0]
    out = []
    for name in ("padded_00", "padded_ff"):
        f.setInputDepth(**dc.kwargs(dc.CASES[name]))
        f.filter()
        out.append(f.inputCloud().tobytes())
    assert out[0] == out[1]


def test_division_not_multiply(handles, models):
    """the case's depths give another float under d * 0.001f: the cloud's z is the division's"""
    c = dc.CASES["u16_division_not_multiply"]
    f = handles["none"][0]
    f.setInputDepth(**dc.kwargs(c))
    f.filter()
    z = f.inputCloud()["z"]
    d = c["depth"].ravel().astype(np.float32)
    assert (z == d / np.float32(1000.0)).all()
    assert np.count_nonzero(z != d * np.float32(0.001)) >= 100


# ---- 2. the pipeline behind it -------------------------------------------------------------------------------------
def same_pipeline(fd, fr, depth_kwargs, model_cloud, asynchronous=False):
    fr.setInputCloud(model_cloud)
    want = fr.filter()
    want_counts, want_idx = fr.counts(), fr.passIndices()
    fd.setInputDepth(**depth_kwargs)
    if asynchronous:
        fd.filterAsync()
        got = fd.output()
    else:
        got = fd.filter()
    assert fd.counts() == want_counts
    assert got.tobytes() == want.tobytes()
    np.testing.assert_array_equal(fd.passIndices(), want_idx)
    return want_counts


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(dc.CASES))
def test_pipeline_equals_the_record_path(handles, models, name, kind):
    fd, fr = handles[kind]
    n_pass, n_out = same_pipeline(fd, fr, dc.kwargs(dc.CASES[name]), models[name])
    if name == "u16_all_zero":  # no valid pixel: an empty output where the NaN records are dropped, never an error
        assert (n_pass, n_out) == ((210, 210) if kind == "none" else (0, 0))


@pytest.mark.parametrize("kind", KINDS)
def test_pipeline_at_qhd(handles, qhd, kind):
    kw, model = qhd
    fd, fr = handles[kind]
    n_pass, n_out = same_pipeline(fd, fr, kw, model)
    assert len(model) == 518400 and 0 < n_out <= n_pass
    if kind != "none":  # the invalid pixels and the far strip are gone
        assert n_pass < np.count_nonzero(kw["depth"])
    assert fd.inputCloud().tobytes() == model.tobytes()


# ---- 3. one handle through changing sizes ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_handle_depth_and_records_alternate(F, handles, models, qhd, kind):
    fd, fr = make_filter(F, kind), handles[kind][1]
    fd._set(max_points=1024)  # the handle starts small and grows with the frames
    records = scene.make_scene(50000)[:5000]
    for step in ("size_65x2", "records", "size_257x5", "size_1x1", "u16_all_zero", "qhd"):
        if step == "records":
            fr.setInputCloud(records)
            want = fr.filter()
            fd.setInputCloud(records)
            assert fd.filter().tobytes() == want.tobytes() and fd.counts() == fr.counts()
            assert fd.inputCloud().tobytes() == records.tobytes()  # the handle owns the upload of a host cloud
        elif step == "qhd":
            same_pipeline(fd, fr, qhd[0], qhd[1])
        else:
            counts = same_pipeline(fd, fr, dc.kwargs(dc.CASES[step]), models[step])
            if step == "u16_all_zero" and kind != "none":
                assert counts == (0, 0) and len(fd.output()) == 0


def test_input_of_a_device_cloud_is_not_the_handles(F, handles):
    import torch

    f = handles["none"][0]
    cloud = scene.make_scene(50000)[:2000]
    keep = torch.from_numpy(cloud.view(np.uint8).reshape(-1)).cuda()
    f.setInputCloudDevice(keep.data_ptr(), len(cloud), keepalive=keep)
    f.filter()
    for call in (f.inputCloud, f.inputDevice):
        with pytest.raises(F.PftError) as e:
            call()
        assert e.value.status == 7  # PFT_ERR_STATE
    f.setInputDepth(**dc.kwargs(dc.CASES["size_63x3"]))
    f.filter()
    assert len(f.inputCloud()) == 189


# ---- 4. pinned slots ------------------------------------------------------------------------------------------------
def test_pinned_slots(F, handles, models):
    fd, fr = make_filter(F, "approx"), handles["approx"][1]
    names = ["size_257x5", "f32_random"]
    want = []
    for name in names:
        fr.setInputCloud(models[name])
        want.append((fr.filter().tobytes(), fr.counts()))
    got = []
    for slot, name in enumerate(names):
        c = dc.CASES[name]
        d, col = fd.depthHostBuffers(slot, c["depth"].shape, c["depth"].dtype, c["color_format"])
        assert d.shape == c["depth"].shape and d.dtype == c["depth"].dtype and col.shape == c["color"].shape
        assert fd.depthSlotDone(slot)  # nothing in flight yet
        d[...] = c["depth"]
        col[...] = c["color"]
        fd.setInputDepth(d, col, c["camera"], c["depth_divisor"], c["color_format"])
        fd.filterAsync()
        if slot == 0:
            continue  # the second frame is filled and enqueued while the first is in flight
        got.append((fd.output().tobytes(), fd.counts()))
    assert got[0] == want[1]
    assert fd.depthSlotDone(0, wait=True) and fd.depthSlotDone(1, wait=True)
    assert fd.depthSlotDone(0) and fd.depthSlotDone(1)
    # an apply from a slot that may still be busy waits for the slot's earlier upload and is served: the same frame twice
    # back to back, then the other slot's frame synchronously
    c = dc.CASES[names[0]]
    d, col = fd.depthHostBuffers(0, c["depth"].shape, c["depth"].dtype, c["color_format"])
    fd.setInputDepth(d, col, c["camera"], c["depth_divisor"], c["color_format"])
    fd.filterAsync()
    fd.filterAsync()
    assert (fd.output().tobytes(), fd.counts()) == want[0]
    assert fd.depthSlotDone(0, wait=True)


def test_async_depth_images_may_be_reused_at_once(F, handles, models):
    fd, fr = handles["approx"]
    c = dc.CASES["size_257x5"]
    fr.setInputCloud(models["size_257x5"])
    want = fr.filter()
    d, col = c["depth"].copy(), c["color"].copy()
    fd.setInputDepth(d, col, c["camera"], c["depth_divisor"], c["color_format"])
    fd.filterAsync()
    d[...] = 0  # caller memory is only borrowed for the call
    col[...] = 0xFF
    assert fd.output().tobytes() == want.tobytes()


# ---- 5. hand-off to the trackers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kld", [False, True])
def test_hand_off_equals_the_record_path(F, kld):
    from pcl_tracking_amd import tracker as T

    model = scene.make_model(512)
    frames = [scene.make_depth_images(320, 180, obj_pose=scene.advance_pose(scene.GT_POSE, k)) for k in range(3)]

    def new_tracker():
        t = T.make_reference_tracker(particle_num=400, seed=5, kld=kld)
        t.setReferenceCloud(model)
        t.setTrans(scene.initial_trans())
        return t

    ta, tb = new_tracker(), new_tracker()
    fa, fb = make_filter(F, "approx"), make_filter(F, "approx")
    for depth, bgr, camera in frames:
        fa.setInputDepth(depth, bgr, camera)
        fa.filterAsync()
        ta.setInputCloudFromFilter(fa)
        ta.compute()
        fb.setInputCloud(dm.deproject(depth, bgr, camera))
        p, n = fb.filterDevice()
        assert n > 1000
        tb.setInputCloudDevice(p, n, keepalive=fb)
        tb.compute()
        assert ta.getResult().tobytes() == tb.getResult().tobytes()
        assert ta.getParticles().tobytes() == tb.getParticles().tobytes()
        assert fa.counts() == fb.counts()


# ---- 6. the organised cloud where it lies ---------------------------------------------------------------------------
def test_segmenter_on_the_input_device(F):
    from pcl_tracking_amd import segment

    depth, bgr, camera = scene.make_depth_images(320, 180)
    f = make_filter(F, "approx")
    f.setInputDepth(depth, bgr, camera)
    f.filterAsync()
    a, b = segment.ModelSegmenter(), segment.ModelSegmenter()
    a.applyDevice(*f.inputDevice(), keepalive=f)
    b.setInputCloud(dm.deproject(depth, bgr, camera))
    b.apply()
    assert a.plane()["status"] == b.plane()["status"] and a.plane()["inliers"] == b.plane()["inliers"]
    np.testing.assert_array_equal(a.planeInliers(), b.planeInliers())
    np.testing.assert_array_equal(a.clusterSizes(), b.clusterSizes())
    for (ia, pa), (ib, pb) in zip(a.clusters(), b.clusters()):
        np.testing.assert_array_equal(ia, ib)
        assert pa.tobytes() == pb.tobytes()


# ---- 7. errors ------------------------------------------------------------------------------------------------------
def test_every_error_names_its_field(F):
    from pcl_tracking_amd import _lib

    L = _lib.load()
    f = make_filter(F, "approx")
    f._ensure()
    depth = np.full((4, 6), 1000, np.uint16)
    color = np.zeros((4, 6, 4), np.uint8)

    def apply(depth_ptr=True, color_ptr=True, fn=L.pft_filter_apply_depth, **kw):
        d = _lib.DepthFrame()
        L.pft_depth_frame_default(C.byref(d))
        d.width, d.height = 6, 4
        for k, v in kw.items():
            setattr(d, k, v)
        st = fn(f._h, C.byref(d), C.c_void_p(depth.ctypes.data) if depth_ptr else None,
                C.c_void_p(color.ctypes.data) if color_ptr else None)
        return st, L.pft_filter_last_error_string(f._h).decode()

    assert apply()[0] == 0
    INVALID, CAPACITY = 1, 6
    nan, inf = float("nan"), float("inf")
    bad = [("fx", v) for v in (0.0, -1.0, nan, inf)] + [("fy", v) for v in (0.0, -540.0, nan, inf)]
    bad += [("depth_divisor", v) for v in (0.0, -1000.0, nan, inf)]
    bad += [("cx", v) for v in (nan, inf, -inf)] + [("cy", v) for v in (nan, inf, -inf)]
    bad += [("depth_format", 2), ("depth_format", -1), ("color_format", 5), ("color_format", -1)]
    bad += [("depth_stride", 11), ("depth_stride", 1), ("color_stride", 17), ("width", 0), ("height", 0), ("width", -3)]
    for fn in (L.pft_filter_apply_depth, L.pft_filter_apply_depth_async):
        for field, value in bad:
            st, text = apply(fn=fn, **{field: value})
            assert st == INVALID and field in text, (field, value, st, text)
        st, text = apply(fn=fn, depth_format=_lib.DEPTH_F32, depth_stride=23)
        assert st == INVALID and "depth_stride" in text
        st, text = apply(fn=fn, color_format=_lib.COLOR_BGRA8, color_stride=23)
        assert st == INVALID and "color_stride" in text
        st, text = apply(fn=fn, depth_ptr=False)
        assert st == INVALID and "depth" in text and "null" in text
        st, text = apply(fn=fn, color_ptr=False)
        assert st == INVALID and "color" in text and "missing" in text
        assert apply(fn=fn, color_ptr=False, color_format=_lib.COLOR_NONE)[0] == 0  # no format, no pointer needed
        assert apply(fn=fn, depth_format=_lib.DEPTH_F32, depth_divisor=nan, depth_stride=24)[0] == 0  # the divisor is U16's
        for field in ("width", "height"):
            st, text = apply(fn=fn, **{field: _lib.DEPTH_MAX_AXIS + 1})
            assert st == CAPACITY and "PFT_DEPTH_MAX_AXIS" in text
    # the handle still works
    st, _ = apply()
    assert st == 0 and f.counts()[0] == 24

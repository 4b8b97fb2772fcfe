"""The frame without a host round trip: InputFilter.filterAsync() and ParticleFilterTracker.setInputCloudFromFilter()
(pft_filter_apply*_async, pft_set_input_from_filter).  The yardstick everywhere is the existing synchronous path on the
same inputs -- filter() / filterDevice() + setInputCloudDevice(ptr, n) -- and every comparison is of bytes: the
asynchronous path runs the same kernels on the same data, only the input count reaches the crop through a device word
instead of a kernel argument, so there is no tolerance anywhere in this file."""
import subprocess

import numpy as np
import pytest

from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu

WG = 1024  # points per crop workgroup (k_crop_onepass, k_crop_count / k_crop_scatter)


@pytest.fixture(scope="module")
def F():
    from pcl_tracking_amd import filters

    return filters


@pytest.fixture(scope="module")
def T():
    from pcl_tracking_amd import tracker

    return tracker


@pytest.fixture(scope="module")
def model():
    return scene.make_model(512)


@pytest.fixture(scope="module")
def frames():
    """six sensor frames of the moving object, 192 x 108 as smoke() uses"""
    return [scene.make_depth_frame(192, 108, obj_pose=scene.advance_pose(scene.GT_POSE, f)) for f in range(6)]


def reference_filter(F):
    return F.make_reference_input_filter()


# ---- front end ------------------------------------------------------------------------------------------------------
def _filters(F):
    def approx():
        return reference_filter(F)  # PassThrough z in [0, 10] + ApproximateVoxelGrid(0.01)

    def exact():
        f = F.InputFilter()
        f.setVoxelMode(F.VOXEL_EXACT)
        f.setLeafSize(0.01)
        return f

    def pass_only():
        f = F.InputFilter()
        f.setVoxelMode(F.VOXEL_NONE)
        return f

    def exact_leaf_too_small():
        f = F.InputFilter()
        f.setPassThrough(enable=False)
        f.setVoxelMode(F.VOXEL_EXACT)
        f.setLeafSize(1e-4)  # (extent / leaf)^3 overflows 2^31 cells: PCL hands the input through
        return f

    return dict(approx=approx, exact=exact, pass_only=pass_only, exact_leaf_too_small=exact_leaf_too_small)


@pytest.mark.parametrize("kind", ["approx", "exact", "pass_only", "exact_leaf_too_small"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_async_apply_equals_filter(F, frames, kind, where):
    """filterAsync() followed by the accessors gives the bytes and counts of filter()"""
    import torch

    frame = frames[0]
    if kind == "exact_leaf_too_small":
        frame = frame[np.isfinite(frame["x"])]
    keep = torch.from_numpy(frame.view(np.uint8).reshape(-1)).cuda()

    def feed(f):
        if where == "host":
            f.setInputCloud(frame)
        else:
            f.setInputCloudDevice(keep.data_ptr(), len(frame), keepalive=keep)

    fs, fa = _filters(F)[kind](), _filters(F)[kind]()
    feed(fs)
    want = fs.filter()
    want_counts, want_idx = fs.counts(), fs.passIndices()
    if kind == "exact_leaf_too_small":
        assert want.tobytes() == frame.tobytes()  # the fallback it is about
    else:
        assert 0 < len(want) < len(frame)
    feed(fa)
    fa.filterAsync()
    assert fa.counts() == want_counts
    got = fa.output()
    assert got.tobytes() == want.tobytes()
    np.testing.assert_array_equal(fa.passIndices(), want_idx)
    assert fa.lastMilliseconds() > 0
    p, n = fa.outputDevice()
    assert p and n == len(want)
    # and the synchronous call on the handle that ran asynchronously (one code path)
    feed(fa)
    assert fa.filter().tobytes() == want.tobytes()


def test_async_host_cloud_may_be_reused_at_once(F, frames):
    f, g = reference_filter(F), reference_filter(F)
    g.setInputCloud(frames[0])
    want = g.filter()
    buf = frames[0].copy()
    f.setInputCloud(buf)
    f.filterAsync()
    buf.view(np.uint8)[:] = 0xFF  # the caller's buffer is only borrowed for the call
    assert f.output().tobytes() == want.tobytes()


def test_two_async_applies_back_to_back(F, frames):
    """no accessor between them: the second frame's result"""
    f, g = reference_filter(F), reference_filter(F)
    g.setInputCloud(frames[1])
    want = g.filter()
    f.setInputCloud(frames[0])
    f.filterAsync()
    f.setInputCloud(frames[1])
    f.filterAsync()
    assert f.counts() == g.counts()
    assert f.output().tobytes() == want.tobytes()


def test_async_apply_of_an_empty_cloud(F):
    f = reference_filter(F)
    f.setInputCloud(np.zeros(0, scene.POINT_DTYPE))
    f.filterAsync()
    assert f.counts() == (0, 0) and len(f.output()) == 0


# ---- the crop under a device count ----------------------------------------------------------------------------------
N_IN = 40 * WG  # input of the filter: with max_points = 0 the crop's grid is 40 workgroups whatever the count is


@pytest.fixture(scope="module")
def base_cloud():
    c = scene.make_scene(50000)[:N_IN].copy()
    assert np.isfinite(c["x"]).all() and (c["z"] > 0).all() and (c["z"] < 10).all()
    return c


def cloud_with_k_survivors(base, k):
    """PassThrough z in [0, 10] keeps exactly the k points of `base` nearest to the object, wherever they lie in the
    cloud; every other point is moved behind the far limit"""
    g = scene.model_gt_pose()
    d2 = (base["x"] - g[0]) ** 2 + (base["y"] - g[1]) ** 2 + (base["z"] - g[2]) ** 2
    keep = np.zeros(len(base), bool)
    keep[np.argsort(d2, kind="stable")[:k]] = True
    c = base.copy()
    c["z"][~keep] += np.float32(100.0)
    return c


def pass_filter(F):
    f = F.PassThrough()
    f.setFilterFieldName("z")
    f.setFilterLimits(0, 10)
    return f


def eval_particles(n=24, seed=3):
    rng = np.random.default_rng(seed)
    g = scene.model_gt_pose()
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    for i, k in enumerate(("x", "y", "z", "roll", "pitch", "yaw")):
        p[k] = (g[i] + rng.normal(0, 0.01 if i < 3 else 0.05, n)).astype(np.float32)
    p["weight"] = 1.0 / n
    return p


def new_tracker(T, model, particle_num=64, **kw):
    t = T.make_reference_tracker(particle_num=particle_num, **kw)
    t.setReferenceCloud(model)
    t.setTrans(scene.initial_trans())
    return t


def same_eval(a, b):
    for k in ("raw", "nn_idx", "nn_d2", "crop_idx", "bbox"):
        assert a[k].tobytes() == b[k].tobytes(), k


COUNTS = [1, WG - 1, WG, WG + 1, 3 * WG, 3 * WG + 1]


@pytest.fixture(scope="module")
def crop_reference(F, T, model, base_cloud):
    """the synchronous results, computed once: count -> evalWeights of setInputCloudDevice(ptr, n)"""
    ref = {}
    t = new_tracker(T, model)
    f = pass_filter(F)
    for k in COUNTS:
        f.setInputCloud(cloud_with_k_survivors(base_cloud, k))
        p, n = f.filterDevice()
        assert n == k  # by construction
        t.setInputCloudDevice(p, n, keepalive=f)
        ref[k] = t.evalWeights(eval_particles(), want_nn=True)
        assert len(ref[k]["crop_idx"]) > 0
    return ref


@pytest.mark.parametrize("two_pass", [False, True])
@pytest.mark.parametrize("bound", ["input", "count"])
@pytest.mark.parametrize("k", COUNTS)
def test_crop_under_a_device_count(F, T, model, base_cloud, crop_reference, monkeypatch, k, bound, two_pass):
    """max_points = 0: the bound is the filter's input, 40 workgroups of which at most 4 are live (surplus workgroups
    take their ticket and leave); max_points = the count: none is surplus"""
    if two_pass:
        monkeypatch.setenv("PFT_CROP_TWO_PASS", "1")  # latched by pft_create: a fresh handle
    t = new_tracker(T, model)
    f = pass_filter(F)
    f.setInputCloud(cloud_with_k_survivors(base_cloud, k))
    f.filterAsync()
    t.setInputCloudFromFilter(f, 0 if bound == "input" else k)
    got = t.evalWeights(eval_particles(), want_nn=True)
    same_eval(got, crop_reference[k])
    assert f.counts() == (k, k)
    # the later crops of a frame read the handle's own copy of the count: evaluate again, the filter re-applied meanwhile
    f.setInputCloud(cloud_with_k_survivors(base_cloud, 7))
    f.filterAsync()
    same_eval(t.evalWeights(eval_particles(), want_nn=True), crop_reference[k])


# ---- whole frames, several objects ----------------------------------------------------------------------------------
CONFIGS = {
    "fixed400": dict(particle_num=400),
    "kld": dict(particle_num=400, kld=True),
    "pcl_sums": dict(particle_num=400, sum_order="pcl"),
    "change_detector": dict(particle_num=400, change_detector=(10, 5, 0.05)),
    "exact_nn": dict(particle_num=100, exact=True),
    "sorted_builder": dict(particle_num=400, env=("PFT_FORCE_BUILDER", "sorted")),
    "graph": dict(particle_num=400, env=("PFT_GRAPH", "1")),
}


def make_objects(T, model, cfg, n_obj=3, report=True):
    from pcl_tracking_amd.tracker import (DistanceCoherence, HSVColorCoherence, NearestPairPointCloudCoherence,
                                          OctreeSearch)

    cfg = dict(cfg)
    cfg.pop("env", None)
    exact = cfg.pop("exact", False)
    objs = []
    for o in range(n_obj):
        t = T.make_reference_tracker(seed=11 + o, **cfg)
        if exact:
            coh = NearestPairPointCloudCoherence()
            coh.addPointCoherence(DistanceCoherence())
            col = HSVColorCoherence()
            col.setWeight(0.1)
            coh.addPointCoherence(col)
            coh.setSearchMethod(OctreeSearch(0.01))
            coh.setMaximumDistance(0.1)
            t.setCloudCoherence(coh)
        t.setReferenceCloud(model)
        tr = scene.initial_trans().copy()
        tr[0, 3] += 0.002 * o  # three objects = three slightly different starts on the same scene
        t.setTrans(tr)
        if report:
            t.setReportCloud(model)
        objs.append(t)
    return objs


def drive(F, objs, frames, asynchronous, report=True):
    f = reference_filter(F)
    for fr in frames:
        f.setInputCloud(fr)
        if asynchronous:  # reads nothing until the last frame: the events alone keep filter and trackers in order
            f.filterAsync()
            for t in objs:
                t.setInputCloudFromFilter(f)
                t.compute()
                if report:
                    t.computeReport()
        else:
            p, n = f.filterDevice()
            for t in objs:
                t.setInputCloudDevice(p, n, keepalive=f)
                t.compute()
                if report:
                    t.computeReport()
            for t in objs:
                t.getResult()
    out = []
    for t in objs:
        r = t.getResult()
        rep = t.getReport() if report else None
        out.append((t.getParticles().tobytes(), r.tobytes(),
                    None if rep is None else b"".join(np.asarray(getattr(rep, k)).tobytes() for k in
                                                      ("transform", "centroid", "covariance", "axes", "box_centre",
                                                       "box_quat", "box_size"))))
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_three_objects_six_frames(F, T, model, frames, monkeypatch, name):
    cfg = CONFIGS[name]
    if "env" in cfg:
        monkeypatch.setenv(*cfg["env"])
    report = name != "exact_nn"  # (the report does not depend on the coherence; one configuration goes without)
    want = drive(F, make_objects(T, model, cfg, report=report), frames, False, report)
    got = drive(F, make_objects(T, model, cfg, report=report), frames, True, report)
    for o, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], "particles of object %d" % o
        assert g[1] == w[1], "result of object %d" % o
        assert g[2] == w[2], "report of object %d" % o
    assert len({w[1] for w in want}) == len(want)  # the objects did run apart


# ---- error cases ----------------------------------------------------------------------------------------------------
def test_device_count_of_zero(F, T, model, frames):
    from pcl_tracking_amd._lib import PftError

    t = new_tracker(T, model, 400)
    f = reference_filter(F)
    f.setPassThrough("z", 50.0, 60.0)  # keeps nothing
    f.setInputCloud(frames[0])
    f.filterAsync()
    t.setInputCloudFromFilter(f)
    t.compute()
    with pytest.raises(PftError) as e:
        t.getResult()
    assert e.value.status == 2 and "pft_set_input_from_filter" in str(e.value)  # PFT_ERR_NO_INPUT
    assert f.counts() == (0, 0)
    # The handle tracks on once the next frame has points.  The empty frame moved the particles by two steps of noise
    # (sigma 1.5 cm per axis): their mean, the pose, moves by about sigma * sqrt(2 / 400) = 1 mm, far inside the 10 cm
    # gate, so the next frames find the object as usual; 4 cm is the bound the driver tests put on a tracked position
    g = reference_filter(F)
    for fr in frames[1:3]:
        g.setInputCloud(fr)
        g.filterAsync()
        t.setInputCloudFromFilter(g)
        t.compute()
    rt = t.getResult()
    gt = scene.model_gt_pose(scene.advance_pose(scene.GT_POSE, 2))
    for i, k in enumerate(("x", "y", "z")):
        print(k, float(rt[k]), gt[i])
        assert abs(float(rt[k]) - gt[i]) < 0.04


def test_device_count_above_max_points(F, T, model, base_cloud):
    from pcl_tracking_amd._lib import PftError

    k, bound = 3 * WG + 1, 2 * WG + 5
    t = new_tracker(T, model)
    t._cfg.max_input_points = 8 * WG
    f = pass_filter(F)
    # fill the handle's input records: 5 000 points through the ordinary path
    f.setInputCloud(cloud_with_k_survivors(base_cloud, 5000))
    t.setInputCloudDevice(*f.filterDevice(), keepalive=f)
    t.evalWeights(eval_particles())
    before = t.debugInputRecords(0, 8 * WG)
    f.setInputCloud(cloud_with_k_survivors(base_cloud, k))
    f.filterAsync()
    t.setInputCloudFromFilter(f, bound)
    with pytest.raises(PftError) as e:
        t.evalWeights(eval_particles())
    assert e.value.status == 6 and "pft_set_input_from_filter" in str(e.value)  # PFT_ERR_CAPACITY
    after = t.debugInputRecords(0, 8 * WG)
    out = f.output()
    assert len(out) == k
    want = np.stack([out["x"].view(np.uint32), out["y"].view(np.uint32), out["z"].view(np.uint32), out["rgba"]], 1)
    assert after[:bound].tobytes() == want[:bound].tobytes()  # the crop read max_points points ...
    assert after[bound:].tobytes() == before[bound:].tobytes()  # ... and nothing behind the bound was written
    assert before[bound:k].tobytes() != want[bound:k].tobytes()
    # the handle goes on with a frame that fits
    f.setInputCloud(cloud_with_k_survivors(base_cloud, WG))
    f.filterAsync()
    t.setInputCloudFromFilter(f, bound)
    assert len(t.evalWeights(eval_particles())["crop_idx"]) > 0


def test_refusals(F, T, model, frames):
    from pcl_tracking_amd._lib import PftError

    f = reference_filter(F)
    f.setInputCloud(frames[0])
    f.filterAsync()
    sharded = T.make_reference_tracker(particle_num=64, rank=0, world_size=2)
    sharded.setReferenceCloud(model)
    with pytest.raises(PftError) as e:
        sharded.setInputCloudFromFilter(f)
    assert e.value.status == 1 and "sharded" in str(e.value)
    never = reference_filter(F)
    never._ensure()
    t = new_tracker(T, model)
    with pytest.raises(PftError) as e:
        t.setInputCloudFromFilter(never)
    assert e.value.status == 7 and "not been applied" in str(e.value)
    import torch

    other = F.InputFilter(device_id=1)
    other.setInputCloud(frames[0])
    if torch.cuda.device_count() < 2:
        # one device: a filter on another device cannot come into being (pft_filter_create refuses the ordinal), which
        # is all there is to check of that refusal here; with two devices the hand-off itself is refused below
        with pytest.raises(PftError) as e:
            other.filterAsync()
        assert e.value.status == 1
        return
    other.filterAsync()
    with pytest.raises(PftError) as e:
        t.setInputCloudFromFilter(other)
    assert e.value.status == 1 and "another device" in str(e.value)
    assert other.counts()[1] > 0


def test_filter_applied_again_before_the_first_crop(F, T, model, frames):
    """the output a tracker was handed is gone when the filter runs again before the tracker's first crop"""
    from pcl_tracking_amd._lib import PftError

    t = new_tracker(T, model)
    f = reference_filter(F)
    f.setInputCloud(frames[0])
    f.filterAsync()
    t.setInputCloudFromFilter(f)
    f.filterAsync()
    with pytest.raises(PftError) as e:
        t.compute()
    assert e.value.status == 2 and "applied again" in str(e.value)


def test_either_handle_may_be_destroyed_first(F, T, model, frames):
    """run once: a filter destroyed before its tracker, and the reverse"""
    t = new_tracker(T, model, 400)
    f = reference_filter(F)
    f.setInputCloud(frames[0])
    f.filterAsync()
    t.setInputCloudFromFilter(f)
    t.compute()
    t._keep = None
    f.close()  # the tracker's frame is in flight; its later crops read the handle's own records
    r = t.getResult()
    assert np.isfinite(float(r["x"]))
    t.close()
    t = new_tracker(T, model, 400)
    f = reference_filter(F)
    f.setInputCloud(frames[0])
    f.filterAsync()
    t.setInputCloudFromFilter(f)
    t.compute()
    t.close()
    f.setInputCloud(frames[1])
    f.filterAsync()  # settles the link the tracker left behind
    assert f.counts()[1] > 0
    f.close()


# ---- driver ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_report", [False, True])
def test_driver_async_equals_raw(tmp_path, model, frames, device_report):
    from pcl_tracking_amd import build

    exe = build.build_example()
    off = np.array(scene.model_gt_pose()[:3], np.float32)
    paths = []
    for o in range(2):
        c = model.copy()
        for k, name in enumerate(("x", "y", "z")):
            c[name] = c[name] + off[k] + np.float32(0.002 * o)
        c.tofile(tmp_path / ("m%d.bin" % o))
        paths.append(str(tmp_path / ("m%d.bin" % o)))
    fr = []
    for i, x in enumerate(frames[:3]):
        x.tofile(tmp_path / ("f%d.bin" % i))
        fr.append(str(tmp_path / ("f%d.bin" % i)))
    outs = []
    for extra in ([], ["--async"]):
        args = paths + ["--frames"] + fr + ["--raw", "--model-leaf", "0"] + (["--device-report"] if device_report else [])
        r = subprocess.run([exe] + args + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r)
    assert outs[0].stdout == outs[1].stdout
    assert len(outs[0].stdout.splitlines()) == 2 * 3 * (2 if device_report else 1)
    down = [l for l in outs[0].stderr.splitlines() if "downsampled" in l]
    assert down and down == [l for l in outs[1].stderr.splitlines() if "downsampled" in l]

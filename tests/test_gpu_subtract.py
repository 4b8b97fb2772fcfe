"""GPU checks of scene subtraction (include/pft_subtract.h; pcl_tracking_amd/csrc/pft_subtract.hip) against the all-pairs
NumPy model (tests/subtract_model.py): owner, d2 (as bits), support, the counts, the residual's indices and its bytes,
every one with assert_array_equal.  The inputs live in tests/subtract_cases.py; tests/test_subtract_host.py shows by the
model alone that each of them tests what it claims."""
import functools

import numpy as np
import pytest

import segment_model as sg
import subtract_cases as sc
import subtract_model as sm
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu
F = np.float32
P = 64


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import subtract, tracker

    class G:
        pass

    g = G()
    g.subtract, g.tracker = subtract, tracker
    return g


def fetch(sub):
    return dict(counts=sub.counts(), owner=sub.owners(), d2=sub.sqDistances(), support=sub.support(),
                residual_idx=sub.residualIndices(), residual=sub.residual())


def compare(dev, frame, slots, radius=sc.R):
    """the device's results of one apply against the model's for the same slots"""
    exp = sm.subtract(sm.xyz_of(frame), slots, radius)
    assert dev["counts"] == (exp["n_in"], exp["n_explained"], exp["n_residual"])
    np.testing.assert_array_equal(dev["owner"], exp["owner"])
    np.testing.assert_array_equal(dev["d2"].view(np.uint32), exp["d2"].view(np.uint32))
    np.testing.assert_array_equal(dev["support"], exp["support"])
    np.testing.assert_array_equal(dev["residual_idx"], exp["residual_idx"])
    assert dev["residual"].tobytes() == frame[exp["residual_idx"]].tobytes()
    return exp


def fill(sub, slots):
    for s, (model, T) in slots.items():
        sub.setObject(s, sc.records(model, seed=s), T)


def apply_and_compare(sub, frame, slots, radius=sc.R):
    sub.apply(frame)
    return compare(fetch(sub), frame, slots, radius)


# ---- 1. neighbour cells ----
@pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated"])
@pytest.mark.parametrize("where", list(sc.OFFSETS))
def test_neighbour_cells(gpu, where, rotated):
    c = sc.neighbour_case(where, rotated)
    slots = {0: (c["model"], c["T"])}
    sub = gpu.subtract.SceneSubtraction()
    fill(sub, slots)
    frame = sc.records(c["frame"], seed=1)
    apply_and_compare(sub, frame, slots)
    T, moved = sub.object(0)
    np.testing.assert_array_equal(T.view(np.uint32), c["T"].view(np.uint32))
    np.testing.assert_array_equal(moved.view(np.uint32), sm.xform(c["T"], c["model"]).view(np.uint32))


# ---- 2. coarse cells and degenerate extents ----
def test_coarse_cells_and_degenerate_extents(gpu):
    c = sc.degenerate_case()
    sub = gpu.subtract.SceneSubtraction()
    fill(sub, c["slots"])
    exp = apply_and_compare(sub, sc.records(c["frame"], seed=2), c["slots"])
    assert exp["support"][12] == 0
    T, moved = sub.object(12)  # the empty slot is a filled slot
    assert moved.shape == (0, 3)
    assert sub.object(5)[1].shape == (5000, 3)


# ---- 3. several slots ----
def test_64_slots_with_ties(gpu):
    c = sc.many_slots_case()
    sub = gpu.subtract.SceneSubtraction()
    fill(sub, c["slots"])
    exp = apply_and_compare(sub, sc.records(c["frame"], seed=3), c["slots"])
    assert exp["ties"].sum() >= 1
    with pytest.raises(gpu.subtract.PftError) as e:
        sub.setObject(64, sc.records(c["slots"][0][0]), sc.matrix())
    assert e.value.status == 1 and "slot 64" in str(e.value)


def test_slots_with_gaps_removed_and_refilled(gpu):
    c = sc.many_slots_case()
    frame = sc.records(c["frame"], seed=4)
    slots = {s: c["slots"][s] for s in (1, 6, 7, 20, 63)}
    sub = gpu.subtract.SceneSubtraction()
    fill(sub, slots)
    apply_and_compare(sub, frame, slots)
    sub.removeObject(7)  # the slots behind it move up in the pool
    del slots[7]
    apply_and_compare(sub, frame, slots)
    with pytest.raises(gpu.subtract.PftError) as e:
        sub.object(7)
    assert e.value.status == 7
    slots[7] = c["slots"][33]  # refilled with another object
    sub.setObject(7, sc.records(slots[7][0]), slots[7][1])
    apply_and_compare(sub, frame, slots)
    sub.clear()
    apply_and_compare(sub, frame, {})


# ---- 4. frame sizes around the compaction tile ----
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 70001])
def test_frame_sizes(gpu, n):
    c = sc.sized_frame(n)
    sub = gpu.subtract.SceneSubtraction()
    fill(sub, c["slots"])
    exp = apply_and_compare(sub, sc.records(c["frame"], seed=n), c["slots"])
    if n >= 1023:
        assert 0 < exp["n_explained"] < n


def test_everything_and_nothing_explained(gpu):
    c = sc.sized_frame(1025)
    slab = c["slots"][3][0]
    sub = gpu.subtract.SceneSubtraction()
    fill(sub, c["slots"])
    rng = np.random.default_rng(5)
    every = np.concatenate([slab, slab[rng.choice(len(slab), 2000)] + rng.uniform(-0.004, 0.004, (2000, 3)).astype(F)])
    exp = apply_and_compare(sub, sc.records(every, seed=5), c["slots"])
    assert exp["n_residual"] == 0 and sub.residualDevice() == (0, 0)
    nothing = sc.records(every + F(5.0), seed=6)
    exp = apply_and_compare(sub, nothing, c["slots"])
    assert exp["n_explained"] == 0
    none = gpu.subtract.SceneSubtraction()  # no filled slot: the residual is the input
    none.apply(nothing)
    d = fetch(none)
    assert d["counts"] == (len(nothing), 0, len(nothing)) and (d["owner"] == -1).all() and np.isinf(d["d2"]).all()
    assert d["residual"].tobytes() == nothing.tobytes()
    # non-finite frame points stay in the residual byte for byte
    bad = sc.records(every[:300], seed=7)
    bad["x"][::7] = np.nan
    bad["y"][3::11] = np.inf
    bad["z"][5::13] = -np.inf
    exp = apply_and_compare(sub, bad, c["slots"])
    assert 0 < exp["n_residual"] < 300


def test_other_radius_and_the_strict_gate(gpu):
    sub = gpu.subtract.SceneSubtraction(radius=0.25)
    slots = {0: (np.zeros((1, 3), F), sc.matrix())}
    fill(sub, slots)
    at = F(0.25)
    below = np.nextafter(at, F(0))
    frame = sc.records(np.array([[at, 0, 0], [below, 0, 0], [0, -at, 0], [0, 0, -below], [0, at, at]], F))
    exp = apply_and_compare(sub, frame, slots, radius=0.25)
    np.testing.assert_array_equal(exp["owner"], [-1, 0, -1, 0, -1])


# ---- 5. reuse ----
def test_reuse_of_a_handle(gpu):
    big, small = sc.sized_frame(70001), sc.sized_frame(1023)
    slots = big["slots"]
    fb, fs = sc.records(big["frame"], seed=8), sc.records(small["frame"], seed=9)
    sub = gpu.subtract.SceneSubtraction()
    fill(sub, slots)
    sub.apply(fb)
    first = fetch(sub)
    sub.apply(fb)
    second = fetch(sub)
    fresh = gpu.subtract.SceneSubtraction()
    fill(fresh, slots)
    fresh.apply(fb)
    third = fetch(fresh)
    for other in (second, third):
        assert other["counts"] == first["counts"]
        for k in ("owner", "d2", "support", "residual_idx", "residual"):
            assert other[k].tobytes() == first[k].tobytes(), k
    compare(first, fb, slots)
    apply_and_compare(sub, fs, slots)  # a small frame after a large one: nothing stale
    # a larger model after a smaller one: the pool grows
    many = sc.many_slots_case()
    fill(sub, many["slots"])
    apply_and_compare(sub, sc.records(many["frame"], seed=10), many["slots"])


def test_set_object_matrix_moves_the_object(gpu):
    c = sc.sized_frame(1025)
    model = c["slots"][3][0]
    frame = sc.records(c["frame"], seed=11)
    sub = gpu.subtract.SceneSubtraction()
    sub.setObject(3, sc.records(model), sc.matrix())
    a = apply_and_compare(sub, frame, {3: (model, sc.matrix())})
    T2 = sc.matrix((0.05, -0.03, 0.02), (0.2, 0.1, -0.3))
    sub.setObjectMatrix(3, T2)
    b = apply_and_compare(sub, frame, {3: (model, T2)})
    assert not np.array_equal(a["owner"], b["owner"])
    np.testing.assert_array_equal(sub.object(3)[0].view(np.uint32), T2.view(np.uint32))
    for bad in (np.full(12, np.nan, F), np.r_[np.inf, np.zeros(11)].astype(F)):
        with pytest.raises(gpu.subtract.PftError) as e:
            sub.setObjectMatrix(3, bad)
        assert e.value.status == 1 and "non-finite" in str(e.value)
    with pytest.raises(gpu.subtract.PftError) as e:
        sub.setObjectMatrix(4, T2)
    assert e.value.status == 7
    nan_model = sc.records(model[:10])
    nan_model["y"][4] = np.nan
    with pytest.raises(gpu.subtract.PftError) as e:
        sub.setObject(5, nan_model, T2)
    assert e.value.status == 1 and "point 4" in str(e.value)
    apply_and_compare(sub, frame, {3: (model, T2)})  # the refusals changed nothing


# ---- 6. bound trackers ----
@functools.lru_cache(maxsize=None)
def model300():
    return scene.make_model(300)


def make_tracker(gpu, kld=False, exact=False, seed=3, **kw):
    t = gpu.tracker.make_reference_tracker(particle_num=P, seed=seed, kld=kld, **kw)
    if exact:
        coh = gpu.tracker.NearestPairPointCloudCoherence()
        coh.addPointCoherence(gpu.tracker.DistanceCoherence())
        hc = gpu.tracker.HSVColorCoherence()
        hc.setWeight(0.1)
        coh.addPointCoherence(hc)
        coh.setSearchMethod(gpu.tracker.OctreeSearch(0.01))
        coh.setMaximumDistance(0.1)
        t.setCloudCoherence(coh)
    if kld:
        t.setMaximumParticleNum(100)
    t.setIterationNum(2)
    t.setReferenceCloud(model300())
    t.setTrans(sc.small_world()["trans"])
    return t


def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


@pytest.mark.parametrize("kind", ["fixed", "kld", "exact"])
def test_bound_tracker_equals_the_explicit_form(gpu, kind):
    t = make_tracker(gpu, kld=kind == "kld", exact=kind == "exact")
    frame = sc.small_frame(0)
    t.setInputCloud(frame)
    t.compute()
    sub = gpu.subtract.SceneSubtraction()
    sub.bindTracker(2, t)
    sub.apply(frame)
    dev = fetch(sub)
    T, moved = sub.object(2)
    want = t.debugPoseToMatrix(np.array([t.getResult()]))[0]
    np.testing.assert_array_equal(T.view(np.uint32), want.view(np.uint32))
    mxyz = sm.xyz_of(model300())
    np.testing.assert_array_equal(sorted_rows(moved).view(np.uint32), sorted_rows(sm.xform(T, mxyz)).view(np.uint32))
    exp = compare(dev, frame, {2: (mxyz, T)})
    assert exp["n_explained"] > 1000  # the tracker is on the object
    ex = gpu.subtract.SceneSubtraction()
    ex.setObject(2, model300(), T)
    ex.apply(frame)
    got = fetch(ex)
    for k in ("owner", "d2", "support", "residual_idx", "residual"):
        assert got[k].tobytes() == dev[k].tobytes(), k


def test_bound_apply_without_a_host_wait(gpu):
    f0, f1 = sc.small_frame(0), sc.small_frame(1)
    a, b, never = make_tracker(gpu), make_tracker(gpu), make_tracker(gpu)
    sa, sb = gpu.subtract.SceneSubtraction(), gpu.subtract.SceneSubtraction()
    sa.bindTracker(0, a)
    sb.bindTracker(0, b)
    # a: compute, apply, compute -- nothing waits in between
    a.setInputCloud(f0)
    a.compute()
    sa.apply(f0)
    a.setInputCloud(f1)
    a.compute()
    # b: the same with a wait after every call
    b.setInputCloud(f0)
    b.compute()
    b.synchronize()
    sb.apply(f0)
    want = fetch(sb)
    Tb = sb.object(0)[0]
    b.setInputCloud(f1)
    b.compute()
    b.synchronize()
    got = fetch(sa)
    np.testing.assert_array_equal(sa.object(0)[0].view(np.uint32), Tb.view(np.uint32))
    assert got["counts"] == want["counts"]
    for k in ("owner", "d2", "support", "residual_idx", "residual"):
        assert got[k].tobytes() == want[k].tobytes(), k
    compare(got, f0, {0: (sm.xyz_of(model300()), Tb)})
    # a tracker with a bound slot computes what a twin that was never bound computes
    for f in (f0, f1):
        never.setInputCloud(f)
        never.compute()
    assert a.getResult().tobytes() == never.getResult().tobytes() == b.getResult().tobytes()
    assert a.getParticles().tobytes() == never.getParticles().tobytes()
    # the second apply takes the new pose
    sa.apply(f1)
    T1 = sa.object(0)[0]
    np.testing.assert_array_equal(T1.view(np.uint32), a.debugPoseToMatrix(np.array([a.getResult()]))[0].view(np.uint32))
    compare(fetch(sa), f1, {0: (sm.xyz_of(model300()), T1)})


def test_bound_tracker_refusals(gpu):
    frame = sc.small_frame(0)
    sub = gpu.subtract.SceneSubtraction()
    t = make_tracker(gpu)
    sub.bindTracker(0, t)
    with pytest.raises(gpu.subtract.PftError) as e:  # before the tracker's first frame: refused by the apply
        sub.apply(frame)
    assert e.value.status == 7 and "pft_compute" in str(e.value)
    with pytest.raises(gpu.subtract.PftError) as e:  # ... and there is no result of that apply
        sub.counts()
    assert e.value.status == 7
    t.setInputCloud(frame)
    t.compute()
    sub.apply(frame)
    assert sub.counts()[1] > 1000
    t.resetTracking()
    with pytest.raises(gpu.subtract.PftError) as e:
        sub.apply(frame)
    assert e.value.status == 7
    sharded = gpu.tracker.make_reference_tracker(particle_num=P, seed=3, rank=0, world_size=2)
    sharded.setReferenceCloud(model300())
    with pytest.raises(gpu.subtract.PftError) as e:
        sub.bindTracker(1, sharded)
    assert e.value.status == 1 and "sharded" in str(e.value)
    rep = gpu.subtract.SceneSubtraction(cloud="report")
    with pytest.raises(gpu.subtract.PftError) as e:
        rep.bindTracker(0, t)
    assert e.value.status == 7 and "report cloud" in str(e.value)


def test_report_cloud_and_removal_before_the_tracker_goes(gpu):
    frame = sc.small_frame(0)
    t = make_tracker(gpu)
    dense = scene.make_model(2000)
    t.setReportCloud(dense)
    t.setInputCloud(frame)
    t.compute()
    rep = gpu.subtract.SceneSubtraction(cloud="report")
    rep.bindTracker(0, t)
    slab = sc.sized_frame(1025)["slots"][3]
    rep.setObject(1, sc.records(slab[0]), slab[1])
    rep.apply(frame)
    T, moved = rep.object(0)
    assert moved.shape == (2000, 3)
    np.testing.assert_array_equal(moved.view(np.uint32), sm.xform(T, sm.xyz_of(dense)).view(np.uint32))
    compare(fetch(rep), frame, {0: (sm.xyz_of(dense), T), 1: slab})
    rep.removeObject(0)
    t.close()  # the slot was removed first: the tracker may go
    apply_and_compare(rep, frame, {1: slab})


# ---- 7. end to end ----
def test_track_subtract_segment(gpu):
    from pcl_tracking_amd import segment

    t = make_tracker(gpu)
    for f in (0, 1):
        frame = sc.small_frame(f, second=True)  # a second object stands beside the tracked one
        t.setInputCloud(frame)
        t.compute()
    sub = gpu.subtract.SceneSubtraction()
    sub.bindTracker(0, t)
    sub.apply(frame)
    seg = segment.ModelSegmenter()
    seg.configure(plane=False, box_enable=(0, 0, 0), tolerance=sc.SEGMENT["tol"], min_size=sc.SEGMENT["min_size"],
                  max_size=sc.SEGMENT["max_size"])
    got = sub.segmentResidual(seg)
    T = sub.object(0)[0]
    exp = compare(fetch(sub), frame, {0: (sm.xyz_of(model300()), T)})
    ridx = exp["residual_idx"]
    want = sg.pipeline(frame[ridx], plane=False, box_enable=(0, 0, 0), **sc.SEGMENT)["clusters"]
    assert len(got) == len(want) >= 1
    owner = sub.owners()
    for (gi, gp), wi in zip(got, want):
        np.testing.assert_array_equal(gi, ridx[wi])
        assert gp.tobytes() == frame[ridx[wi]].tobytes()
        assert (owner[gi] < 0).all()
    # the object's cluster is in the full frame's clustering and not in the residual's
    on_object = np.linalg.norm(sm.xyz_of(frame).astype(np.float64) - sc.small_world()["gt"], axis=1) < 0.3
    seg.setInputCloud(frame)
    seg.apply()
    assert any(on_object[i].mean() > 0.9 for i, _ in seg.clusters())
    assert not any(on_object[i].mean() > 0.5 for i, _ in got)

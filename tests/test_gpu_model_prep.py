"""Model preparation on the device (include/pft_model.h) against the CPU oracle's restatement of the "set object to
track" block (auto_tracking.cpp:643-677): remove_zero_points -> compute_3d_centroid(is_dense=True) -> recentre_model ->
voxel_grid.  Everything is compared as bytes: the three counts, the 16 floats of trans, the re-centred cloud and the
reference cloud as raw 32-byte records."""
import functools

import numpy as np
import pytest

from pcl_tracking_amd import scene
from pcl_tracking_amd._lib import PftError

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 25000]


# ---- clouds and the oracle chain ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cluster(n, seed=0):
    """n points uniform in a 0.3 m cube around (0.1, -0.1, 0.8) with random colours (and random padding words: every
    byte of a record has to come through).  From 65 points on, mixed in at random places: a NaN in each coordinate in
    turn, points inside the 1 cm cube at the origin, per axis the values 0.01f, nextafter(0.01f, 1) and -0.01f with the
    other two coordinates near zero, and two identical points."""
    rng = np.random.default_rng(1000 + seed * 100003 + n)
    c = np.zeros(n, scene.POINT_DTYPE)
    xyz = (rng.uniform(-0.15, 0.15, (n, 3)) + [0.1, -0.1, 0.8]).astype(F)
    c["x"], c["y"], c["z"], c["w"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 1.0
    c["rgba"] = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    c["pad"] = rng.integers(0, 2 ** 32, (n, 3), dtype=np.uint32)
    if n >= 65:
        special = []
        for a in range(3):  # NaN in each coordinate in turn
            v = [0.1, -0.1, 0.8]
            v[a] = np.nan
            special.append(v)
        for _ in range(4):  # inside the 1 cm cube at the origin
            special.append(list(rng.uniform(-0.0099, 0.0099, 3)))
        edge = [F(0.01), np.nextafter(F(0.01), F(1)), F(-0.01)]
        for a in range(3):  # on the boundary of that cube, the other two coordinates near zero
            for e in edge:
                v = list(rng.uniform(-0.001, 0.001, 3))
                v[a] = e
                special.append(v)
        at = rng.choice(n - 2, len(special), replace=False)
        for i, v in zip(at, special):
            c["x"][i], c["y"][i], c["z"][i] = F(v[0]), F(v[1]), F(v[2])
        plain = np.setdiff1d(np.arange(n - 2), at)
        c[n - 1] = c[plain[0]]  # two identical points
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _orc():
    import oracle

    oracle.lib()
    return oracle


def oracle_chain(cloud, leaf):
    """-> dict(counts, trans, recentred, reference) by the oracle; leaf <= 0 or a leaf PCL refuses: reference = recentred"""
    orc = _orc()
    nz = orc.remove_zero_points(cloud)
    c, used = orc.compute_3d_centroid(nz, is_dense=True)
    assert used == len(nz)
    rec, trans = orc.recentre_model(nz, c)
    ref = orc.voxel_grid(rec, leaf) if leaf > 0 else rec
    if ref is None:
        ref = rec
    return dict(counts=(len(cloud), len(nz), len(ref)), trans=trans, recentred=rec, reference=ref)


@functools.lru_cache(maxsize=None)
def oracle_of(n, leaf, seed=0):
    return oracle_chain(cluster(n, seed), leaf)


def result_of(mp):
    return dict(counts=mp.counts(), trans=mp.trans(), recentred=mp.recentred(), reference=mp.reference())


def assert_same(got, want, what=""):
    assert tuple(got["counts"]) == tuple(want["counts"]), what
    assert np.asarray(got["trans"], F).tobytes() == np.asarray(want["trans"], F).tobytes(), what
    assert got["recentred"].tobytes() == want["recentred"].tobytes(), what
    assert got["reference"].tobytes() == want["reference"].tobytes(), what


def new_model():
    from pcl_tracking_amd import model

    return model.ModelPreparation()


# ---- 1. the stages against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_stages_against_the_oracle(n):
    mp = new_model()
    mp.prepare(cluster(n), leaf=0.01)
    want = oracle_of(n, 0.01)
    if n >= 65:
        assert want["counts"][1] == n - 3 - 4 - 6  # the NaNs, the cube's inside, 0.01f and -0.01f per axis
    assert_same(result_of(mp), want, "n=%d" % n)


@pytest.mark.parametrize("leaf", [0.0, 1e-6])
def test_reference_is_the_recentred_cloud(leaf):
    """leaf 0: no gridSample; leaf 1e-6: PCL refuses the leaf (the oracle returns None) and hands the cloud through"""
    if leaf > 0:
        orc = _orc()
        assert orc.voxel_grid(oracle_of(4097, 0.0)["recentred"], leaf) is None
    mp = new_model()
    mp.prepare(cluster(4097), leaf=leaf)
    want = oracle_of(4097, leaf)
    assert want["counts"][2] == want["counts"][1]
    assert_same(result_of(mp), want, "leaf=%g" % leaf)


# ---- 2. nothing left after stage 1 -------------------------------------------------------------------------------------
def test_empty_after_remove_zero_points():
    rng = np.random.default_rng(5)
    c = np.zeros(300, scene.POINT_DTYPE)
    for k in "xyz":
        c[k] = rng.uniform(-0.0099, 0.0099, 300).astype(F)
    c["x"][::7] = np.nan
    mp = new_model()
    with pytest.raises(PftError) as e:
        mp.prepare(c)
    assert e.value.status == 2 and "removeZeroPoints" in str(e.value)
    with pytest.raises(PftError):
        mp.counts()
    mp.prepare(cluster(1025))
    assert_same(result_of(mp), oracle_of(1025, 0.01), "after the refusal")


# ---- 3. three entrances, one result ------------------------------------------------------------------------------------
def test_three_entrances_one_result():
    from pcl_tracking_amd import segment

    cloud = scene.make_scene(50000)
    seg = segment.make_scene_segmenter()
    seg.configure(plane_rounds=(16, 0.3), max_iterations=100, distance_threshold=0.02, min_size=50)
    seg.setInputCloud(cloud)
    seg.apply()
    sizes = [int(s) for s in seg.clusterSizes()]
    assert len(sizes) >= 2 and min(sizes) >= 50
    host = seg.clusters()
    ptr, dev_sizes = seg.clustersDevice()
    assert ptr and [int(s) for s in dev_sizes] == sizes
    kept = []
    off = 0
    for j, n in enumerate(sizes):
        pts = host[j][1]
        assert len(pts) == n
        want = oracle_chain(pts, 0.01)
        a, b, c = new_model(), new_model(), new_model()
        a.prepareFromSegmenter(seg, j, leaf=0.01)
        b.prepare(pts.copy(), leaf=0.01)
        c.prepareDevice(ptr + 32 * off, n, leaf=0.01)
        for name, mp in (("segmenter", a), ("host", b), ("device", c)):
            assert_same(result_of(mp), want, "cluster %d through %s" % (j, name))
        kept.append((a, want))
        off += n
    # the models hold copies: another apply of the segmenter leaves them alone
    seg.setInputCloud(scene.make_scene(20000))
    seg.apply()
    for j, (mp, want) in enumerate(kept):
        assert_same(result_of(mp), want, "cluster %d after the segmenter's next apply" % j)


# ---- 4. handle reuse ---------------------------------------------------------------------------------------------------
def test_handle_reuse():
    mp = new_model()
    for n, seed in ((25000, 0), (3, 0), (25000, 1)):
        mp.prepare(cluster(n, seed))
        fresh = new_model()
        fresh.prepare(cluster(n, seed))
        assert_same(result_of(mp), result_of(fresh), "n=%d on a used handle" % n)
        assert_same(result_of(mp), oracle_of(n, 0.01, seed), "n=%d against the oracle" % n)


# ---- 5. a tracker cannot tell the difference ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames():
    return [scene.make_scene(20000, obj_pose=scene.advance_pose(scene.GT_POSE, f)) for f in range(3)]


@pytest.mark.parametrize("kld", [False, True])
def test_tracker_cannot_tell_the_difference(kld):
    from pcl_tracking_amd import tracker

    m = scene.make_model(512).copy()
    off = np.array(scene.model_gt_pose(M=512)[:3], F)
    for k, name in enumerate("xyz"):
        m[name] = m[name] + off[k]
    want = oracle_chain(m, 0.01)
    a = tracker.make_reference_tracker(particle_num=64, seed=7, kld=kld)
    a.setReferenceCloud(want["reference"])
    a.setTrans(want["trans"])
    a.setReportCloud(want["recentred"])
    mp = new_model()
    mp.prepare(m, leaf=0.01)
    b = tracker.make_reference_tracker(particle_num=64, seed=7, kld=kld)
    b.setObjectFromModel(mp, report_cloud=True)
    assert b._ref.tobytes() == want["reference"].tobytes() and b._report_cloud.tobytes() == want["recentred"].tobytes()
    for f, frame in enumerate(_frames()):
        out = []
        for t in (a, b):
            t.setInputCloud(frame)
            t.compute()
            t.computeReport()
            rep = t.getReport()
            out.append((t.getResult().tobytes(), t.getParticles().tobytes(),
                        b"".join(np.ascontiguousarray(getattr(rep, k)).tobytes() for k in rep.FIELDS) +
                        bytes([rep.info]) + rep.n_points.to_bytes(4, "little"), t.getTrackedCloud().tobytes()))
        for k, name in enumerate(("getResult", "getParticles", "getReport", "getTrackedCloud")):
            assert out[0][k] == out[1][k], "frame %d %s" % (f, name)
    # the cached clouds survive a re-creation of the handle
    b.close()
    b.setInputCloud(_frames()[0])
    b.compute()
    b.computeReport()
    assert b.getReport().n_points == want["counts"][1]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    from pcl_tracking_amd import segment, tracker

    mp = new_model()
    seg = segment.make_scene_segmenter()
    seg.configure(min_size=50)
    never = segment.make_scene_segmenter()
    never._ensure()
    with pytest.raises(PftError) as e:
        mp.prepareFromSegmenter(never, 0)
    assert e.value.status == 7 and "not been applied" in str(e.value)
    seg.setInputCloud(scene.make_scene(50000))
    seg.apply()
    nc = len(seg.clusterSizes())
    assert nc >= 1
    with pytest.raises(PftError) as e:
        mp.prepareFromSegmenter(seg, nc)
    assert e.value.status == 1 and "cluster" in str(e.value)
    mp.prepareFromSegmenter(seg, nc - 1)

    frame = scene.make_scene(20000)[:2000]
    t = tracker.make_reference_tracker(particle_num=64)
    with pytest.raises(PftError) as e:
        t.setObjectFromModel(new_model())
    assert e.value.status == 7
    sharded = tracker.make_reference_tracker(particle_num=64, rank=0, world_size=2)
    with pytest.raises(PftError) as e:
        sharded.setObjectFromModel(mp, report_cloud=True)
    assert e.value.status == 1 and "the object report is not supported on a sharded handle" in str(e.value)
    # nothing was applied: no cached clouds, and the handle still has no reference cloud
    assert sharded._ref is None and sharded._report_cloud is None
    assert np.array_equal(sharded._trans, np.eye(4, dtype=F))
    sharded.setInputCloud(frame)
    with pytest.raises(PftError) as e:
        sharded.compute()
    assert e.value.status == 3
    # without the report cloud the same handle takes the model
    sharded.setObjectFromModel(mp)
    assert sharded._ref.tobytes() == mp.reference().tobytes()
    with pytest.raises(PftError) as e:
        sharded.compute()
    assert e.value.status == 7 and "sharded" in str(e.value)

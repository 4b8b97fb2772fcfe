"""GPU checks of PCL's change detector (pft_set_change_detector; k_change_detect in pft_change.hip and the gate the
builders, the likelihood, the population and the resample launches read): the detector against the NumPy model
(tests/change_detector_model.py, which uses the unmodified oracle's box and key arithmetic), bit-identity with the
detector off whenever every test finds a change, the per-call schedule inside a tracker, the static fixed point, PCL's
defaults on the reference's 1 cm input, and the surroundings (pft_eval_weights, state save / restore, PFT_GRAPH=1, the
capacity error, the refused combinations)."""
import ctypes as C

import numpy as np
import pytest

from change_detector_model import ChangeDetectorModel, CounterModel
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu

_clouds = {}


def moving(f):
    if ("m", f) not in _clouds:
        _clouds[("m", f)] = scene.make_scene(50000, obj_pose=scene.advance_pose(scene.GT_POSE, f))
    return _clouds[("m", f)]


def static():
    return moving(0)


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


def make(gpu, P=400, kld=False, sum_order="tree", cd=None, iterations=2, seed=11):
    t = gpu.make_reference_tracker(particle_num=P, seed=seed, kld=kld, sum_order=sum_order, change_detector=cd)
    t.setIterationNum(iterations)
    t.setReferenceCloud(scene.make_model(2048))
    t.setTrans(scene.initial_trans())
    return t


def snapshot(t):
    return t.getResult().tobytes(), t.getParticles().tobytes(), t.getFitRatio()


def get_crop(t):
    n = C.c_size_t()
    t._check(t._L.pft_debug_get_crop(t._h, None, 0, C.byref(n)))
    crop = np.zeros(n.value, np.int32)
    if n.value:
        t._check(t._L.pft_debug_get_crop(t._h, crop.ctypes.data, n.value, C.byref(n)))
    return crop


def cloud(xyz):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return scene.make_points(xyz, np.full((len(xyz), 3), 100, np.uint8))


# ---- 1. the detector against the model -------------------------------------------------------------------------------
def _sequences():
    rng = np.random.default_rng(5)
    base = rng.uniform(-0.2, 0.2, (600, 3))
    seq = [base, base]  # first call, repeated cloud
    for a in range(3):  # shifted / grown in all six directions
        for s in (-1.0, 1.0):
            d = np.zeros(3)
            d[a] = s * 0.9
            seq.append(np.vstack([base, base[:200] + d]))
    seq.append(base + 0.013)
    faces = np.round(base / 0.02) * 0.02  # points on (or within rounding of) voxel faces of a 0.01 / 0.02 grid
    seq += [faces, np.zeros((0, 3)), faces]
    return [cloud(x) for x in seq]


@pytest.mark.parametrize("min_points", [0, 1, 10])
@pytest.mark.parametrize("res", [0.01, 0.05])
def test_detector_matches_the_model(gpu, orc, min_points, res):
    t = make(gpu)
    t.setInputCloud(static())
    m = ChangeDetectorModel(orc, res)
    for k, c in enumerate(_sequences()):
        got = t.debugChangeDetect(c, min_points, res, reset=(k == 0))
        idx, nv, box, depth = m.test(c, min_points)
        assert got.tolist() == idx.tolist(), k
        st = t.debugChangeState(1)
        assert st["ring"][-1][2] == nv and st["ring"][-1][1] == (nv > 0), k
        if len(np.concatenate(m.clouds)):
            assert st["box"].tobytes() == box.tobytes(), k
            assert st["depth"] == depth, k


def test_detector_matches_the_model_on_a_large_cloud(gpu, orc):
    """about 105 000 points: the size of configs[2]'s crop"""
    t = make(gpu)
    t.setInputCloud(static())
    rng = np.random.default_rng(9)
    a = rng.uniform(-0.5, 0.5, (105000, 3))
    b = np.vstack([a[:100000], rng.uniform(0.4, 0.7, (5000, 3))])
    m = ChangeDetectorModel(orc, 0.01)
    for k, x in enumerate((a, b)):
        c = cloud(x)
        got = t.debugChangeDetect(c, 1, 0.01, reset=(k == 0))
        idx, nv, box, depth = m.test(c, 1)
        assert got.tolist() == idx.tolist()
        st = t.debugChangeState(1)
        assert st["box"].tobytes() == box.tobytes() and st["depth"] == depth


def test_depth_overflow_raises_capacity_on_every_later_test(gpu):
    """the box is never reset: once it is deeper than 21 levels every later test of that detector raises bit 5 (and
    evaluates); only a new detector is clean again"""
    t = make(gpu)
    t.setInputCloud(static())
    for k in range(3):
        with pytest.raises(gpu.PftError) as e:
            t.debugChangeDetect(cloud([[0, 0, 0], [30000.0, 0, 0]] if k == 0 else [[0, 0, 0]]), 1, 0.01, reset=(k == 0))
        assert e.value.status == 6 and "bit5" in str(e.value)
        assert t.debugChangeState(1)["depth"] > 21
    t.debugChangeDetect(cloud([[0, 0, 0]]), 1, 0.01, reset=True)  # a fresh detector


def test_points_on_voxel_faces_match_the_model(gpu, orc):
    """points exactly on the detector's voxel faces: min + j * res of the box the first test defined, in double, rounded
    to float (the box is centred on the first point ever inserted, so the faces are not at multiples of res)"""
    res = 0.02
    t = make(gpu)
    t.setInputCloud(static())
    m = ChangeDetectorModel(orc, res)
    rng = np.random.default_rng(3)
    first = cloud(rng.uniform(-0.2, 0.2, (400, 3)))
    assert t.debugChangeDetect(first, 1, res, reset=True).tolist() == m.test(first, 1)[0].tolist()
    box = t.debugChangeState(1)["box"]
    j = rng.integers(0, 20, (500, 3))
    faces = (box[:3][None, :] + j * res).astype(np.float32)
    faces[::3, 1] = (box[1] + (j[::3, 1] + 0.5) * res).astype(np.float32)  # some on faces of one axis only
    for k, x in enumerate((faces, faces, faces[::-1], faces + np.float32(res))):
        c = cloud(x)
        got = t.debugChangeDetect(c, 1, res, reset=False)
        idx, nv, box_m, depth = m.test(c, 1)
        assert got.tolist() == idx.tolist(), k
        st = t.debugChangeState(1)
        assert st["box"].tobytes() == box_m.tobytes() and st["depth"] == depth, k


# ---- 2. equivalence with the detector off ----------------------------------------------------------------------------
@pytest.mark.parametrize("P,kld", [(400, False), (400, True), (8192, False)])
@pytest.mark.parametrize("sum_order", ["tree", "pcl"])
def test_first_test_only_is_bit_identical_to_off(gpu, P, kld, sum_order):
    off = make(gpu, P, kld, sum_order)
    on = make(gpu, P, kld, sum_order, cd=(1000, 1, 0.01))
    for f in range(16):
        for t in (off, on):
            t.setInputCloud(moving(f))
            t.compute()
        assert snapshot(on) == snapshot(off), f
    ring = on.debugChangeState()["ring"]
    assert ring[0][0] == 1 and ring[0][1] == 1 and not ring[1:, 0].any()


@pytest.mark.parametrize("kld", [False, True])
def test_moving_scene_small_interval_is_bit_identical_to_off(gpu, kld):
    off = make(gpu, 400, kld)
    on = make(gpu, 400, kld, cd=(1, 1, 0.01))
    for f in range(12):
        for t in (off, on):
            t.setInputCloud(moving(f))
            t.compute()
        st = on.debugChangeState()
        tested = st["ring"][st["ring"][:, 0] == 1]
        assert tested[:, 1].all(), "precondition: every test on the moving scene finds a change"
        assert snapshot(on) == snapshot(off), f


# ---- 3. the per-call schedule inside a tracker -----------------------------------------------------------------------
@pytest.mark.parametrize("kld", [False, True])
def test_schedule_matches_the_model(gpu, orc, kld):
    res, minp = 0.05, 5
    t = make(gpu, 400, kld, cd=(0, minp, res), iterations=1)
    m, cm = ChangeDetectorModel(orc, res), CounterModel()
    frames = [static()] * 5 + [moving(f) for f in range(1, 6)]
    for k, c in enumerate(frames):
        t.setInputCloud(c)
        t.compute()
        crop = c[get_crop(t)]
        want = cm.step(True, 0, lambda: m.test(crop, minp)[1] > 0)
        st = t.debugChangeState()
        r = st["ring"][-1]
        assert (bool(r[0]), bool(r[1]), int(r[4])) == want, k
        assert st["counter"] == want[2] and st["gate"] == int(want[1])


# ---- 4. the static fixed point ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sum_order", ["tree", "pcl"])
@pytest.mark.parametrize("kld", [False, True])
def test_static_scene_fixed_point(gpu, orc, sum_order, kld):
    t = make(gpu, 400, kld, sum_order, cd=(0, 10, 0.05))
    # the crop follows the particles, so the first tests on an unchanged input still see new voxels at its edge; once a
    # test finds none, nothing moves any more
    for f in range(40):
        t.setInputCloud(static())
        t.compute()
        if t.debugChangeState()["ring"][-1][1] == 0:
            break
    else:
        pytest.fail("no test found the unchanged input unchanged")
    norm = orc.normalize_weights if sum_order == "pcl" else orc.normalize_weights_tree
    keys = ("x", "y", "z", "roll", "pitch", "yaw")
    prev, res0 = t.getParticles(), t.getResult().tobytes()
    for f in range(4):
        t.setInputCloud(static())
        t.compute()
        st = t.debugChangeState()
        assert st["ring"][-2:, 0].all() and not st["ring"][-2:, 1].any(), "unchanged input: both iterations skip"
        cur = t.getParticles()
        assert len(cur) == len(prev) and all(cur[k].tobytes() == prev[k].tobytes() for k in keys)
        assert t.getResult().tobytes() == res0
        w = prev["weight"].copy()
        for _ in range(2):  # each iteration renormalises the weights it holds
            w, fit = norm(w)
        assert cur["weight"].tobytes() == np.asarray(w, np.float32).tobytes()
        assert t.getFitRatio() == fit
        prev = cur


# ---- 5. PCL's defaults on the reference's 1 cm input ------------------------------------------------------------------
@pytest.mark.parametrize("kld", [False, True])
def test_pcl_defaults_on_1cm_input_never_evaluate(gpu, kld):
    t = make(gpu, 400, kld, cd=(10, 10, 0.01))
    init = scene.initial_trans()
    want = np.zeros(1, scene.PARTICLE_DTYPE)
    t._L.pft_to_state(init.astype(np.float32).ctypes.data, want.ctypes.data)
    for f in range(6):
        t.setInputCloud(moving(f))
        t.compute()
        st = t.debugChangeState()
        assert st["ring"][:, 0].all() and not st["ring"][:, 1].any()
        r = t.getResult()
        for k in ("x", "y", "z", "roll", "pitch", "yaw"):
            assert r[k] == want[0][k]


# ---- 6. surroundings ----------------------------------------------------------------------------------------------------
def skipped_in_frame(t, seen):
    """tested-and-unchanged decisions of the frame just run (seen: decisions counted before it)"""
    st = t.debugChangeState()
    k = st["n_calls"] - seen
    rows = st["ring"][len(st["ring"]) - k:]
    return int(((rows[:, 0] == 1) & (rows[:, 1] == 0)).sum()), st["n_calls"]


STATIC_THEN_MOVING = [("s", 0)] * 40 + [("m", f) for f in range(1, 6)]


def frame(key):
    return static() if key[0] == "s" else moving(key[1])


def test_eval_weights_between_frames_leaves_the_run_alone(gpu):
    a = make(gpu, 400, cd=(0, 10, 0.05))
    b = make(gpu, 400, cd=(0, 10, 0.05))
    seen, skipped = 0, 0
    for f, key in enumerate(STATIC_THEN_MOVING):
        for t in (a, b):
            t.setInputCloud(frame(key))
            t.compute()
        b.evalWeights(b.getParticles()[:400])
        assert snapshot(a) == snapshot(b), f
        n, seen = skipped_in_frame(b, seen)
        skipped += n
    assert skipped > 0, "the compared frames include skipped iterations"


def test_state_save_restore_replays_a_detector_frame(gpu):
    t = make(gpu, 400, cd=(0, 10, 0.05))
    seen = 0
    for f in range(40):  # until a test finds the unchanged input unchanged
        t.setInputCloud(static())
        t.compute()
        n, seen = skipped_in_frame(t, seen)
        if n:
            break
    assert n, "no skipped iteration to replay"
    t.debugStateSave()
    runs = []
    for rep in range(2):
        if rep:
            t.debugStateRestore()
        out = []
        for c in (static(), static(), moving(1)):  # skipped frames, then a change
            t.setInputCloud(c)
            t.compute()
            st = t.debugChangeState()
            out.append((snapshot(t), st["ring"][-2:].tolist(), st["gate"], st["counter"], st["box"].tobytes()))
        runs.append(out)
    assert runs[0] == runs[1]
    assert not any(r[1][0][1] or r[1][1][1] for r in runs[0][:2]), "the replayed static frames skip"


def test_state_restore_refuses_a_detector_enabled_after_the_save(gpu):
    t = make(gpu, 400)
    t.setInputCloud(static())
    t.compute()
    t.debugStateSave()
    t.setUseChangeDetector(True)
    with pytest.raises(gpu.PftError) as e:
        t.debugStateRestore()
    assert e.value.status == 7


def test_graph_mode_matches_direct_launches(gpu, monkeypatch):
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PFT_GRAPH", mode)
        t = make(gpu, 400, cd=(0, 10, 0.05))
        seq, seen, skipped_graphed = [], 0, 0
        for f, key in enumerate(STATIC_THEN_MOVING):
            t.setInputCloud(frame(key))
            t.compute()
            seq.append(snapshot(t))
            n, seen = skipped_in_frame(t, seen)
            if f >= 3:  # frames from the third on are replayed as a graph in mode 1
                skipped_graphed += n
        out[mode] = (seq, t.debugChangeState()["ring"].tolist())
        assert skipped_graphed > 0, "graphed frames include skipped iterations"
        t.close()
    assert out["0"] == out["1"]


def test_refused_combinations(gpu):
    t = gpu.make_reference_tracker(particle_num=400)
    t.setCloudCoherence(_exact_coherence(gpu))
    t.setReferenceCloud(scene.make_model(256))
    t.setInputCloud(static())
    with pytest.raises(gpu.PftError) as e:
        t.setUseChangeDetector(True)
    assert e.value.status == 1 and "exact" in str(e.value)
    assert not t.getUseChangeDetector()
    s = gpu.ParticleFilterTracker(world_size=2)
    s.setParticleNum(400)
    s.setReferenceCloud(scene.make_model(256))
    s.setInputCloud(static())
    with pytest.raises(gpu.PftError) as e:
        s.setUseChangeDetector(True)
    assert e.value.status == 1 and "sharded" in str(e.value)


def _exact_coherence(gpu):
    c = gpu.NearestPairPointCloudCoherence()
    c.addPointCoherence(gpu.DistanceCoherence())
    h = gpu.HSVColorCoherence()
    h.setWeight(0.1)
    c.addPointCoherence(h)
    c.setSearchMethod(gpu.OctreeSearch(0.01))
    c.setMaximumDistance(0.1)
    return c

"""GPU checks of PCL's summation order (pft_config::sum_order = PFT_SUM_PCL, k_population_seq in pft_population.hip):
normalizeWeight adds the weights one after the other in index order in double, update() adds (float)(x * (double)w)
one after the other in float.  The oracle's default sum mode restates that order (orc_normalize_weights /
orc_weighted_mean), so in this mode the device must equal it bit for bit where the arithmetic is the same, and whole
tracking runs with the same trig on both sides stay bit-identical where the tree order parts after a few frames
(DESIGN.md sections 3.3 and 4)."""
import numpy as np
import pytest

from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "roll", "pitch", "yaw")
FRAMES = 32
# first frame over 1e-4 of the TREE order against the full-PCL oracle (trig 0, sum 0), seeds 11 / 21 / 22
# (profiles/r03_longrun_attribution.txt)
TREE_FIRST_OVER = {(400, False): (14, 17, 10), (8192, False): (6, 4, 2), (400, True): (2, 9, 2)}


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def particles_around(pose, n, seed, sig_t=0.015, sig_r=0.09):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    for k, name in enumerate(("x", "y", "z")):
        p[name] = pose[k] + rng.normal(0, sig_t, n)
    for k, name in enumerate(("roll", "pitch", "yaw")):
        p[name] = pose[3 + k] + rng.normal(0, sig_r, n)
    p["w"] = 1.0
    w = rng.random(n).astype(np.float32)
    p["weight"] = w / w.sum()
    return p


# ---- the stages on explicit inputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 400, 500, 8192, 16385, 65536])
def test_weighted_mean_is_pcls_bit_for_bit(gpu, orc, n):
    g = gpu.make_reference_tracker(particle_num=64, sum_order="pcl")
    p = particles_around(scene.model_gt_pose(), n, n + 7)
    want = orc.weighted_mean(p)
    assert g.debugWeightedMean(p).tobytes() == want.tobytes()
    if n >= 400:  # the input tells the two orders apart
        assert want.tobytes() != orc.weighted_mean_tree(p).tobytes()


@pytest.mark.parametrize("n", [1, 2, 400, 8192, 65536])
def test_normalize_follows_pcls_sum(gpu, orc, n):
    """The weight sum is a double sum of floats, so the two orders' sums differ by ~sqrt(n) ulp(double) and their
    casts to float part only ~2^-21 of the time: no practical seed search finds an input on which the float divisor
    differs, and this test checks the mode's normalisation against PCL's on ordinary inputs; the long runs below are
    the ones that tell the orders apart."""
    g = gpu.make_reference_tracker(particle_num=64, sum_order="pcl")
    rng = np.random.default_rng(n + 3)
    raw = (-rng.random(n) * 2000).astype(np.float32)
    raw[rng.random(n) < 0.05] = 0.0
    want, fw = orc.normalize_weights(raw)
    got, fg = g.debugNormalize(raw)
    assert fw == fg
    assert ulp_diff(got, want).max() <= 1  # exp() in double: glibc vs ocml may differ in the last bit
    assert (got == want).mean() > 0.999
    for special in (np.zeros(n, np.float32), np.full(n, -3.0, np.float32)):
        np.testing.assert_array_equal(g.debugNormalize(special)[0], orc.normalize_weights(special)[0])


@pytest.mark.parametrize("n", [1, 2, 3, 400, 1000, 8192, 16385, 65536])
def test_alias_table_in_pcl_mode(gpu, orc, n):
    g = gpu.make_reference_tracker(particle_num=64, sum_order="pcl")
    rng = np.random.default_rng(n + 1)
    cases = []
    w = rng.random(n).astype(np.float32) ** 6
    w[rng.random(n) < 0.15] = 0
    cases.append(w / max(w.sum(), 1e-30))
    cases.append(np.full(n, np.float32(1) / np.float32(n), np.float32))
    w = np.zeros(n, np.float32)
    w[n // 2] = 1.0
    cases.append(w)
    w = np.full(n, np.float32(1) / np.float32(n), np.float32)
    w[: n // 2] *= np.float32(0.5)
    cases.append(w)
    for w in cases:
        a_w, q_w = orc.gen_alias_table(w)
        a_g, q_g = g.debugAlias(w)
        np.testing.assert_array_equal(a_g, a_w)
        np.testing.assert_allclose(q_g, q_w, atol=1e-9 * max(1, n), rtol=0)


# ---- long runs (the frame schedule of test_gpu_longrun.py) ----------------------------------------------------------
_clouds = {}


def frame_cloud(f):
    if f not in _clouds:
        pose = scene.advance_pose(scene.GT_POSE, f)
        if f % 8 == 5:
            _clouds[f] = scene.make_scene(50000, obj_pose=pose)
        elif (f // 3) % 2 == 1:
            _clouds[f] = scene.make_scene(320 * 240, obj_pose=pose, mode="organized")
        else:
            _clouds[f] = scene.make_scene(160 * 120, obj_pose=pose, mode="organized")
    return _clouds[f]


def make_pair(gpu, orc, P, seed, kld, trig_mode):
    model = scene.make_model(2048)
    g = gpu.make_reference_tracker(particle_num=P, seed=seed, kld=kld, sum_order="pcl")
    o = orc.Tracker(orc.default_config(particle_num=P, seed=seed, threads=0, emulate_pcl_alloc=0,
                                       kld_adaptive=1 if kld else 0))
    o.set_trig_mode(trig_mode)
    o.set_sum_mode(0)  # PCL's sequential sums
    for ref, tr in ((g.setReferenceCloud, g.setTrans), (o.set_reference, o.set_trans)):
        ref(model)
        tr(scene.initial_trans())
    return g, o


@pytest.mark.parametrize("P,kld", [(400, False), (8192, False), (400, True)])
def test_long_run_same_trig_pcl_sums_is_bit_identical(gpu, orc, P, kld):
    g, o = make_pair(gpu, orc, P, seed=11, kld=kld, trig_mode=1)
    for f in range(FRAMES):
        cloud = frame_cloud(f)
        g.setInputCloud(cloud)
        o.set_input(cloud)
        g.compute()
        assert o.compute() == 0
        rg, ro = g.getResult(), o.get_result()
        hs = g.debugHostStat()
        assert hs[2] == 0 and hs[3] == 0, (f, hs)
        assert rg.tobytes() == ro.tobytes(), (f, rg, ro)
        pg, po = g.getParticles(), o.get_particles()
        assert len(pg) == len(po), (f, len(pg), len(po))
        np.testing.assert_array_equal(pg.view(np.uint32), po.view(np.uint32), err_msg="frame %d" % f)


@pytest.mark.parametrize("P,kld", [(400, False), (8192, False), (400, True)])
def test_long_run_own_trig_pcl_sums(gpu, orc, P, kld, record_property):
    """the north_star bar: the device's own trig against the full-PCL oracle; only cosf / sinf still differ, and every
    seed's first frame over 1e-4 comes strictly later than with the tree order (measured: 400 fixed 23 / none / none,
    8 192 fixed 16 / 17 / 30, KLD 23 / 30 / 20)"""
    firsts = []
    for seed in (11, 21, 22):
        g, o = make_pair(gpu, orc, P, seed=seed, kld=kld, trig_mode=0)
        first_bad = None
        for f in range(FRAMES):
            cloud = frame_cloud(f)
            g.setInputCloud(cloud)
            o.set_input(cloud)
            g.compute()
            assert o.compute() == 0
            rg, ro = g.getResult(), o.get_result()
            assert all(np.isfinite(float(rg[k])) for k in KEYS)
            if max(abs(float(rg[k]) - float(ro[k])) for k in KEYS) >= 1e-4:
                first_bad = f
                break
        firsts.append(first_bad)
    record_property("first_frame_over_1e-4_seeds_11_21_22", firsts)
    print("own-trig run, PCL sums, P=%d kld=%s: first frame over 1e-4 per seed (11, 21, 22): %s" % (P, kld, firsts))
    for f, tree in zip(firsts, TREE_FIRST_OVER[(P, kld)]):
        assert f is None or f > tree, (firsts, TREE_FIRST_OVER[(P, kld)])


# ---- sharding, graphs, the option itself ----------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_pcl_sums_equal_one_handle(gpu, world):
    import torch

    from pcl_tracking_amd.dist import HipPhases

    P, frames, seed = 8192, 3, 3
    model, cloud = scene.make_model(1024), scene.make_scene(50000)[:20000]
    dev = torch.device("cuda", 0)
    single = gpu.make_reference_tracker(particle_num=P, seed=seed, sum_order="pcl")
    single.setReferenceCloud(model)
    single.setTrans(scene.initial_trans())
    phs = [HipPhases(P, r, world, dev, seed=seed, sum_order="pcl") for r in range(world)]
    for ph in phs:
        ph.set_reference(model)
        ph.set_trans(scene.initial_trans())
    for f in range(frames):
        single.setInputCloud(cloud)
        single.compute()
        want = single.getResult().tobytes()
        for ph in phs:
            ph.set_input(cloud)
            ph.begin_frame()
        for it in range(2):
            for ph in phs:
                ph.phase_a(it)
            bb = torch.stack([ph.bbox6 for ph in phs]).max(0).values  # all-reduce(MAX)
            for ph in phs:
                ph.bbox6.copy_(bb)
                ph.phase_b()
            g = torch.cat([ph.shard for ph in phs])  # all-gather, rank order
            for ph in phs:
                ph.gathered.copy_(g)
                ph.phase_c()
        for r, ph in enumerate(phs):
            assert ph.get_result().tobytes() == want, (f, r)
    want_p = single.getParticles().view(np.uint32)
    for r, ph in enumerate(phs):
        np.testing.assert_array_equal(ph.get_particles().view(np.uint32), want_p, err_msg="rank %d" % r)


def _run(tr, frames=6):
    tr.setReferenceCloud(scene.make_model(1024))
    tr.setTrans(scene.initial_trans())
    out = []
    for f in range(frames):
        tr.setInputCloud(frame_cloud(f))
        tr.compute()
        out.append(tr.getResult().tobytes() + tr.getParticles().tobytes())
    return out


@pytest.mark.parametrize("kld", [False, True])
def test_graph_launches_give_the_same_bits(gpu, monkeypatch, kld):
    direct = _run(gpu.make_reference_tracker(particle_num=400, seed=5, kld=kld, sum_order="pcl"))
    monkeypatch.setenv("PFT_GRAPH", "1")
    graphed = _run(gpu.make_reference_tracker(particle_num=400, seed=5, kld=kld, sum_order="pcl"))
    assert graphed == direct


def test_explicit_tree_order_is_the_default(gpu):
    assert _run(gpu.make_reference_tracker(particle_num=400, seed=6, sum_order=0), 3) == \
        _run(gpu.make_reference_tracker(particle_num=400, seed=6), 3)


def test_unknown_sum_order_is_rejected(gpu):
    from pcl_tracking_amd._lib import PftError

    t = gpu.make_reference_tracker(particle_num=400, sum_order=2)
    t.setReferenceCloud(scene.make_model(256))
    with pytest.raises(PftError) as e:
        t.setInputCloud(frame_cloud(0))  # the handle is created here
    assert e.value.status == 1

"""The sampling stage at parameters in which no two axes agree (run with -m gpu): k_init_particles, k_resample<TABLE>,
k_resample4<BOX, GATED>, k_resample_kld<TABLE, GATED> with particle_sample / normal_pair (pft_device_utils.h).

Every other test of these kernels runs the reference application's parameter set: step sigma equal within x/y/z and within
roll/pitch/yaw, one initial covariance with mean zero, one bin size, delta / epsilon / motion_ratio at their defaults.  A
sigma, mean or bin size read from the wrong axis, or a delta that never reaches the kernel, computes the same there.  The
cases, parameter sets and populations are in tests/sampling_cases.py; tests/test_sampling_cases_host.py proves on the CPU
that each case reaches the regime it is named after.

Without an oracle (relations between the device's own outputs, exact):
  * scaling  -- cov[k] * 4**(k + 1) scales sigma[k] by exactly 2**(k + 1): with all poses zero and mean zero, component k of
    every drawn particle is 2**(k + 1) times the base run's, bit for bit (same seed, epoch, ids), in every kernel
  * mean     -- with zero covariance every init particle is rep + float(mean[k]) per axis
  * bins     -- bins[:, i] == trunc(float(x_i) / float(bin_i)) from the device's own particles
  * stop     -- the sequential loop replayed over the device's own bins stops at the returned n and nowhere earlier, and
    counts the returned k
  * matrices -- the matrices the KLD launch writes are debugPoseToMatrix of its particles
Against the oracle: n, k and bins equal, poses within 1e-6, at most max(1, floor(0.001 * 6 n)) floats differ and those by
one ulp (the bar of test_gpu_kld.py::test_kld_resample_bit_exact restated per float: Box-Muller's log / sin / cos in double
are ocml on one side and glibc on the other); init and fixed resample with the bars of test_gpu_parity.py; short whole-tracker
runs bit-identical in the same-trig, same-sum mode of test_gpu_longrun.py.
PARITY UNPINNED: the oracle restates PCL 1.8.0, which is not available here (oracle/pft_oracle.h)."""
import numpy as np
import pytest

import sampling_cases as S
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu
KEYS = S.KEYS
IDS = lambda c: c.name  # noqa: E731
TABLE = (True, False)
TABLE_IDS = ("table", "prefix")


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


def fixed_tracker(gpu, n, step_cov=None, init_cov=None, init_mean=None, reference=False):
    g = gpu.make_reference_tracker(particle_num=n, seed=S.SEED)
    if step_cov is not None:
        g.setStepNoiseCovariance(step_cov)
    if init_cov is not None:
        g.setInitialNoiseCovariance(init_cov)
    if init_mean is not None:
        g.setInitialNoiseMean(init_mean)
    if reference:  # (the fused box instance needs the support subset of a reference cloud)
        g.setReferenceCloud(scene.make_model(2048))
    return g


def kld_tracker(gpu, c):
    g = gpu.make_reference_tracker(particle_num=c.n_old, seed=S.SEED, kld=True)
    g.setMaximumParticleNum(c.maxn)
    g.setDelta(c.delta)
    g.setEpsilon(c.epsilon)
    g.setBinSize(c.bins)
    g.setMotionRatio(c.motion_ratio)
    g.setStepNoiseCovariance(c.step_cov)
    assert g.getMotionRatio() == c.motion_ratio
    return g


def assert_scaled(base, big, tag, first=0):
    xb, xg = S.poses(base), S.poses(big)
    assert xb.shape == xg.shape, tag
    for k in range(6):
        want = (xb[:, k] * np.float32(S.SCALE[k])).view(np.uint32)
        bad = np.flatnonzero(xg[:, k].view(np.uint32) != want)
        assert bad.size == 0, (tag, KEYS[k], bad[:4], xb[bad[:4], k], xg[bad[:4], k])
    # the noise is there: no component is zero, and no two agree (z0 != z1 throughout)
    assert (xb[first:] != 0).all() and len(np.unique(xb[first:])) == xb[first:].size, tag


# ---- oracle-free: scaling and mean ---------------------------------------------------------------------------------
def test_init_noise_scales_per_axis(gpu):
    rep = S.particle()
    out = [fixed_tracker(gpu, S.N_INIT, init_cov=cov).debugInitParticles(rep, 0, S.N_INIT) for cov in (S.COV, S.COV_SCALED)]
    assert_scaled(out[0], out[1], "init")


def test_init_mean_lands_on_its_own_axis(gpu):
    rep = S.particle(S.REP)
    g = fixed_tracker(gpu, S.N_INIT, init_cov=(0.0,) * 6, init_mean=S.MEAN)
    x = S.poses(g.debugInitParticles(rep, 0, S.N_INIT))
    want = np.asarray(S.MEAN, np.float64).astype(np.float32) + S.poses(rep)[0]  # float add, as StateT operator+
    assert want.dtype == np.float32
    for k in range(6):
        assert (x[:, k].view(np.uint32) == want[k:k + 1].view(np.uint32)).all(), (KEYS[k], x[:2, k], want[k])


def test_table_resample_noise_scales_per_axis(gpu):
    old = S.zero_pose_population(S.N_RESAMPLE, 1)
    rep = S.particle(weight=0.25)
    g = [fixed_tracker(gpu, S.N_RESAMPLE, step_cov=cov) for cov in (S.COV, S.COV_SCALED)]
    a, q = g[0].debugAlias(old["weight"])
    for epoch in S.EPOCHS:
        out = [t.debugResample(old, a, q, rep, epoch) for t in g]
        assert out[0][0].tobytes() == rep[0].tobytes() and out[1][0].tobytes() == rep[0].tobytes()
        assert_scaled(out[0], out[1], ("table", epoch), first=1)


@pytest.mark.parametrize("instance", [0, 1, 2])
def test_product_resample_noise_scales_per_axis(gpu, instance):
    """k_resample<false>, k_resample4<false, *> and k_resample4<true, *>: in the four-lane kernels lane r of a quad holds
    sigma[2r - 2] and sigma[2r - 1]"""
    old = S.zero_pose_population(S.N_RESAMPLE, 1)
    rep = S.particle(weight=0.25)
    g = [fixed_tracker(gpu, S.N_RESAMPLE, step_cov=cov, reference=instance == 2) for cov in (S.COV, S.COV_SCALED)]
    for epoch in S.EPOCHS:
        out = [t.debugResamplePrefix(old, rep, epoch, instance=instance) for t in g]
        assert out[0][0].tobytes() == rep[0].tobytes() and out[1][0].tobytes() == rep[0].tobytes()
        assert_scaled(out[0], out[1], ("prefix", instance, epoch), first=1)


@pytest.mark.parametrize("table", TABLE, ids=TABLE_IDS)
def test_kld_resample_noise_scales_per_axis(gpu, table):
    """no motion and one bin for everything: both runs keep all maxn candidates"""
    old = S.zero_pose_population(S.N_KLD_OLD, 2)
    c = S._case("scaling", "zero", S.MAXN_KLD_SCALING, n_old=S.N_KLD_OLD, bins=(S.BIN_ALL_IN_ONE,) * 6)
    g = [kld_tracker(gpu, c._replace(step_cov=cov)) for cov in (S.COV, S.COV_SCALED)]
    a, q = g[0].debugAlias(old["weight"]) if table else (None, None)
    for epoch in S.EPOCHS:
        out = []
        for t in g:
            p, bins, k = t.debugKldResample(old, a, q, S.particle(), epoch)
            assert len(p) == c.maxn and k == 1 and (bins == 0).all()
            out.append(p)
        assert_scaled(out[0], out[1], ("kld", table, epoch))


# ---- KLD: every case, with a table and without ---------------------------------------------------------------------
_device_runs = {}


def device_runs(gpu, c, table):
    """one launch per epoch, shared by the tests of a case: [(particles, bins, k, matrices, a, q), ..].  The explicit table
    is the one debugAlias materialises from the prefix form, so both instances draw from the same entries"""
    key = (c.name, table)
    if key not in _device_runs:
        g = kld_tracker(gpu, c)
        old = S.case_population(c)
        a, q = g.debugAlias(old["weight"])
        runs = []
        for epoch in S.EPOCHS:
            ta, tq = (a, q) if table else (None, None)
            runs.append(g.debugKldResample(old, ta, tq, S.case_motion(c), epoch, want_mats=True) + (a, q))
        g.close()
        _device_runs[key] = runs
    return _device_runs[key]


@pytest.mark.parametrize("table", TABLE, ids=TABLE_IDS)
@pytest.mark.parametrize("c", S.KLD_CASES + S.MATS_CASES, ids=IDS)
def test_kld_bins_and_stop_rule_follow_from_the_kernels_own_output(gpu, orc, c, table):
    bound = lambda k: orc.kld_bound(k, c.delta, c.epsilon)  # noqa: E731  (the host formula: checked against the library's below)
    for epoch, (p, bins, k, mats, a, q) in zip(S.EPOCHS, device_runs(gpu, c, table)):
        tag = (c.name, table, epoch)
        n = len(p)
        assert 1 <= n <= c.maxn and bins.shape == (n, 6), tag
        want = S.bins_of(p, c.bins)
        bad = np.argwhere(bins != want)
        assert bad.size == 0, (tag, bad[:4], bins[bad[:4, 0]], want[bad[:4, 0]])
        assert S.replay_stop_rule(bins, c.maxn, bound) == (n, k), (tag, n, k, S.replay_stop_rule(bins, c.maxn, bound))
        if n > 1:
            assert S.replay_stop_rule(bins[:-1], c.maxn, bound) is None, tag
        np.testing.assert_array_equal(p["w"], np.float32(1.0))


@pytest.mark.parametrize("table", TABLE, ids=TABLE_IDS)
@pytest.mark.parametrize("c", S.KLD_CASES + S.MATS_CASES, ids=IDS)
def test_kld_resample_matches_the_oracle(gpu, orc, c, table):
    """a failure here with the test above passing for the case, on n, k or bins: look for a candidate whose x / bin lies
    within 1 ulp of an integer (a 1-ulp pose difference carried across a bin edge) before anything else"""
    old = S.case_population(c)
    cfg = S.oracle_config(orc, c)
    for epoch, (got, gbins, gk, mats, a, q) in zip(S.EPOCHS, device_runs(gpu, c, table)):
        tag = (c.name, table, epoch)
        want, wbins, wk = orc.kld_resample(cfg, old, a, q, S.case_motion(c), epoch)
        print("%s: n %d (oracle %d), k %d (oracle %d)" % (tag, len(got), len(want), gk, wk))
        assert len(got) == len(want) and gk == wk, (tag, len(got), len(want), gk, wk)
        np.testing.assert_array_equal(gbins, wbins)
        xg, xw = S.poses(got), S.poses(want)
        assert np.abs(xg.astype(np.float64) - xw.astype(np.float64)).max() <= 1e-6, tag
        d = S.ulp_diff(xg, xw)
        n_off = int((xg.view(np.uint32) != xw.view(np.uint32)).sum())
        print("%s: floats that differ %d of %d, worst %d ulp" % (tag, n_off, xg.size, int(d.max())))
        assert d.max() <= 1, tag
        assert n_off <= max(1, int(np.floor(0.001 * 6 * len(got)))), (tag, n_off)
        np.testing.assert_array_equal(got["weight"].view(np.uint32), want["weight"].view(np.uint32))
        np.testing.assert_array_equal(got["w"].view(np.uint32), want["w"].view(np.uint32))


@pytest.mark.parametrize("table", TABLE, ids=TABLE_IDS)
@pytest.mark.parametrize("c", S.MATS_CASES, ids=IDS)
def test_kld_launch_writes_the_matrices_of_its_particles(gpu, c, table):
    """the pose -> matrix step k_resample_kld fuses (as under compute()), on both sides of the LDS / HBM switch"""
    g = kld_tracker(gpu, c)
    for epoch, (p, bins, k, mats, a, q) in zip(S.EPOCHS, device_runs(gpu, c, table)):
        assert mats.shape == (len(p), 3, 4)
        assert mats.tobytes() == g.debugPoseToMatrix(p).tobytes(), (c.name, table, epoch)
        assert np.abs(mats[:, :, :3]).max() <= 1.0 and (mats[:, :, 3] == S.poses(p)[:, :3]).all()
        # the hook without the matrices returns the same particles
        ta, tq = (a, q) if table else (None, None)
        p2, bins2, k2 = g.debugKldResample(S.case_population(c), ta, tq, S.case_motion(c), epoch)
        assert p2.tobytes() == p.tobytes() and bins2.tobytes() == bins.tobytes() and k2 == k


def test_host_quantile_and_bound_match_the_oracle(gpu, orc):
    L = gpu._lib.load()
    deltas = sorted(set(S.DELTAS) | {c.delta for c in S.KLD_CASES} | {WHOLE_KLD["delta"]})
    epsilons = sorted(set(S.EPSILONS) | {c.epsilon for c in S.KLD_CASES} | {WHOLE_KLD["epsilon"]})
    for d in deltas:
        assert L.pft_kld_normal_quantile(d) == orc.kld_normal_quantile(d), d
        for e in epsilons:
            for k in (2, 3, 10, 77, 400, 4097, 16384):
                assert L.pft_kld_bound(k, d, e) == orc.kld_bound(k, d, e), (k, d, e)
    assert len({L.pft_kld_normal_quantile(d) for d in deltas}) == len(deltas)


# ---- init and fixed resample at per-axis parameters, against the oracle ---------------------------------------------
def test_init_particles_per_axis_parameters(gpu, orc):
    """the asserts of test_gpu_parity.py::test_init_particles"""
    g = fixed_tracker(gpu, S.N_INIT, init_cov=S.COV, init_mean=S.MEAN)
    cfg = orc.default_config(particle_num=S.N_INIT, seed=S.SEED, init_cov=S.COV, init_mean=S.MEAN)
    rep = S.particle(S.REP, weight=1e-3)
    want = orc.init_particles(cfg, rep, 0, S.N_INIT)
    got = g.debugInitParticles(rep, 0, S.N_INIT)
    for k in KEYS:
        assert S.ulp_diff(got[k], want[k]).max() <= 1, k
        assert (got[k] == want[k]).mean() > 0.999, k
    np.testing.assert_array_equal(got["weight"], want["weight"])
    np.testing.assert_array_equal(g.debugInitParticles(rep, 600, 400).view(np.uint8), got[600:].view(np.uint8))


def resample_population(n):
    old = S.realistic_population(n, n, 0.06)
    rng = np.random.default_rng(n + 1)
    w = rng.random(n).astype(np.float32) ** 4
    w[rng.random(n) < 0.1] = 0
    old["weight"] = w / w.sum()
    return old


def test_table_resample_per_axis_step_noise(gpu, orc):
    """the asserts of test_gpu_parity.py::test_resample"""
    P = 2048
    g = fixed_tracker(gpu, P, step_cov=S.COV)
    cfg = orc.default_config(particle_num=P, seed=S.SEED, step_cov=S.COV)
    old = resample_population(P)
    a, q = orc.gen_alias_table(old["weight"])
    rep = S.particle(S.REP, weight=0.5)
    for epoch in S.EPOCHS:
        want = orc.resample(cfg, old, a, q, rep, epoch)
        got = g.debugResample(old, a, q, rep, epoch)
        assert got[0].tobytes() == rep[0].tobytes()
        for k in KEYS:
            assert S.ulp_diff(got[k], want[k]).max() <= 1, (epoch, k)
            assert (got[k] == want[k]).mean() > 0.999, (epoch, k)
        np.testing.assert_array_equal(got["weight"], want["weight"])
    np.testing.assert_array_equal(g.debugResample(old, a, q, rep, 3, 512, 256).view(np.uint8), got[512:768].view(np.uint8))


def test_product_resample_per_axis_step_noise(gpu, orc):
    """the three product instances against the oracle fed debugAlias's table, as test_gpu_resample_prefix.py::check_case
    (b) and (d) do; 4097 particles: more than one block, a coarse stride of 2 or more, a shard with id_offset != 0"""
    P = 4097
    g = fixed_tracker(gpu, P, step_cov=S.COV, reference=True)
    cfg = orc.default_config(particle_num=P, seed=S.SEED, step_cov=S.COV)
    old = resample_population(P)
    a, q = g.debugAlias(old["weight"])
    rep = S.particle(S.REP, weight=0.5)
    for epoch in S.EPOCHS:
        for off, nl in ((0, P), (2049, 63)):
            tag = (epoch, off, nl)
            want = orc.resample(cfg, old, a, q, rep, epoch, off, nl)
            got, mats = g.debugResamplePrefix(old, rep, epoch, off, nl, instance=1, want_mats=True)
            for k in KEYS:
                assert S.ulp_diff(got[k], want[k]).max() <= 1, (tag, k)
            assert (got.view(np.uint8) == want.view(np.uint8)).mean() > 0.999, tag
            np.testing.assert_array_equal(got["weight"].view(np.uint32), want["weight"].view(np.uint32))
            np.testing.assert_array_equal(got["w"].view(np.uint32), want["w"].view(np.uint32))
            if off == 0:
                assert got[0].tobytes() == rep[0].tobytes(), tag
            for instance in (0, 2):
                got_i, mats_i = g.debugResamplePrefix(old, rep, epoch, off, nl, instance=instance, want_mats=True)
                assert got_i.tobytes() == got.tobytes(), (tag, instance)
                assert mats_i.tobytes() == mats.tobytes(), (tag, instance)
            assert g.debugPoseToMatrix(got).tobytes() == mats.tobytes(), tag


# ---- one short whole-tracker run per variant -----------------------------------------------------------------------
WHOLE_FRAMES = 4
WHOLE_KLD = dict(bins=S.BINS, delta=0.9, epsilon=0.1, step_cov=S.COV, motion_ratio=0.6)
# a per-axis initial mean small enough to leave the object in view (MEAN is metres and radians away)
WHOLE_INIT_MEAN = tuple(0.01 * m for m in S.MEAN)


def whole_pair(gpu, orc, kld):
    """the same-trig, same-sum oracle of test_gpu_longrun.py::make_pair at the parameters above"""
    model, cloud = scene.make_model(512), scene.make_scene(20000)
    if kld:
        P = 300
        g = gpu.make_reference_tracker(particle_num=P, seed=S.SEED, kld=True)
        g.setDelta(WHOLE_KLD["delta"])
        g.setEpsilon(WHOLE_KLD["epsilon"])
        g.setBinSize(WHOLE_KLD["bins"])
        g.setMotionRatio(WHOLE_KLD["motion_ratio"])
        g.setStepNoiseCovariance(WHOLE_KLD["step_cov"])
        cfg = orc.default_config(particle_num=P, seed=S.SEED, threads=0, emulate_pcl_alloc=0, kld_adaptive=1,
                                 kld_bin_size=WHOLE_KLD["bins"], kld_delta=WHOLE_KLD["delta"],
                                 kld_epsilon=WHOLE_KLD["epsilon"], motion_ratio=WHOLE_KLD["motion_ratio"],
                                 step_cov=WHOLE_KLD["step_cov"])
    else:
        P = 400
        g = fixed_tracker(gpu, P, step_cov=S.COV, init_cov=S.COV, init_mean=WHOLE_INIT_MEAN)
        cfg = orc.default_config(particle_num=P, seed=S.SEED, threads=0, emulate_pcl_alloc=0, step_cov=S.COV,
                                 init_cov=S.COV, init_mean=WHOLE_INIT_MEAN)
    o = orc.Tracker(cfg)
    o.set_trig_mode(1)
    o.set_sum_mode(1)
    for ref, tr, inp in ((g.setReferenceCloud, g.setTrans, g.setInputCloud), (o.set_reference, o.set_trans, o.set_input)):
        ref(model)
        tr(scene.initial_trans())
        inp(cloud)
    return g, o


@pytest.mark.parametrize("kld", [True, False], ids=["kld", "fixed"])
def test_whole_tracker_at_per_axis_parameters_is_bit_stable(gpu, orc, kld):
    g, o = whole_pair(gpu, orc, kld)
    counts = []
    for f in range(WHOLE_FRAMES):
        g.compute()
        assert o.compute() == 0
        rg, ro = g.getResult(), o.get_result()
        pg, po = g.getParticles(), o.get_particles()
        counts.append((len(pg), len(po)))
        assert len(pg) == len(po), (f, counts)
        assert rg.tobytes() == ro.tobytes(), (f, rg, ro)
    print("whole tracker kld=%s: particle counts %s" % (kld, [c[0] for c in counts]))
    if not kld:
        assert all(c[0] == 400 for c in counts)

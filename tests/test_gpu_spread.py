"""GPU checks of the population statistics (pft_spread; k_spread_partial / k_spread_final in
pcl_tracking_amd/csrc/pft_spread.hip) and the spread rule: every field of the block against tests/spread_model.py on the
population read back from the same handle -- integers equal, the 29 sums and every double and float field bit for bit --
on explicit populations at the sizes where the reduction changes shape and after real frames (fixed, KLD, exact-NN, PCL
sums, a skipped last iteration); the rule against the model; no side effects on the tracker; handles in flight; a failed
iteration; the refusals; and the C++ driver's --spread lines.

Sizes: the workgroup block of k_spread_partial is 256 particles, k_spread_final takes four blocks per lane and 256 per wave
up to 1 024 blocks and 16 per lane beyond: 1, 2, 3, 63, 64, 65 (the wave), 255, 256, 257 (the block), 513 (two blocks + 1),
4 100 (above 4 096: 17 blocks, the final launch's lane level), 65 793 (258 blocks: its wave level), 262 913 (1 028 blocks:
the 16-blocks-per-lane instance; three patterns).  Frames: test_gpu_match's scene, 300-point model, about 4 000
points, 64 particles (KLD: at most 5 000)."""
import subprocess

import numpy as np
import pytest

import spread_model as sm
import test_gpu_match as tgm
from pcl_tracking_amd.scene import PARTICLE_DTYPE

pytestmark = pytest.mark.gpu
P = tgm.P
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 513, 4100, 65793, 262913)
CENTRE = np.array([0.3, -0.2, 1.1, 0.1, -0.4, 2.0])
SIGMA = np.array([0.02, 0.03, 0.01, 0.1, 0.05, 0.2])
KLD_CAPACITY = 5000  # the KL bound asks for fewer on these frames: the device-side count stays below the launch size


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


def pose_trans(gpu, pose6):
    """the 4x4 whose state (pft_to_state) pft_set_particles makes the representative state"""
    p = np.zeros(1, PARTICLE_DTYPE)
    for a, k in enumerate(sm.POSE):
        p[0][k] = pose6[a]
    return gpu.ParticleFilterTracker().toEigenMatrix(p[0])


def population(poses, weights):
    p = np.zeros(len(weights), PARTICLE_DTYPE)
    for a, k in enumerate(sm.POSE):
        p[k] = np.asarray(poses)[:, a].astype(np.float32)
    p["w"] = 1.0
    p["weight"] = np.asarray(weights, np.float32)
    return p


def patterns(n, rng, centre=CENTRE):
    """label -> population of n particles: the weight patterns of the issue"""
    poses = rng.normal(0.0, 1.0, (n, 6)) * SIGMA + centre  # mixed signs of d in every component
    w = rng.uniform(0.0, 1.0, n)
    out = {"mixed": population(poses, w / w.sum())}
    wz = w.copy()
    wz[rng.uniform(size=n) < 0.3] = 0.0
    out["zeros"] = population(poses, wz / max(wz.sum(), 1e-30))
    one = np.zeros(n)
    one[int(rng.integers(n))] = 1.0
    out["one_mass"] = population(poses, one)
    out["all_zero"] = population(poses, np.zeros(n))
    left = poses.copy()
    left[:, 0] = centre[0] - np.abs(left[:, 0] - centre[0]) - 0.001  # every x offset negative: the sums' zero is -0.0
    out["all_zero_one_side"] = population(left, np.zeros(n))
    eq = np.minimum(w, 0.5) / n
    ties = np.unique(rng.integers(0, n, 5))  # several equal maxima, in different waves and blocks when n allows
    eq[ties] = eq.max() * 2.0
    eq[n - 1] = eq[ties[0]]
    out["equal_maxima"] = population(poses, eq)
    return out


def check(t, label, thr=(np.inf, 0.0, 1), prev_streak=0):
    """one computeSpread() on the handle against the model on the population and result read back from it"""
    t.computeSpread()
    got = t.getSpread()
    particles, result = t.getParticles(), t.getResult()
    want = sm.stats(particles, result, *thr, prev_streak=prev_streak)
    bad = sm.compare(got, want, label)
    for b in bad[:4]:
        print(b)
    assert not bad, (label, [b[1] for b in bad])
    return got, want, particles


# ---- 1. explicit populations --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_explicit_populations(gpu, n):
    rng = np.random.default_rng(1000 + n)
    t = gpu.make_reference_tracker(particle_num=n)
    t.setTrans(pose_trans(gpu, CENTRE + 0.3 * SIGMA))  # the pivot: near the population, not its mean
    calls = 0
    for label, p in patterns(n, rng).items():
        if n > 100000 and label not in ("zeros", "all_zero_one_side", "equal_maxima"):
            continue
        t.setParticles(p)
        got, want, back = check(t, "n=%d %s" % (n, label))
        calls += 1
        assert back.tobytes() == p.tobytes() and got.calls == calls and got.n == n and got.evaluated
        if label == "zeros":
            assert got.n_zero == int((p["weight"] == 0).sum()) and (n < 8 or got.n_zero > 0)
        if label == "one_mass":
            assert got.n_eff == 1.0 and got.n_zero == n - 1 and got.i_max == int(np.flatnonzero(p["weight"])[0])
            assert not got.cov.any()
        if label.startswith("all_zero"):
            assert got.n_zero == n and got.sum_w == 0.0 and got.i_max == 0 and not got.cov.any() and not got.mean.any()
        if label == "all_zero_one_side" and n & (n - 1) == 0:
            assert np.signbit(got.s[0]), "a power of two has no padding: the root keeps the sign of its -0.0 terms"
        if label == "equal_maxima":
            first = int(np.flatnonzero(p["weight"] == p["weight"].max())[0])
            assert got.i_max == first and (n == 1 or first < n - 1), "the last particle ties with an earlier one"
    t.close()


@pytest.mark.parametrize("n", (65, 513))
def test_coordinates_of_a_kilometre(gpu, n):
    """10^3 m: around the representative state the second moments do not cancel -- finite, and the model's bits"""
    rng = np.random.default_rng(2000 + n)
    centre = CENTRE + np.array([1000.0, -1000.0, 1000.0, 0, 0, 0])
    t = gpu.make_reference_tracker(particle_num=n)
    t.setTrans(pose_trans(gpu, centre))
    p = patterns(n, rng, centre)["mixed"]
    t.setParticles(p)
    got, _, _ = check(t, "far n=%d" % n)
    assert np.isfinite(got.cov).all() and (np.diag(got.cov) > 0).all()
    # a float at 1 000 has steps of 6e-5: the position sigmas are those of the rounded cloud, still near the drawn ones
    assert 0.5 * SIGMA[1] < float(got.pos_sigma[2]) < 2.0 * SIGMA[1]
    assert np.allclose(got.rpy_sigma, SIGMA[3:], rtol=0.5)
    t.close()


def test_kld_handle_reads_its_count_on_the_device(gpu):
    rng = np.random.default_rng(7)
    t = gpu.make_reference_tracker(particle_num=P, kld=True)
    t.setMaximumParticleNum(300)  # capacity: two blocks
    t.setTrans(pose_trans(gpu, CENTRE))
    for n in (37, 256, 257, 300, 1):
        t.setParticles(patterns(n, rng)["zeros"])
        got, _, back = check(t, "kld n=%d" % n)
        assert got.n == n == len(back)
    t.close()


# ---- 2. after real frames -----------------------------------------------------------------------------------------------
def make(gpu, kld=False, exact=False, seed=3, iterations=2, **kw):
    t = gpu.make_reference_tracker(particle_num=P, seed=seed, kld=kld, **kw)
    if kld:
        t.setMaximumParticleNum(KLD_CAPACITY)
    if exact:
        t.setCloudCoherence(tgm._exact_coherence(gpu))
    t.setIterationNum(iterations)
    t.setReferenceCloud(tgm.model())
    t.setTrans(tgm._world()["trans"])
    return t


def step(t, cloud):
    t.setInputCloud(cloud)
    t.compute()


@pytest.mark.parametrize("kind", ["fixed", "kld", "exact", "pcl_sums"])
def test_after_real_frames(gpu, kind):
    t = make(gpu, kld=kind == "kld", exact=kind == "exact", **({"sum_order": "pcl"} if kind == "pcl_sums" else {}))
    for f in range(2):
        step(t, tgm.frame(f))
        got, _, particles = check(t, "%s frame %d" % (kind, f))
        assert got.evaluated and got.calls == f + 1 and got.n == len(particles) and got.solve_info == 0
        assert abs(got.sum_w - 1.0) < 1e-5 and 1.0 <= got.n_eff <= got.n  # weights normalised
        assert np.allclose(got.mean, [float(t.getResult()[k]) for k in sm.POSE], rtol=0, atol=1e-5)  # update()'s mean, in double
        assert 0.0 < float(got.pos_sigma[2]) < 0.1 and (got.pos_sigma[:-1] <= got.pos_sigma[1:]).all()
        if kind == "kld":
            print("kld frame %d: %d particles of %d" % (f, got.n, KLD_CAPACITY))
            assert got.n < KLD_CAPACITY, "precondition: the device-side count is below the capacity"
    t.close()


def test_skipped_last_iteration_is_evaluated(gpu):
    t = make(gpu)
    t.setMinPointsOfChangeDetection(100000)  # (as test_gpu_match: once in use, the detector skips every iteration)
    t.setIntervalOfChangeDetection(0)
    step(t, tgm.frame(0))
    check(t, "before the detector")
    t.setUseChangeDetector(True)
    step(t, tgm.frame(1))
    ring = t.debugChangeState()["ring"]
    assert ring[-1][0] == 1 and ring[-1][1] == 0, "precondition: the last iteration was tested and skipped"
    got, _, _ = check(t, "skipped")
    assert got.evaluated and got.calls == 2 and abs(got.sum_w - 1.0) < 1e-5
    t.close()


# ---- 3. the rule --------------------------------------------------------------------------------------------------------
def test_spread_rule_follows_the_model_and_reset_clears_it(gpu):
    rng = np.random.default_rng(11)
    t = gpu.make_reference_tracker(particle_num=64)
    t.setTrans(pose_trans(gpu, CENTRE))
    thr = (0.05, 8.0, 2)
    t.setSpreadThreshold(*thr)
    tight = patterns(64, rng)["mixed"]                      # pos sigma about 0.03, n_eff about 48
    wide = tight.copy()
    wide["y"] = (CENTRE[1] + 4.0 * (tight["y"] - CENTRE[1])).astype(np.float32)  # sigma above 0.05
    few = patterns(64, rng)["one_mass"]                     # n_eff 1
    rule = sm.SpreadRule(*thr)
    seq = [tight, wide, few, tight, tight, wide, wide, wide, tight]
    fired = []
    for k, p in enumerate(seq):
        t.setParticles(p)
        got, want, _ = check(t, "rule %d" % k, thr, prev_streak=rule.streak)
        assert (got.uncertain, got.streak, got.flagged) == rule.step(got.pos_sigma[2], got.n_eff), k
        fired.append(got.flagged)
        assert t.isUncertain() == got.flagged
    assert fired == [False, False, True, False, False, False, True, True, False], "the threshold fires and clears"
    t.setParticles(wide)
    check(t, "before reset", thr, prev_streak=0)
    assert t.getSpread().streak == 1
    t.resetTracking()
    st = t.getSpread()
    assert (st.uncertain, st.streak, st.flagged) == (False, 0, False) and st.calls == len(seq) + 1, "the streak is cleared"
    with pytest.raises(gpu.PftError) as e:  # the handle forgot its population
        t.computeSpread()
    assert e.value.status == 7
    t.setParticles(wide)
    t.setReferenceCloud(tgm.model())  # a new object clears it as well
    check(t, "after a new reference", thr, prev_streak=0)
    t.setReferenceCloud(tgm.model())
    assert t.getSpread().streak == 0
    t.close()


# ---- 4. no side effects, handles in flight ------------------------------------------------------------------------------
@pytest.mark.parametrize("kld", [False, True])
def test_spread_leaves_the_tracker_alone(gpu, kld):
    a, b = make(gpu, kld=kld), make(gpu, kld=kld)
    for f in range(6):
        step(a, tgm.frame(f % 4))
        a.computeSpread()
        step(b, tgm.frame(f % 4))
        assert tgm.snapshot(a) == tgm.snapshot(b), f
    assert a.getSpread().calls == 6
    a.close()
    b.close()


def blob(st):
    return tuple(np.asarray(getattr(st, f)).tobytes() for f in sm.DOUBLE_FIELDS + sm.FLOAT_FIELDS) + \
        tuple(int(getattr(st, f)) for f in sm.INT_FIELDS)


def test_four_handles_in_flight_equal_each_alone(gpu):
    alone = []
    for k in range(4):
        t = make(gpu, seed=10 + k, kld=k == 3)
        per_frame = []
        for f in range(2):
            step(t, tgm.frame(f))
            t.computeSpread()
            per_frame.append((tgm.snapshot(t), blob(t.getSpread())))
        alone.append(per_frame)
        t.close()
    ts = [make(gpu, seed=10 + k, kld=k == 3) for k in range(4)]
    for f in range(2):
        for t in ts:  # compute and statistics of all four enqueued before anyone synchronises
            step(t, tgm.frame(f))
            t.computeSpread()
        for k, t in enumerate(ts):
            assert (tgm.snapshot(t), blob(t.getSpread())) == alone[k][f], (k, f)
    for t in ts:
        t.close()


# ---- 5. a failed iteration, the refusals --------------------------------------------------------------------------------
def test_failed_last_iteration_is_not_evaluated(gpu):
    t = make(gpu, iterations=1)  # the injection lands behind the NEXT crop: with one iteration that is the frame's last
    t.setSpreadThreshold(1e-6, 0.0, 1)  # a streak to keep
    step(t, tgm.frame(0))
    a, _, _ = check(t, "before the failure", (1e-6, 0.0, 1))
    assert a.evaluated and a.calls == 1 and a.streak == 1
    t.debugInjectError(4)
    step(t, tgm.frame(1))
    t.computeSpread()
    with pytest.raises(gpu.PftError) as e:
        t.getSpread()
    assert e.value.status == 5 and "bit2" in str(e.value)
    b = t.getSpread()  # reported once
    assert not b.evaluated and b.calls == 2
    assert blob(b)[:-len(sm.INT_FIELDS)] == blob(a)[:-len(sm.INT_FIELDS)], "the block is unchanged"
    assert (b.n, b.n_zero, b.i_max, b.solve_info, b.uncertain, b.streak, b.flagged) == \
        (a.n, a.n_zero, a.i_max, a.solve_info, a.uncertain, a.streak, a.flagged)
    step(t, tgm.frame(2))  # per iteration, not sticky
    c, _, _ = check(t, "after the failure", (1e-6, 0.0, 1), prev_streak=1)
    assert c.evaluated and c.calls == 3 and c.streak == 2
    t.close()


def test_refusals(gpu):
    s = gpu.ParticleFilterTracker(world_size=2)
    s.setParticleNum(P)
    s.setReferenceCloud(tgm.model())
    s.setInputCloud(tgm.frame(0))
    with pytest.raises(gpu.PftError) as e:
        s.computeSpread()
    assert e.value.status == 1 and "sharded" in str(e.value)
    s.close()

    t = make(gpu)
    t.setInputCloud(tgm.frame(0))
    with pytest.raises(gpu.PftError) as e:
        t.computeSpread()
    assert e.value.status == 7 and "there is no population yet" in str(e.value)
    with pytest.raises(gpu.PftError) as e:
        t.getSpread()
    assert e.value.status == 7 and "before the first pft_spread" in str(e.value)
    for bad in ((-1.0, 0.0, 1), (0.1, -1.0, 1), (float("nan"), 0.0, 1), (0.1, float("nan"), 1), (0.1, 0.0, 0)):
        st = t._L.pft_set_spread_threshold(t._h, bad[0], bad[1], bad[2])  # the C entry point itself
        assert st == 1 and b"pft_set_spread_threshold" in t._L.pft_last_error_string(t._h), bad
    t.compute()
    t.computeSpread()
    assert t.getSpread().evaluated
    # allowed where the match is refused: after the test hooks that replace the population or rebuild the tree
    t.evalWeights(t.getParticles()[:8])
    check(t, "after evalWeights")
    t.setParticles(t.getParticles())
    check(t, "after setParticles")
    t.close()


def test_with_the_frame_graph(gpu, monkeypatch):
    """PFT_GRAPH=1: the statistics are launched outside the captured frame"""
    monkeypatch.setenv("PFT_GRAPH", "1")
    t = make(gpu)
    for f in range(5):  # the third frame on is replayed as a graph
        step(t, tgm.frame(f % 4))
        got, _, _ = check(t, "graph frame %d" % f)
        assert got.calls == f + 1
    t.close()


# ---- 6. the C++ driver --------------------------------------------------------------------------------------------------
def test_cpp_driver_prints_the_models_values(gpu, orc, tmp_path):
    from pcl_tracking_amd import build

    w = tgm._world()
    cluster = w["obj"][np.random.default_rng(7).choice(2000, 300, replace=False)]
    frames = [tgm.frame(0), tgm.frame(1)]
    c, _ = orc.compute_3d_centroid(cluster)
    ref, trans = orc.recentre_model(cluster, c)
    thr = (0.004, 0.0, 2)
    t = tgm.make(gpu, seed=1, reference=ref, trans=trans)  # what the driver's "set object to track" step forms
    want, streak = [], 0
    for cloud in frames:
        step(t, cloud)
        want.append(sm.stats(t.getParticles(), t.getResult(), *thr, prev_streak=streak))
        streak = want[-1]["streak"]
    t.close()
    tgm.write_pcd(str(tmp_path / "model.pcd"), cluster)
    paths = []
    for f, cloud in enumerate(frames):
        paths.append(str(tmp_path / ("frame%d.pcd" % f)))
        tgm.write_pcd(paths[-1], cloud)
    base = [build.build_example(), str(tmp_path / "model.pcd"), "--frames"] + paths + \
        ["--particles", str(P), "--seed", "1", "--model-leaf", "0"]
    with_flag = subprocess.run(base + ["--spread=%g,%g,%d" % thr], capture_output=True, text=True, timeout=300)
    without = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert with_flag.returncode == 0 and without.returncode == 0, with_flag.stderr[-2000:]
    lines = [ln for ln in with_flag.stdout.splitlines() if ln.startswith("spread obj ")]
    assert len(lines) == 2
    for ln, m in zip(lines, want):
        tok = ln.split()
        assert tok[:3] == ["spread", "obj", "0:"]
        val = {k: tok[tok.index(k) + 1:] for k in ("n_eff", "n", "zero", "w_max", "pos_sigma", "rpy_sigma", "evaluated",
                                                    "uncertain", "streak", "flagged")}
        assert float(val["n_eff"][0]) == m["n_eff"] and int(val["n"][0]) == m["n"] and int(val["zero"][0]) == m["n_zero"]
        assert np.float32(val["w_max"][0]) == m["w_max"]
        assert [np.float32(v) for v in val["pos_sigma"][:3]] == m["pos_sigma"].tolist()
        assert [float(v) for v in val["rpy_sigma"][:3]] == m["rpy_sigma"].tolist()
        assert [int(val[k][0]) for k in ("evaluated", "uncertain", "streak", "flagged")] == \
            [m["evaluated"], m["uncertain"], m["streak"], m["flagged"]]
    assert [m["flagged"] for m in want] == [0, 1], "precondition: the threshold fires on the second frame"
    # the flag only adds its lines: everything else is what the driver prints without it
    assert "spread" not in without.stdout and "spread" not in without.stderr
    assert [ln for ln in with_flag.stdout.splitlines() if not ln.startswith("spread obj ")] == without.stdout.splitlines()
    assert with_flag.stderr == without.stderr

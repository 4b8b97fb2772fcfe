"""CPU-only proof, with the oracle alone, that the cases of tests/sampling_cases.py reach the regimes the GPU tests
(tests/test_gpu_sampling_cases.py) take them for, so that a case that has silently become degenerate cannot pass there:
the one-bin cases hold k == 1 to maxn, the tiny-bin cases open a bin per candidate, every delta x epsilon case stops
strictly inside (2, maxn) and delta moves the count, the zero-centred cases straddle bin 0 on all six axes, every swap of
two per-axis bin sizes changes the bins, and the scaling / mean relations the GPU tests assert bit for bit hold in the oracle.
The two helpers the GPU tests replay the device's own output with (bins_of, replay_stop_rule) are checked against the
oracle's bins and counts on every case."""
import itertools

import numpy as np
import pytest

import sampling_cases as S

IDS = lambda c: c.name  # noqa: E731


@pytest.fixture(scope="module")
def runs(orc):
    """every KLD case once per epoch on the oracle's own Walker table: name -> [(particles, bins, k), ..]"""
    out = {}
    for c in S.KLD_CASES + S.MATS_CASES:
        old = S.case_population(c)
        a, q = orc.gen_alias_table(old["weight"])
        cfg = S.oracle_config(orc, c)
        out[c.name] = [orc.kld_resample(cfg, old, a, q, S.case_motion(c), e) for e in S.EPOCHS]
    return out


def test_parameter_sets_have_no_two_axes_alike():
    for vals in (S.COV, S.COV_SCALED, S.MEAN, S.BINS, S.MOTION6):
        assert len(set(vals)) == 6 and all(v != 0 for v in vals)
        assert len(set(np.float32(v) for v in vals)) == 6
    # the scaled partner is exact: sqrt(cov * 4**j) == sqrt(cov) * 2**j in double
    for k in range(6):
        assert np.sqrt(np.float64(S.COV_SCALED[k])) == np.sqrt(np.float64(S.COV[k])) * S.SCALE[k]
    assert len(set(S.REP)) == 6


@pytest.mark.parametrize("c", S.CASES_K1, ids=IDS)
def test_one_bin_cases_hold_k_1_to_the_end(runs, c):
    for p, bins, k in runs[c.name]:
        assert k == 1 and len(p) == c.maxn
        assert (bins == 0).all()


@pytest.mark.parametrize("c", S.CASES_KN, ids=IDS)
def test_tiny_bin_cases_open_a_bin_per_candidate(runs, c):
    for p, bins, k in runs[c.name]:
        assert k == len(p) == c.maxn
        assert np.abs(bins).max() < 2 ** 15  # far from the int32 range


def test_capacity_cases_saturate_below_2049_and_stop_inside_above(runs):
    for c in S.CASES_CAPACITY:
        for p, bins, k in runs[c.name]:
            if c.maxn <= 1025:
                assert len(p) == c.maxn, c.name
            else:
                assert 2 < len(p) < c.maxn, c.name
            assert 1 <= k <= len(p)
    # maxn = 2: the rule is not consulted before n == maxn whatever k is
    assert [len(r[0]) for r in runs["cap-400-2"]] == [2, 2]


@pytest.mark.parametrize("c", S.CASES_DELTA_EPS, ids=IDS)
def test_delta_epsilon_cases_stop_strictly_inside(runs, c):
    for p, bins, k in runs[c.name]:
        assert 2 < len(p) < c.maxn and 2 <= k < len(p)


def test_delta_and_epsilon_each_move_the_count(runs):
    for e, epoch in itertools.product(S.EPSILONS, range(len(S.EPOCHS))):
        n = [len(runs["delta-%g-eps-%g" % (d, e)][epoch][0]) for d in S.DELTAS]
        print("epsilon %g epoch %d: n over delta %s = %s" % (e, S.EPOCHS[epoch], S.DELTAS, n))
        if e == 0.1:
            assert len(set(n)) >= 2, n
    for d, epoch in itertools.product(S.DELTAS, range(len(S.EPOCHS))):
        n = [len(runs["delta-%g-eps-%g" % (d, e)][epoch][0]) for e in S.EPSILONS]
        assert n[0] != n[1], (d, n)


@pytest.mark.parametrize("c", S.CASES_ZERO + S.CASES_AXIS_BINS, ids=IDS)
def test_zero_centred_cases_straddle_bin_0_on_all_axes(runs, c):
    for p, bins, k in runs[c.name]:
        x = S.poses(p)
        for i in range(6):
            assert (bins[:, i] == 0).any() and (bins[:, i] < 0).any() and (bins[:, i] > 0).any(), (c.name, i)
            # bin 0 is double width: it holds values of both signs
            in0 = x[bins[:, i] == 0, i]
            assert (in0 < 0).any() and (in0 > 0).any(), (c.name, i)


def test_every_swap_of_two_bin_sizes_changes_the_bins(orc, runs):
    (c,) = S.CASES_AXIS_BINS
    old = S.case_population(c)
    a, q = orc.gen_alias_table(old["weight"])
    for epoch_i, epoch in enumerate(S.EPOCHS):
        base = runs[c.name][epoch_i][1]
        for i, j in itertools.combinations(range(6), 2):
            b = list(c.bins)
            b[i], b[j] = b[j], b[i]
            _, bins, _ = orc.kld_resample(S.oracle_config(orc, c._replace(bins=tuple(b))), old, a, q, S.case_motion(c), epoch)
            # the candidates are the same (the bins do not enter them): compare the common prefix, element by element
            m = min(len(bins), len(base))
            assert (bins[:m] != base[:m]).any(), (i, j)
            assert (bins[:m, i] != base[:m, i]).any() and (bins[:m, j] != base[:m, j]).any(), (i, j)


def test_motion_ratio_cases_move_nobody_and_everybody(orc, runs):
    stay, move = (runs[c.name] for c in S.CASES_MOTION)
    c = S.CASES_MOTION[0]
    old = S.case_population(c)
    a, q = orc.gen_alias_table(old["weight"])
    m = S.poses(S.case_motion(c))[0]
    for epoch_i, epoch in enumerate(S.EPOCHS):
        # the default ratio moves some: 0 and 1 are the two ends
        mid = orc.kld_resample(S.oracle_config(orc, c._replace(motion_ratio=0.25)), old, a, q, S.case_motion(c), epoch)[0]
        n = min(len(stay[epoch_i][0]), len(move[epoch_i][0]), len(mid))
        xs, xm, xd = S.poses(stay[epoch_i][0])[:n], S.poses(move[epoch_i][0])[:n], S.poses(mid)[:n]
        np.testing.assert_array_equal(xm, xs + m[None, :])  # float add, as StateT operator+
        assert (xm != xs).all()
        moved = (xd != xs).any(axis=1)
        assert 0 < moved.sum() < n


@pytest.mark.parametrize("c", S.KLD_CASES + S.MATS_CASES, ids=IDS)
def test_helpers_reproduce_the_oracle(orc, runs, c):
    """bins_of from the oracle's particles gives the oracle's bins, and the plain-Python loop over them its n and k"""
    for epoch_i in range(len(S.EPOCHS)):
        p, bins, k = runs[c.name][epoch_i]
        np.testing.assert_array_equal(S.bins_of(p, c.bins), bins)
        bound = lambda kk: orc.kld_bound(kk, c.delta, c.epsilon)  # noqa: E731
        assert S.replay_stop_rule(bins, c.maxn, bound) == (len(p), k)
        if len(p) > 1:
            assert S.replay_stop_rule(bins[:-1], c.maxn, bound) is None  # it stops nowhere earlier


# ---- the relations the GPU tests assert bit for bit ---------------------------------------------------------------
def scaled(base, big):
    """component k of big == 2**(k + 1) * component k of base, bit for bit; and the noise is not degenerate"""
    xb, xg = S.poses(base), S.poses(big)
    assert xb.shape == xg.shape
    for k in range(6):
        np.testing.assert_array_equal(xg[:, k].view(np.uint32), (xb[:, k] * np.float32(S.SCALE[k])).view(np.uint32))
    return xb


def test_scaling_relation_holds_in_the_oracle(orc):
    rep = S.particle()
    # init
    out = [orc.init_particles(orc.default_config(particle_num=S.N_INIT, seed=S.SEED, init_cov=cov), rep, 0, S.N_INIT)
           for cov in (S.COV, S.COV_SCALED)]
    xb = scaled(*out)
    assert (xb != 0).all() and len(np.unique(xb)) == xb.size
    # fixed resample
    old = S.zero_pose_population(S.N_RESAMPLE, 1)
    a, q = orc.gen_alias_table(old["weight"])
    rep = S.particle(weight=0.25)
    for epoch in S.EPOCHS:
        out = [orc.resample(orc.default_config(particle_num=S.N_RESAMPLE, seed=S.SEED, step_cov=cov), old, a, q, rep, epoch)
               for cov in (S.COV, S.COV_SCALED)]
        xb = scaled(*out)
        assert out[0][0].tobytes() == rep[0].tobytes() and out[1][0].tobytes() == rep[0].tobytes()
        assert (xb[1:] != 0).all()
    # KLD: one bin, no motion -> both runs keep all maxn candidates
    old = S.zero_pose_population(S.N_KLD_OLD, 2)
    a, q = orc.gen_alias_table(old["weight"])
    for epoch in S.EPOCHS:
        out = []
        for cov in (S.COV, S.COV_SCALED):
            cfg = orc.default_config(kld_adaptive=1, seed=S.SEED, kld_max_particles=S.MAXN_KLD_SCALING, step_cov=cov,
                                     kld_bin_size=(S.BIN_ALL_IN_ONE,) * 6)
            p, bins, k = orc.kld_resample(cfg, old, a, q, S.particle(), epoch)
            assert len(p) == S.MAXN_KLD_SCALING and k == 1
            out.append(p)
        assert (scaled(*out) != 0).all()


def test_mean_relation_holds_in_the_oracle(orc):
    rep = S.particle(S.REP)
    cfg = orc.default_config(particle_num=S.N_INIT, seed=S.SEED, init_cov=(0.0,) * 6, init_mean=S.MEAN)
    x = S.poses(orc.init_particles(cfg, rep, 0, S.N_INIT))
    want = np.asarray(S.MEAN, np.float64).astype(np.float32) + S.poses(rep)[0]
    assert want.dtype == np.float32
    np.testing.assert_array_equal(x.view(np.uint32), np.broadcast_to(want, x.shape).view(np.uint32))
    # a mean on the wrong axis would show: no two axes of the expectation agree under any swap of two means
    m32 = np.asarray(S.MEAN, np.float64).astype(np.float32)
    for i, j in itertools.combinations(range(6), 2):
        assert m32[j] + S.poses(rep)[0][i] != want[i]

"""Parameter sets, populations and KLD cases of the sampling-stage tests (tests/test_gpu_sampling_cases.py): k_init_particles,
k_resample<TABLE>, k_resample4<BOX, GATED> and k_resample_kld<TABLE, GATED> with particle_sample / normal_pair, at
parameters in which no two axes agree, so that a parameter read from the wrong axis changes a result.  The reference
application's set (tracker.make_reference_tracker) has sigma equal within x/y/z and within roll/pitch/yaw, one initial noise
on all six axes with mean zero, and one bin size.

tests/test_sampling_cases_host.py proves with the oracle alone, on the CPU, that every case below reaches the regime it is
named after.  Nothing here touches a GPU.
"""
import collections

import numpy as np

from pcl_tracking_amd import scene

KEYS = ("x", "y", "z", "roll", "pitch", "yaw")
SEED = 11
EPOCHS = (0, 3)

# ---- parameter sets: six distinct values each ------------------------------------------------------------------------
COV = (1e-4, 2.3e-4, 3.1e-4, 1.7e-3, 2.9e-3, 4.3e-3)
# the scaled partner: cov[k] * 4**(k + 1) is exact in double, and so is sqrt of it = sigma[k] * 2**(k + 1)
COV_SCALED = tuple(c * 4.0 ** (k + 1) for k, c in enumerate(COV))
SCALE = tuple(2.0 ** (k + 1) for k in range(6))
MEAN = (0.125, -0.3, 1.7, 0.01, -2.5, 3.0)
BINS = (0.05, 0.1, 0.2, 0.15, 0.3, 0.6)
MOTION6 = (0.004, -0.007, 0.011, -0.02, 0.013, 0.031)  # all six components distinct and non-zero
MOTION_DEFAULT = (0.004, 0.0, 0.0, 0.0, 0.0, -0.02)  # the motion of test_gpu_kld.py

# the reference application's values (tracker.make_reference_tracker / the oracle's default_config)
STEP_COV_DEFAULT = (0.015 * 0.015,) * 3 + (0.015 * 0.015 * 40.0,) * 3
BINS_DEFAULT = (0.1,) * 6

# particle counts of the scaling runs
N_INIT, N_RESAMPLE, N_KLD_OLD, MAXN_KLD_SCALING = 1000, 512, 200, 300
BIN_ALL_IN_ONE = 1e6  # one bin holds every candidate: k == 1, the loop runs to maxn
BIN_ALL_APART = 1e-4  # every candidate opens its own bin: k == n (|bin| of the order 1e4 for poses around 1)


# ---- populations -----------------------------------------------------------------------------------------------------
def _population(n, seed, spread, centre):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    for k, name in enumerate(KEYS):
        p[name] = centre[k] + rng.normal(0, spread, n)
    p["w"] = 1.0
    w = rng.random(n).astype(np.float32) ** 4
    p["weight"] = w / w.sum()
    return p


def realistic_population(n, seed, spread):
    """the population of test_gpu_kld.py: poses around the model's"""
    return _population(n, seed, spread, scene.model_gt_pose())


def zero_centred_population(n, seed, spread):
    """the same draws around pose zero: bins straddle 0 on all six axes ((int) truncates toward zero, so bin 0 is double
    width and holds values of both signs)"""
    return _population(n, seed, spread, (0.0,) * 6)


def zero_pose_population(n, seed):
    """every pose exactly zero, random weights: a drawn particle is 0 + (float)(z * sigma + mean) whichever entry the
    alias draw picks"""
    p = _population(n, seed, 0.0, (0.0,) * 6)
    assert all((p[k] == 0).all() for k in KEYS)
    return p


def particle(pose=(0.0,) * 6, weight=0.0):
    p = np.zeros(1, scene.PARTICLE_DTYPE)
    for k, name in enumerate(KEYS):
        p[name] = pose[k]
    p["w"] = 1.0
    p["weight"] = weight
    return p


REP = (0.3, -0.2, 1.1, 0.05, -0.4, 0.7)  # a representative state with six distinct components


# ---- KLD cases -------------------------------------------------------------------------------------------------------
KldCase = collections.namedtuple(
    "KldCase", "name pop n_old pop_seed spread maxn bins delta epsilon motion_ratio motion step_cov")


# spread 0.06 with the reference's bins and step noise: the count saturates up to maxn = 1025 and the rule stops the loop
# between 1500 and 1900 above (test_sampling_cases_host.py), so both ends of the loop condition are met at the capacities
def _case(name, pop, maxn, n_old=400, spread=0.06, pop_seed=None, bins=BINS_DEFAULT, delta=0.99, epsilon=0.2,
          motion_ratio=0.25, motion=MOTION_DEFAULT, step_cov=STEP_COV_DEFAULT):
    return KldCase(name, pop, n_old, n_old + maxn if pop_seed is None else pop_seed, spread, maxn, tuple(bins), delta,
                   epsilon, motion_ratio, tuple(motion), tuple(step_cov))


CAPACITY_EDGES = ((400, 1), (400, 2), (400, 63), (400, 1023), (400, 1024), (400, 1025), (400, 2049), (400, 4097),
                  (400, 16384), (3000, 500))
DELTAS = (0.5, 0.9, 0.999)
EPSILONS = (0.1, 0.3)

# maxn <= 1024: table and bins in LDS, above in HBM; 1025 / 2049 / 4097: the table of 2 * pow2 entries and the two
# per-candidate arrays behind it end within 132 words of the 6 * maxn + 128 allocation; (3000, 500): n_old > maxn
CASES_CAPACITY = [_case("cap-%d-%d" % (n_old, maxn), "realistic", maxn, n_old=n_old) for n_old, maxn in CAPACITY_EDGES]
CASES_K1 = [_case("k1-%d" % maxn, "realistic", maxn, bins=(BIN_ALL_IN_ONE,) * 6) for maxn in (500, 1025)]
CASES_KN = [_case("kn-%d" % maxn, "realistic", maxn, bins=(BIN_ALL_APART,) * 6) for maxn in (1024, 16384)]
CASES_ZERO = [_case("zero-%d" % maxn, "zero", maxn) for maxn in (500, 4097)]
CASES_AXIS_BINS = [_case("axis-bins-1025", "zero", 1025, spread=0.2, bins=BINS)]
CASES_DELTA_EPS = [_case("delta-%g-eps-%g" % (d, e), "zero", 4097, spread=0.05, delta=d, epsilon=e)
                   for d in DELTAS for e in EPSILONS]
# the motion coin: nobody moves, everybody moves; per-axis step noise under it
CASES_MOTION = [_case("motion-ratio-%g" % r, "realistic", 500, motion_ratio=r, motion=MOTION6, step_cov=COV)
                for r in (0.0, 1.0)]
KLD_CASES = CASES_CAPACITY + CASES_K1 + CASES_KN + CASES_ZERO + CASES_AXIS_BINS + CASES_DELTA_EPS + CASES_MOTION
# the cases whose matrices are compared too (LDS and HBM side of the switch)
MATS_CASES = [_case("mats-%d" % maxn, "realistic", maxn, motion=MOTION6, step_cov=COV) for maxn in (500, 1025)]


def case_population(c):
    f = {"realistic": realistic_population, "zero": zero_centred_population}[c.pop]
    return f(c.n_old, c.pop_seed, c.spread)


def case_motion(c):
    return particle(c.motion)


def oracle_config(orc, c, **kw):
    return orc.default_config(kld_adaptive=1, seed=SEED, particle_num=c.n_old, kld_max_particles=c.maxn,
                              kld_bin_size=c.bins, kld_delta=c.delta, kld_epsilon=c.epsilon,
                              motion_ratio=c.motion_ratio, step_cov=c.step_cov, **kw)


# ---- the checks that need no oracle ----------------------------------------------------------------------------------
def poses(p):
    return np.stack([np.ascontiguousarray(p[k], np.float32) for k in KEYS], axis=1)


def bins_of(particles, bin_size):
    """bin[i] = (int)(x[i] / bin_size[i]) in float, as upstream: numpy's float32 division is IEEE like the C one and the
    device's, and the cast truncates toward zero"""
    q = poses(particles) / np.asarray(bin_size, np.float64).astype(np.float32)[None, :]
    assert q.dtype == np.float32 and np.abs(q).max(initial=0.0) < 2.0 ** 30
    return np.trunc(q).astype(np.int32)


def replay_stop_rule(bins, maxn, bound):
    """the sequential loop of KLDAdaptiveParticleFilterTracker::resample over the bins given, in plain Python:
    do { k += new bin; ++n } while (n < maxn && (k < 2 || n < bound(k))) -> (n, k), or None when the loop would go on
    past the bins given.  bound(k) is calcKLBound"""
    seen, n = set(), 0
    for row in np.asarray(bins).tolist():
        seen.add(tuple(row))
        n += 1
        k = len(seen)
        if not (n < maxn and (k < 2 or n < bound(k))):
            return n, k
    return None


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)

"""The resample kernels pft_compute launches, on explicit inputs, against the CPU oracle (run with -m gpu).

test_gpu_parity.py::test_resample and test_gpu_kld.py::test_kld_resample_bit_exact drive the explicit-table instances
(k_resample<true>, k_resample_kld<true, false>).  The product instances have no table: k_resample4<BOX, GATED>,
k_resample<false> and k_resample_kld<false, *> evaluate the drawn entry on demand from the prefix-sum form that
k_population / k_population_seq leave in HBM, through a 256-entry coarse level of the running sums staged in LDS
(pcl_tracking_amd/csrc/pft_alias.h).  Here debugResamplePrefix / debugKldResample(old, None, None, ..) build the prefix
form from the given weights and launch those instances.

The drawn index is observable: old[i].x = i (exact below 2^24) and the step noise is ~3 mm, so the index of every slot
is rint(out.x).

(a) decoded indices, every slot: equal to those of orc.resample with the table debugAlias materialises from the same
    prefix form by the plain one-level search (same alias_q arithmetic: only the search path differs) -- no tolerance
(b) whole particles: <= 1 ulp per component of that oracle output and > 0.999 of the bytes identical (the bars of
    test_resample for the Box-Muller log / sin / cos), weight bit-equal, slot 0 the representative state verbatim
(c) against the oracle's own sequential Walker table: a decoded index may differ only where the slot's draw falls
    between q_dev[k] and q_orc[k] (rounding of prefix sums against sequential updates) with a_dev == a_orc everywhere;
    the number of such slots is printed, and at most 2 per case are excused
(d) the three instances (one lane, four lanes, four lanes + box) return the same bytes, and the matrices they write are
    debugPoseToMatrix(out) bit for bit

Shapes (alias_cases.py): where the coarse stride s = ceil(m / 256) resp. ceil(nh / 256) steps, where the last coarse
block is ragged, m = 0, nh = 1, ties in E; shards with id_offset != 0 and n_local not a multiple of 16 quads.
"""
import numpy as np
import pytest

import alias_cases as AC
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu
KEYS = ("x", "y", "z", "roll", "pitch", "yaw")
SEED = 5
EPOCHS = (0, 3)
ORDERS = ("tree", "pcl")


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


@pytest.fixture(scope="module")
def handles(gpu):
    """one handle per summation order, both with a reference cloud (the fused box instance needs its support subset)"""
    model = scene.make_model(2048)
    out = {}
    for order in ORDERS:
        g = gpu.make_reference_tracker(particle_num=64, seed=SEED, sum_order=order)
        g.setReferenceCloud(model)
        out[order] = g
    return out


def indexed_population(n, w, seed):
    """x = the particle's index, the other five pose components random"""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    p["x"] = np.arange(n, dtype=np.float32)
    for k in KEYS[1:]:
        p[k] = rng.normal(0, 0.5, n)
    p["w"] = 1.0
    p["weight"] = w
    return p


def decode(out):
    return np.rint(out["x"].astype(np.float64)).astype(np.int64)


def shards_of(n):
    if n < 8192:
        return [(0, n)]
    if n == 8192:
        return [(0, n)] + [(off, nl) for off in (0, 4000) for nl in (1, 63, 64, 65)]
    return [(0, 4096), (n - 4097, 4097), (n // 2 + 1, 63)]


def check_case(orc, g, label, w, shards, pop_seed):
    n = len(w)
    cfg = orc.default_config(particle_num=n, seed=SEED)
    old = indexed_population(n, w, pop_seed)
    a_dev, q_dev = g.debugAlias(w)
    a_orc, q_orc = orc.gen_alias_table(w)
    rep = old[:1].copy()
    rep["x"] = -7.0  # (decodes to no particle: slot 0 is recognisable)
    rep["yaw"] += 0.5
    for epoch in EPOCHS:
        for off, nl in shards:
            tag = (label, n, epoch, off, nl)
            want = orc.resample(cfg, old, a_dev, q_dev, rep, epoch, off, nl)
            got, mats = g.debugResamplePrefix(old, rep, epoch, off, nl, instance=1, want_mats=True)
            # (a)
            ig, iw = decode(got), decode(want)
            bad = np.flatnonzero(ig != iw)
            assert bad.size == 0, (tag, bad[:8], ig[bad[:8]], iw[bad[:8]])
            # (b)
            for k in KEYS:
                assert ulp_diff(got[k], want[k]).max() <= 1, (tag, k)
            assert (got.view(np.uint8) == want.view(np.uint8)).mean() > 0.999, tag
            np.testing.assert_array_equal(got["weight"].view(np.uint32), want["weight"].view(np.uint32))
            np.testing.assert_array_equal(got["w"].view(np.uint32), want["w"].view(np.uint32))
            if off == 0:
                assert got[0].tobytes() == rep[0].tobytes(), tag
            else:
                assert 0 <= ig[0] < n, tag  # an ordinary draw
            # (c)
            io = decode(orc.resample(cfg, old, a_orc, q_orc, rep, epoch, off, nl))
            diff = np.flatnonzero(ig != io)
            print("excused slots %s: %d" % (tag, diff.size))
            if diff.size:
                assert diff.size <= 2, tag
                np.testing.assert_array_equal(a_dev, a_orc)
                for li in diff:
                    u = orc.rng_uniform(SEED, off + int(li), 0, epoch, 1) * float(n)
                    k = int(u)
                    frac = u - k
                    assert min(q_dev[k], q_orc[k]) <= frac < max(q_dev[k], q_orc[k]), (tag, li, k, frac, q_dev[k], q_orc[k])
            # (d)
            got0, mats0 = g.debugResamplePrefix(old, rep, epoch, off, nl, instance=0, want_mats=True)
            got2, mats2 = g.debugResamplePrefix(old, rep, epoch, off, nl, instance=2, want_mats=True)
            assert got0.tobytes() == got.tobytes(), tag
            assert got2.tobytes() == got.tobytes(), tag
            assert mats2.tobytes() == mats.tobytes(), tag
            assert mats0.tobytes() == mats.tobytes(), tag
            assert g.debugPoseToMatrix(got).tobytes() == mats.tobytes(), tag


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 511, 513, 4097, 8192, 16385, 65536, 300000])
def test_product_resample_instances(gpu, orc, handles, n, order):
    rng = np.random.default_rng(n + 1)
    for label, w in AC.basic(n, rng):
        check_case(orc, handles[order], label, w, shards_of(n), n)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", [1024, 8192])
def test_product_resample_constructed_small_and_large_counts(gpu, orc, handles, n, order):
    """m resp. nh of 1, 255, 256, 257, 512, 513: s = 1 full, s = 1 -> 2 and 2 -> 3 with a ragged last block"""
    rng = np.random.default_rng(n + 2)
    for label, w in AC.constructed(n, rng):
        check_case(orc, handles[order], label, w, [(0, n)], n)


def test_fused_box_instance_needs_a_reference_cloud(gpu):
    from pcl_tracking_amd._lib import PftError

    g = gpu.make_reference_tracker(particle_num=64, seed=SEED)
    old = indexed_population(64, AC.uniform(64), 0)
    g.debugResamplePrefix(old, old[:1], 0, instance=1)
    with pytest.raises(PftError) as e:
        g.debugResamplePrefix(old, old[:1], 0, instance=2)
    assert e.value.status == 7  # PFT_ERR_STATE


# ---- KLD ---------------------------------------------------------------------------------------------------------
def realistic_population(n, seed, spread):
    """the population of test_gpu_kld.py: poses around the model's, realistic bins"""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    gt = scene.model_gt_pose()
    for k, name in enumerate(KEYS):
        p[name] = gt[k] + rng.normal(0, spread, n)
    p["w"] = 1.0
    w = rng.random(n).astype(np.float32) ** 4
    p["weight"] = w / w.sum()
    return p


def check_kld(gpu, orc, old, motion, maxn, order, tag):
    n_old = len(old)
    g = gpu.make_reference_tracker(particle_num=n_old, seed=11, kld=True, sum_order=order)
    g.setMaximumParticleNum(maxn)
    a_dev, q_dev = g.debugAlias(old["weight"])
    cfg = orc.default_config(kld_adaptive=1, seed=11, kld_max_particles=maxn)
    for epoch in EPOCHS:
        want, wbins, wk = orc.kld_resample(cfg, old, a_dev, q_dev, motion, epoch)
        got, gbins, gk = g.debugKldResample(old, None, None, motion, epoch)
        assert len(got) == len(want) and gk == wk, (tag, epoch, len(got), len(want), gk, wk)
        np.testing.assert_array_equal(gbins, wbins)
        for k in KEYS:
            assert np.abs(got[k] - want[k]).max() <= 1e-6, (tag, epoch, k)
        assert (got.view(np.uint8) == want.view(np.uint8)).mean() > 0.999, (tag, epoch)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n_old,maxn", [(1, 500), (2, 500), (37, 500), (255, 500), (256, 500), (257, 500), (500, 500),
                                        (400, 4000), (400, 16000), (3000, 4000), (3000, 16000)])
def test_product_kld_resample(gpu, orc, n_old, maxn, order):
    """maxn = 500: bin table and bins in LDS; 4 000 / 16 000: in HBM, and with n_old = 3 000 the coarse stride is >= 2.
    x = index and motion.x = 0: every candidate opens a bin of its own in x, k grows with n and the stop rule runs on"""
    rng = np.random.default_rng(n_old + maxn)
    motion = np.zeros(1, scene.PARTICLE_DTYPE)
    motion["yaw"] = -0.02
    for label, w in (("skewed", AC.skewed(n_old, rng)), ("single", AC.single_mass(n_old)), ("ties", AC.ties(n_old))):
        check_kld(gpu, orc, indexed_population(n_old, w, n_old), motion, maxn, order, (label, n_old, maxn))


@pytest.mark.parametrize("order", ORDERS)
def test_product_kld_resample_realistic_bins(gpu, orc, order):
    motion = np.zeros(1, scene.PARTICLE_DTYPE)
    motion["x"], motion["yaw"] = 0.004, -0.02
    for n_old, spread, maxn in ((400, 0.02, 500), (3000, 0.5, 16000)):
        check_kld(gpu, orc, realistic_population(n_old, n_old + maxn, spread), motion, maxn, order, ("population", n_old, maxn))


def test_kld_hook_wants_both_table_arrays_or_none(gpu):
    import ctypes as C

    g = gpu.make_reference_tracker(particle_num=16, seed=11, kld=True)
    old = indexed_population(16, AC.uniform(16), 0)
    g._ensure()
    out = np.zeros(500, scene.PARTICLE_DTYPE)
    motion = np.zeros(1, scene.PARTICLE_DTYPE)
    a = np.arange(16, dtype=np.int32)
    q = np.ones(16, np.float64)
    n = C.c_uint32()
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    for aa, qq in ((a, None), (None, q)):
        st = g._L.pft_debug_kld_resample(g._h, vp(old), 16, vp(aa), vp(qq), vp(motion), 0, vp(out), None, C.byref(n), None)
        assert st == 1  # PFT_ERR_INVALID_ARG

"""The wave reductions and scans of the small kernels (k_population, k_resample4<BOX>, k_aabb, k_crop_onepass,
k_crop_scatter) as DPP moves, and the population kernel's load chains (run with -m gpu).

The DPP helpers (pft_device_utils.h) must give the bytes the __shfl forms gave: the weight sum and the six weighted-pose
sums are adjacent-pair trees in double, min / max and the integer scans do not depend on the pairing.

Population: sizes around every wave / workgroup edge, the smallest n of each K > 1 instance (pftk_population: 128
workgroups of 256 threads hold K = 1 up to 32 768 particles), and five weight patterns; everything is compared with the
oracle WITHOUT tolerance, except the alias probabilities q, whose bar is test_alias_table's (the oracle updates q
sequentially, the kernel forms it from prefix sums).  The "spread" pattern has weights over 40 binades and pose
components that cancel pairwise across the halves of the population: its sums depend on the association in the bits
the float result keeps, which the test first asserts on the CPU (adjacent-pair tree against the sequential sum and
against the tree with the partner distances 32 .. 1 inside every block of 64) -- otherwise it could not fail.

Box and crop: particle and point counts that are no multiple of 64, NaN and infinite scene points, and workgroups
(1 024 input points each) that keep 0, 1, 63, 64, 65 and all of their points, against the oracle; the split paths
(PFT_SPLIT_RESAMPLE, PFT_CROP_TWO_PASS) use the same helpers and must agree with the default ones byte for byte.  (The
NaN points are scene points: a reference cloud must be finite -- a NaN query is outside k_likelihood's domain)
"""
import numpy as np
import pytest

from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu
KEYS = ("x", "y", "z", "roll", "pitch", "yaw")
K_EDGES = [32769, 65537, 131073, 262145]  # the smallest n of k_population<2>, <4>, <8>, <16>
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1024, 4097, 8192] + K_EDGES
ORDER_MIN_N = 63  # below this the three summation orders of the CPU check need not differ
NCHUNKS = [1, 8, 9, 11, 16, 17, 35]


@pytest.fixture(scope="module")
def g():
    from pcl_tracking_amd import tracker

    return tracker.make_reference_tracker(particle_num=64)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def weight_patterns(n, rng):
    """normalised float32 weights (the alias table's and the mean's input)"""
    out = {}
    w = rng.random(n).astype(np.float32) ** 4
    out["random"] = w / max(w.sum(), np.float32(1e-30))
    out["equal"] = np.full(n, np.float32(1) / np.float32(n), np.float32)
    w = out["random"].copy()
    drop = rng.random(n) < 0.3
    drop[np.argmax(w)] = False  # zeros MIXED IN: an all-zero population (n = 1) is no input of these stages
    w[drop] = 0
    out["zeros"] = w
    w = np.zeros(n, np.float32)
    w[(2 * n) // 3] = 1.0
    out["single"] = w
    out["spread"] = spread_weights(n, rng, rng.permutation(n // 2))
    return out


def spread_weights(n, rng, perm):
    """magnitudes 2^-e, e over 0 .. 40, full mantissas (the products with a pose component need 48 bits, so the double
    sums round at every level); particle h + perm[i] of the second half carries the weight of particle i of the first"""
    h = n // 2
    e = rng.uniform(0, 30, max(h, 1))
    tiny = rng.random(len(e)) < 0.125
    e[tiny] = rng.uniform(36, 40, int(tiny.sum()))
    wh = np.exp2(-e).astype(np.float32)
    w = np.full(n, np.float32(2.0 ** -38), np.float32)
    w[:h] = wh[:h]
    w[h + perm] = wh[:h]
    return w


def spread_population(n, rng):
    """weights over 40 binades; every particle of the first half has a partner in the second (a random pairing, so no
    block of the second half mirrors one of the first) with the same weight and the pose components negated where the
    weight is large (the products cancel exactly in exact arithmetic) or repeated where it is tiny: every partial sum
    is O(1), the result O(2^-36), so the rounding of each association shows in the float result"""
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    p["w"] = 1.0
    h = n // 2
    perm = rng.permutation(h)
    w = spread_weights(n, rng, perm)
    p["weight"] = w
    sign = np.where(w[:h] > 2.0 ** -33, np.float32(-1), np.float32(1))
    for k in KEYS:
        c = rng.normal(0, 1, n).astype(np.float32)
        c[h + perm] = sign * c[:h]
        p[k] = c
    return p


def tree_adjacent(x):
    x = np.asarray(x, np.float64)
    m = 1
    while m < len(x):
        m <<= 1
    x = np.concatenate([x, np.zeros(m - len(x))])
    while len(x) > 1:
        x = x[0::2] + x[1::2]
    return x[0]


def tree_far_first(x):
    """partner distance 32, 16, .. 1 inside every block of 64, adjacent pairs above"""
    x = np.asarray(x, np.float64)
    m = 64
    while m < len(x):
        m <<= 1
    x = np.concatenate([x, np.zeros(m - len(x))]).reshape(-1, 64)
    o = 32
    while o:
        x = x[:, :o] + x[:, o:2 * o]
        o >>= 1
    return tree_adjacent(x[:, 0])


def sequential(x):
    return np.cumsum(np.asarray(x, np.float64))[-1]


def random_population(n, rng, w):
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    gt = scene.model_gt_pose()
    for k, name in enumerate(KEYS):
        p[name] = gt[k] + rng.normal(0, 0.1, n)
    p["w"] = 1.0
    p["weight"] = w
    return p


def raw_patterns(n, rng):
    """raw likelihood weights (<= 0) for normalizeWeight"""
    out = {}
    out["random"] = (-rng.random(n) * 80 - 900).astype(np.float32)
    out["equal"] = np.full(n, -3.0, np.float32)  # wmax == wmin
    r = out["random"].copy()
    r[rng.random(n) < 0.3] = 0.0
    out["zeros"] = r
    r = np.zeros(n, np.float32)
    r[(2 * n) // 3] = -41.5
    out["single"] = r  # min == max over the non-zero weights
    out["spread"] = (-np.exp2(-np.floor(rng.uniform(0, 40, n)))).astype(np.float32)
    return out


# ---- the population kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_weighted_mean_is_the_adjacent_pair_tree(g, orc, n):
    rng = np.random.default_rng(1000 + n)
    cases = [(name, random_population(n, rng, w)) for name, w in weight_patterns(n, rng).items() if name != "spread"]
    sp = spread_population(n, rng)
    if n >= ORDER_MIN_N:
        # the CPU check: this input's result (six floats) tells the specified tree from the two other orders
        terms = [sp[k].astype(np.float64) * sp["weight"].astype(np.float64) for k in KEYS]
        t, s, f = ([np.float32(fn(x)) for x in terms] for fn in (tree_adjacent, sequential, tree_far_first))
        assert t != s and t != f, (n, t, s, f)
        assert t == [orc.weighted_mean_tree(sp)[k] for k in KEYS], n
    cases.append(("spread", sp))
    for name, p in cases:
        got, want = g.debugWeightedMean(p), orc.weighted_mean_tree(p)
        print(n, name, got, want)
        assert got.tobytes() == want.tobytes(), (n, name, got, want)


@pytest.mark.parametrize("n", SIZES)
def test_normalize_is_the_adjacent_pair_tree(g, orc, n):
    rng = np.random.default_rng(2000 + n)
    for name, raw in raw_patterns(n, rng).items():
        got, fg = g.debugNormalize(raw)
        want, fw = orc.normalize_weights_tree(raw)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        print(n, name, "fit", fg, fw, "differing weights", bad.size)
        assert fg == fw, (n, name)
        assert bad.size == 0, (n, name, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("n", SIZES)
def test_alias_lists_and_prefix_sums(g, orc, n):
    rng = np.random.default_rng(3000 + n)
    for name, w in weight_patterns(n, rng).items():
        a_w, q_w = orc.gen_alias_table(w)
        a_g, q_g = g.debugAlias(w)
        np.testing.assert_array_equal(a_g, a_w, err_msg="%d %s" % (n, name))
        # (test_alias_table's bar: prefix sums against the oracle's sequential updates of q)
        np.testing.assert_allclose(q_g, q_w, atol=1e-9 * max(1, n), rtol=0, err_msg="%d %s" % (n, name))


@pytest.mark.parametrize("nchunk", NCHUNKS)
def test_raw_weights_from_partial_rows(g, orc, nchunk):
    """from_partials: the raw weight is -(float) of the row's sum in chunk order (the loads go out in rounds of eight:
    one round, a full and a ragged one, two full ones, more), then normalizeWeight as above"""
    for n in (1, 65, 513, 8192):
        rng = np.random.default_rng(4000 + 64 * n + nchunk)
        rows = rng.normal(0, 1, (n, nchunk)) * np.exp2(rng.integers(-30, 8, (n, nchunk)))
        if nchunk > 2:  # the last chunk cancels the others up to 2^-40 of their sum: the order of the additions shows
            rows[:, -1] = -rows[:, :-1].cumsum(axis=1)[:, -1] * (1.0 + 2.0 ** -40 * rng.random(n))
        if n > 1:
            rows[rng.random(n) < 0.1] = 0.0  # particles without a match: raw weight zero
        v = np.zeros(n)
        for c in range(nchunk):
            v = v + rows[:, c]
        raw = -(v.astype(np.float32))
        if n >= 513 and nchunk > 2:  # (the CPU check: chunk order differs from the reversed order in the float)
            assert (raw != -(rows[:, ::-1].cumsum(axis=1)[:, -1].astype(np.float32))).mean() > 0.5
        got, fg = g.debugNormalizePartials(rows)
        want, fw = orc.normalize_weights_tree(raw)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        print(n, nchunk, "fit", fg, fw, "differing weights", bad.size)
        assert fg == fw, (n, nchunk)
        assert bad.size == 0, (n, nchunk, bad[:8], got[bad[:8]], want[bad[:8]])
        got2, fg2 = g.debugNormalize(raw)  # the other from_partials setting on the same raw weights
        assert fg2 == fg and got2.tobytes() == got.tobytes(), (n, nchunk)


# ---- resample on the prefix form, box, crop -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return scene.make_model(333, seed=7)  # (333 points: no multiple of 64)


def model_pose():
    return scene.model_gt_pose(M=333, seed=7)


def test_product_resample_on_the_prefix_form(orc, model):
    """the drawn indices of the four-lane instance (old[i].x = i) equal the oracle's on the table debugAlias materialises;
    the fused box instance returns the same particles and matrices"""
    from pcl_tracking_amd import tracker

    t = tracker.make_reference_tracker(particle_num=64, seed=5)
    t.setReferenceCloud(model)
    for n in (65, 257, 8192):
        rng = np.random.default_rng(5000 + n)
        w = weight_patterns(n, rng)["zeros"]
        old = random_population(n, rng, w)
        old["x"] = np.arange(n, dtype=np.float32)
        rep = old[:1].copy()
        rep["x"] = -7.0
        a_dev, q_dev = t.debugAlias(w)
        want = orc.resample(orc.default_config(particle_num=n, seed=5), old, a_dev, q_dev, rep, 3, 0, n)
        got, mats = t.debugResamplePrefix(old, rep, 3, 0, n, instance=1, want_mats=True)
        np.testing.assert_array_equal(np.rint(got["x"]).astype(np.int64), np.rint(want["x"]).astype(np.int64))
        got2, mats2 = t.debugResamplePrefix(old, rep, 3, 0, n, instance=2, want_mats=True)
        assert got2.tobytes() == got.tobytes() and mats2.tobytes() == mats.tobytes(), n


def make_tracker_pair(orc, model, cloud, P):
    from pcl_tracking_amd import tracker

    t = tracker.make_reference_tracker(particle_num=P, seed=1)
    o = orc.Tracker(orc.default_config(particle_num=P, seed=1, threads=0, emulate_pcl_alloc=0))
    for ref, tr, inp in ((t.setReferenceCloud, t.setTrans, t.setInputCloud), (o.set_reference, o.set_trans, o.set_input)):
        ref(model)
        tr(scene.initial_trans())
        inp(cloud)
    return t, o


def particles_around(pose, n, seed, sig_t=0.015, sig_r=0.09):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    for k, name in enumerate(KEYS):
        p[name] = pose[k] + rng.normal(0, sig_t if k < 3 else sig_r, n)
    p["w"] = 1.0
    p["weight"] = 1.0 / n
    return p


@pytest.mark.parametrize("two_pass", [False, True])
def test_box_and_crop_edges(orc, model, two_pass, monkeypatch):
    """97 particles x 333 points (k_aabb: ragged waves on both sides); a scene with NaN points whose workgroups keep
    0, 1, 63, 64, 65, all, 0 and 7 of their points (the last workgroup ragged)"""
    if two_pass:
        monkeypatch.setenv("PFT_CROP_TWO_PASS", "1")  # latched by pft_create: fresh handles below
    P = 97
    p = particles_around(model_pose(), P, 21)
    probe = scene.make_scene(2000)
    t, o = make_tracker_pair(orc, model, probe, P)
    mats = t.debugPoseToMatrix(p)
    G, O = t.evalWeights(p), o.eval_weights(p, mats=mats)
    np.testing.assert_array_equal(G["bbox"], O["bbox"].astype(np.float32))
    np.testing.assert_array_equal(G["crop_idx"], O["crop_idx"])
    box = G["bbox"].astype(np.float64)  # xmin, xmax, ymin, ymax, zmin, zmax
    assert (box[1::2] > box[0::2]).all()
    # the constructed scene: kept points lie inside the box, the others 10 m away or are NaN
    keep_per_wg = [0, 1, 63, 64, 65, 1024, 0, 7]
    N = 8 * 1024 - 300
    rng = np.random.default_rng(33)
    cloud = probe[rng.integers(0, len(probe), N)].copy()
    cloud["x"] = box[1] + 10.0 + rng.random(N)
    expect = []
    for b, cnt in enumerate(keep_per_wg):
        size = min(1024, N - 1024 * b)
        idx = 1024 * b + (np.sort(rng.choice(size, cnt, replace=False)) if cnt < size else np.arange(size))
        expect.append(idx)
    expect = np.concatenate(expect)
    for a, name in enumerate(("x", "y", "z")):
        cloud[name][expect] = rng.uniform(box[2 * a], box[2 * a + 1], len(expect)).astype(np.float32).clip(
            np.float32(box[2 * a]), np.float32(box[2 * a + 1]))
    out_idx = np.setdiff1d(np.arange(N), expect)
    nan_idx = rng.choice(out_idx, 200, replace=False)
    cloud["x"][nan_idx[:100]] = np.nan  # (outside points made non-finite: PassThrough drops them)
    cloud["z"][nan_idx[100:]] = np.inf
    t.setInputCloud(cloud)
    o.set_input(cloud)
    G, O = t.evalWeights(p), o.eval_weights(p, mats=mats)
    np.testing.assert_array_equal(G["bbox"], O["bbox"].astype(np.float32))
    np.testing.assert_array_equal(G["crop_idx"], expect)
    np.testing.assert_array_equal(G["crop_idx"], O["crop_idx"])


@pytest.mark.parametrize("P", [97, 1000])
def test_fused_box_with_ragged_waves_equals_the_split_path(model, P, monkeypatch):
    """k_resample4<BOX> (default) against k_resample4 + k_aabb (PFT_SPLIT_RESAMPLE=1) over three frames, for particle
    counts that leave the last wave and the last workgroup ragged: same box, crop and particles"""
    import ctypes as C
    from pcl_tracking_amd import tracker

    cloud = scene.make_scene(20000)
    runs = []
    for split in (False, True):
        monkeypatch.delenv("PFT_SPLIT_RESAMPLE", raising=False)
        if split:
            monkeypatch.setenv("PFT_SPLIT_RESAMPLE", "1")
        t = tracker.make_reference_tracker(particle_num=P, seed=3)
        t.setReferenceCloud(scene.make_model(2048))
        t.setTrans(scene.initial_trans())
        t.setInputCloud(cloud)
        frames = []
        for _ in range(3):
            t.compute()
            t.synchronize()
            bbox = np.zeros(6, np.float32)
            t._check(t._L.pft_debug_get_bbox(t._h, bbox.ctypes.data_as(C.c_void_p)))
            n = C.c_size_t()
            t._check(t._L.pft_debug_get_crop(t._h, None, 0, C.byref(n)))
            idx = np.zeros(n.value, np.int32)
            t._check(t._L.pft_debug_get_crop(t._h, idx.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
            frames.append((bbox, idx, t.getParticles().copy(), t.getResult().copy()))
        runs.append(frames)
    for (b0, i0, p0, r0), (b1, i1, p1, r1) in zip(*runs):
        np.testing.assert_array_equal(b0, b1)
        np.testing.assert_array_equal(i0, i1)
        assert p0.tobytes() == p1.tobytes() and r0.tobytes() == r1.tobytes()
        assert len(i0) > 100

"""GPU checks of the colour path (DistanceCoherence x HSVColorCoherence and the integer RGB2HSV behind it) term by term:
the crop kernels' conversion at every one of the 2^24 colours, k_pack_reference's float triples bit for bit, and the pair
value of each restatement (likelihood_items in both leaf-record forms and the DEBUG_NN instance, exact_pair_value through
the three exact search paths) on rigs where a particle's weight is ONE pair, so that a wrong term cannot hide in a sum.
The inputs are tests/colour_cases.py; tests/test_colour_cases_host.py proves on the CPU that they are what they claim.
mt_pair_value has its case in tests/test_gpu_match.py."""
import numpy as np
import pytest

import colour_cases as cc
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu

# name -> (environment latched at pft_create, exact search, ask for the NN arrays)
VARIANTS = {
    "product_leaf_direct": ({"PFT_LEAF_INDIRECT": "0"}, False, False),
    "product_leaf_indirect": ({"PFT_LEAF_INDIRECT": "1"}, False, False),
    "debug_nn": ({}, False, True),
    "exact_sorted": ({}, True, True),
    "exact_per_query": ({"PFT_EXACT_PER_QUERY": "1"}, True, True),
    "exact_shells": ({"PFT_EXACT_SHELLS_ONLY": "1"}, True, True),
}
PAIR_AMP = 0.01  # with seeds 0 .. 7: the rigs tests/test_colour_cases_host.py proves


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


def make_gpu(gpu, P, exact=False, max_distance=0.1, argorder=1, **w):
    g = gpu.ParticleFilterTracker(seed=1)
    g.setParticleNum(P)
    coh = gpu.NearestPairPointCloudCoherence() if exact else gpu.ApproxNearestPairPointCloudCoherence()
    coh.addPointCoherence(gpu.DistanceCoherence())
    hc = gpu.HSVColorCoherence()
    hc.setWeight(w.get("hsv_weight", 0.1))
    hc.setHWeight(w.get("h_weight", 1.0))
    hc.setSWeight(w.get("s_weight", 1.0))
    hc.setVWeight(w.get("v_weight", 0.0))
    coh.addPointCoherence(hc)
    coh.setSearchMethod(gpu.OctreeSearch(0.01))
    coh.setMaximumDistance(max_distance)
    g.setCloudCoherence(coh)
    g._cfg.hsv_pcl180_argorder = argorder
    g.setTrans(np.eye(4, dtype=np.float32))
    return g


def make_oracle(orc, P, exact=False, max_distance=0.1, argorder=1, **w):
    return orc.Tracker(orc.default_config(particle_num=P, threads=0, emulate_pcl_alloc=0, exact_nearest=int(exact),
                                          max_distance=max_distance, hsv_pcl180_argorder=argorder, **w))


def run_rig(g, o, rig, want_nn):
    p = rig["particles"]
    for ref, inp in ((g.setReferenceCloud, g.setInputCloud), (o.set_reference, o.set_input)):
        ref(rig["model"])
        inp(rig["cloud"])
    G = g.evalWeights(p, want_nn=want_nn)
    O = o.eval_weights(p, want_nn=True, mats=g.debugPoseToMatrix(p))  # the same matrices on both sides
    np.testing.assert_array_equal(G["crop_idx"], O["crop_idx"])
    return G, O


def check_neighbours(G, O, exact, gate):
    if exact:  # inside the gate: the same neighbour; outside: the device does not search
        inside = O["nn_d2"].astype(np.float64) < gate
        np.testing.assert_array_equal(G["nn_idx"][inside], O["nn_idx"][inside])
        np.testing.assert_array_equal(G["nn_d2"][inside], O["nn_d2"][inside])
        assert (G["nn_idx"][~inside] == -1).all()
    else:
        np.testing.assert_array_equal(G["nn_idx"], O["nn_idx"])
        np.testing.assert_array_equal(G["nn_d2"], O["nn_d2"])


# ---- a. the crop kernels' RGB2HSV at every colour -------------------------------------------------------------------------
CHUNK = 1 << 18
SLICES = 4  # per (argument order, crop form): 64 chunks of 2^18 colours in 4 tests of 16 chunks (measured: 0.13 s a test)


def lattice():
    """64^3 points at 1 cm pitch and the eight corners of their box grown by 0.3 m: an identity particle crops them all"""
    i = np.arange(64, dtype=np.float32)
    x, y, z = np.meshgrid((i - 32) * np.float32(0.01), (i - 32) * np.float32(0.01), 1 + i * np.float32(0.01), indexing="ij")
    xyz = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)
    lo, hi = xyz.min(0) - 0.3, xyz.max(0) + 0.3
    corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], np.float32)
    return scene.make_points(xyz, np.zeros((CHUNK, 3))), scene.make_points(corners, np.full((8, 3), 128))


@pytest.mark.parametrize("sl", range(SLICES))
@pytest.mark.parametrize("two_pass", [False, True], ids=["one_pass", "two_pass"])
@pytest.mark.parametrize("argorder", [1, 0])
def test_crop_conversion_at_every_colour(gpu, orc, monkeypatch, argorder, two_pass, sl):
    """k_crop_onepass, or k_crop_scatter under PFT_CROP_TWO_PASS=1: the packed h | s << 8 | v << 16 of every cropped point
    against the oracle, byte for byte, for the colours [sl, sl + 1) * 2^24 / SLICES with random alpha bytes"""
    if two_pass:
        monkeypatch.setenv("PFT_CROP_TWO_PASS", "1")
    cloud, model = lattice()
    g = make_gpu(gpu, 1, argorder=argorder)
    g.setReferenceCloud(model)
    cfg = orc.default_config(hsv_pcl180_argorder=argorder)
    p = np.zeros(1, scene.PARTICLE_DTYPE)
    p["w"], p["weight"] = 1.0, 1.0
    rng = np.random.default_rng(sl)
    per = (1 << 24) // CHUNK // SLICES
    for c in range(sl * per, (sl + 1) * per):
        cloud["rgba"] = np.arange(c * CHUNK, (c + 1) * CHUNK, dtype=np.uint32) | (rng.integers(0, 256, CHUNK).astype(np.uint32) << 24)
        g.setInputCloud(cloud)
        G = g.evalWeights(p)
        np.testing.assert_array_equal(G["crop_idx"], np.arange(CHUNK))
        got = g.debugGetTree()["crop_pts"][:, 3]
        want = orc.hsv_pack_many(cfg, cloud["rgba"])
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "chunk %d: %d colours differ, first rgba %#x: device %#x oracle %#x" % (
            c, len(bad), cloud["rgba"][bad[0]], got[bad[0]], want[bad[0]])
    g.close()


# ---- b. the reference side: k_pack_reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("argorder", [1, 0])
def test_reference_conversion(gpu, orc, argorder):
    """the float triples h / 180.0f, s / 255.0f, v / 255.0f: IEEE divisions on both sides, so the bits are equal"""
    g = make_gpu(gpu, 1, argorder=argorder)
    cfg = orc.default_config(hsv_pcl180_argorder=argorder)
    rng = np.random.default_rng(7)
    gb = np.arange(1 << 16, dtype=np.uint32)
    grey = np.arange(256, dtype=np.uint32) * np.uint32(0x010101)
    sets = dict(red255=np.uint32(0xff0000) | gb, greys=grey, edges=cc.rgba_of(cc.EDGES, 0),
                random=rng.integers(0, 1 << 24, 1 << 16).astype(np.uint32))
    for n in (1, 255, 256, 257):  # the tail workgroup of a 256-lane launch
        sets["n%d" % n] = rng.integers(0, 1 << 24, n).astype(np.uint32)
    for name, rgb in sets.items():
        pts = np.zeros(len(rgb), scene.POINT_DTYPE)
        pts["x"] = np.arange(len(rgb))
        pts["rgba"] = rgb | (rng.integers(0, 256, len(rgb)).astype(np.uint32) << 24)
        got = g.debugPackReference(pts)
        want = orc.hsv_floats_many(cfg, pts["rgba"])
        assert got[:, :3].tobytes() == want.tobytes(), name
        assert (got[:, 3] == 0).all(), name
    g.close()


def test_pack_reference_hook_leaves_the_reference_cloud_alone(gpu, orc):
    rig = cc.pair_rig(cc.refs()[1][5], cc.targets()[1], 0, PAIR_AMP)
    g, o = make_gpu(gpu, 256), make_oracle(orc, 256)
    before, _ = run_rig(g, o, rig, False)
    g.debugPackReference(rig["cloud"])
    after = g.evalWeights(rig["particles"])
    np.testing.assert_array_equal(before["raw"], after["raw"])
    g.close()


# ---- c. pair values, one term per particle --------------------------------------------------------------------------------
PASSES = [
    ("hsv4_hsv111", dict(hsv_weight=4.0, h_weight=1.0, s_weight=1.0, v_weight=1.0), None),
    ("hsv4_edges_weights", dict(hsv_weight=4.0, h_weight=0.5, s_weight=2.0, v_weight=1.0), len(cc.EDGES)),
    ("defaults", dict(), None),
]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_pair_value_one_term_per_particle(gpu, orc, monkeypatch, name):
    """every reference colour of REFS against the 256 TARGETS: A7's own criteria (within 1 float ulp, bit-equal for more than
    99 % of the particles) on a single pair value.  hsv_weight = 4 turns one hue step into many float ulps of the value.
    The device forms rcp(A * B) within 2 ulp(double) of PCL's two divisions, so a float that differs is a 2^-28 event"""
    env, exact, want_nn = VARIANTS[name]
    for k, v in env.items():  # the switches are latched at pft_create
        monkeypatch.setenv(k, v)
    _, rrgba = cc.refs()
    _, trgba = cc.targets()
    n_diff = n_all = 0
    for label, w, n_refs in PASSES:
        g, o = make_gpu(gpu, 256, exact=exact, **w), make_oracle(orc, 256, exact=exact, **w)
        for r, ref in enumerate(rrgba[:n_refs]):
            rig = cc.pair_rig(ref, trgba, r % 8, PAIR_AMP)
            G, O = run_rig(g, o, rig, want_nn)
            own = cc.own_paired(O) & (O["nn_d2"][:, 0].astype(np.float64) < 0.1 * 0.1)
            assert own.mean() >= (1.0 if exact else 0.90), (label, r)
            assert (O["raw"][own] != 0).all(), (label, r)
            if want_nn:
                check_neighbours(G, O, exact, 0.1 * 0.1)
            d = ulp_diff(G["raw"], O["raw"])
            assert d.max() <= 1, (label, r, int(d.max()), int(d.argmax()))
            assert (d == 0).mean() > 0.99, (label, r)
            n_diff, n_all = n_diff + int((d != 0).sum()), n_all + len(d)
            if exact:  # the instance without the NN arrays: the same bytes
                assert g.evalWeights(rig["particles"])["raw"].tobytes() == G["raw"].tobytes(), (label, r)
        g.close()
    print("%s: %d of %d pair values differ from the oracle's float" % (name, n_diff, n_all))
    assert n_diff <= 4, "float flips are 2^-28 events: more than a handful is a finding"


# ---- d. the gate at equality ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VARIANTS))
def test_gate_at_equality(gpu, orc, monkeypatch, name):
    """a squared distance equal to max_distance^2 is outside (PCL compares strictly); one float inside must survive the
    exact search's float pruning bounds; one float outside must not pair"""
    env, exact, want_nn = VARIANTS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rig = cc.gate_rig()
    kind = rig["kind"]
    g, o = make_gpu(gpu, 256, exact=exact, max_distance=0.125), make_oracle(orc, 256, exact=exact, max_distance=0.125)
    G, O = run_rig(g, o, rig, want_nn)
    own = cc.own_paired(O)
    for k in range(3):
        n = int((own & (kind == k)).sum())
        assert n == (kind == k).sum() if exact else n >= 50, (k, n)
    assert (O["nn_d2"][own & (kind == 0), 0] == np.float32(0.015625)).all()
    assert (O["raw"][own & (kind != 1)] == 0).all() and (O["raw"][own & (kind == 1)] != 0).all()
    zero = O["raw"] == 0
    assert G["raw"][zero].tobytes() == O["raw"][zero].tobytes()  # exactly zero on the device as well
    d = ulp_diff(G["raw"], O["raw"])
    assert d.max() <= 1, (int(d.max()), int(d.argmax()))
    if want_nn:
        check_neighbours(G, O, exact, 0.015625)
    if exact:
        assert (G["nn_idx"][kind != 1] == -1).all() and (G["nn_idx"][:, 1] == -1).all()
        np.testing.assert_array_equal(G["nn_idx"][kind == 1, 0], O["nn_idx"][kind == 1, 0])
        np.testing.assert_array_equal(g.evalWeights(rig["particles"])["raw"], G["raw"])
    g.close()

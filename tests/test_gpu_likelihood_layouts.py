"""Every LDS layout and descent branch of k_likelihood (pcl_tracking_amd/csrc/pft_likelihood.hip), each with both leaf-record
forms, built on purpose and compared with the CPU oracle pair by pair.

The kernel's DEBUG_NN instance records the branch it took (PftHeader::lik_layout, tracker.evalWeights()["lik_layout"]); each
case asserts that the record is the intended code and that tests/likelihood_layout_model.py predicts the same code from the
device's own tree sizes.  The inputs were found offline with the model on the oracle's trees (LDS of 80 KiB per workgroup,
the MI355X's 160 KiB / 2) and frozen here; test_layout_cases_select_their_codes_on_the_oracle re-checks that choice on the
CPU, and test_case_list_covers_every_reachable_code fails when the model gains a code that no case builds.
"""
import functools

import numpy as np
import pytest

from likelihood_layout_model import builder_jump_level, code, code_of_record, predict, reachable_codes
from pcl_tracking_amd import scene

LDS_BYTES_MI355X = 81920


def particles_around(pose, n, seed, sig_t=0.015, sig_r=0.09):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    for k, name in enumerate(("x", "y", "z")):
        p[name] = pose[k] + rng.normal(0, sig_t, n)
    for k, name in enumerate(("roll", "pitch", "yaw")):
        p[name] = pose[3 + k] + rng.normal(0, sig_r, n)
    p["w"] = 1.0
    p["weight"] = 1.0 / n
    return p


def scattered(n_loc, n_pts, span, seed):
    """n_pts points on n_loc random locations of a span^3 box (every location used; the rest repeat them: many points per
    leaf), and a 256-point model of some of these points plus the corners of the box grown by 0.3 m: particles near the
    identity crop the whole cloud"""
    rng = np.random.default_rng(seed)
    loc = rng.uniform(0, span, (n_loc, 3)) + np.array([-span / 2, -span / 2, 1.0])
    idx = np.concatenate([np.arange(n_loc), rng.integers(0, n_loc, n_pts - n_loc)])
    xyz = loc[idx].astype(np.float32)
    cloud = scene.make_points(xyz, rng.integers(0, 256, (n_pts, 3)))
    lo, hi = xyz.min(0) - 0.3, xyz.max(0) + 0.3
    corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], np.float32)
    mxyz = np.concatenate([xyz[rng.choice(n_pts, 248, replace=False)], corners])
    model = scene.make_points(mxyz, rng.integers(0, 256, (256, 3)))
    return model, cloud, particles_around(np.zeros(6), 16, seed, sig_t=0.002, sig_r=0.0005)


@functools.lru_cache(maxsize=None)
def _frames():
    return dict(model=scene.make_model(2048), scene=scene.make_scene(50000), gt=scene.model_gt_pose())


@functools.lru_cache(maxsize=None)
def _organized():
    return scene.make_scene(307200, mode="organized")


def scene_near():  # the tracking frame, particles near the object: a few thousand cropped points
    f = _frames()
    return f["model"], f["scene"], particles_around(f["gt"], 64, 21)


def scene_wide():  # particles spread over metres: 47 k cropped points, words beyond LDS
    f = _frames()
    return f["model"], f["scene"], particles_around(f["gt"], 128, 4, sig_t=0.6, sig_r=1.0)


def scene_branch_only():  # 5 mm leaves, depth 10: branch levels + jump table fit, the leaf starts do not
    f = _frames()
    gt, P, sig = f["gt"], 64, 0.18
    rng = np.random.default_rng(3)
    p = np.zeros(P, scene.PARTICLE_DTYPE)
    for k, name in enumerate(("x", "y", "z")):
        p[name] = gt[k] + rng.normal(0, sig, P)
    for k, name in enumerate(("roll", "pitch", "yaw")):
        p[name] = gt[3 + k] + rng.normal(0, sig, P)
    p["w"] = 1.0
    p["weight"] = 1.0 / P
    return f["model"], f["scene"], p


def organized_frame():  # 640 x 480 without downsampling: 112 k cropped points, many per leaf
    f = _frames()
    return f["model"], _organized(), particles_around(f["gt"], 64, 7, sig_t=0.1)


# name -> (inputs, octree resolution, fast descent allowed, layout, descent, jump table dropped)
CASES = {
    "u16_fast": (scene_near, 0.01, True, "u16_leaf_starts", "fast", False),
    "u16_table_generic": (scene_near, 0.01, False, "u16_leaf_starts", "table_generic", False),
    "u16_no_table": (lambda: scattered(1200, 1200, 10.0, 1), 0.01, True, "u16_leaf_starts", "no_table", False),
    "u16_fast_nojump": (lambda: scattered(2525, 2525, 2.5, 1), 0.01, True, "u16_leaf_starts", "fast", True),
    "u32_fast": (organized_frame, 0.01, True, "u32_words", "fast", False),
    "u32_table_generic": (organized_frame, 0.01, False, "u32_words", "table_generic", False),
    "u32_no_table": (lambda: scattered(1200, 70000, 10.0, 1), 0.01, True, "u32_words", "no_table", False),
    "u32_fast_nojump": (lambda: scattered(2000, 70000, 2.5, 1), 0.01, True, "u32_words", "fast", True),
    "branch_only_fast": (scene_branch_only, 0.005, True, "branch_only", "fast", False),
    "branch_only_table_generic": (scene_branch_only, 0.005, False, "branch_only", "table_generic", False),
    "hybrid_fast": (scene_wide, 0.01, True, "hybrid", "fast", False),
    "hybrid_table_generic": (scene_wide, 0.01, False, "hybrid", "table_generic", False),
    "hybrid_no_table": (lambda: scattered(3000, 3000, 10.0, 1), 0.01, True, "hybrid", "no_table", False),
}
# the whole cloud cropped, every point on 300 locations: the largest crop of the u16 leaf starts (sentinel 65 535) and the
# smallest of the u32 words
EDGES = {65535: "u16_leaf_starts", 65536: "u32_words"}


def case_codes():
    return {code(c[3], c[4], c[5], ind) for c in CASES.values() for ind in (False, True)}


def test_case_list_covers_every_reachable_code():
    assert case_codes() == reachable_codes()


def _oracle_tree(orc, model, cloud, p, res):
    o = orc.Tracker(orc.default_config(particle_num=len(p), seed=1, threads=0, emulate_pcl_alloc=0, octree_resolution=res))
    o.set_reference(model)
    o.set_trans(scene.initial_trans())
    o.set_input(cloud)
    crop = o.eval_weights(p)["crop_idx"]
    info = orc.Octree(np.ascontiguousarray(cloud)[crop], resolution=res).info()
    return len(crop), info


@pytest.mark.parametrize("name", sorted(CASES))
def test_layout_cases_select_their_codes_on_the_oracle(orc, name):
    """the frozen inputs still give their code with the oracle's trees (MI355X LDS size): no GPU needed"""
    inputs, res, fast, layout, descent, dropped = CASES[name]
    n_crop, info = _oracle_tree(orc, *inputs(), res)
    got = predict(info["depth"], n_crop, info["leaves"], info["branches"] + info["leaves"] + 1, LDS_BYTES_MI355X, fast)
    assert code(got["layout"], got["descent"], got["jump_dropped"], False) == code(layout, descent, dropped, False), got


@pytest.mark.parametrize("n", sorted(EDGES))
def test_u16_leaf_start_edges_on_the_oracle(orc, n):
    n_crop, info = _oracle_tree(orc, *scattered(300, n, 0.5, 2), 0.01)
    assert n_crop == n
    got = predict(info["depth"], n_crop, info["leaves"], info["branches"] + info["leaves"] + 1, LDS_BYTES_MI355X)
    assert (got["layout"], got["descent"]) == (EDGES[n], "fast")


# ---- on the device --------------------------------------------------------------------------------------------------
def make_pair(orc, model, cloud, P, res):
    from pcl_tracking_amd import tracker as gpu

    g = gpu.make_reference_tracker(particle_num=P, seed=1)
    coh = gpu.ApproxNearestPairPointCloudCoherence()
    coh.addPointCoherence(gpu.DistanceCoherence())
    hc = gpu.HSVColorCoherence()
    hc.setWeight(0.1)
    coh.addPointCoherence(hc)
    coh.setSearchMethod(gpu.OctreeSearch(res))
    coh.setMaximumDistance(0.1)
    g.setCloudCoherence(coh)
    o = orc.Tracker(orc.default_config(particle_num=P, seed=1, threads=0, emulate_pcl_alloc=0, octree_resolution=res))
    for ref, tr, inp in ((g.setReferenceCloud, g.setTrans, g.setInputCloud), (o.set_reference, o.set_trans, o.set_input)):
        ref(model)
        tr(scene.initial_trans())
        inp(cloud)
    return g, o


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def run_and_check(orc, model, cloud, p, res, fast, indirect, monkeypatch):
    """one DEBUG_NN evaluation against the oracle (tests/test_gpu_parity.py check_eval's bars), the product instance
    against it, and the descent statistics against the recorded descent; returns (record, device result)"""
    import ctypes as C

    monkeypatch.setenv("PFT_LEAF_INDIRECT", "1" if indirect else "0")
    monkeypatch.setenv("PFT_GENERIC_DESCENT", "0" if fast else "1")
    g, o = make_pair(orc, model, cloud, len(p), res)
    G = g.evalWeights(p, want_nn=True)
    dbg = np.zeros(32, np.uint64)
    g._check(g._L.pft_debug_get_descent_stats(g._h, dbg.ctypes.data_as(C.c_void_p)))
    hard = np.zeros(5, np.uint64)
    g._check(g._L.pft_debug_get_hard_steps(g._h, hard.ctypes.data_as(C.c_void_p)))
    O = o.eval_weights(p, want_nn=True, mats=g.debugPoseToMatrix(p))
    np.testing.assert_array_equal(G["bbox"], O["bbox"].astype(np.float32))
    np.testing.assert_array_equal(G["crop_idx"], O["crop_idx"])
    assert len(G["crop_idx"]) > 0
    assert G["octree_depth"] == O["octree_depth"]
    np.testing.assert_array_equal(G["octree_min"], O["octree_min"])
    np.testing.assert_array_equal(G["octree_max"], O["octree_max"])
    ot = orc.Octree(np.ascontiguousarray(cloud)[O["crop_idx"]], resolution=res)
    np.testing.assert_array_equal(G["point_keys"], ot.point_keys())
    assert G["n_leaves"] == ot.info()["leaves"]
    np.testing.assert_array_equal(G["nn_idx"], O["nn_idx"])
    np.testing.assert_array_equal(G["nn_d2"].view(np.uint32), O["nn_d2"].view(np.uint32))
    assert G["scan_queries"] == O["scan_queries"] and G["scan_points"] == O["scan_points"]
    d = ulp_diff(G["raw"], O["raw"])
    assert d.max() <= 1, d.max()
    assert (d == 0).mean() > 0.99
    rec = G["lik_layout"]
    assert rec["valid"] and rec["indirect"] == rec["leaf_indirect"] == indirect, rec
    # the kernel's choice equals the model's prediction from the device's own header sizes
    D = G["octree_depth"]
    want = predict(D, len(G["crop_idx"]), G["n_leaves"], G["n_words"], rec["lds_bytes"], fast, rec["margin_cells"])
    assert code_of_record(rec) == code(want["layout"], want["descent"], want["jump_dropped"], indirect), (rec, want)
    assert (rec["J"], rec["n_lds_words"]) == (want["J"], want["n_lds_words"]), (rec, want)
    # the jump table is used exactly when the fast descent has one
    if rec["descent"] == "fast" and rec["J"] > 0:
        assert dbg[11] > 0
    else:
        assert dbg[11] == 0
    if rec["descent"] != "fast":
        assert dbg[14] == 0  # no fast level anywhere
    # every query lands in one bucket of the generic-level histogram and one of the hard-step histogram (which used to share
    # dbg[27..31] with the box's point counts and lose two buckets to them)
    assert dbg[0:11].sum() == hard.sum() == G["scan_queries"], (dbg, hard)
    assert not dbg[27:30].any() and dbg[30] <= dbg[31] == len(model), dbg  # [30], [31]: the box's reference points
    # the product instance (no NN arrays) takes the same branch: raw weights bit for bit
    R = g.evalWeights(p, want_nn=False)
    np.testing.assert_array_equal(R["raw"].view(np.uint32), G["raw"].view(np.uint32))
    assert not R["lik_layout"]["valid"]  # only the DEBUG_NN instance records
    return rec, G


@pytest.mark.gpu
@pytest.mark.parametrize("indirect", [False, True], ids=["direct", "indirect"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_layout_case_against_the_oracle(orc, name, indirect, monkeypatch):
    inputs, res, fast, layout, descent, dropped = CASES[name]
    model, cloud, p = inputs()
    rec, G = run_and_check(orc, model, cloud, p, res, fast, indirect, monkeypatch)
    assert code_of_record(rec) == code(layout, descent, dropped, indirect), rec
    if dropped:
        assert builder_jump_level(G["octree_depth"]) > 0 and rec["J"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("indirect", [False, True], ids=["direct", "indirect"])
@pytest.mark.parametrize("n", sorted(EDGES))
def test_u16_leaf_start_edges_against_the_oracle(orc, n, indirect, monkeypatch):
    model, cloud, p = scattered(300, n, 0.5, 2)
    rec, G = run_and_check(orc, model, cloud, p, 0.01, True, indirect, monkeypatch)
    assert len(G["crop_idx"]) == n
    assert (rec["layout"], rec["descent"]) == (EDGES[n], "fast"), rec
    assert len(np.unique(G["nn_idx"])) > 100


@pytest.mark.gpu
def test_switches_are_latched_per_handle(orc, monkeypatch):
    """a handle keeps the descent and leaf-record form of the environment it was created in: handle A (generic descent,
    copied records) evaluates again after the switches were cleared and handle B (the defaults) was created"""
    inputs, res = CASES["u16_fast"][:2]
    model, cloud, p = inputs()
    monkeypatch.setenv("PFT_GENERIC_DESCENT", "1")
    monkeypatch.setenv("PFT_LEAF_INDIRECT", "0")
    a, _ = make_pair(orc, model, cloud, len(p), res)
    monkeypatch.delenv("PFT_GENERIC_DESCENT")
    monkeypatch.delenv("PFT_LEAF_INDIRECT")
    b, _ = make_pair(orc, model, cloud, len(p), res)
    runs = [(t, t.evalWeights(p, want_nn=True)) for t in (a, b, a)]
    for t, G in runs:
        rec = G["lik_layout"]
        want = ("table_generic", False) if t is a else ("fast", True)
        assert rec["valid"] and (rec["descent"], rec["indirect"]) == want, rec
    raw = [G["raw"].view(np.uint32) for _, G in runs]
    np.testing.assert_array_equal(raw[0], raw[1])
    np.testing.assert_array_equal(raw[0], raw[2])

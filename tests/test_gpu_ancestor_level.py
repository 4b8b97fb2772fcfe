"""The level of k_likelihood's ancestor table, chosen per build (pcl_tracking_amd/csrc/pft_frame.hip pick_anc_up).

The table of a tree of depth D lies at level D - 1 where that window fits its 2^18 entries, else at D - 2, else there is none;
the host picks the level from the window sizes the PREVIOUS build published, hands it to the builder and launches the
likelihood instance compiled for it (ANC_UP 1, 2, or 0: no table code).  The level decides time only: every weight is the
same bytes at every level, a wrong guess included, and the table is the deepest existing ancestor of each of its cells.
PFT_ANC_UP_FORCE=0|1|2 fixes the request of a handle.  pft_eval_weights never asks for D - 1 by itself (its DEBUG_NN form has
the D - 2 code only), so the choice itself is exercised through compute().
"""
import ctypes as C
import functools

import numpy as np
import pytest

from pcl_tracking_amd import scene
from test_gpu_likelihood_layouts import CASES, _frames, make_pair, particles_around

CAP_BITS = 18
CAP = 1 << CAP_BITS
RES = 0.01


def anc_table(g):
    info = np.zeros(10, np.uint32)
    tab = np.zeros(CAP, np.uint32)
    g._check(g._L.pft_debug_get_ancestor_table(g._h, info.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p), CAP))
    n = 1 << int(info[5:8].sum()) if info[1] else 0
    return info, tab[:n]


# ---- inputs whose tree and window the oracle alone fixes ---------------------------------------------------------------
def lattice(n, ext, seed):
    """n[0] x n[1] x n[2] isolated points over ext metres (spacing far above the 1 cm leaves).  The minimum corner comes
    first and the maximum corner second: PCL's box then grows upwards on the longest axis only (a shorter axis is lowered by
    the last doubling), the tree's minimum there is one cell below the first point and its depth is
    ceil(log2((max(ext) + res) / res)) -- checked against the oracle by the tests"""
    n, ext = np.asarray(n), np.asarray(ext, np.float64)
    g = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    rest = rng.permutation(np.arange(1, len(g) - 1))
    g = g[np.concatenate([[0, len(g) - 1], rest])]
    xyz = (g * (ext / (n - 1)) + np.array([-0.4, -0.3, 1.0])).astype(np.float32)
    return scene.make_points(xyz, rng.integers(0, 256, (len(xyz), 3)))


def blob(n_pts, side, seed):
    """n_pts points in a cube of `side` metres (many per leaf), corners first: a shallow tree under a crop large enough for
    the gather launch"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0.0, side, (n_pts, 3))
    xyz[0], xyz[1] = 0.0, side
    xyz = (xyz + np.array([-0.05, -0.05, 1.0])).astype(np.float32)
    return scene.make_points(xyz, rng.integers(0, 256, (n_pts, 3)))


def box_model(cloud, margin, seed):
    """248 points of the cloud and the corners of its box grown by `margin`: particles near the identity crop the whole
    cloud, and the crop box ends `margin` beyond it on every side"""
    rng = np.random.default_rng(seed)
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
    lo, hi = xyz.min(0) - margin, xyz.max(0) + margin
    corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], np.float32)
    mxyz = np.concatenate([xyz[rng.choice(len(xyz), 248, replace=False)], corners])
    return scene.make_points(mxyz, rng.integers(0, 256, (256, 3)))


def gather_crop():
    """the tracking frame with 64 particles spread widely enough around the object for the gather launch: 6 055 cropped
    points, depth 9, the u16-leaf-start layout with the fast descent, a D - 2 window of 32^3 cells (the D - 1 window fits the
    table exactly)"""
    f = _frames()
    return f["model"], f["scene"], particles_around(f["gt"], 64, 21, sig_t=0.18)


LEVEL_CASES = dict(CASES, gather_crop=(gather_crop, 0.01, True, "u16_leaf_starts", "fast", False))


def near_identity(n, seed):
    return particles_around(np.zeros(6), n, seed, sig_t=0.002, sig_r=0.0005)


# the three crops of the cap boundary: (lattice points per axis, extent, crop margin) -> depth, log2 cells of the D - 2 window.
# The window is the crop box cut to the tree's box, in level D - 2 cells of 4 cm, rounded up to a power of two per axis; the
# D - 1 window has 8 cells for each.
#   fits_d1: depth 7, the whole tree: 32^3 -> 2^15, at D - 1 exactly 2^18
#   fits_d2: depth 8 (the last doubling lowers the tree's y and z minimum by 1.28 m); x 0 .. 1.76 m = cells 0 .. 44 -> 64,
#            y and z 1.14 .. 2.34 m = cells 28 .. 58 -> 32: 2^16, at D - 1 2^19 (one doubling more)
#   over:    depth 9, 0 .. 3.31 m = 83 cells -> 128 per axis: 2^21 at D - 2 already
BOUNDARY = {
    "fits_d1": ((18, 18, 18), (1.0, 1.0, 1.0), 0.3, 7, 15),
    "fits_d2": ((22, 16, 16), (1.6, 0.9, 0.9), 0.15, 8, 16),
    "over": ((18, 18, 18), (3.0, 3.0, 3.0), 0.3, 9, 21),
}


@functools.lru_cache(maxsize=None)
def boundary_cloud(name):
    n, ext = BOUNDARY[name][:2]
    return lattice(n, ext, 5)


def oracle_depth(orc, cloud):
    return orc.Octree(cloud, resolution=RES).info()["depth"]


def restate_window_bits(depth, omin, bbox):
    """pft_anc_window's sizes from the tree's depth and minimum and the crop box: log2 cells at D - 2, per axis"""
    L2 = depth - 2
    bits = []
    for a in range(3):
        om, inv = np.float32(omin[a]), np.float32(1.0 / RES)
        f0 = max(float(np.floor((np.float32(bbox[2 * a]) - om) * inv)), 0.0)
        f1 = max(float(np.floor((np.float32(bbox[2 * a + 1]) - om) * inv)), 0.0)
        top = (1 << L2) - 1
        c0, c1 = min(int(f0) >> 2, top), min(int(f1) >> 2, top)
        n = c1 - c0 + 1
        bits.append(int(n - 1).bit_length() if n > 1 else 0)
    return bits


# ---- the table against the linearised tree ----------------------------------------------------------------------------
def restate_from_tree(tree, info):
    """for every window cell (x fastest) the walk from the root along the cell's key over the node words read back from the
    device: the deepest existing ancestor at a level <= L, as (level << 27) | node"""
    L = int(info[1])
    lo, bits = info[2:5].astype(np.int64), info[5:8].astype(np.int64)
    c = np.arange(1 << int(bits.sum()), dtype=np.int64)
    x = lo[0] + (c & ((1 << bits[0]) - 1))
    y = lo[1] + ((c >> bits[0]) & ((1 << bits[1]) - 1))
    z = lo[2] + (c >> (bits[0] + bits[1]))
    words = tree["words"].astype(np.int64)
    node = np.zeros(len(c), np.int64)
    lvl = np.zeros(len(c), np.int64)
    alive = np.ones(len(c), bool)
    for l in range(L):
        sh = L - l - 1
        ch = (((x >> sh) & 1) << 2) | (((y >> sh) & 1) << 1) | ((z >> sh) & 1)
        w = words[node]
        ex = alive & (((w >> ch) & 1) == 1)
        below = w & 0xFF & ((1 << ch) - 1)
        pop = np.zeros(len(c), np.int64)
        for b in range(8):
            pop += (below >> b) & 1
        node = np.where(ex, (w >> 8) + pop, node)
        lvl = np.where(ex, l + 1, lvl)
        alive = ex
    return ((lvl << 27) | node).astype(np.uint32), (x, y, z)


def forced_handle(orc, model, cloud, p, res, fast, monkeypatch, table="1", force=None):
    """a fresh handle with direct leaf records, evaluated twice: the first build sizes the second (the table is filled behind
    builds of more than 5 000 points)"""
    monkeypatch.setenv("PFT_ANCESTOR_TABLE", table)
    if force is None:
        monkeypatch.delenv("PFT_ANC_UP_FORCE", raising=False)
    else:
        monkeypatch.setenv("PFT_ANC_UP_FORCE", str(force))
    monkeypatch.setenv("PFT_LEAF_INDIRECT", "0")
    monkeypatch.setenv("PFT_GENERIC_DESCENT", "0" if fast else "1")
    g, _ = make_pair(orc, model, cloud, len(p), res)
    g.evalWeights(p, want_nn=False)
    R = g.evalWeights(p, want_nn=False)
    return g, R


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LEVEL_CASES))
def test_weights_are_the_same_bytes_at_every_level(orc, name, monkeypatch):
    inputs, res, fast, layout, descent, _ = LEVEL_CASES[name]
    model, cloud, p = inputs()
    carries = layout == "u16_leaf_starts" and descent == "fast"
    g0, R0 = forced_handle(orc, model, cloud, p, res, fast, monkeypatch, table="0")
    assert g0.debugAncestorLevel()["instance"] == 0 and anc_table(g0)[0][0] == 0
    ref = R0["raw"].view(np.uint32)
    D, n_crop = R0["octree_depth"], len(R0["crop_idx"])
    if name == "gather_crop":  # the one case of the list whose tables are filled
        assert n_crop > 5000 and D in (8, 9), (n_crop, D)
    if carries:  # every level asked for by force; a table where the gather launch follows the build
        for force in (0, 1, 2):
            g, R = forced_handle(orc, model, cloud, p, res, fast, monkeypatch, force=force)
            np.testing.assert_array_equal(R["raw"].view(np.uint32), ref)
            info, _ = anc_table(g)
            lv = g.debugAncestorLevel()
            filled = force > 0 and n_crop > 5000
            assert lv["instance"] == lv["anc_up"] == (force if n_crop > 5000 else 0), (lv, n_crop)
            assert info[0] == (1 if filled else 0) and info[1] == (D - force if filled else 0), (info, D, force)
    else:  # no table possible: left to itself the handle launches the instance without table code
        g, R = forced_handle(orc, model, cloud, p, res, fast, monkeypatch)
        np.testing.assert_array_equal(R["raw"].view(np.uint32), ref)
        if layout in ("hybrid", "u32_words") or descent == "no_table":
            lv = g.debugAncestorLevel()
            assert lv["instance"] == 0 and lv["anc_up"] == 0 and anc_table(g)[0][0] == 0, lv


def content_inputs(which):
    if which == "tracking_frame":  # a crop of the tracking frame: a few thousand points, depth 9
        return gather_crop() + (RES,)
    if which == "odd_window":
        # depth 6 (0.64 m box); the crop box ends 0.57 m above the tree's minimum: cells 0 .. 28 at D - 1 (29 of them) and
        # 0 .. 14 at D - 2 (15), odd on every axis -- the last D - 1 pair and the last parent are half / partly outside
        cloud = lattice((18, 18, 18), (0.5, 0.5, 0.5), 6)
        return box_model(cloud, 0.06, 7), cloud, near_identity(16, 8), RES
    cloud = blob(6000, 0.14, 9)  # depth 4: the jump table (J = D - 1 = 3) reaches the level of the D - 1 table
    return box_model(cloud, 0.3, 10), cloud, near_identity(16, 11), RES


@pytest.mark.gpu
@pytest.mark.parametrize("force", [1, 2])
@pytest.mark.parametrize("which", ["tracking_frame", "odd_window", "depth4"])
def test_table_is_the_deepest_existing_ancestor_at_both_levels(orc, which, force, monkeypatch):
    model, cloud, p, res = content_inputs(which)
    g, R = forced_handle(orc, model, cloud, p, res, True, monkeypatch, force=force)
    D = R["octree_depth"]
    assert len(R["crop_idx"]) > 5000
    tree = g.debugGetTree()
    info, tab = anc_table(g)
    assert info[0] == 1 and info[1] == D - force and info[8] == info[9], (info, D)
    if which == "depth4":
        assert D == 4 and tree["jump_level"] == 3, (D, tree["jump_level"])
    if which == "odd_window":
        assert D == 6 == oracle_depth(orc, cloud)
        for a in range(3):
            end = int(np.floor((np.float32(R["bbox"][2 * a + 1]) - np.float32(R["octree_min"][a])) * np.float32(1.0 / res)))
            assert (end >> 1) + 1 == 29 and (end >> 2) + 1 == 15, (a, end)
    if force == 1:  # whole parent cells from an even first cell: the paired stores are aligned and stay inside the window
        assert (info[2:5] % 2 == 0).all() and (info[5:8] >= 1).all(), info
    want, (x, y, z) = restate_from_tree(tree, info)
    np.testing.assert_array_equal(tab, want)
    assert int(info[5:8].sum()) <= CAP_BITS and (np.array([x.max(), y.max(), z.max()]) < (1 << int(info[1]))).all()


# ---- the choice itself: compute() on handles left to themselves ------------------------------------------------------
def same(a, b):
    pa, pb = np.ascontiguousarray(a.getParticles()), np.ascontiguousarray(b.getParticles())
    assert pa.tobytes() == pb.tobytes()


def tracking_pair(P, model, cloud, monkeypatch, graph=False):
    """two trackers on the same inputs, the second without a table; a population that stays put (the crop box is the
    model's box), direct leaf records"""
    from pcl_tracking_amd import tracker

    out = []
    for table in ("1", "0"):
        monkeypatch.setenv("PFT_ANCESTOR_TABLE", table)
        monkeypatch.setenv("PFT_LEAF_INDIRECT", "0")
        monkeypatch.setenv("PFT_GRAPH", "1" if graph else "0")
        monkeypatch.delenv("PFT_ANC_UP_FORCE", raising=False)
        t = tracker.make_reference_tracker(particle_num=P, seed=3)
        t.setStepNoiseCovariance([1.0e-8] * 6)
        t.setReferenceCloud(model)
        t.setTrans(np.eye(4, dtype=np.float32))
        t.setInputCloud(cloud)
        out.append(t)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_cap_boundary(orc, name, monkeypatch):
    margin, depth, bits_d2 = BOUNDARY[name][2:]
    cloud = boundary_cloud(name)
    assert oracle_depth(orc, cloud) == depth
    on, off = tracking_pair(64, box_model(cloud, margin, 12), cloud, monkeypatch)
    for _ in range(7):  # (D - 1 is asked for once eight builds in a row, two per frame, have seen its window fit)
        on.compute()
        off.compute()
        same(on, off)
    lv = on.debugAncestorLevel()
    info, _ = anc_table(on)
    assert (lv["bits_d1"], lv["bits_d2"]) == (bits_d2 + 3, bits_d2), lv
    up = 1 if bits_d2 + 3 <= CAP_BITS else 2 if bits_d2 <= CAP_BITS else 0
    assert lv["anc_up"] == lv["instance"] == up, lv
    assert info[0] == (1 if up else 0) and info[1] == (depth - up if up else 0), (info, depth, up)
    if up:
        assert int(info[5:8].sum()) == (bits_d2 + 3 if up == 1 else bits_d2)
    assert off.debugAncestorLevel()["instance"] == 0
    # the published sizes are pft_anc_window's of this tree and crop box, and the weights are the table-less handle's
    p = on.getParticles()
    Ron, Roff = on.evalWeights(p), off.evalWeights(p)
    assert sum(restate_window_bits(Ron["octree_depth"], Ron["octree_min"], Ron["bbox"])) == bits_d2
    np.testing.assert_array_equal(Ron["raw"].view(np.uint32), Roff["raw"].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_level_follows_the_window_over_frames(graph, monkeypatch):
    """the input grows past the D - 1 cap and shrinks back: the level goes 1 -> 2 -> 1, the frame after each change runs on a
    guess that does not fit its tree, and every frame equals the handle's without a table; a PFT_GRAPH=1 handle instantiates
    its graph anew when the likelihood instance changes"""
    small, large = boundary_cloud("fits_d1"), boundary_cloud("fits_d2")
    on, off = tracking_pair(256, box_model(large, 0.15, 13), small, monkeypatch, graph=graph)
    levels, builds = [], []
    for f in range(21):  # (seven frames per phase: D - 1 wants eight builds in a row, two per frame, with a fitting window)
        cloud = large if 7 <= f < 14 else small
        for t in (on, off):
            t.setInputCloud(cloud)
            t.compute()
        same(on, off)
        lv = on.debugAncestorLevel()
        levels.append(lv["anc_up"])
        builds.append(lv["graph_builds"])
    runs = [levels[0]] + [b for a, b in zip(levels, levels[1:]) if a != b]
    assert runs[-3:] == [1, 2, 1] and set(runs[:-3]) <= {0, 2}, levels
    assert levels[6] == 1 and levels[13] == 2 and levels[20] == 1, levels
    assert on.debugAncestorLevel()["changes"] >= 2
    if graph:
        assert builds[6] >= 1 and builds[13] > builds[6] and builds[20] > builds[13], builds
    else:
        assert builds[-1] == 0

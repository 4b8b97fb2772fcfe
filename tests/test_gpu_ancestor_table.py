"""The ancestor table of k_likelihood's fast descent (PFT_ANCESTOR_TABLE, pcl_tracking_amd/csrc/pft_likelihood.hip).

For a query whose leaf cell is k, the fast descent ends at the deepest existing ancestor of k at a level <= lim.  After a
build of the single-workgroup builder whose leaf records k_leaf_gather copies, that launch also tabulates, for every level
L = depth - 2 cell of a window over the crop box, the deepest existing ancestor at a level <= L; the kernel starts the
descent there.  Results with and without the table must be bit-identical, and the table must be what it says it is.
"""
import ctypes as C

import numpy as np
import pytest

from pcl_tracking_amd import scene
from test_gpu_likelihood_layouts import CASES, make_pair, particles_around

CAP = 1 << 18


def anc_table(g):
    info = np.zeros(10, np.uint32)
    tab = np.zeros(CAP, np.uint32)
    g._check(g._L.pft_debug_get_ancestor_table(g._h, info.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p), CAP))
    n = 1 << int(info[5:8].sum()) if info[1] else 0
    return info, tab[:n]


def eval_case(orc, name, table, indirect, monkeypatch):
    """the layout case evaluated three times on a fresh handle: the first build sizes the next one (the table is filled
    behind builds of more than 5 000 points), then DEBUG_NN and the product instance"""
    inputs, res, fast = CASES[name][:3]
    model, cloud, p = inputs()
    monkeypatch.setenv("PFT_ANCESTOR_TABLE", "1" if table else "0")
    monkeypatch.setenv("PFT_LEAF_INDIRECT", "1" if indirect else "0")
    monkeypatch.setenv("PFT_GENERIC_DESCENT", "0" if fast else "1")
    g, _ = make_pair(orc, model, cloud, len(p), res)
    g.evalWeights(p, want_nn=False)
    G = g.evalWeights(p, want_nn=True)
    R = g.evalWeights(p, want_nn=False)
    info, tab = anc_table(g)
    return G, R, info, tab


def restate(keys, depth, info):
    """numpy restatement: for every window cell (x fastest), the deepest level a <= L at which the cell's ancestor holds a
    point of the crop"""
    L = int(info[1])
    lo, bits = info[2:5].astype(np.int64), info[5:8].astype(np.int64)
    c = np.arange(1 << int(bits.sum()), dtype=np.int64)
    x = lo[0] + (c & ((1 << bits[0]) - 1))
    y = lo[1] + ((c >> bits[0]) & ((1 << bits[1]) - 1))
    z = lo[2] + (c >> (bits[0] + bits[1]))
    k = keys.reshape(-1, 3).astype(np.int64)
    a = np.zeros(len(c), np.int64)
    for lvl in range(1, L + 1):
        s = depth - lvl
        occ = np.unique((k[:, 0] >> s) | ((k[:, 1] >> s) << 21) | ((k[:, 2] >> s) << 42))
        t = L - lvl
        a = np.where(np.isin((x >> t) | ((y >> t) << 21) | ((z >> t) << 42), occ), lvl, a)
    return a, (x, y, z)


def check_table(G, info, tab):
    D = G["octree_depth"]
    assert info[0] == 1 and info[1] == D - 2 and info[8] == info[9], info
    a, (x, y, z) = restate(G["point_keys"], D, info)
    np.testing.assert_array_equal(tab >> 27, a)
    node = tab & 0x7FFFFFF
    assert (node[a == 0] == 0).all()
    for lvl in np.unique(a):  # one node per existing ancestor cell, a different one for every other cell
        m = a == lvl
        t = int(info[1]) - int(lvl)
        cell = (x[m] >> t) | ((y[m] >> t) << 21) | ((z[m] >> t) << 42)
        pairs = np.unique(np.stack([cell, node[m].astype(np.int64)]), axis=1)
        assert len(np.unique(pairs[0])) == len(np.unique(pairs[1])) == pairs.shape[1]


@pytest.mark.gpu
@pytest.mark.parametrize("indirect", [False, True], ids=["direct", "indirect"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_table_on_and_off_are_bit_identical(orc, name, indirect, monkeypatch):
    G1, R1, info1, tab1 = eval_case(orc, name, True, indirect, monkeypatch)
    G0, R0, info0, _ = eval_case(orc, name, False, indirect, monkeypatch)
    assert info0[1] == 0 and info0[0] == 0  # no table on the handle created with PFT_ANCESTOR_TABLE=0
    np.testing.assert_array_equal(G1["nn_idx"], G0["nn_idx"])
    np.testing.assert_array_equal(G1["nn_d2"].view(np.uint32), G0["nn_d2"].view(np.uint32))
    np.testing.assert_array_equal(G1["raw"].view(np.uint32), G0["raw"].view(np.uint32))
    np.testing.assert_array_equal(R1["raw"].view(np.uint32), R0["raw"].view(np.uint32))
    np.testing.assert_array_equal(R1["raw"].view(np.uint32), G1["raw"].view(np.uint32))
    if info1[0]:  # filled for this tree: it is the restatement's
        assert not indirect and len(G1["crop_idx"]) > 5000
        check_table(G1, info1, tab1)
    if indirect:  # the indirect form's builds fill no table
        assert info1[0] == 0


def same(a, b):
    pa, pb = np.ascontiguousarray(a.getParticles()), np.ascontiguousarray(b.getParticles())
    assert pa.tobytes() == pb.tobytes()


def tracking_pair(P, monkeypatch, **env):
    from pcl_tracking_amd import tracker

    out = []
    for table in ("1", "0"):
        monkeypatch.setenv("PFT_ANCESTOR_TABLE", table)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        t = tracker.make_reference_tracker(particle_num=P, seed=3)
        t.setReferenceCloud(scene.make_model(2048))
        t.setTrans(scene.initial_trans())
        t.setInputCloud(scene.make_scene(50000))
        out.append(t)
    return out


@pytest.mark.gpu
def test_table_of_the_tracking_frame_is_the_deepest_existing_ancestor(monkeypatch):
    """the steady-state tracking frame (crop of several thousand points): the table after a build equals the restatement
    from the crop's keys, the descent with it is bit-identical to the one without, and it takes fewer fast trips"""
    on, off = tracking_pair(2048, monkeypatch, PFT_LEAF_INDIRECT="0")
    for _ in range(20):
        on.compute()
        off.compute()
    same(on, off)
    p = on.getParticles()
    stats = []
    for t in (on, off):
        t.evalWeights(p, want_nn=False)
        G = t.evalWeights(p, want_nn=True)
        dbg = np.zeros(32, np.uint64)
        t._check(t._L.pft_debug_get_descent_stats(t._h, dbg.ctypes.data_as(C.c_void_p)))
        stats.append((G, dbg, anc_table(t)))
    (G1, d1, (info, tab)), (G0, d0, _) = stats
    assert len(G1["crop_idx"]) > 5000, len(G1["crop_idx"])
    check_table(G1, info, tab)
    np.testing.assert_array_equal(G1["nn_idx"], G0["nn_idx"])
    np.testing.assert_array_equal(G1["nn_d2"].view(np.uint32), G0["nn_d2"].view(np.uint32))
    np.testing.assert_array_equal(G1["raw"].view(np.uint32), G0["raw"].view(np.uint32))
    # per wave iteration: the worst lane's fast trips (dbg[14]: their sum) -- at most two from an entry of level L
    assert d1[14] < 0.75 * d0[14], (d1[12:16], d0[12:16])
    # only the queries outside the window or near a face still take the jump table
    assert d1[11] < d0[11]


@pytest.mark.gpu
def test_stale_tables_are_not_used(monkeypatch):
    """builds that fill no table leave a table of an earlier tree behind: an evalWeights of other particles between the
    frames of a running handle, the sorted builder with too few radix passes (the rescue launch rebuilds), change-detector
    frames -- every frame equals the handle's without a table, bit for bit"""
    on, off = tracking_pair(2048, monkeypatch, PFT_LEAF_INDIRECT="0")
    q = particles_around(scene.model_gt_pose(), 64, 9)
    for f in range(12):
        for t in (on, off):
            t.compute()
            if f % 3 == 1:
                t.evalWeights(q, want_nn=False)  # a tree of other particles, and a table of its own or none
        same(on, off)

    on, off = tracking_pair(2048, monkeypatch, PFT_FORCE_BUILDER="sorted", PFT_LEAF_INDIRECT="0")
    for t in (on, off):
        t._check(t._L.pft_debug_set_limits(t._h, 0, 1))  # one radix pass: the rescue launch rebuilds every tree
    for f in range(6):
        on.compute()
        off.compute()
        same(on, off)
    info, _ = anc_table(on)
    assert info[0] == 0 and info[1] == 0  # the sorted builder and its rescue fill no table

    on, off = tracking_pair(2048, monkeypatch, PFT_LEAF_INDIRECT="0")
    for t in (on, off):
        t.setUseChangeDetector(True)
        t.setMinPointsOfChangeDetection(10)
        t.setIntervalOfChangeDetection(2)
    for f in range(10):
        on.compute()
        off.compute()
        same(on, off)

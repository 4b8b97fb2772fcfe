"""tests/octree_model.py against hand-derived trees and against the CPU oracle's keys, and the proof that its checks have
teeth: every listed corruption of a model tree is caught.  No GPU: tests/test_gpu_octree_structure.py holds the device's
trees against the same model."""
import time

import numpy as np
import pytest

import octree_model as om
from pcl_tracking_amd import scene


def check_known(depth, keys, words, lvl_start, leaf_order, jump_entries):
    t = om.linearise(depth, np.array(keys, np.uint32))
    assert t["words"].tolist() == words
    assert t["lvl_start"].tolist() == lvl_start
    assert t["leaf_order"].tolist() == leaf_order
    assert (t["leaf_start"], t["n_leaves"], t["n_words"]) == (lvl_start[-2], lvl_start[-1] - lvl_start[-2], len(words))
    J = om.jump_level(depth)
    assert t["jump_level"] == J and len(t["jump"]) == (8 ** J if J else 0)
    assert {int(i): int(t["jump"][i]) for i in np.flatnonzero(t["jump"])} == jump_entries
    assert t["use_table"] == 1
    got = om.walk(t["words"], t["lvl_start"], depth, t["leaf_order"], len(keys))
    assert got == om.key_groups(keys)
    return t


# ---- hand-derived known answers ------------------------------------------------------------------------------------------
def test_known_one_point():
    # key (1, 0, 1): child 1 << 2 | 0 << 1 | 1 = 5; root = bit 5 | first child 1 << 8
    check_known(1, [[1, 0, 1]], [0x120, 0, 1], [0, 1, 2], [0], {})


def test_known_two_points_in_one_leaf():
    check_known(1, [[0, 0, 0], [0, 0, 0]], [0x101, 0, 2], [0, 1, 2], [0, 1], {})


def test_known_eight_children_inserted_in_reverse():
    keys = [[c >> 2, (c >> 1) & 1, c & 1] for c in range(7, -1, -1)]
    check_known(1, keys, [0x1FF, 0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 1, 9], [7, 6, 5, 4, 3, 2, 1, 0], {})


def test_known_depth_4_three_points():
    # insertion order B = (15, 15, 15) digits 7777, A = (0, 0, 0) digits 0000, C = (15, 15, 14) digits 7776
    words = [0x181,            # root: children 0 and 7, first child at 1
             0x301, 0x480,     # level 1: node 0 -> child 0 at 3; node 7 -> child 7 at 4
             0x501, 0x680,     # level 2
             0x701, 0x8C0,     # level 3: 000 -> leaf 0000 at 7; 777 -> leaves 7776, 7777 at 8
             0, 1, 2,          # leaves in Morton order: A, C, B
             3]                # sentinel
    check_known(4, [[15, 15, 15], [0, 0, 0], [15, 15, 14]], words, [0, 1, 3, 5, 7, 10], [1, 2, 0],
                {0: 1, 7 | 7 << 3 | 7 << 6: 2})  # J = 3: level-3 cells (0, 0, 0) and (7, 7, 7)


def test_known_depth_5_jump_entries():
    # digits (level 1 first): P0 = (31, 0, 0) 44444, P1 = (0, 0, 1) 00001, P2 = (0, 0, 0) 00000, P3 = (0, 2, 0) 00020
    words = [0x111,
             0x301, 0x410,
             0x501, 0x610,
             0x705, 0x910,           # 000 -> children 0 and 2 at 7; 444 -> child 4 at 9
             0xA03, 0xC01, 0xD10,    # 0000 -> leaves 0, 1 at 10; 0002 -> leaf 0 at 12; 4444 -> leaf 4 at 13
             0, 1, 2, 3,
             4]
    # J = 4: level-4 cells of the keys >> 1: (0, 0, 0) -> 1, (0, 1, 0) -> 2 at index 1 << 4, (15, 0, 0) -> 3 at index 15
    check_known(5, [[31, 0, 0], [0, 0, 1], [0, 0, 0], [0, 2, 0]], words, [0, 1, 3, 5, 7, 10, 14], [2, 1, 3, 0],
                {0: 1, 16: 2, 15: 3})


def test_jump_level_and_table_rule():
    assert [om.jump_level(d) for d in range(1, 13)] == [0, 0, 0, 3, 4, 4, 4, 4, 4, 4, 0, 0]
    k = np.array([[0, 0, 0], [2047, 5, 9]], np.uint32)
    assert om.linearise(10, k % 1024)["use_table"] == 1 and om.linearise(11, k)["use_table"] == 0
    assert len(om.linearise(11, k)["jump"]) == 0


def test_header_floats_formula():
    # res 0.01, depth 6, box reaching 2 m: eta = 2 * 2^-23, s_top = 0.32; E = 9 eta + 40 * 2^-24 * 0.32
    m, inv, omin = om.header_floats(6, 0.01, [-2.0, 0.5, 1.0], [-1.36, 1.14, 1.64])
    E = 9 * 2.0 * 2.0 ** -23 + 40 * 2.0 ** -24 * 0.32
    assert np.array([m], np.uint32).view(np.float32)[0] == np.float32(2 * E / 0.01 + 1e-3)
    assert np.array([inv], np.uint32).view(np.float32)[0] == np.float32(100.0)
    assert omin.view(np.float32).tolist() == [-2.0, 0.5, 1.0]
    # a margin of a quarter cell or more switches the fast descent off: the field holds 1
    m, _, _ = om.header_floats(10, 0.0001, [5000.0] * 3, [5000.1] * 3)
    assert np.array([m], np.uint32).view(np.float32)[0] == np.float32(1.0)


# ---- the model against the oracle -----------------------------------------------------------------------------------------
def _cloud(xyz):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return scene.make_points(xyz, np.full((len(xyz), 3), 90, np.uint8))


def _clouds():
    rng = np.random.default_rng(12)
    out = {"scene_40000": scene.make_scene(50000)[:40000], "scene_1": scene.make_scene(50000)[:1]}
    for n in (2, 65, 3000):
        out["uniform_%d" % n] = _cloud(rng.uniform(-0.4, 0.4, (n, 3)) + [0, 0, 1.0])
    centres = rng.uniform(-1.0, 1.0, (30, 3))
    cl = centres[rng.integers(0, 30, 5000)] + rng.normal(0, 0.004, (5000, 3))
    cl[rng.integers(0, 5000, 1500)] = cl[17]  # duplicates of one point among the others
    out["clustered_duplicates_5000"] = _cloud(cl)
    out["lattice_on_cell_faces_4096"] = _cloud(np.stack(np.meshgrid(*[np.arange(16) * 0.01] * 3), -1).reshape(-1, 3)[rng.permutation(4096)])
    out["far_from_origin_2000"] = _cloud(rng.uniform(0, 0.6, (2000, 3)) + [40.0, -40.0, 40.0])
    return out


CLOUDS = _clouds()


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_model_against_the_oracle(orc, name):
    cloud = CLOUDS[name]
    ot = orc.Octree(cloud)
    info, keys = ot.info(), ot.point_keys()
    D, n = info["depth"], len(cloud)
    t0 = time.perf_counter()
    t = om.linearise(D, keys, 0.01, info["min"], info["max"])
    groups = om.walk(t["words"], t["lvl_start"], D, t["leaf_order"], n)
    dt = time.perf_counter() - t0
    assert dt < 1.0, "linearise + walk of %d points took %.2f s" % (n, dt)
    # exactly the groups of equal oracle keys, each in ascending insertion index
    assert groups == om.key_groups(keys)
    assert t["n_leaves"] == info["leaves"] == len(groups)
    assert t["n_words"] == info["branches"] + info["leaves"] + 1
    # every point's own key leads from the root to the leaf that lists it
    node, lvl = om.descend_all(t["words"], D, keys)
    assert (lvl == D).all()
    s, e = t["words"][node].astype(np.int64), t["words"][node + 1].astype(np.int64)
    pos = np.empty(n, np.int64)
    pos[t["leaf_order"]] = np.arange(n)
    assert ((s <= pos) & (pos < e)).all()
    # every level-J cell: the jump entry is the integer descent's node (0 where the descent stops early)
    J = t["jump_level"]
    assert J == om.jump_level(D)
    if J:
        idx = np.arange(8 ** J)
        cells = np.stack([idx & ((1 << J) - 1), (idx >> J) & ((1 << J) - 1), idx >> (2 * J)], 1)
        node, lvl = om.descend_all(t["words"], J, cells)
        want = np.where(lvl == J, node - int(t["lvl_start"][J]) + 1, 0)
        assert (t["jump"].astype(np.int64) == want).all()
        assert np.count_nonzero(t["jump"]) == t["lvl_start"][J + 1] - t["lvl_start"][J]


# ---- teeth ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_tree(orc):
    cloud = CLOUDS["clustered_duplicates_5000"]
    ot = orc.Octree(cloud)
    D, keys = ot.info()["depth"], ot.point_keys()
    return D, keys, om.linearise(D, keys)


def _caught(D, keys, t, words=None, leaf_order=None, jump=None):
    """True when walk, the comparison of its groups with the keys', or the equality against linearise fails"""
    words = t["words"] if words is None else words
    leaf_order = t["leaf_order"] if leaf_order is None else leaf_order
    jump = t["jump"] if jump is None else jump
    try:
        walked = om.walk(words, t["lvl_start"], D, leaf_order, len(keys)) == om.key_groups(keys)
    except (AssertionError, IndexError):
        walked = False
    equal = (words == t["words"]).all() and (leaf_order == t["leaf_order"]).all() and (jump == t["jump"]).all()
    return not walked, not equal


def test_teeth_intact_tree_passes(model_tree):
    assert _caught(*model_tree) == (False, False)


def test_teeth_mask_bit_flipped(model_tree):
    D, keys, t = model_tree
    for node in (0, int(t["lvl_start"][3]) + 1, int(t["leaf_start"]) - 1):
        for bit in (0, 7):
            w = t["words"].copy()
            w[node] ^= np.uint32(1 << bit)
            assert _caught(D, keys, t, words=w) == (True, True), (node, bit)


def test_teeth_child_base_off_by_one(model_tree):
    D, keys, t = model_tree
    for node in (0, int(t["lvl_start"][4]), int(t["leaf_start"]) - 1):
        for d in (1, -1):
            w = t["words"].copy()
            w[node] = np.uint32(int(w[node]) + (d << 8))
            assert _caught(D, keys, t, words=w) == (True, True), (node, d)


def test_teeth_leaf_order_swapped_inside_a_leaf(model_tree):
    D, keys, t = model_tree
    starts = t["words"][t["leaf_start"]:]
    leaf = int(np.argmax(np.diff(starts.astype(np.int64)) >= 2))
    s = int(starts[leaf])
    lo = t["leaf_order"].copy()
    lo[[s, s + 1]] = lo[[s + 1, s]]
    assert _caught(D, keys, t, leaf_order=lo) == (True, True)


def test_teeth_two_leaf_starts_swapped(model_tree):
    D, keys, t = model_tree
    w = t["words"].copy()
    a = int(t["leaf_start"]) + 5
    w[[a, a + 1]] = w[[a + 1, a]]
    assert _caught(D, keys, t, words=w) == (True, True)


def test_teeth_sentinel_changed(model_tree):
    D, keys, t = model_tree
    for d in (1, -1):
        w = t["words"].copy()
        w[-1] = np.uint32(int(w[-1]) + d)
        assert _caught(D, keys, t, words=w) == (True, True)


def test_teeth_jump_entries(model_tree):
    D, keys, t = model_tree
    assert t["jump_level"] == 4
    occupied, empty = np.flatnonzero(t["jump"]), np.flatnonzero(t["jump"] == 0)
    for i, v in ((occupied[0], 0), (occupied[-1], 0), (empty[0], 1), (empty[-1], int(t["jump"].max()))):
        j = t["jump"].copy()
        j[i] = v
        assert _caught(D, keys, t, jump=j) == (False, True)  # (the walk does not read the table: the equality does)


def test_teeth_level_not_in_morton_order(model_tree):
    """two nodes of a level exchanged together with their parents' bases (their own words, so their subtrees, move with
    them): still a well-formed tree with the right groups -- walk passes -- but the level is no longer in Morton order,
    and the equality against linearise fails"""
    D, keys, t = model_tree
    l = 5
    assert D > l
    w = t["words"].copy()
    parents = range(int(t["lvl_start"][l - 1]), int(t["lvl_start"][l]))
    single = [p for p in parents if bin(int(w[p]) & 0xff).count("1") == 1]
    p, q = single[0], single[-1]
    assert p != q
    cp, cq = int(w[p]) >> 8, int(w[q]) >> 8
    w[[cp, cq]] = w[[cq, cp]]
    w[p] = np.uint32((int(w[p]) & 0xff) | cq << 8)
    w[q] = np.uint32((int(w[q]) & 0xff) | cp << 8)
    assert _caught(D, keys, t, words=w) == (False, True)


# ---- predict_variant at each threshold ------------------------------------------------------------------------------------
LDS = 153600  # bytes k_octree_build is launched with on an MI355X: (160 KiB - 10 KiB) & ~15


def _pv(n, depth=8, n_words=None, expected=None, forced="single", indirect=False, **kw):
    n_words = n // 4 + 16 if n_words is None else n_words
    return om.decode_variant(om.predict_variant(n, depth, n_words, LDS, n if expected is None else expected, forced, indirect, **kw))


def test_predict_variant_store_steps():
    want = {1: 1, 4095: 1, 4096: 1, 4097: 2, 8191: 2, 8192: 2, 8193: 3, 14335: 3, 14336: 3, 14337: 4, 18431: 4, 18432: 4,
            18433: 5, 40000: 5}
    assert {n: _pv(n)["store"] for n in want} == want
    for n in (100, 5000, 10000, 16000):  # 21-bit keys whatever the size
        assert _pv(n, depth=10)["store"] != 5 and _pv(n, depth=11)["store"] == 5
    assert [_pv(100, depth=d)["dense_top"] for d in (3, 4, 10, 11)] == [False, True, True, False]


def test_predict_variant_carve():
    n_fit = (LDS // 4 - 64) * 2 // 5
    while (n_fit + 1) * 5 // 2 + 64 <= LDS // 4:
        n_fit += 1
    assert n_fit * 5 // 2 + 64 <= LDS // 4 < (n_fit + 1) * 5 // 2 + 64 and n_fit == 15334
    assert [_pv(n)["tmp_lds"] for n in (n_fit - 1, n_fit, n_fit + 1)] == [True, True, False]
    assert all(_pv(n)["words_lds"] and not _pv(n)["lds_abandoned"] for n in (n_fit - 1, n_fit, n_fit + 1))


def test_predict_variant_lds_fallback():
    n = 6000
    cap = LDS // 4 - ((n + 3) & ~3)
    for n_words, fits in ((cap - 2, True), (cap - 1, True), (cap, False), (cap + 1, False)):  # the last level's end + 2 <= cap
        v = _pv(n, n_words=n_words)
        assert (v["words_lds"], v["tmp_lds"], v["lds_abandoned"]) == (fits, fits, not fits), n_words
    n = 16000  # past the carve: the node words have all of LDS
    for n_words, fits in ((LDS // 4 - 1, True), (LDS // 4, False)):
        v = _pv(n, n_words=n_words)
        assert (v["words_lds"], v["tmp_lds"], v["lds_abandoned"]) == (fits, False, not fits), n_words


def test_predict_variant_leaf_modes():
    assert [_pv(3000, expected=e)["leaf_mode"] for e in (0, 4999, 5000, 5001)] == [1, 1, 1, 0]
    assert [_pv(3000, expected=e, indirect=True)["leaf_mode"] for e in (0, 5000, 5001)] == [2, 2, 2]


def test_predict_variant_builder_choice_and_passes():
    assert [_pv(100, expected=e, forced=None)["store"] for e in (17999, 18000, 18001)] == [1, 1, 6]
    assert _pv(100, expected=0, forced="sorted") == dict(store=6, words_lds=False, tmp_lds=False, lds_abandoned=False,
                                                         dense_top=False, rescue=False, leaf_mode=0, npass=4)
    # passes from the previous depth: ceil(3 (d + 1) / 8), all eight when it is unknown
    assert [om.sorted_npass(d) for d in (0, 1, 4, 5, 7, 8, 9, 10, 12, 20, 30)] == [8, 1, 2, 3, 3, 4, 4, 5, 5, 8, 8]
    assert _pv(100, depth=9, forced="sorted", last_depth=0)["npass"] == 8
    # too few passes for the depth (3 D > 8 npass): the rescue launch builds, always with the builder's own leaf copy
    assert _pv(100, depth=8, forced="sorted", forced_npass=3)["store"] == 6
    v = _pv(5000, depth=8, forced="sorted", forced_npass=1, indirect=True, expected=20000)
    assert (v["store"], v["rescue"], v["leaf_mode"], v["words_lds"], v["dense_top"]) == (2, True, 1, True, True)
    assert _pv(100, depth=3, forced="sorted", forced_npass=1)["rescue"] is True
    assert _pv(100, depth=2, forced="sorted", forced_npass=1)["rescue"] is False

"""The constructions of tests/search_cases.py, proved on the CPU with the oracle alone: every declared tie between children is
bit-equal when mt_min_child's arithmetic is recomputed in numpy (and is met at the declared node and level of a descent
recomputed from the oracle's keys), the oracle takes the lower child at the tie and the other child one float step above it,
each gate pair straddles its g*g, the crop of every pose is the whole cloud, and the case list holds what the GPU tests rely
on.  A construction whose precondition fails is a failing test, never a skip."""
import numpy as np
import pytest

import search_cases as sc

F = np.float32


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sc.all_cases()}


@pytest.fixture(scope="module")
def oracle_eval(orc, cases):
    """case name -> the oracle's search of every pose of the case (computed once)"""
    out = {}

    def get(name):
        if name not in out:
            c = cases[name]
            o = orc.Tracker(orc.default_config(particle_num=len(c.poses), seed=1, threads=0, emulate_pcl_alloc=0,
                                               octree_resolution=c.resolution))
            o.set_reference(c.model)
            o.set_trans(np.eye(4, dtype=F))
            o.set_input(c.cloud)
            out[name] = o.eval_weights(sc.particles_of(c.poses), want_nn=True, mats=c.matrices())
        return out[name]

    return get


def descent(keys, omin, res, D, q):
    """mt_search's descent in numpy over the tree the oracle's point keys imply (a child exists iff a record's key starts
    with it): double centre, cast to float, float difference, float square, X + (Y + Z), the first existing child and later
    ones when strictly smaller, the minimum child's key handed down.  -> [(level, parent key, mask, dc[8], chosen)]"""
    q = np.asarray(q, F)
    k, steps = [0, 0, 0], []
    for lvl in range(D):
        shift = D - lvl - 1
        vs = float(res) * float(1 << shift)
        sq = []
        for a in range(3):
            c0 = F((float(2 * k[a]) + 0.5) * vs + float(omin[a]))
            c1 = F((float(2 * k[a] + 1) + 0.5) * vs + float(omin[a]))
            d0, d1 = F(c0 - q[a]), F(c1 - q[a])
            sq.append((F(d0 * d0), F(d1 * d1)))
        dc = np.array([F(sq[0][(c >> 2) & 1] + F(sq[1][(c >> 1) & 1] + sq[2][c & 1])) for c in range(8)], F)
        under = ((keys >> (shift + 1)) == np.array(k, np.uint32)).all(axis=1)
        child = (keys[under] >> shift) & 1
        mask = 0
        for x, y, z in child:
            mask |= 1 << int(4 * x + 2 * y + z)
        bc, best = None, None
        for c in range(8):
            if (mask >> c) & 1 and (bc is None or dc[c] < best):
                bc, best = c, dc[c]
        steps.append((lvl, tuple(k), mask, dc, bc))
        k = [2 * k[a] + ((bc >> (2 - a)) & 1) for a in range(3)]
    return steps


def test_the_case_list_holds_what_the_gpu_tests_rely_on(cases):
    assert tuple(cases) == sc.CASE_NAMES
    for c in cases.values():
        assert 64 <= len(c.model) <= 256 and len(c.cloud) <= 5001 and 2 <= len(c.poses) <= 16, c.name
        assert c.poses[c.expect_pose] == c.shift and len(set(c.poses)) == len(c.poses)
        assert np.isfinite(c.queries()).all() and all(np.isfinite(c.cloud[f]).all() for f in "xyz")
    d = cases["descent"]
    assert d.resolution == 2.0 ** -7
    single = {(t["axes"][0], t["level"]) for t in d.ties if len(t["axes"]) == 1}
    assert single >= {(a, j) for a in range(3) for j in (1, 2, 3)}, "three axes times child sides 2, 4 and 8 cells"
    assert {len(t["tied"]) for t in d.ties} >= {2, 4, 7, 8}
    assert {(a, s) for _, a, s in d.outside} == {(a, s) for a in range(3) for s in (-1, 1)}
    assert len(d.only_farther) == 1
    assert [g for _, g in sc.GATES] == [0.1, 0.02, 0.05]
    assert {(n, inside) for _, _, n, _, inside in cases["gates"].gate} == {(n, i) for n, _ in sc.GATES for i in (True, False)}
    assert any(c.leaf_ties for c in cases.values()) and any(not c.whole_crop for c in cases.values())
    assert {len(c.cloud) for c in cases.values()} >= {1, 5000, 5001}


def test_every_declared_tie_is_bit_equal_in_the_kernels_arithmetic(orc, cases):
    c = cases["descent"]
    tree = orc.Octree(c.cloud, c.resolution)
    info, keys = tree.info(), tree.point_keys()
    assert info["depth"] == c.depth == 6 and info["min"].tobytes() == c.omin.tobytes()
    assert (keys[0] == 0).all() and (keys[1] == 63).all()
    Q = c.queries()
    for t in c.ties:
        lvl = c.depth - t["level"] - 1  # the level whose children have side 2^level cells
        parent = tuple(int(v) >> (t["level"] + 1) for v in keys[t["tied"][0]])
        exist = 0
        for ch in t["children"]:
            exist |= 1 << ch
        for qi, what in ((t["query"], "tie"), (t["up"], "up"), (t["down"], "down")):
            step = descent(keys, info["min"], c.resolution, c.depth, Q[qi])[lvl]
            assert step[1] == parent and step[2] == exist, (t["name"], what, "the descent meets the declared node")
            dc = step[3][t["children"]]
            if what == "tie":
                assert len(set(v.tobytes() for v in dc)) == 1, (t["name"], dc)
                assert step[4] == t["children"][0]
            elif what == "up":  # strictly the closest: the highest child
                assert (dc[-1] < dc[:-1]).all() and step[4] == t["children"][-1], (t["name"], dc)
            elif t["children"][0] == 0:
                assert (dc[0] < dc[1:]).all() and step[4] == 0, (t["name"], dc)
        # the record behind the later child is the nearer one: taking it at equality shows in the index and the distance
        xyz = np.stack([c.cloud[f] for f in "xyz"], 1)
        assert sc.d2_of(xyz[t["winner_up"]], Q[t["query"]]) < sc.d2_of(xyz[t["winner"]], Q[t["query"]])


def test_the_numpy_descent_is_the_oracles(orc, cases, oracle_eval):
    """the restatement above reaches the leaf of the record the oracle reports, for every query of the two 2^-7 / 0.01
    constructed clouds: what the tie proof rests on"""
    for name in ("descent", "gates"):
        c = cases[name]
        tree = orc.Octree(c.cloud, c.resolution)
        info, keys = tree.info(), tree.point_keys()
        O = oracle_eval(name)
        Q = c.queries()
        for qi in range(len(Q)):
            steps = descent(keys, info["min"], c.resolution, info["depth"], Q[qi])
            leaf = [2 * steps[-1][1][a] + ((steps[-1][4] >> (2 - a)) & 1) for a in range(3)]
            assert keys[O["nn_idx"][c.expect_pose, qi]].tolist() == leaf, (name, qi)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_the_oracle_gives_the_constructed_answers(orc, cases, oracle_eval, name):
    c = cases[name]
    O = oracle_eval(name)
    if not c.whole_crop:
        assert len(O["crop_idx"]) == 0 and not c.expect
        return
    np.testing.assert_array_equal(O["crop_idx"], np.arange(len(c.cloud)))  # the crop of all the poses is the whole cloud
    for p in range(len(c.poses)):  # ... and of every pose alone (the match and the refinement crop for one pose)
        o = orc.Tracker(orc.default_config(particle_num=1, threads=0, emulate_pcl_alloc=0, octree_resolution=c.resolution))
        o.set_reference(c.model)
        o.set_input(c.cloud)
        E = o.eval_weights(sc.particles_of(c.poses[p:p + 1]), want_nn=True, mats=c.matrices()[p:p + 1])
        np.testing.assert_array_equal(E["crop_idx"], np.arange(len(c.cloud)))
        np.testing.assert_array_equal(E["nn_idx"][0], O["nn_idx"][p])
    idx, d2 = O["nn_idx"][c.expect_pose], O["nn_d2"][c.expect_pose]
    assert c.expect
    for qi, want, dd in c.expect:
        assert idx[qi] == want and d2[qi].tobytes() == F(dd).tobytes(), (name, qi, idx[qi], want)
    xyz = np.stack([c.cloud[f] for f in "xyz"], 1)
    Q = c.queries()
    for qi, tie in c.leaf_ties:  # inside one leaf: the same float distance, the earliest record
        assert len({sc.d2_of(xyz[i], Q[qi]).tobytes() for i in tie}) == 1 and idx[qi] == min(tie)
    for t in c.ties:
        assert idx[t["query"]] == t["winner"] and idx[t["up"]] == t["winner_up"], t["name"]
        assert Q[t["up"]].tobytes() != Q[t["query"]].tobytes() != Q[t["down"]].tobytes()
        for a in t["axes"]:  # one float step on every tie axis
            assert np.nextafter(Q[t["query"]][a], F(2)) == Q[t["up"]][a] and np.nextafter(Q[t["query"]][a], F(0)) == Q[t["down"]][a]
        if t["children"][0] == 0:
            assert idx[t["down"]] == t["winner"]
    for qi, rec, gname, g, inside in c.gate:
        gg = np.float64(g) * np.float64(g)
        assert idx[qi] == rec and (np.float64(d2[qi]) < gg) == inside, (name, gname)
        assert abs(np.float64(d2[qi]) - gg) <= 2.0 * np.spacing(F(gg)), "within two float steps of the gate"
    for gname in {g[2] for g in c.gate}:
        assert {g[4] for g in c.gate if g[2] == gname} == {True, False}


def test_outside_and_only_farther_are_what_they_say(orc, cases, oracle_eval):
    c = cases["descent"]
    tree = orc.Octree(c.cloud, c.resolution)
    info, keys = tree.info(), tree.point_keys()
    Q = c.queries().astype(np.float64)
    for p in range(len(c.poses)):
        Qp = c.queries(p).astype(np.float64)
        for qi, a, side in c.outside:  # 0.3 m outside at every pose (the poses move by micrometres)
            gap = info["min"][a] - Qp[qi][a] if side < 0 else Qp[qi][a] - info["max"][a]
            assert abs(gap - 0.3) < 1e-4, (qi, a, side, gap)
            assert oracle_eval("descent")["nn_idx"][p, qi] >= 0
    (qi, rec), = c.only_farther
    cell = np.floor((Q[qi] - info["min"]) / c.resolution).astype(np.int64)
    assert (cell >> 4).tolist() == (keys[rec].astype(np.int64) >> 4).tolist(), "the same 16-cell node"
    assert (cell[0] >> 3) + 1 == int(keys[rec][0]) >> 3, "the record lies in the upper x child, the query in the lower"
    assert (((keys.astype(np.int64) >> 4) == (cell >> 4)).all(axis=1)).sum() == 1, "the node holds that one record"
    assert 2 <= cell[0] % 8 <= 5, "deep inside the empty child"


def test_the_one_point_crop_is_a_one_level_tree(orc, cases):
    c = cases["one_point"]
    assert len(c.cloud) == 1 and orc.Octree(c.cloud, c.resolution).info()["depth"] == 1

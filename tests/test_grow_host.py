"""Host-side checks of the model-growth cases (tests/grow_cases.py) with the NumPy restatement alone
(tests/grow_model.py): each case tests what it claims, shown by concrete counts.  tests/test_gpu_grow.py then holds the
device to the same restatement."""
import numpy as np

import grow_cases as gc
import grow_model as gm

F = np.float32
N, P, FAR, K, U, C, A = range(7)  # NONFINITE PLANE FAR KNOWN UNREACHED CANDIDATE ADDED


def test_constants_and_inverse():
    g = gm.Grow()
    assert g.inv_leaf == F(100.0) and g.max_r2 == F(0.25)
    T = gc.matrix((0.3, -0.2, 1.1), (0.4, -0.3, 0.7))
    Ti = gm.inverse(T)
    np.testing.assert_array_equal(Ti[:, :3], T[:, :3].T)
    p = np.array([[0.1, 0.2, 0.3]], F)
    assert np.abs(gm.xform(Ti, gm.xform(T, p)) - p).max() < 1e-6
    assert np.signbit(gm.inverse(gc.IDENT)[:, 3]).all()  # -(0) is -0: the bits the device must return


def test_keys_case():
    c = gc.keys_case()
    g, states, stats = gc.run(c)
    s = states[0]
    assert s[0] == A and s[1] == A  # negative coordinates: floor, not truncation (truncation makes point 1 KNOWN)
    k, ok = gm.cells(gm.xyz_of(c["ops"][1][1]), g.inv_leaf)
    assert k[0].tolist() == [-1, -2, -3] and k[1].tolist() == [-1, 0, 0]
    # |k| = 2^20 - 1 has a key, 2^20 has none, on every axis and both signs
    assert s[2:10].tolist() == [A, FAR, A, FAR, A, FAR, A, FAR]
    assert [int(np.abs(k[i]).max()) for i in (2, 4, 6, 8)] == [gc.LIMIT - 1] * 4 and not ok[[3, 5, 7, 9]].any()
    # points exactly on cell faces, float(j * leaf): with inv_leaf = 100 the float product is j for all of them, so the
    # face belongs to the cell above it
    np.testing.assert_array_equal(k[10:27, 0], np.arange(-3, 14))
    assert s[10:27].tolist() == [U, A, C, K, A, A, U, U, U, U, U, A, A, K, A, A, U]
    assert stats[0]["n_added"] == 13
    # the point whose cell differs between the fused and the unfused transform
    Ti = gm.inverse(c["T"])
    ku = np.floor(gm.xform(Ti, c["E"][None]) * g.inv_leaf)[0]
    kf = np.floor(gc.fused_xform(Ti, c["E"][None]) * g.inv_leaf)[0]
    assert (ku != kf).any() and np.abs(ku - kf).max() == 1
    assert states[1].tolist() == [A] and g.debug_table()["keys"][0].tolist() == ku.astype(int).tolist()


def test_rules_case():
    g, states, stats = gc.run(gc.rules_case())
    assert states[0].tolist() == [N, N, P, P, U, P, U, FAR, K, A, C, U, FAR]
    assert states[1].tolist() == [N, N, P, P, U, P, U, FAR, K, K, K, U, FAR]
    assert stats[0]["n_state"] == dict(NONFINITE=2, PLANE=3, FAR=2, KNOWN=1, UNREACHED=3, CANDIDATE=1, ADDED=1)


def test_reach_cases():
    for r in (1, 2, 3, 4):
        c = gc.reach_case(r)
        g, states, stats = gc.run(c)
        cheb = np.abs(np.array(c["keys"])).max(axis=1)
        assert sorted(set(cheb.tolist())) == [r, r + 1]
        np.testing.assert_array_equal(states[0], np.where(cheb == r, A, U))  # exactly r: reached; r + 1: not
        # the voxel at r + 1 touches only voxels confirmed in the first apply: UNREACHED then, ADDED in the second
        np.testing.assert_array_equal(states[1], np.where(cheb == r, K, A))
        assert [s["n_added"] for s in stats] == [8, 7]


def test_crowd_cases():
    for name, (m, first) in gc.CROWDS.items():
        c = gc.crowd_case(name)
        frame = c["ops"][1][1]
        assert len(c["where"]) == m and c["where"][0] == first and len(frame) == 2240
        g, states, stats = gc.run(c)
        assert [(s["n_candidate_voxels"], s["n_added"], s["n_pending_live"]) for s in stats] == [(1, 0, 1), (1, 0, 1), (1, 1, 0)]
        for a in (0, 1):
            assert (states[a] == C).sum() == m and (states[a][c["where"]] == C).all()
        assert states[2][first] == A and (states[2] == C).sum() == m - 1
        t = g.debug_table()
        assert t["hits"].tolist() == [0, 3] and t["last_seen"].tolist() == [0, 3]  # one hit per apply, whatever m
        rec = g.cloud[-1]
        assert (rec["x"], rec["y"], rec["z"], rec["rgba"]) == tuple(frame[first][k] for k in ("x", "y", "z", "rgba"))
        assert rec["w"] == 1.0 and not rec["pad"].any() and frame[first]["pad"].any()
    assert gc.CROWDS["1_last_in_wave"][1] % 64 == 63 and gc.CROWDS["64_first_in_last_wave"][1] == 2240 - 64


def test_confirm_and_forget_cases():
    for cfm in (1, 2, 3):
        _, _, stats = gc.run(gc.confirm_case(cfm))
        assert [s["n_added"] for s in stats] == [2 if a == cfm else 0 for a in (1, 2, 3)]
    # seen at applies 1, 2, 4, 5, 6: forget = 2 bridges the gap (hits 3 at apply 4); forget = 1 starts again at apply 4
    _, _, two = gc.run(gc.forget_case(2))
    _, _, one = gc.run(gc.forget_case(1))
    assert [s["n_added"] for s in two] == [0, 0, 0, 1, 0, 0]
    assert [s["n_added"] for s in one] == [0, 0, 0, 0, 0, 1]
    assert [s["n_pending_live"] for s in one] == [1, 1, 1, 1, 1, 0] and one[2]["n_in"] == 0


def test_frontier_case():
    _, states, stats = gc.run(gc.frontier_case())
    # reach = 2 rows of 8 voxels per confirm = 3 applies; the face (5 rows, one of them in the model) is complete after 6
    assert [s["n_model_voxels"] for s in stats] == [48, 48, 64, 64, 64, 80, 80]
    assert [s["n_added"] for s in stats] == [0, 0, 16, 0, 0, 16, 0]
    assert (states[6] == K).all()
    _, _, fast = gc.run(gc.frontier_case(reach=1, confirm=1, applies=5))
    assert [s["n_added"] for s in fast] == [8, 8, 8, 8, 0]


def test_plane_cases():
    g, states, stats = gc.run(gc.plane_case(True))
    assert (states[0][-len(gc.PLANE_PATCH):] == P).all() and (states[0][:40] != P).all()
    assert [s["n_model_voxels"] for s in stats] == [64, 80] + [80] * 6
    assert not (g.debug_table()["keys"][:, 2] == -1).any()  # no plane voxel ever enters
    # the documented hazard: without the plane the model creeps along it until max_radius
    g, states, stats = gc.run(gc.plane_case(False))
    assert [s["n_model_voxels"] for s in stats] == [175, 253, 307, 364, 396, 396, 396, 396]
    keys = g.debug_table()["keys"]
    assert (keys[:, 2] == -1).sum() == 316 and np.abs(keys[:, :2]).max() == 10
    assert (states[-1] == FAR).sum() == 708 and (states[-1] == U).sum() == 0


def test_capacity_cases():
    g, states, stats = gc.run(gc.capacity_case())
    pick = lambda k: [s[k] for s in stats]
    assert pick("overflow") == [0, 1, 0, 0, 0]
    assert pick("occupied") == [64, 1, 64, 64, 64]  # exactly full is accepted; one more drops every pending voxel
    assert pick("n_pending_live") == [63, 0, 63, 63, 0] and pick("n_candidate_voxels") == [63, 0, 63, 63, 63]
    assert pick("n_added") == [0, 0, 0, 0, 63] and pick("n_model_points") == [1, 1, 1, 1, 64]
    assert (states[1] == C).all() and len(states[1]) == 64  # state[] still holds rules 1-6
    assert pick("n_rebuilds") == [0, 1, 1, 2, 3]
    small = gc.run(gc.rebuild_case(64))
    large = gc.run(gc.rebuild_case(1 << 16))
    assert small[2][-1]["n_rebuilds"] == 5 and large[2][-1]["n_rebuilds"] == 0
    assert [s["occupied"] for s in small[2]] == [22, 42, 42, 43, 43, 42, 42]
    assert [s["occupied"] for s in large[2]] == [22, 42, 62, 83, 103, 123, 143]
    for a, b in zip(small[1], large[1]):
        np.testing.assert_array_equal(a, b)
    assert small[0].cloud.tobytes() == large[0].cloud.tobytes() and len(small[0].cloud) == 2
    for k, v in small[0].debug_table().items():
        np.testing.assert_array_equal(v, large[0].debug_table()[k])
    g = gm.Grow(max_voxels=64)
    g.set_model(gc.too_many_voxels_model(32))
    try:
        g.set_model(gc.too_many_voxels_model(33))
        raise AssertionError("accepted")
    except gm.GrowError as e:
        assert e.status == gm.ERR_CAPACITY


def test_shape_cases():
    assert len(gc.shape_model("one_view")) == 2048 and len(gc.shape_model("sixty_four")) == 64
    g = gm.Grow()
    g.set_model(gc.shape_model("one_view"))
    assert g.n_model_voxels == 1554  # several points per voxel
    g.set_model(gc.shape_model("sixty_four"))
    assert g.n_model_voxels == 16
    _, states, stats = gc.run(gc.shape_case("one_view", 4099))
    assert stats[0]["n_state"] == dict(NONFINITE=43, PLANE=0, FAR=2, KNOWN=679, UNREACHED=1874, CANDIDATE=1501, ADDED=0)
    assert stats[1]["n_added"] == 1244 and stats[1]["n_state"]["CANDIDATE"] == 257
    _, states, stats = gc.run(gc.shape_case("empty", 4099))
    assert stats[1]["n_state"]["UNREACHED"] == 4056 and stats[1]["n_model_points"] == 0  # an empty model never grows
    for n in gc.SIZES:
        assert "shape_one_view_%d" % n in gc.CASES


def test_ghost_case():
    """the object of make_scene(50000) rolled by +0.5 rad against the one-face model at the true pose: 808 of its frame points
    lie 2 cm or more from every model point and would be a cluster of their own (the cluster minimum is 500); after growth
    with confirm = 1, applied until nothing is added, none is left"""
    n = gc.ghost_counts()
    assert n == dict(object=1122, before=808, after=0)
    assert n["before"] >= 500 > n["after"]
    g, states, stats = gc.ghost_run()
    assert len(stats) == 25 and stats[-1]["n_added"] == 0 and stats[-1]["n_model_points"] == 6577

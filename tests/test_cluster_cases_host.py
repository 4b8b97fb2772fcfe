"""The clustering cases of tests/cluster_cases.py, CPU side (no GPU): every builder delivers what its docstring promises,
the brute-force reference agrees with hand-computed toy cases, and brute force, the model's clusters
(tests/segment_model.py, cKDTree pre-filter) and the analytic expectations agree with each other.  The device runs the
same cases in tests/test_gpu_cluster_topology.py."""
import numpy as np
import pytest

import cluster_cases as cc
import segment_model as M

F = np.float32
BRUTE_LIMIT = 6000


def _same(got, want):
    assert [len(g) for g in got] == [len(w) for w in want]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def _survivors(cloud):
    xyz = cc.cloud_xyz(cloud)
    surv = np.flatnonzero(M.keep_nonzero(xyz))
    return xyz[surv], surv


# ---- the reference against hand-computed cases ---------------------------------------------------------------------------
def test_brute_strict_at_the_tolerance():
    # 0, 15/64 (below 0.25), then a step of exactly 0.25, then 15/64 again
    x = np.array([0.0, 15 / 64, 15 / 64 + 0.25, 30 / 64 + 0.25], F)
    xyz = np.stack([x, np.ones(4, F), np.full(4, 2, F)], 1)
    got = cc.brute_clusters(xyz, 0.25, 1, 10)
    assert [g.tolist() for g in got] == [[0, 1], [2, 3]]
    assert [g.tolist() for g in cc.brute_clusters(xyz, 0.25 + 2.0 ** -20, 1, 10)] == [[0, 1, 2, 3]]


def test_brute_size_tie_and_order():
    # components {4, 1}, {0, 3} (a tie: the one with index 0 first), {2, 5, 6} (largest), {7} alone
    x = np.array([10.0, 0.0, 20.0, 10.1, 0.1, 20.1, 20.2, 30.0], F)
    xyz = np.stack([x, np.ones(8, F), np.full(8, 2, F)], 1)
    assert [g.tolist() for g in cc.brute_clusters(xyz, 0.15, 1, 10)] == [[2, 5, 6], [0, 3], [1, 4], [7]]
    assert [g.tolist() for g in cc.brute_clusters(xyz, 0.15, 2, 2)] == [[0, 3], [1, 4]]
    assert [g.tolist() for g in cc.brute_clusters(xyz, 0.15, 3, 10)] == [[2, 5, 6]]


def test_brute_min_above_max_keeps_nothing():
    xyz = np.array([[0, 1, 2], [0.1, 1, 2], [5, 1, 2]], F)
    assert cc.brute_clusters(xyz, 0.15, 3, 2) == []
    assert cc.brute_clusters(np.zeros((0, 3), F), 0.15, 1, 10) == []


# ---- what the builders promise -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.CASES))
def test_every_cloud_drops_points_and_has_distinct_colours(name):
    cloud, tol, mn, mx, expected = cc.get(name)
    assert cloud.dtype == cc.scene.POINT_DTYPE and not cloud.flags.writeable
    assert len(np.unique(cloud["rgba"])) == len(cloud)
    xyz = cc.cloud_xyz(cloud)
    keep = M.keep_nonzero(xyz)
    nan = np.isnan(xyz).any(axis=1)
    assert nan.sum() >= 4 and abs(nan.sum() - max(4, keep.sum() // 50)) <= 1       # about 2 %
    assert (~keep & ~nan).sum() == 3                                               # inside RULE zero's cube
    assert xyz[keep][:, 2].min() >= 1.0
    assert not np.array_equal(np.flatnonzero(keep), np.arange(keep.sum()))         # survivor index != input index
    if expected is not None:
        members = np.concatenate(expected)
        assert keep[members].all() and len(np.unique(members)) == len(members)     # input indices of survivors
        assert all(np.all(np.diff(e) > 0) for e in expected)
        sizes = [len(e) for e in expected]
        assert all(mn <= s <= mx for s in sizes)
        assert sizes == sorted(sizes, reverse=True)
        assert all(a[0] < b[0] for a, b in zip(expected, expected[1:]) if len(a) == len(b))


@pytest.mark.parametrize("name", ["offsets-near", "offsets-far"])
def test_offsets_cover_all_124(name):
    info = cc.get_info(name)
    assert len(cc.OFFSETS) == 124
    assert info["link_offsets"] == set(cc.OFFSETS)      # a pair below tol whose cells differ by exactly each offset
    assert info["control_offsets"] == set(cc.OFFSETS)   # and one at or above tol
    expected = cc.get(name)[4]
    sizes = [len(e) for e in expected]
    assert sizes == [2] * 124 + [1] * (249 if name == "offsets-far" else 248)
    if name == "offsets-far":
        assert 120000 < info["dims"][0] <= cc.MAX_AXIS_CELLS
        x = np.sort(_survivors(cc.get(name)[0])[0][:, 0])
        assert x[0] < 0.51 and x[1] > 15900          # the anchor, and everything else far out
    else:
        assert info["dims"].max() < 200


def test_offsets_control_pairs_include_exactly_tol():
    cloud, tol, *_ = cc.get("offsets-near")
    xyz, _ = _survivors(cloud)
    d = xyz[:, None, :] - xyz[None, :, :]
    dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert (dd == F(tol * tol)).sum() == 2 * 6          # the six one-cell axis offsets, both directions
    off = ~np.eye(len(xyz), dtype=bool)
    assert (dd[off] < F(tol * tol)).sum() == 2 * 124    # the linking pairs and nothing else


@pytest.mark.parametrize("order", ["ascending", "descending", "random", "bit_reversed"])
def test_chain_orders(order):
    o = cc.chain_order(order, cc.CHAIN_N)
    assert np.array_equal(np.sort(o), np.arange(cc.CHAIN_N))
    if order == "bit_reversed":
        assert o[:4].tolist() == [0, 16384, 8192, 4096]
    cloud, tol, *_ = cc.get("chains-%s" % order)
    xyz, _ = _survivors(cloud)
    assert np.array_equal(np.argsort(xyz[:, 0], kind="stable"), np.argsort(o, kind="stable"))
    step = np.diff(np.sort(xyz[:, 0]))
    assert np.all(step == F(0.25 - 2.0 ** -6))
    info = cc.get_info("chains-%s" % order)
    assert info["cells"] == cc.CHAIN_N and info["dims"].tolist() == [36362, 1, 1]    # one point per cell


def test_chain_gap_and_spiral():
    cloud, tol, mn, mx, expected = cc.get("chains-gap")
    xyz, surv = _survivors(cloud)
    step = np.diff(np.sort(xyz[:, 0]))
    assert (step == F(0.25)).sum() == 1 and step[cc.CHAIN_N // 2 - 1] == F(0.25)
    assert [len(e) for e in expected] == [10000, 10000] and expected[0][0] == surv[0] < expected[1][0]
    cloud, tol, mn, mx, expected = cc.get("chains-spiral")
    info = cc.get_info("chains-spiral")
    assert info["n"] == 19927 and info["dims"][1] > 1 and info["dims"][2] == 1
    assert [len(e) for e in expected] == [19927]


def test_crowded_cells_only_the_last_pair_links():
    info = cc.get_info("crowded_cells")
    assert info["cells"] == 4
    assert info["cell_counts_0"] == info["cell_counts_1"] == (256, 256)
    assert info["below"][0] == [info["last_0"]]   # the highest survivor index of both cells, and no other pair
    assert info["below"][1] == []                 # the control
    assert [len(e) for e in cc.get("crowded_cells")[4]] == [512, 256, 256]


def test_size_rule_blobs():
    assert cc.get_info("size_rule-5-40")["cells_per_blob"] == [1] * 7
    assert [len(e) for e in cc.get("size_rule-5-40")[4]] == [40, 40, 17, 5, 5]
    assert [len(e) for e in cc.get("size_rule-5-5")[4]] == [5, 5]
    assert [len(e) for e in cc.get("size_rule-1-1000000")[4]] == [41, 40, 40, 17, 5, 5, 4]
    cloud, _, _, _, expected = cc.get("size_rule-5-40")
    xyz, surv = _survivors(cloud)
    assert all(np.diff(np.searchsorted(surv, e)).max() > 1 for e in expected)   # members interleaved in index order
    _, _, mn, mx, expected = cc.get("size_rule-isolated")
    assert (mn, mx) == (1, 1) and len(expected) == 30000
    assert np.all(np.diff([e[0] for e in expected]) > 0)


@pytest.mark.parametrize("m", cc.TILE_EDGE_M)
def test_tile_edges_survivor_count_and_boundary(m):
    cloud, tol, *_ = cc.get("tile_edges-%d" % m)
    xyz, surv = _survivors(cloud)
    assert len(surv) == m and tol == 0.02
    info = cc.get_info("tile_edges-%d" % m)
    assert info["straddles"] == (m > cc.TILE)
    if m >= 1023:
        assert info["tiles"] == (m + cc.TILE - 1) // cc.TILE
        keys = cc.cell_sorted_keys(xyz, tol)
        assert (keys[cc.TILE - 1] == keys[cc.TILE]) if m > cc.TILE else True


def test_near_full_grid_dims():
    info = cc.get_info("near_full_grid")
    assert info["dims"].tolist() == [120000, 30000, 1] and 3.5e9 < info["cells"] < cc.MAX_GRID_CELLS
    over = cc.get_info(cc.REFUSED_CASE)
    assert over["dims"].tolist() == [120000, 40000, 1] and over["cells"] >= cc.MAX_GRID_CELLS
    assert cc.get(cc.REFUSED_CASE)[4] is None
    sizes = [len(e) for e in cc.get("near_full_grid")[4]]
    assert sizes == [2] * 5 + [1] * 2        # four corner pairs, the diagonal pair, and the pair at exactly tol


def test_over_a_million_counts():
    cloud, tol, mn, mx, expected = cc.get("over_a_million")
    xyz, surv = _survivors(cloud)
    assert len(surv) == 1096703 > 1024 * 1024 and (mn, mx) == (1, 1000)
    sizes = np.array([len(e) for e in expected])
    assert len(sizes) == 1100 and sizes.sum() == len(surv)
    assert np.array_equal(np.unique(sizes), np.arange(994, 1001)) and np.bincount(sizes)[994:].min() >= 157


# ---- brute force == the model == the analytic expectation ----------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in cc.EXPECTED_CASES if n != "over_a_million"])
def test_expectation_against_model_and_brute_force(name):
    cloud, tol, mn, mx, expected = cc.get(name)
    xyz, surv = _survivors(cloud)
    _same([surv[c] for c in M.clusters(xyz, tol, mn, mx)], expected)
    if len(surv) <= BRUTE_LIMIT:
        _same([surv[c] for c in cc.brute_clusters(xyz, tol, mn, mx)], expected)


def test_over_a_million_builder_at_six_blocks():
    """the builder of the largest case at a size brute force can take: its analytic expectation against both references"""
    cloud, tol, mn, mx, expected = cc.over_a_million(blocks=6)
    xyz, surv = _survivors(cloud)
    assert [len(e) for e in expected] == [1000, 999, 998, 997, 996, 995]
    _same([surv[c] for c in cc.brute_clusters(xyz, tol, mn, mx)], expected)
    _same([surv[c] for c in M.clusters(xyz, tol, mn, mx)], expected)

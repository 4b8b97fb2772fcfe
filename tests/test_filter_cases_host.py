"""CPU: the plain model of the input filters (tests/filters_model.py) against the C oracle
(oracle/pft_oracle_filters.c) on every case of tests/filter_cases.py, bit for bit; the structural condition every case
exists for, from a key emulation that is neither of the two; and hand-derived known answers for the model itself, so
that it is not pinned by the oracle alone.  tests/test_gpu_filters_edges.py runs the same cases on the device."""
import numpy as np
import pytest

import filter_cases as fc
import filters_model as model
from pcl_tracking_amd import scene

F = np.float32


def same_cloud(got, want):
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()


def same_cloud_nan_positions(got, want):
    """NaN centroids: same places; every other value, and the colours, bit for bit (payload bits are not compared)"""
    assert len(got) == len(want)
    for k in ("x", "y", "z"):
        nan = np.isnan(want[k])
        np.testing.assert_array_equal(np.isnan(got[k]), nan)
        np.testing.assert_array_equal(got[k][~nan].view(np.uint32), want[k][~nan].view(np.uint32))
    for k in ("w", "rgba", "pad"):
        np.testing.assert_array_equal(got[k], want[k])


def pts(rows):
    """rows of (x, y, z, r, g, b[, a])"""
    p = np.zeros(len(rows), scene.POINT_DTYPE)
    for i, r in enumerate(rows):
        p["x"][i], p["y"][i], p["z"][i] = r[0], r[1], r[2]
        a = r[6] if len(r) > 6 else 255
        p["rgba"][i] = (a << 24) | (r[3] << 16) | (r[4] << 8) | r[5]
    p["w"] = 1.0
    return p


# ---- model against oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fc.grid_cases() + fc.pass_cases(), ids=lambda c: c.name)
def test_model_and_oracle_agree(orc, c):
    want, got = fc.expected(orc, c), fc.expected(model, c)
    assert got.n_pass == want.n_pass and got.handed_through == want.handed_through
    np.testing.assert_array_equal(got.pass_idx, want.pass_idx)
    same_cloud(got.out, want.out)


def test_model_and_oracle_agree_on_huge_and_infinite_coordinates(orc):
    c = fc.huge_and_inf("approx")
    got, want = fc.expected(model, c), fc.expected(orc, c)
    same_cloud_nan_positions(got.out, want.out)
    x = want.out["x"]
    # infinite centroids, a NaN one (+inf and -inf in one voxel), and the huge cells do merge points
    assert np.isinf(x).any() and np.isnan(x).sum() == 1 and len(want.out) < len(c.cloud)


@pytest.mark.parametrize("mode", sorted(fc.REUSE_MODES))
def test_model_and_oracle_agree_on_the_reuse_clouds(orc, mode):
    m, pass_ = fc.REUSE_MODES[mode]
    for cloud in fc.reuse_clouds():
        c = fc.case("reuse", cloud, m, pass_=pass_)
        want, got = fc.expected(orc, c), fc.expected(model, c)
        assert got.n_pass == want.n_pass
        same_cloud(got.out, want.out)
        if pass_ is not None and len(cloud) > 1:
            assert 0 < want.n_pass < len(cloud)  # the limit drops part of every cloud


# ---- the structural conditions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
def test_exact_long_runs_reaches_the_emit_paths(orc, white):
    c = fc.exact_long_runs(white)
    heads, kept = fc.sorted_heads(c.cloud, c.leaf)
    s = fc.long_run_structure(heads, kept)
    assert s["head_free_tiles"] == [3, 4, 5, 6, 9]      # R == 0 tiles
    assert s["head_on_tile_start"] == [1024]
    assert s["whole_rounds_past_tile"] == [1]           # 1025 .. 2304: ends on tile end + 256
    assert s["longest"] == 5000 > 4096
    assert s["max_rounds"] == 17                        # 2304 .. 7304 continues 4232 points past tile 2
    assert s["short_last_tile"]
    # the points of a voxel are NOT consecutive in the input (the sort has to be stable, not merely grouping)
    keys = fc.exact_keys(c.cloud, c.leaf)
    assert (np.diff(keys) != 0).mean() > 0.5
    # dropped points lie among the kept ones, and the last voxel is a single point in front of them
    bad = np.flatnonzero(~fc.finite_mask(c.cloud))
    assert len(bad) == 37 and bad.min() < 2000 and bad.max() > 9000
    want = fc.expected(orc, c).out
    assert len(want) == len(fc.LONG_RUNS)
    if white:
        assert (want["rgba"] == 0xFFFFFFFF).all()        # 5000 x 255 / 5000: exact


def test_one_voxel_cases(orc):
    for build in (fc.exact_one_voxel, fc.exact_one_voxel_behind_pass):
        for mode in ("exact", "approx"):
            e = fc.expected(orc, build(mode))
            assert len(e.out) == 1
    assert fc.expected(orc, fc.exact_one_voxel_behind_pass()).n_pass == 20000 - 7


@pytest.mark.parametrize("leaf", [0.01, (0.05, 0.02, 0.1)], ids=["iso", "aniso"])
def test_cell_faces_land_on_both_sides(leaf):
    below = at = 0
    for lf in fc.leaf3(leaf):
        b, a, other = fc.face_landing(lf)
        assert other == 0
        below, at = below + b, at + a
    assert below >= 10 and at >= 10
    if np.isscalar(leaf):
        assert fc.face_landing(leaf) == (15, 106, 0)
    # the cloud holds every face float and both neighbours on every axis
    c = fc.cell_faces(leaf, "exact").cloud
    for a, k in enumerate("xyz"):
        v = fc.face_values(fc.leaf3(leaf)[a])
        have = set(c[k].view(np.uint32).tolist())
        for w in (v, np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))):
            assert set(w.view(np.uint32).tolist()) <= have


def test_denormal_cells_tell_the_sign(orc):
    d = fc.DENORMALS
    assert (d[:4] < np.finfo(F).tiny).all() and (d[:3] * F(100) < np.finfo(F).tiny).all() and (d > 0).all()
    assert (fc.cell_index(d, 0.01) == 0).all() and (fc.cell_index(-d, 0.01) == -1).all()
    assert fc.cell_index(F(-0.0), 0.01) == 0
    for mode in ("exact", "approx"):
        c = fc.denormal_cells(mode)
        out = fc.expected(orc, c).out
        # x and y fall into cells -1 and 0 only; some centroid is itself a denormal, so denormal sums were formed
        assert len(np.unique(fc.cell_index(c.cloud["x"], 0.01))) == 2
        assert len(out) < len(c.cloud) // 2
        assert ((np.abs(out["x"]) < np.finfo(F).tiny) & (out["x"] != 0)).any()


@pytest.mark.parametrize("mirror", [False, True])
def test_far_narrow_cells_are_past_2_24(orc, mirror):
    c = fc.far_narrow("exact", mirror)
    cells = fc.cell_index(c.cloud["x"], c.leaf)
    assert np.abs(cells).max() > 2**24 and np.abs(cells).max() > 2.00004e7
    assert len(np.unique(cells)) > 300   # and they still tell the points apart
    assert len(fc.expected(orc, c).out) >= 2990
    assert len(fc.expected(orc, fc.far_narrow("approx", mirror)).out) >= 2990


def test_product_limit_sits_on_both_sides_of_int32_max(orc):
    c = fc.product_limit(1290)
    assert fc.cell_extents(c.cloud, c.leaf) == [1290] * 3 and 1290**3 <= 2**31 - 1
    assert fc.exact_keys(c.cloud, c.leaf).max() == 1290**3 - 1 >= 2**24   # the fourth radix byte
    assert not fc.expected(orc, c).handed_through
    c = fc.product_limit(1291)
    assert fc.cell_extents(c.cloud, c.leaf) == [1291] * 3 and 1291**3 > 2**31 - 1
    assert orc.voxel_grid(c.cloud, c.leaf) is None
    c = fc.product_limit_two_factors()
    d = fc.cell_extents(c.cloud, c.leaf)
    assert d[0] * d[1] > 2**31 - 1 and max(d) < 2**31 and d[0] * d[1] * d[2] < 2**63
    assert orc.voxel_grid(c.cloud, c.leaf) is None


def test_huge_and_inf_behind_pass(orc):
    c = fc.huge_and_inf("exact", behind_pass=True, big=(3e6, -4e6))
    d = fc.cell_extents(c.cloud, c.leaf)
    assert d[0] * d[1] * d[2] < 2**63 and d[0] * d[1] > 2**31 - 1   # the oracle's int64 product stays defined
    e = fc.expected(orc, c)
    assert orc.voxel_grid(c.cloud[e.pass_idx], c.leaf) is None and e.handed_through
    assert 0 < e.n_pass < len(c.cloud) and (np.abs(e.out["x"]) > 1e6).any() and fc.finite_mask(e.out).all()
    c = fc.huge_and_inf("approx", behind_pass=True)
    e = fc.expected(orc, c)
    assert (e.out["x"] == F(3e7)).any() and (e.out["y"] == F(-4e8)).any()


def test_pass_edges_hit_the_limits(orc):
    for c in fc.pass_cases():
        field, lo, hi, neg = c.pass_
        v = c.cloud[field]
        assert (v == F(lo)).any() and (v == F(hi)).any()
        e = fc.expected(orc, c)
        fin = fc.finite_mask(c.cloud)
        if lo > hi:
            assert e.n_pass == (int(fin.sum()) if neg else 0)
        elif lo == -fc.FLT_MAX:
            assert e.n_pass == (0 if neg else int(fin.sum()))
        else:
            assert 0 < e.n_pass < int(fin.sum())
        assert fin[e.pass_idx].all() and not fin.all()
    # limits included; their outer float neighbours, the negative denormals and -FLT_MAX are not; both zeros are
    c = fc.pass_edges("y", 0.0, 10.0, False)
    kept = set(c.cloud["y"][fc.expected(orc, c).pass_idx].view(np.uint32).tolist())
    bits = lambda v: int(np.asarray(v, F).view(np.uint32))
    for v in (0.0, -0.0, 10.0, np.nextafter(F(0), F(1)), np.nextafter(F(10), F(0)), 1e-45):
        assert bits(v) in kept
    for v in (np.nextafter(F(10), F(11)), -1e-45, np.nextafter(F(0), F(-1)), -fc.FLT_MAX, fc.FLT_MAX):
        assert bits(v) not in kept


def test_every_history_size_merges_points(orc):
    n = len(fc.long_runs_cloud(0))
    outs = []
    for h in fc.HIST_SIZES:
        want = fc.expected(orc, fc.hist_sizes(h)).out
        assert len(want) < n
        outs.append(want.tobytes())
    assert len(set(outs)) == len(outs)  # the table size decides the output order: no size stands in for another


def test_pairings_drop_points_on_both_stages(orc):
    for p in fc.PAIRING_PASSES:
        for mode in ("approx", "exact"):
            c = fc.pairings(p, mode)
            e = fc.expected(orc, c)
            assert 0 < len(e.out) < e.n_pass < int(fc.finite_mask(c.cloud).sum())


# ---- known answers for the model, derived by hand --------------------------------------------------------------------
def test_model_floor_to_int():
    assert model.floor_to_int(F(-0.5)) == -1 and model.floor_to_int(F(2.0)) == 2 and model.floor_to_int(F(-3.0)) == -3
    for v in (np.nan, np.inf, -np.inf, 2147483648.0, 3e9, -2147483904.0):
        assert model.floor_to_int(F(v)) == -(2**31)
    assert model.floor_to_int(F(-2147483648.0)) == -(2**31) and model.floor_to_int(F(2147483520.0)) == 2147483520


def test_model_pass_through_by_hand():
    nan, inf = float("nan"), float("inf")
    c = pts([(0, 0, -0.1, 1, 1, 1), (0, 0, 0.0, 1, 1, 1), (0, 0, 10.0, 1, 1, 1), (0, 0, 10.001, 1, 1, 1),
             (nan, 0, 5.0, 1, 1, 1), (0, -inf, 5.0, 1, 1, 1), (0, 0, nan, 1, 1, 1)])
    assert model.pass_through(c, "z", 0.0, 10.0).tolist() == [1, 2]
    assert model.pass_through(c, "z", 0.0, 10.0, negative=True).tolist() == [0, 3]
    assert model.pass_through(c, "z", 10.0, 0.0).tolist() == []
    assert model.pass_through(c, "z", 10.0, 0.0, negative=True).tolist() == [0, 1, 2, 3]
    assert model.pass_through(c, "x", -1.0, 1.0).dtype == np.int32


def test_model_approx_two_points_one_voxel_and_colour_truncation():
    A, B = (0.001, 0.001, 0.001, 10, 20, 30), (0.003, 0.005, 0.007, 20, 30, 41)
    out = model.approx_voxel_grid(pts([A, B]), 0.01, 512)
    assert len(out) == 1
    assert out["x"][0] == (F(A[0]) + F(B[0])) / F(2) and out["y"][0] == (F(A[1]) + F(B[1])) / F(2)
    assert out["rgba"][0] == (15 << 16) | (25 << 8) | 35      # 35.5 truncates; alpha byte 0
    assert out["w"][0] == 1.0 and (out["pad"] == 0).all()


def test_model_approx_flush_order_by_hand():
    # leaf 0.01, 512 entries: cell (0,0,0) -> entry 0; cell (512,0,0): 512 * 7171 & 511 = 0, the same entry;
    # cell (1,0,0) -> 7171 & 511 = 3; cell (-1,0,0) -> -7171 & 511 = 509
    A, C_, E = (0.001, 0.001, 0.001, 1, 1, 1), (5.125, 0.002, 0.002, 2, 2, 2), (0.015, 0.001, 0.001, 3, 3, 3)
    D, Fp = (0.004, 0.004, 0.004, 4, 4, 4), (-0.001, 0.001, 0.001, 5, 5, 5)
    out = model.approx_voxel_grid(pts([A, C_, E, D, Fp]), 0.01, 512)
    # C_ flushes A, D flushes C_; then the open entries in table order: 0 (D), 3 (E), 509 (Fp)
    assert [int(v) & 255 for v in out["rgba"]] == [1, 2, 4, 3, 5]
    # one entry: every voxel change flushes, the last voxel leaves at the end
    out = model.approx_voxel_grid(pts([A, D, E, E, A]), 0.01, 1)
    assert [int(v) & 255 for v in out["rgba"]] == [2, 3, 1] and out["x"][0] == (F(A[0]) + F(D[0])) / F(2)
    # 2048 entries keep cell (512,0,0) (512 * 7171 & 2047 = 1536) apart from cell (0,0,0): A and D merge, nothing is
    # flushed early; cell (1,0,0) -> 7171 & 2047 = 1027, cell (-1,0,0) -> -7171 & 2047 = 1021
    out = model.approx_voxel_grid(pts([A, C_, E, D, Fp]), 0.01, 2048)
    assert [int(v) & 255 for v in out["rgba"]] == [2, 5, 3, 2]   # entries 0 (A + D: 5 / 2 -> 2), 1021, 1027, 1536


def test_model_approx_sums_in_arrival_order():
    # float32: (1 + 2^-24) + 2^-24 = 1 (both adds round to even), 2^-24 + 2^-24 + 1 = 1 + 2^-23
    t = float(2.0**-24)
    up = model.approx_voxel_grid(pts([(1.0, 0, 0, 0, 0, 0), (t, 0, 0, 0, 0, 0), (t, 0, 0, 0, 0, 0)]), 4.0, 512)
    down = model.approx_voxel_grid(pts([(t, 0, 0, 0, 0, 0), (t, 0, 0, 0, 0, 0), (1.0, 0, 0, 0, 0, 0)]), 4.0, 512)
    assert up["x"][0] == F(1.0) / F(3) and down["x"][0] == (F(1.0) + F(2.0**-23)) / F(3)
    assert up["x"][0] != down["x"][0]


def test_model_voxel_grid_by_hand():
    cloud = pts([(0.021, 0.001, 0.001, 100, 0, 0, 255), (0.001, 0.001, 0.001, 10, 20, 30, 200),
                 (0.002, 0.003, 0.004, 20, 40, 61, 101), (float("nan"), 0, 0, 9, 9, 9), (0.001, 0.011, 0.001, 1, 2, 3, 4)])
    out = model.voxel_grid(cloud, 0.01)
    # index = ix + iy * 3 + iz * 6 (div = 3, 2, 1): voxel 0 {1, 2}, voxel 2 {0}, voxel 3 {4}
    assert len(out) == 3
    assert out["x"][0] == (F(0.001) + F(0.002)) / F(2) and out["z"][0] == (F(0.001) + F(0.004)) / F(2)
    assert out["rgba"][0] == (150 << 24) | (15 << 16) | (30 << 8) | 45          # 150.5, 45.5 truncate
    assert out["x"][1] == F(0.021) and out["rgba"][1] == (255 << 24) | (100 << 16)
    assert out["y"][2] == F(0.011) and out["rgba"][2] == (4 << 24) | (1 << 16) | (2 << 8) | 3
    # sums inside a voxel follow the input order
    t = float(2.0**-24)
    a = model.voxel_grid(pts([(1.0, 0, 0, 0, 0, 0), (t, 0, 0, 0, 0, 0), (t, 0, 0, 0, 0, 0)]), 4.0)
    b = model.voxel_grid(pts([(t, 0, 0, 0, 0, 0), (t, 0, 0, 0, 0, 0), (1.0, 0, 0, 0, 0, 0)]), 4.0)
    assert a["x"][0] == F(1.0) / F(3) and b["x"][0] == (F(1.0) + F(2.0**-23)) / F(3)
    # leaf too small: 1e7 cells per axis; empty and all-NaN clouds: empty
    assert model.voxel_grid(pts([(0, 0, 0, 1, 1, 1), (1000, 1000, 1000, 1, 1, 1)]), 0.0001) is None
    assert len(model.voxel_grid(cloud[:0], 0.01)) == 0 and len(model.voxel_grid(cloud[3:4], 0.01)) == 0

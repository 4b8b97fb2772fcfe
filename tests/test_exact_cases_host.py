"""CPU-only proof, with the oracle alone, that the inputs of tests/exact_cases.py reach the capacity fallbacks of
pcl_tracking_amd/csrc/pft_exact_nn.hip that tests/test_gpu_exact_routes.py takes them for.  The queries are the reference
cloud under the oracle's own matrices, the crop and its box are the oracle's, and the grid, the candidate-list lengths and
the LDS count table are the float32 restatements in exact_cases.  Every case crosses its capacity with a margin of at least
2x, so that rounding differences between this model and the device cannot flip the route; the GPU tests then prove from the
device's own state that the route ran.  Each test prints the modelled figures next to the capacity they must cross.

The cases at other resolutions (exact_cases.RES_NAMES) have no capacity to cross but a precondition each, proved here in
the same way: a query inside the box whose cell lies outside the grid, a grid of one cell, a cube of more than 64 slabs, a
doubled millimetre cell, and pairs in the outermost ring and cube that can hold an in-gate neighbour."""
import functools

import numpy as np
import pytest

import exact_cases as ec

MARGIN = 2


@functools.lru_cache(maxsize=None)
def modelled(name):
    """the oracle's evaluation of a case and the device's grid, hit cells and candidate lists as exact_cases models them"""
    import oracle as orc

    case = ec.build(name)
    p = case["particles"]
    o = orc.Tracker(orc.default_config(particle_num=len(p), threads=0, emulate_pcl_alloc=0, exact_nearest=1,
                                       max_distance=case["gate"]))
    o.set_reference(case["model"])
    o.set_input(case["cloud"])
    O = o.eval_weights(p, want_nn=True)
    geo = ec.grid_geometry(O["bbox"], case["res"])
    q = np.stack([ec.xyz_of(orc.transform_cloud(case["model"], orc.get_transformation(*[float(pp[k]) for k in ec.POSE])))
                  for pp in p])  # (P, M, 3)
    qcell = ec.query_cell(geo, q.reshape(-1, 3)).reshape(len(p), -1)
    hit = np.unique(qcell[qcell >= 0])
    crop_xyz = ec.xyz_of(case["cloud"])[O["crop_idx"]]
    in_gate = O["nn_d2"].astype(np.float64) < case["gate"] ** 2
    return dict(case=case, O=O, geo=geo, q=q, qcell=qcell, hit=hit, crop_xyz=crop_xyz, in_gate=in_gate)


def lists_of(m):
    if "lengths" not in m:
        m["lengths"] = ec.list_lengths(m["geo"], m["hit"], m["crop_xyz"], m["case"]["gate"])
    return m["lengths"]


def report(name, m, **more):
    geo = m["geo"]
    line = "%s: crop %d, grid %s cells of %.2f m (%d at 2 cm, capacity %d), cells hit %d (slots %d), in-gate share %.3f" % (
        name, len(m["crop_xyz"]), geo["ncells"], float(geo["g"]), geo["cells_at_resolution"], ec.EG_CAP, len(m["hit"]),
        ec.EC_SLOTS, m["in_gate"].mean())
    print(line + "".join(", %s %s" % kv for kv in more.items()))


def test_restated_capacities_and_hash():
    assert (ec.EQ_TAB, ec.EQ_PROBES, ec.EC_STAGE, ec.EC_CHUNK) == (8192, 48, 448, 512)
    assert int(ec.eq_hash(np.array([0xffffffff], np.uint64))[0]) < ec.EQ_TAB
    assert len(np.unique(ec.eq_hash(np.arange(1 << 16)))) == ec.EQ_TAB  # 13 bits, all of them used
    assert (ec.tile_particles(4), ec.tile_particles(96), ec.tile_particles(257), ec.tile_particles(8192), ec.tile_particles(65536)) == (1, 1, 2, 32, 32)


def test_grid_geometry_restatement():
    geo = ec.grid_geometry([0.0, 1.0, 0.0, 0.5, -0.25, 0.25])
    assert geo["g"] == np.float32(0.02) and geo["dim"].tolist() == [51, 26, 26] and geo["ncells"] == 51 * 26 * 26
    big = ec.grid_geometry([0.0, 4.0, 0.0, 4.0, 0.0, 4.0])  # 201^3 = 8.1 M cells at 2 cm, 101^3 at 4 cm
    assert big["g"] == np.float32(0.04) and big["ncells"] == 101 ** 3 <= ec.EG_CAP < big["cells_at_resolution"]
    assert ec.query_cell(geo, np.array([[-0.001, 0.1, 0.0], [0.5, 0.25, 0.0], [1.001, 0.5, 0.25]], np.float32)).tolist() == [
        -1, (12 * 26 + 12) * 51 + 25, (25 * 26 + 25) * 51 + 50]
    assert ec.cell_of(geo, np.array([[-0.001, 0.1, 0.0]], np.float32)).tolist() == [(12 * 26 + 5) * 51 + 0]


@pytest.mark.parametrize("name", ["long_lists", "pool_at_ceiling"])
def test_pool_cases_cross_the_list_and_pool_capacities(name):
    m = modelled(name)
    L = lists_of(m)
    demand = ec.pool_demand(L)
    report(name, m, longest_list=int(L.max()), staging=ec.EC_STAGE, own_piece_above=ec.EC_CHUNK // 2,
           lists_above_staging=int((L > ec.EC_STAGE).sum()), demand=demand, first_pool=ec.EC_POOL_MIN, ceiling=ec.EC_POOL)
    assert L.max() >= MARGIN * ec.EC_STAGE and (L >= MARGIN * ec.EC_STAGE).sum() >= 10 and (L > ec.EC_STAGE).sum() >= 1000
    assert demand >= MARGIN * ec.EC_POOL_MIN  # the first evaluation on a fresh handle finds the pool full
    assert 0.02 < m["in_gate"].mean() < 0.98
    if name == "long_lists":
        # ... and one growth (demand + a quarter, rounded up to a power of two, at most the ceiling) holds every list.  This is
        # a capacity the case must NOT cross: the demand, with a whole chunk wasted by every wave that serves a short list (8
        # workgroups of 4 waves per CU), stays a third below the ceiling -- the model and the device differ by the few points
        # within rounding of a list's radius, far below a percent
        waste = min(int(((L > 0) & (L <= ec.EC_CHUNK // 2)).sum()), 8 * 4 * ec.NUM_CUS) * ec.EC_CHUNK
        assert 1.5 * (demand + waste) <= ec.EC_POOL
    else:
        assert demand >= MARGIN * ec.EC_POOL
        lo_placed, lo_refused = ec.placed_bounds(L[L > 0], ec.EC_POOL)
        print("%s: of %d lists at least %d placed and at least %d refused at the ceiling" % (name, (L > 0).sum(), lo_placed, lo_refused))
        assert lo_placed >= 0.1 * len(m["hit"]) and lo_refused >= 0.1 * len(m["hit"])


@pytest.mark.parametrize("name", ["grid_doubles", "slots_capped"])
def test_grid_case_has_more_cells_than_the_cell_arrays(name):
    m = modelled(name)
    geo = m["geo"]
    report(name, m, slot_limit=m["case"]["slots"])
    assert geo["cells_at_resolution"] >= MARGIN * ec.EG_CAP
    assert geo["g"] == np.float32(0.04) and geo["ncells"] <= ec.EG_CAP  # one doubling, then it fits
    assert 0.02 < m["in_gate"].mean() < 0.98
    assert (m["qcell"] >= 0).all()
    if name == "slots_capped":
        assert len(m["hit"]) >= MARGIN * m["case"]["slots"]
        # which cells get the slots is up to the device; queries of both kinds are left over whichever it picks: there are
        # twice as many in-gate (out-of-gate) queries as the `slots` cells richest in them hold
        for kind in (m["in_gate"], ~m["in_gate"]):
            counts = np.sort(np.unique(m["qcell"][kind], return_counts=True)[1])[::-1]
            most = int(counts[:m["case"]["slots"]].sum())
            print("%s: %d queries of this kind, at most %d of them in %d cells" % (name, kind.sum(), most, m["case"]["slots"]))
            assert kind.sum() >= MARGIN * most


@pytest.mark.parametrize("name", ["window_full", "window_full_partial"])
def test_window_cases_overflow_the_count_table_of_every_tile(name):
    m = modelled(name)
    P, M = m["qcell"].shape
    ppw = ec.tile_particles(P)
    tiles = [m["qcell"][t:t + ppw].ravel() for t in range(0, P, ppw)]
    # every tile is modelled for its distinct cells; the sequential table only for the first, the last and two in between
    distinct = [len(np.unique(t[t >= 0])) for t in tiles]
    sim = {k: ec.tile_table(tiles[k]) for k in sorted({0, len(tiles) // 3, 2 * len(tiles) // 3, len(tiles) - 1})}
    report(name, m, M=M, P=P, particles_per_tile=ppw, tiles=len(tiles), distinct_cells_per_tile="%d..%d" % (min(distinct), max(distinct)),
           table=ec.EQ_TAB, simulated="{tile: (distinct, cells outside, queries outside)} %s" % sim)
    assert M % 512 != 0
    full = distinct[:-1] if P % ppw else distinct
    assert min(full) >= MARGIN * ec.EQ_TAB
    for d, out_cells, out_queries in sim.values():
        assert out_cells >= d - ec.EQ_TAB and (d < MARGIN * ec.EQ_TAB or out_queries >= ec.EQ_TAB)
    if name == "window_full_partial":
        assert ppw == 2 and P % ppw == 1 and distinct[-1] > ec.EQ_TAB  # a last tile of one particle, over the table by itself
    else:
        assert ppw == 1
    assert 0.02 < m["in_gate"].mean() < 0.98
    assert len(m["hit"]) < ec.EC_SLOTS and m["geo"]["g"] == np.float32(0.02)  # (no other fallback interferes)


# ---- grid cells other than 2 cm (exact_cases.RES_NAMES) ----
def report_res(name, m, **more):
    geo, b = m["geo"], ec.search_bounds(m["geo"], m["case"]["gate"])
    print("%s: resolution %g, gate %g, crop %d, final g %.9g (fl(1/g) %s 1/g), dim %s, %d cells (%d at the resolution), Kmax %d, "
          "cube slabs %d, R %d, queries outside the grid %d of %d, in-gate share %.3f" % (
              name, m["case"]["res"], m["case"]["gate"], len(m["crop_xyz"]), float(geo["g"]),
              ">" if float(geo["inv_g"]) > 1.0 / float(geo["g"]) else "<=", geo["dim"].tolist(), geo["ncells"],
              geo["cells_at_resolution"], b["Kmax"], b["slabs"], b["R"], (m["qcell"] < 0).sum(), m["qcell"].size,
              m["in_gate"].mean()) + "".join(", %s %s" % kv for kv in more.items()))


@pytest.mark.parametrize("name", ec.RES_NAMES)
def test_resolution_cases_are_small_and_have_pairs_inside_the_gate(name):
    m = modelled(name)
    case = m["case"]
    report_res(name, m)
    assert (case["res"], case["gate"]) == ec.RES_CASES[name] and case["res"] != ec.RES and case["slots"] is None
    assert len(case["model"]) <= 300 and len(case["cloud"]) <= 6000 and len(case["particles"]) <= 16
    assert m["in_gate"].mean() > 0 and len(m["crop_xyz"]) > 0
    assert (ec.cell_coords(m["geo"], m["q"].reshape(-1, 3)) >= 0).all()  # nothing below the box
    if not name.startswith("top_query"):
        assert (m["qcell"] >= 0).all()


def test_old_cases_keep_the_default_resolution():
    assert all(ec.build(name)["res"] == ec.RES for name in ec.NAMES) and not set(ec.NAMES) & set(ec.RES_NAMES)


@pytest.mark.parametrize("name", ["top_query_leaves_grid_g030", "top_query_leaves_grid_g025"])
def test_top_query_leaves_the_grid(name):
    """the query at the box's maximum computes cell `dim` on every axis with a leaving extent, while it lies inside the
    box; the oracle pairs every such query inside the gate, so a lost query changes a weight"""
    m = modelled(name)
    case, geo = m["case"], m["geo"]
    g = np.float32(2.0 * case["res"])
    q = m["q"].reshape(-1, 3)
    box = np.asarray(m["O"]["bbox"], np.float64)
    ref = ec.xyz_of(case["model"])
    np.testing.assert_array_equal(m["q"], np.broadcast_to(ref[None], m["q"].shape))  # identity: query = reference point
    np.testing.assert_array_equal(box, np.stack([ref.min(0), ref.max(0)], 1).ravel().astype(np.float64))
    assert geo["g"] == g and (float(geo["inv_g"]) > 1.0 / float(g) or name.endswith("g025"))
    if name.endswith("g025"):
        assert geo["inv_g"] == np.float32(40.0) and 1.15 < case["gate"] / float(g) < 1.25
    out = m["qcell"].ravel() < 0
    coords = ec.cell_coords(geo, q)
    leaving = case["leaving"]
    report_res(name, m, extents=case["extent"].tolist(), leaving_axes=leaving.tolist(),
               outside_per_particle=int(out.sum()) // len(case["particles"]))
    assert leaving.any() and out.sum() >= len(case["particles"])
    assert (coords >= 0).all()
    assert ((q >= box[0::2][None, :]) & (q <= box[1::2][None, :])).all()  # every query inside [min, max] on every axis
    for a in range(3):
        top = q[:, a] == np.float32(box[2 * a + 1])
        assert top.any() and (coords[top, a] == geo["dim"][a] - 1 + int(leaving[a])).all()
        assert (coords[~top, a] < geo["dim"][a]).all()
        if leaving[a]:  # the two roundings: the grid's cell count by a division, the query's cell by a multiplication
            E = case["extent"][a]
            assert int(np.floor(E / g)) + 1 == geo["dim"][a] == int(np.floor(E * geo["inv_g"]))
    assert m["in_gate"].ravel()[out].all()
    # the cloud holds the maximal corner (binned into the last cell), points within a cell of it and points farther below
    crop = m["crop_xyz"]
    assert len(crop) == len(case["cloud"])
    below = (case["extent"][None, :].astype(np.float64) - crop.astype(np.float64)).max(1) / float(g)
    assert (below == 0).sum() == 1 and ((below > 0) & (below < 1)).sum() >= 3 and (below > 1).sum() >= 3
    corner = ec.cell_of(geo, case["extent"][None, :])[0]
    assert corner == geo["ncells"] - 1


def test_top_query_construction_stays_inside_at_the_default_resolution():
    """why the old cases could not reach the route: at 0.01 (and its doublings) fl(1 / g) is not above 1 / g, no extent
    has the two roundings disagree, and the same construction leaves no query outside"""
    import oracle as orc

    for res in (ec.RES, 2 * ec.RES, 4 * ec.RES):
        assert ec.leaving_extents(res) == []
    assert len(ec.leaving_extents(0.015)) >= 3 and len(ec.leaving_extents(0.0125)) >= 3
    case = ec.top_query_case(ec.RES, 0.1)
    assert not case["leaving"].any()
    o = orc.Tracker(orc.default_config(particle_num=4, threads=0, emulate_pcl_alloc=0, exact_nearest=1, max_distance=0.1))
    o.set_reference(case["model"])
    o.set_input(case["cloud"])
    geo = ec.grid_geometry(o.eval_weights(case["particles"])["bbox"], ec.RES)
    qcell = ec.query_cell(geo, ec.xyz_of(case["model"]))
    print("the construction at resolution %g: dim %s, queries outside the grid %d" % (ec.RES, geo["dim"].tolist(), (qcell < 0).sum()))
    assert (qcell >= 0).all()
    # ... nor at extents a float32 step around whole cells
    g = geo["g"]
    for k in range(2, 80):
        e = np.float32(k) * g
        for e in (np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(1))):
            assert int(np.floor(e * geo["inv_g"])) <= int(np.floor(e / g))


@pytest.mark.parametrize("name,kmax", [("coarse_cell_g050", 3), ("coarse_cell_g100", 2)])
def test_coarse_cell_is_one_cell(name, kmax):
    m = modelled(name)
    b = ec.search_bounds(m["geo"], m["case"]["gate"])
    report_res(name, m, schedule=[min(2, b["Kmax"]), min(4, b["Kmax"]), b["Kmax"]])
    assert m["geo"]["dim"].tolist() == [1, 1, 1] and m["geo"]["ncells"] == 1 and m["geo"]["g"] == np.float32(2.0 * m["case"]["res"])
    assert b["Kmax"] == kmax and b["R"] == 2
    assert 0.02 < m["in_gate"].mean() < 0.98


def test_fine_cell_needs_two_rounds_of_segments():
    m = modelled("fine_cell")
    b = ec.search_bounds(m["geo"], m["case"]["gate"])
    report_res("fine_cell", m, EC_SEGS=64)
    assert m["geo"]["g"] == np.float32(0.003) and m["geo"]["ncells"] == m["geo"]["cells_at_resolution"] <= ec.EG_CAP
    assert (m["geo"]["dim"] <= 100).all()
    assert b["Kmax"] == 36 and b["slabs"] == 73 > 64 and b["R"] == 35
    assert 0.02 < m["in_gate"].mean() < 0.98


def test_far_slabs_pairs_lie_in_the_second_round_of_segments():
    """fine_cell runs the second round of wave_segments_points (slabs 64 .. 72 of the Kmax cube) but no pair of it depends
    on what that round delivers.  fine_cell_far_slabs is made of such pairs: the neighbour lies 64 - Kmax = 28 cells or
    more above its query's cell in z, beyond 64 - KT as well, and nothing else lies in the slabs before, so the restated
    k_ec_build loses every one of them when only the first 64 slabs deliver points -- in the cube walk (D is not found)
    and in the list pass.  Pairs at Chebyshev distance 34 = R - 1 are among them."""
    m = modelled("fine_cell_far_slabs")
    case, geo, O = m["case"], m["geo"], m["O"]
    b = ec.search_bounds(geo, case["gate"])
    q = m["q"].reshape(-1, 3)
    want = np.where(m["in_gate"], O["nn_idx"], -1).ravel()
    d = ec.cell_coords(geo, m["crop_xyz"][np.maximum(want, 0)]) - ec.cell_coords(geo, q)
    P, M = m["qcell"].shape
    sites = np.tile(np.arange(M) >= 8, P)
    far = (want >= 0) & (d[:, 2] >= max(64 - b["Kmax"], 64 - b["KTmax"]) + 1)
    assert geo["g"] == np.float32(0.003) and geo["ncells"] == geo["cells_at_resolution"] <= ec.EG_CAP and (geo["dim"] <= 100).all()
    assert (b["Kmax"], b["slabs"], b["R"], b["last"], b["KTmax"]) == (36, 73, 35, 34, 35)
    assert (want[sites] >= 0).all() and far[sites].all() and not far[~sites].any()
    # every cloud point lies 28 cells or more above every site's cell: a cube's first 64 slabs hold none of them
    site_cz = ec.cell_coords(geo, q[sites])[:, 2]
    assert ec.cell_coords(geo, m["crop_xyz"])[:, 2].min() - site_cz.max() >= 64 - b["Kmax"]
    at_last = (want >= 0) & (np.abs(d).max(1) == b["last"])
    full = ec.list_search(geo, q, m["crop_xyz"], case["gate"])
    first_round = ec.list_search(geo, q, m["crop_xyz"], case["gate"], segs=64)
    rings = ec.shell_search(geo, q, m["crop_xyz"], case["gate"])
    np.testing.assert_array_equal(full, want)
    np.testing.assert_array_equal(rings, want)
    lost = first_round != want
    report_res("fine_cell_far_slabs", m, EC_SEGS=64, KT=b["KTmax"], pairs_in_slabs_from_64=int(far.sum()),
               pairs_at_chebyshev_34=int(at_last.sum()), lost_with_the_first_64_slabs_alone=int(lost.sum()))
    assert far.sum() >= 1 and (lost == far).all() and (first_round[far] == -1).all()
    assert at_last.sum() >= 1
    # the dense fine_cell has no such pair (which is why this case exists)
    f = modelled("fine_cell")
    fw = np.where(f["in_gate"], f["O"]["nn_idx"], -1).ravel()
    fd = ec.cell_coords(f["geo"], f["crop_xyz"][np.maximum(fw, 0)]) - ec.cell_coords(f["geo"], f["q"].reshape(-1, 3))
    print("fine_cell: largest z offset of an in-gate neighbour %d cells" % fd[fw >= 0, 2].max())


def test_fine_cell_doubles_to_a_cell_whose_reciprocal_rounds_up():
    m = modelled("fine_cell_doubles")
    geo = m["geo"]
    report_res("fine_cell_doubles", m, capacity=ec.EG_CAP)
    ext = np.diff(np.asarray(m["O"]["bbox"]).reshape(3, 2), axis=1).ravel()
    assert (ext > 0.3).all() and (ext < 0.5).all()
    assert geo["cells_at_resolution"] > ec.EG_CAP >= geo["ncells"]
    assert geo["g"] == np.float32(0.0022) * np.float32(2.0) and float(geo["inv_g"]) > 1.0 / float(geo["g"])
    assert 0.02 < m["in_gate"].mean() < 0.98


@pytest.mark.parametrize("name", ["last_ring_g030", "last_ring_g003"])
def test_last_ring_pairs_are_isolated(name):
    m = modelled(name)
    case, O = m["case"], m["O"]
    P, M = m["qcell"].shape
    d = np.sqrt(O["nn_d2"].astype(np.float64))
    sites = np.arange(M) >= 8  # (the first eight reference points span the box; the last two sites are the lone pairs)
    assert M == 8 + 78 + 2 and len(m["crop_xyz"]) == len(case["cloud"]) == 2 * 78 + 2
    assert m["in_gate"][:, sites].all() and not m["in_gate"][:, ~sites].any()
    assert (d[:, sites] > case["gate"] - 2.0e-4).all()  # just inside ...
    own = np.concatenate([np.arange(78), 2 * 78 + np.arange(2)])
    np.testing.assert_array_equal(O["nn_idx"][:, sites], np.broadcast_to(own[None], (P, 80)))  # ... its own point
    # no other cloud point inside the gate; the partner on the other side just outside it
    dist = np.sqrt(((m["q"][:, sites, None, :].astype(np.float64) - m["crop_xyz"][None, None].astype(np.float64)) ** 2).sum(3))
    assert ((dist < case["gate"]).sum(2) == 1).all()
    other = dist[:, np.arange(78), 78 + np.arange(78)]
    assert (other > case["gate"]).all() and (other < case["gate"] + 2.0e-4).all()
    assert ((dist[:, 78:] < 2.0 * case["gate"]).sum(2) == 1).all()  # the lone pairs: nothing else within two gates


@pytest.mark.parametrize("name", ["last_ring_g030", "last_ring_g003", "fine_cell_far_slabs", "odd_ratio_r013_gate030", "odd_ratio_r037_gate100",
                                  "odd_ratio_r037_gate030"])
def test_an_off_by_one_in_the_reach_loses_a_pair(name):
    """Sensitivity.  An in-gate neighbour lies at most last = ceil(gate / g) cells from its query's cell on any axis,
    and each of these cases has pairs at exactly that distance (for the cubes of k_ec_build, which span every x: in y or
    z).  R = last + 1 and Kmax >= last + 1 both carry a cell of slack for the float cell assignment, so the outermost
    ring and cube that matter are `last`: the restated searches, which reproduce the oracle's pairs as they stand, lose
    pairs when the rings stop at last - 1 and when the widest cube is last - 1.  Stopping at R - 1 or Kmax - 1 loses
    nothing, which is asserted: these tests, and the GPU tests on the same inputs, cannot tell R from R - 1 or Kmax from
    Kmax - 1 (harmless: the cell of slack is never needed here); the first bound they can see broken is last - 1, which
    is R - 2 and, depending on the ratio, Kmax - 2 to Kmax - 4."""
    m = modelled(name)
    case, geo, O = m["case"], m["geo"], m["O"]
    b = ec.search_bounds(geo, case["gate"])
    q = m["q"].reshape(-1, 3)
    want = np.where(m["in_gate"], O["nn_idx"], -1).ravel()
    cheb3 = np.abs(ec.cell_coords(geo, q) - ec.cell_coords(geo, m["crop_xyz"][np.maximum(want, 0)]))
    at_last = (want >= 0) & (cheb3.max(1) >= b["last"])
    at_last_yz = (want >= 0) & (cheb3[:, 1:].max(1) >= b["last"])
    assert (cheb3[want >= 0].max() <= b["last"]) and at_last.sum() >= 1 and at_last_yz.sum() >= 1
    rings = {k: ec.shell_search(geo, q, m["crop_xyz"], case["gate"], rings=k) for k in (b["R"], b["R"] - 1, b["last"] - 1)}
    cubes = {k: ec.list_search(geo, q, m["crop_xyz"], case["gate"], kmax=k) for k in (b["Kmax"], b["Kmax"] - 1, b["last"] - 1)}
    np.testing.assert_array_equal(rings[b["R"]], want)
    np.testing.assert_array_equal(cubes[b["Kmax"]], want)
    wrong_rings = (rings[b["last"] - 1] != want).sum()
    wrong_cubes = (cubes[b["last"] - 1] != want).sum()
    report_res(name, m, last=b["last"], pairs_at_last=int(at_last.sum()), pairs_at_last_in_y_or_z=int(at_last_yz.sum()),
               wrong_with_rings_to_last_minus_1=int(wrong_rings), wrong_with_cubes_to_last_minus_1=int(wrong_cubes),
               wrong_with_rings_to_R_minus_1=int((rings[b["R"] - 1] != want).sum()),
               wrong_with_cubes_to_Kmax_minus_1=int((cubes[b["Kmax"] - 1] != want).sum()))
    assert wrong_rings >= at_last.sum() >= 1 and wrong_cubes >= 1
    assert (rings[b["R"] - 1] == want).all() and (cubes[b["Kmax"] - 1] == want).all()  # the slack alone
    assert (rings[b["last"] - 1][at_last] != want[at_last]).all()

"""CPU-only proof, with the oracle alone, that the inputs of tests/exact_cases.py reach the capacity fallbacks of
pcl_tracking_amd/csrc/pft_exact_nn.hip that tests/test_gpu_exact_routes.py takes them for.  The queries are the reference
cloud under the oracle's own matrices, the crop and its box are the oracle's, and the grid, the candidate-list lengths and
the LDS count table are the float32 restatements in exact_cases.  Every case crosses its capacity with a margin of at least
2x, so that rounding differences between this model and the device cannot flip the route; the GPU tests then prove from the
device's own state that the route ran.  Each test prints the modelled figures next to the capacity they must cross."""
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
    geo = ec.grid_geometry(O["bbox"])
    q = np.stack([ec.xyz_of(orc.transform_cloud(case["model"], orc.get_transformation(*[float(pp[k]) for k in ec.POSE])))
                  for pp in p])  # (P, M, 3)
    qcell = ec.query_cell(geo, q.reshape(-1, 3)).reshape(len(p), -1)
    hit = np.unique(qcell[qcell >= 0])
    crop_xyz = ec.xyz_of(case["cloud"])[O["crop_idx"]]
    in_gate = O["nn_d2"].astype(np.float64) < case["gate"] ** 2
    return dict(case=case, O=O, geo=geo, qcell=qcell, hit=hit, crop_xyz=crop_xyz, in_gate=in_gate)


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

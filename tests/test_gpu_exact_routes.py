"""The capacity fallbacks of the exact nearest-neighbour search (pcl_tracking_amd/csrc/pft_exact_nn.hip) against the oracle's
brute-force search: every route that replaces the candidate-list walk by another algorithm or another pool layout, on the
inputs of tests/exact_cases.py (proved on the CPU by tests/test_exact_cases_host.py to cross each capacity with a margin of
2x).  Every test also proves from the device's own state (debugExactState: header words, per-slot arrays, the route counters
of the DEBUG_NN instantiations) that its route was taken, so that a changed capacity cannot make it pass vacuously.

Bars, as everywhere for this mode (tests/test_gpu_parity.py): the crop bit-equal; inside the oracle's gate the neighbour's
index and float squared distance bit-equal; outside the gate no neighbour; the raw weight within 1 ulp (a double sum in
another order, rounded to float once); the cell-sorted and the per-query path the same bits; a tracked frame's pose within
1e-4 of the oracle's.

The second part runs the same bars at grid cells other than 2 cm (exact_cases.RES_NAMES: octree resolutions from 1.1 mm to
0.5 m, gates of 0.1 to 33 cells), among them the one route DESIGN.md section 7 names that the default resolution cannot
reach: a query that attains the crop box's maximum and computes a cell one past the grid."""

import numpy as np
import pytest

import exact_cases as ec
from pcl_tracking_amd import scene

pytestmark = pytest.mark.gpu

PATH_ENV = {"sorted": None, "per_query": "PFT_EXACT_PER_QUERY", "shells": "PFT_EXACT_SHELLS_ONLY"}
NOLIST = 0xffffffff


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


@pytest.fixture(scope="module")
def gpu():
    from pcl_tracking_amd import tracker

    return tracker


def coherence(gpu, gate, res=ec.RES):
    coh = gpu.NearestPairPointCloudCoherence()
    coh.addPointCoherence(gpu.DistanceCoherence())
    hc = gpu.HSVColorCoherence()
    hc.setWeight(0.1)
    coh.addPointCoherence(hc)
    coh.setSearchMethod(gpu.OctreeSearch(res))
    coh.setMaximumDistance(gate)
    return coh


def make_gpu(gpu, monkeypatch, case, path, P=None, seed=1, kld=False, iterations=None):
    """a fresh handle on the case's clouds; the search path is latched from the environment when the handle is created"""
    for env in PATH_ENV.values():
        if env:
            monkeypatch.delenv(env, raising=False)
    if PATH_ENV[path]:
        monkeypatch.setenv(PATH_ENV[path], "1")
    P = len(case["particles"]) if P is None else P
    if kld:
        g = gpu.make_reference_tracker(particle_num=P, seed=seed, kld=True)
    else:
        g = gpu.ParticleFilterTracker(seed=seed)
        g.setParticleNum(P)
    if iterations:
        g.setIterationNum(iterations)
    g.setCloudCoherence(coherence(gpu, case["gate"], case["res"]))
    g.setReferenceCloud(case["model"])
    g.setTrans(scene.initial_trans())
    g.setInputCloud(case["cloud"])  # (creates the handle)
    if case["slots"]:
        g.debugSetExactLimits(case["slots"])
    return g


def make_oracle(orc, case, P=None, seed=1, **cfg):
    P = len(case["particles"]) if P is None else P
    o = orc.Tracker(orc.default_config(particle_num=P, seed=seed, threads=0, emulate_pcl_alloc=0, exact_nearest=1,
                                       max_distance=case["gate"], **cfg))
    o.set_reference(case["model"])
    o.set_trans(scene.initial_trans())
    o.set_input(case["cloud"])
    return o


_oracle = {}


def oracle_eval(orc, name, case, g):
    """the oracle's brute-force evaluation of a case, once for all tests and paths (the matrices are the device's, which
    are the same for every handle)"""
    if name not in _oracle:
        p = case["particles"]
        O = make_oracle(orc, case).eval_weights(p, want_nn=True, mats=g.debugPoseToMatrix(p))
        for v in O.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _oracle[name] = O
    return _oracle[name]


def check(G, O, gate):
    np.testing.assert_array_equal(G["crop_idx"], O["crop_idx"])
    inside = O["nn_d2"].astype(np.float64) < gate * gate
    assert inside.any()
    np.testing.assert_array_equal(G["nn_idx"][inside], O["nn_idx"][inside])
    np.testing.assert_array_equal(G["nn_d2"][inside], O["nn_d2"][inside])
    assert (G["nn_idx"][~inside] == -1).all()
    d = ulp_diff(G["raw"], O["raw"])
    assert d.max() <= 1, d.max()
    return inside


def evaluate(gpu, orc, monkeypatch, name, path, evaluations=1, case=None):
    """-> (handle, [(G, state)] per evaluation), each evaluation checked against the oracle"""
    case = ec.build(name) if case is None else case
    g = make_gpu(gpu, monkeypatch, case, path)
    out = []
    for _ in range(evaluations):
        G = g.evalWeights(case["particles"], want_nn=True)
        S = g.debugExactState()
        check(G, oracle_eval(orc, name, case, g), case["gate"])
        out.append((G, S))
    return g, out


def assert_capacities_restated(S):
    assert (S["EC_SLOTS"], S["EC_POOL"], S["EG_CAP"], S["EC_POOL_MIN"]) == (ec.EC_SLOTS, ec.EC_POOL, ec.EG_CAP, ec.EC_POOL_MIN)
    assert S["num_cus"] == ec.NUM_CUS


def placed_lists(S):
    """slots whose cell has a list with candidates"""
    return (S["ec_count"] != NOLIST) & (S["ec_count"] > 0)


def assert_list_ranges(S):
    """every placed list lies inside the pool the kernels were handed, and no two overlap"""
    k = placed_lists(S)
    base, cnt = S["ec_base"][k].astype(np.int64), S["ec_count"][k].astype(np.int64)
    assert len(base) > 0 and (base + cnt <= S["ec_pool_cap"]).all()
    o = np.argsort(base)
    assert (base[o][1:] >= (base + cnt)[o][:-1]).all()


def assert_route_totals(S, path, n_queries):
    """every query is accounted for.  Cell-sorted path: eq_queries are the queries of the cells that got a slot, whatever
    became of the cell's list; per-query path: lik_listed are the queries that found a list, empty ones included"""
    if path == "sorted":
        assert S["eq_queries"] <= n_queries and S["inline_shell"] + S["inline_empty"] <= n_queries
        assert S["inline_shell"] >= n_queries - S["eq_queries"]  # a cell without a slot: the shell search
        assert S["lik_queries"] == 0
    else:
        assert S["lik_queries"] == n_queries and S["lik_listed"] + S["lik_shell"] == n_queries
        assert S["inline_shell"] == S["inline_empty"] == S["window_full"] == 0


def compute_pair(gpu, orc, monkeypatch, name, frames, kld=False, seed=5):
    """tracked frames from the case's particles, the product (non-debug) instantiations against the oracle.  One iteration
    per frame: the first frame weighs the case's particles as they are (no resample before the first weight()), so its
    state is the case's; from the second frame on the population has collapsed onto the best particles"""
    case = ec.build(name)
    p = case["particles"]
    if kld:
        # the reference's own configuration (two iterations per frame), the population drawn around the initial pose
        g = make_gpu(gpu, monkeypatch, case, "sorted", P=300, seed=seed, kld=True)
        o = make_oracle(orc, case, P=300, seed=seed, kld_adaptive=1)
    else:
        g = make_gpu(gpu, monkeypatch, case, "sorted", seed=seed, iterations=1)
        o = make_oracle(orc, case, seed=seed, iteration_num=1)
        g.setParticles(p)
        o.set_particles(p)
    states = []
    for f in range(frames):
        g.compute()
        assert o.compute() == 0
        if kld:
            assert len(g.getParticles()) == len(o.get_particles())
        rg, ro = g.getResult(), o.get_result()
        for k in ec.POSE:
            assert abs(float(rg[k]) - float(ro[k])) < 1e-4, (f, k, rg, ro)
        states.append(g.debugExactState())
    return states


# ---- candidate lists longer than the staging area; the pool full, growing, at its ceiling ----
@pytest.mark.parametrize("path", ["sorted", "per_query"])
def test_pool_grows(gpu, orc, monkeypatch, path):
    """a fresh handle's pool (PFT_EC_POOL_MIN) is a seventh of what the case asks for: the first evaluation leaves cells
    without a list, whose queries the shell search answers; the second finds the pool grown to the demand and every list
    placed.  (The growth is in pftt_stage_crop_octree_likelihood, which evalWeights and compute() share.)"""
    _, ((G1, S1), (G2, S2)) = evaluate(gpu, orc, monkeypatch, "long_lists", path, evaluations=2)
    assert_capacities_restated(S1)
    n = G1["nn_idx"].size
    print("pool_grows[%s]: demand %d / %d, pool %d -> %d, NOLIST slots %d -> %d, shell queries %d -> %d" % (
        path, S1["ec_pool_used"], S2["ec_pool_used"], S1["ec_pool_cap"], S2["ec_pool_cap"], (S1["ec_count"] == NOLIST).sum(),
        (S2["ec_count"] == NOLIST).sum(), S1["inline_shell"] + S1["lik_shell"], S2["inline_shell"] + S2["lik_shell"]))
    assert S1["ec_pool_used"] > S1["ec_pool_cap"] == ec.EC_POOL_MIN
    assert (S1["ec_count"] == NOLIST).any() and placed_lists(S1).any()
    assert (S1["inline_shell"] if path == "sorted" else S1["lik_shell"]) > 0
    assert S2["ec_pool_cap"] > S1["ec_pool_cap"] and S2["ec_pool_used"] <= S2["ec_pool_cap"]
    assert not (S2["ec_count"] == NOLIST).any()
    assert S2["inline_shell"] == 0 and S2["lik_shell"] == 0 and S2["outside"] == 0 and S2["lik_outside"] == 0
    for S in (S1, S2):
        assert_list_ranges(S)
        assert_route_totals(S, path, n)
    np.testing.assert_array_equal(G1["raw"], G2["raw"])  # a list or the shell search: the same neighbour, the same bits


def test_long_lists(gpu, orc, monkeypatch):
    """lists longer than the LDS staging area of k_ec_build (EC_STAGE: walked a second time, stored straight into the pool)
    and longer than half a chunk (a piece of the pool of their own), with the pool grown to hold them all; the three search
    paths against the oracle and against each other"""
    raws = {}
    for path in ("sorted", "per_query", "shells"):
        _, evs = evaluate(gpu, orc, monkeypatch, "long_lists", path, evaluations=1 if path == "shells" else 2)
        G, S = evs[-1]
        raws[path] = G["raw"]
        if path == "shells":
            assert S["ec_nslots"] == 0 and S["lik_shell"] == S["lik_queries"] == G["nn_idx"].size
            continue
        cnt = S["ec_count"][placed_lists(S)]
        print("long_lists[%s]: %d lists, %d above EC_STAGE, %d above EC_CHUNK / 2, longest %d" % (
            path, len(cnt), (cnt > ec.EC_STAGE).sum(), (cnt > ec.EC_CHUNK // 2).sum(), cnt.max()))
        assert (cnt > ec.EC_STAGE).sum() > 0 and (cnt > ec.EC_CHUNK // 2).sum() > 0
        assert not (S["ec_count"] == NOLIST).any()
        # the lists the queries were served from: every in-grid query's cell has one
        assert (S["eq_queries"] if path == "sorted" else S["lik_listed"]) == G["nn_idx"].size
        assert S["inline_shell"] == 0 and S["lik_shell"] == 0
    np.testing.assert_array_equal(raws["sorted"], raws["per_query"])
    assert ulp_diff(raws["sorted"], raws["shells"]).max() <= 1


@pytest.mark.parametrize("path", ["sorted", "per_query"])
def test_pool_at_ceiling(gpu, orc, monkeypatch, path):
    """a demand of three times PFT_EC_POOL: the pool grows to the ceiling and stays there, and on every iteration part of
    the cells keep a list while the rest is answered by the shell search"""
    _, ((G1, S1), (G2, S2)) = evaluate(gpu, orc, monkeypatch, "pool_at_ceiling", path, evaluations=2)
    n = G2["nn_idx"].size
    nolist, placed = (S2["ec_count"] == NOLIST).sum(), placed_lists(S2).sum()
    print("pool_at_ceiling[%s]: demand %d, pool %d -> %d, %d lists placed, %d cells without, shell queries %d of %d" % (
        path, S2["ec_pool_used"], S1["ec_pool_cap"], S2["ec_pool_cap"], placed, nolist, S2["inline_shell"] + S2["lik_shell"], n))
    assert S1["ec_pool_cap"] == ec.EC_POOL_MIN and S2["ec_pool_cap"] == ec.EC_POOL == S2["EC_POOL"]
    assert S2["ec_pool_used"] > ec.EC_POOL
    assert nolist > 0 and placed > 0
    assert (S2["inline_shell"] if path == "sorted" else S2["lik_shell"]) > 0
    assert (n - S2["inline_shell"] - S2["inline_empty"] if path == "sorted" else S2["lik_listed"]) > 0
    for S in (S1, S2):
        assert_list_ranges(S)
        assert_route_totals(S, path, n)
    np.testing.assert_array_equal(G1["raw"], G2["raw"])


def test_pool_at_ceiling_paths_agree(gpu, orc, monkeypatch):
    raws = [evaluate(gpu, orc, monkeypatch, "pool_at_ceiling", path)[1][0][0]["raw"] for path in ("sorted", "per_query", "shells")]
    np.testing.assert_array_equal(raws[0], raws[1])
    assert ulp_diff(raws[0], raws[2]).max() <= 1


# ---- more cells at the resolution than the cell arrays hold ----
def test_grid_doubles(gpu, orc, monkeypatch):
    """a crop box of 5.4 million 2 cm cells: k_eg_setup doubles the cell until the grid fits PFT_EG_CAP, and the counting
    sort, the lists and the shell search work on 4 cm cells"""
    raws = {}
    case = ec.build("grid_doubles")
    for path in ("sorted", "per_query", "shells"):
        _, ((G, S),) = evaluate(gpu, orc, monkeypatch, "grid_doubles", path)
        raws[path] = G["raw"]
        assert_capacities_restated(S)
        print("grid_doubles[%s]: eg_g %.3f, dim %s, %d cells, crop %d, slots %d" % (path, S["eg_g"], S["eg_dim"], S["eg_ncells"],
                                                                                   S["n_crop"], S["ec_nslots"]))
        assert S["eg_g"] > 2.0 * ec.RES * 1.5 and np.float32(S["eg_g"]) == np.float32(4.0 * ec.RES)
        assert S["eg_ncells"] == int(np.prod(S["eg_dim"])) <= ec.EG_CAP
        # the restated geometry (exact_cases.grid_geometry on the device's box) is the device's
        geo = ec.grid_geometry(G["bbox"])
        assert geo["g"] == np.float32(S["eg_g"]) and geo["dim"].tolist() == S["eg_dim"].tolist()
        np.testing.assert_array_equal(geo["mn"], S["eg_min"])
        assert geo["cells_at_resolution"] > ec.EG_CAP
        # the counting sort of the cropped points by cell
        start, order = S["eg_start"].astype(np.int64), S["leaf_order"].astype(np.int64)
        n_crop = S["n_crop"]
        assert n_crop == len(G["crop_idx"]) and len(start) == S["eg_ncells"] + 1
        assert (np.diff(start) >= 0).all() and start[0] == 0 and start[-1] == n_crop
        np.testing.assert_array_equal(np.sort(order), np.arange(n_crop))
        cells = ec.cell_of(geo, ec.xyz_of(case["cloud"])[G["crop_idx"]][order])  # the cell of the point at each sorted position
        pos = np.arange(n_crop)
        assert (start[cells] <= pos).all() and (pos < start[cells + 1]).all()
        assert_route_totals(S, "per_query" if path == "shells" else path, G["nn_idx"].size)
        assert S["outside"] == 0 and S["lik_outside"] == 0
    np.testing.assert_array_equal(raws["sorted"], raws["per_query"])
    assert ulp_diff(raws["sorted"], raws["shells"]).max() <= 1


# ---- cells hit beyond the slot capacity ----
@pytest.mark.parametrize("path", ["sorted", "per_query"])
def test_slots_capped(gpu, orc, monkeypatch, path):
    """the slot capacity lowered to a thirtieth of the cells hit: the cells beyond it get no list and no segment of the
    sorted query array, their queries are answered by the shell search"""
    case = ec.build("slots_capped")
    g, ((G, S),) = evaluate(gpu, orc, monkeypatch, "slots_capped", path)
    n = G["nn_idx"].size
    print("slots_capped[%s]: %d cells hit, %d slots, shell queries %d of %d" % (path, S["ec_nslots"], S["ec_slots_cap"],
                                                                              S["inline_shell"] + S["lik_shell"], n))
    assert S["ec_slots_cap"] == case["slots"] < S["ec_nslots"] and len(S["ec_cells"]) == case["slots"]
    assert len(np.unique(S["ec_cells"])) == case["slots"]
    assert_route_totals(S, path, n)
    # the queries of the cells that did get a slot, counted with the restated geometry on the device's matrices (a query
    # within rounding of a cell face may be counted on the other side: a handful at most)
    m = case["model"]
    ref = np.stack([m["x"], m["y"], m["z"]], 1).astype(np.float32)
    T = np.asarray(g.debugPoseToMatrix(case["particles"]), np.float32).reshape(len(case["particles"]), 3, 4)
    q = (np.einsum("pij,mj->pmi", T[:, :, :3].astype(np.float64), ref.astype(np.float64)) + T[:, None, :, 3]).astype(np.float32)
    geo = ec.grid_geometry(G["bbox"])
    in_slots = np.isin(ec.query_cell(geo, q.reshape(-1, 3)), S["ec_cells"].astype(np.int64)).sum()
    listed = S["eq_queries"] if path == "sorted" else S["lik_listed"]
    shell = S["inline_shell"] if path == "sorted" else S["lik_shell"]
    assert abs(int(listed) - int(in_slots)) <= 8 and shell == n - listed and shell > n // 2
    # the same evaluation without the limit serves every cell from a list, and gives the same bits
    case_free = dict(case, slots=None)
    _, ((G0, S0),) = evaluate(gpu, orc, monkeypatch, "slots_capped", path, case=case_free)
    assert S0["ec_slots_cap"] == ec.EC_SLOTS and S0["inline_shell"] == 0 and S0["lik_shell"] == 0
    np.testing.assert_array_equal(G0["raw"], G["raw"])


# ---- a tile of particles touching more cells than its LDS count table holds ----
@pytest.mark.parametrize("name", ["window_full", "window_full_partial"])
def test_window_full(gpu, orc, monkeypatch, name):
    """every tile's queries fall into more than twice the 8 192 cells its count table holds: the cells that find their probe
    window full are counted with global atomics (k_ec_mark) and their queries placed one by one (k_eq_scatter).  window_full:
    one particle per tile, M no multiple of 512; window_full_partial: two per tile and a last tile of one"""
    case = ec.build(name)
    P, M = len(case["particles"]), len(case["model"])
    g, ((G, S),) = evaluate(gpu, orc, monkeypatch, name, "sorted")
    assert_capacities_restated(S)
    ppw = ec.tile_particles(P, S["num_cus"])
    tiles = -(-P // ppw)
    print("%s: %d tiles of %d, tables %d, cells hit %d, queries placed past a full window %d of %d, pool %d of %d" % (
        name, tiles, ppw, S["eq_tiles_cap"], S["ec_nslots"], S["window_full"], P * M, S["ec_pool_used"], S["ec_pool_cap"]))
    assert S["eq_tiles_cap"] >= tiles and S["eq_cap"] >= P * M  # the tables k_ec_mark left are what k_eq_scatter reads
    assert S["window_full"] > 0 and S["ec_nslots"] > 2 * ec.EQ_TAB
    assert S["ec_nslots"] < S["ec_slots_cap"] and np.float32(S["eg_g"]) == np.float32(2.0 * ec.RES)
    assert_route_totals(S, "sorted", P * M)
    assert S["outside"] == 0
    # the per-query path on the same lists (k_ec_mark's direct counts gave every cell its slot)
    _, ((Gq, Sq),) = evaluate(gpu, orc, monkeypatch, name, "per_query")
    assert Sq["ec_nslots"] == S["ec_nslots"] and Sq["window_full"] == 0
    np.testing.assert_array_equal(G["raw"], Gq["raw"])


def test_window_full_without_saved_tables(gpu, orc, monkeypatch):
    """k_eq_scatter counting its tile again: a handle whose per-tile tables were sized by an earlier, larger evaluation of
    ONE particle holds two of them, so tiles 2 and 3 of the four find none (blockIdx.x >= eq_tiles_cap)"""
    case = ec.build("window_full")
    P, M = len(case["particles"]), len(case["model"])
    g = make_gpu(gpu, monkeypatch, case, "sorted")
    g.setReferenceCloud(np.concatenate([case["model"]] * P))  # P * M queries from one particle: one tile
    g.evalWeights(case["particles"][:1])
    S0 = g.debugExactState()
    g.setReferenceCloud(case["model"])
    G = g.evalWeights(case["particles"], want_nn=True)
    S = g.debugExactState()
    print("window_full, tables %d for %d tiles: queries placed past a full window %d" % (S["eq_tiles_cap"], P, S["window_full"]))
    assert S0["eq_cap"] == S["eq_cap"] == P * M and 0 < S["eq_tiles_cap"] < P == -(-P // ec.tile_particles(P, S["num_cus"]))
    check(G, oracle_eval(orc, "window_full", case, g), case["gate"])
    assert S["window_full"] > 0
    assert_route_totals(S, "sorted", P * M)


# ---- tracked frames: the product instantiations on the same routes ----
@pytest.mark.parametrize("name,frames", [("long_lists", 2), ("pool_at_ceiling", 2), ("grid_doubles", 1), ("slots_capped", 1),
                                         ("window_full", 1)])
def test_tracked_frames_take_the_routes(gpu, orc, monkeypatch, name, frames):
    """compute() from the case's particles, GPU against oracle; the header words show the route where the route leaves one
    (the counters belong to the debug instantiations and stay untouched)"""
    states = compute_pair(gpu, orc, monkeypatch, name, frames)
    S1, S = states[0], states[-1]  # the first frame's state is the case's own; the last has grown what grows
    cnt1 = S1["ec_count"][placed_lists(S1)]
    if name == "long_lists":
        assert S1["ec_pool_used"] > S1["ec_pool_cap"] == ec.EC_POOL_MIN and (S1["ec_count"] == NOLIST).any()
        assert (cnt1 > ec.EC_STAGE).any() and (cnt1 > ec.EC_CHUNK // 2).any()
        assert S["ec_pool_cap"] > ec.EC_POOL_MIN and not (S["ec_count"] == NOLIST).any()
    elif name == "pool_at_ceiling":
        assert S1["ec_pool_used"] > ec.EC_POOL and (S1["ec_count"] == NOLIST).any() and len(cnt1) > 0
        assert S["ec_pool_cap"] == ec.EC_POOL
    elif name == "grid_doubles":
        assert np.float32(S1["eg_g"]) == np.float32(4.0 * ec.RES) and S1["eg_ncells"] <= ec.EG_CAP
    elif name == "slots_capped":
        assert S1["ec_slots_cap"] == ec.SLOTS_LOWERED < S1["ec_nslots"] and S1["eq_queries"] < len(ec.build(name)["particles"]) * 128 // 2
    else:
        assert S1["ec_nslots"] > 2 * ec.EQ_TAB and S1["eq_queries"] == 4 * 24001
    for St in states:
        if placed_lists(St).any():
            assert_list_ranges(St)


def test_tracked_frames_on_a_kld_handle(gpu, orc, monkeypatch):
    """the KLD variant's device-side particle count sizes the tiles of k_ec_mark / k_eq_scatter and the items of the search
    (launches sized for the capacity of 500 particles): two frames of two iterations on the clouds of long_lists, the
    population drawn around the initial pose.  Every cell's list holds most of the 3 000-point ball, so the demand is
    several times the first pool: the first iteration finds it full, and by the second frame it has grown"""
    S1, S2 = compute_pair(gpu, orc, monkeypatch, "long_lists", 2, kld=True, seed=9)
    print("kld: frame 1 demand %d, pool %d, NOLIST %d; frame 2 demand %d, pool %d, NOLIST %d" % (
        S1["ec_pool_used"], S1["ec_pool_cap"], (S1["ec_count"] == NOLIST).sum(), S2["ec_pool_used"], S2["ec_pool_cap"],
        (S2["ec_count"] == NOLIST).sum()))
    cnt1 = S1["ec_count"][placed_lists(S1)]
    assert (cnt1 > ec.EC_STAGE).any()
    # the pool only grows when an iteration asked for more than it held: a grown pool proves that iteration ran with
    # cells left without a list (which of the first iterations sees the growth depends on when the host reads the demand)
    assert S1["ec_pool_used"] > ec.EC_POOL_MIN and S2["ec_pool_cap"] > ec.EC_POOL_MIN
    assert S2["ec_pool_used"] <= S2["ec_pool_cap"] and not (S2["ec_count"] == NOLIST).any()
    for St in (S1, S2):
        assert_list_ranges(St)


# ---- grid cells other than 2 cm ----
def host_cells(case, mats, bbox):
    """the cell of every query as exact_cases restates eg_query_cell, on the device's own matrices and box: (P, M), -1
    outside the grid"""
    p = case["particles"]
    ref = ec.xyz_of(case["model"])
    T = np.asarray(mats, np.float32).reshape(len(p), -1, 4)[:, :3, :]
    q = ref[None, :, :]
    # the device's xform in float32 (exact for the identity matrices of the top_query cases, which is where the count of
    # queries outside the grid is asserted)
    q = (T[:, None, :, 0] * q[..., 0:1] + T[:, None, :, 1] * q[..., 1:2] + T[:, None, :, 2] * q[..., 2:3]) + T[:, None, :, 3]
    geo = ec.grid_geometry(bbox, case["res"])
    return geo, ec.query_cell(geo, q.reshape(-1, 3).astype(np.float32)).reshape(len(p), -1)


_res = {}


def res_evaluate(gpu, orc, monkeypatch, name, path):
    """a case of RES_NAMES on one path, once for all tests: -> (the device's matrices, [(G, S)] per evaluation), every
    evaluation checked against the oracle.  The list paths evaluate twice on the handle (below: pool_may_be_short)"""
    if (name, path) not in _res:
        g, evs = evaluate(gpu, orc, monkeypatch, name, path, evaluations=1 if path == "shells" else 2)
        np.testing.assert_array_equal(evs[0][0]["raw"], evs[-1][0]["raw"])
        _res[name, path] = (g.debugPoseToMatrix(ec.build(name)["particles"]), evs)
    return _res[name, path]


def pool_may_be_short(S):
    """A wave of k_ec_build takes a whole chunk of EC_CHUNK entries for the short lists it serves, and slot s goes to wave
    s modulo the 8 x 4 waves per CU, so up to min(slots, waves) chunks are taken whatever the lists hold; lists above half
    a chunk take their own length besides.  A pool at least that large holds every list: only where this upper limit
    exceeds the pool may cells be left without a list (on a fresh handle: more than 2 048 cells hit), and the next
    evaluation on the handle finds the pool grown to the demand."""
    cnt = S["ec_count"][S["ec_count"] != NOLIST].astype(np.int64)
    own = int(cnt[cnt > ec.EC_CHUNK // 2].sum()) if (S["ec_count"] != NOLIST).all() else ec.EC_POOL
    return min(S["ec_nslots"], 8 * 4 * S["num_cus"]) * ec.EC_CHUNK + own > S["ec_pool_cap"]


@pytest.mark.parametrize("path", ["sorted", "per_query", "shells"])
@pytest.mark.parametrize("name", ec.RES_NAMES)
def test_other_resolutions(gpu, orc, monkeypatch, name, path):
    """every case of exact_cases.RES_NAMES on every search path against the oracle's exhaustive search (check()), the grid
    the device built against the restated k_eg_setup, and the route each case exists for from the device's counters"""
    case = ec.build(name)
    mats, evs = res_evaluate(gpu, orc, monkeypatch, name, path)
    for number, (G, S) in enumerate(evs):
        assert_capacities_restated(S)
        n = G["nn_idx"].size
        geo, qcell = host_cells(case, mats, G["bbox"])
        b = ec.search_bounds(geo, case["gate"])
        outside = int((qcell < 0).sum())
        short = path != "shells" and pool_may_be_short(S)
        print("%s[%s] evaluation %d: eg_g %.9g, dim %s, %d cells, crop %d, slots %d, Kmax %d, R %d, outside %d / %d (host %d), "
              "shell queries %d, pool %d of %d%s" % (
                  name, path, number, S["eg_g"], S["eg_dim"].tolist(), S["eg_ncells"], S["n_crop"], S["ec_nslots"], b["Kmax"], b["R"],
                  S["outside"], S["lik_outside"], outside, S["inline_shell"] + S["lik_shell"], S["ec_pool_used"], S["ec_pool_cap"],
                  " (may be short: %d cells without a list)" % (S["ec_count"] == NOLIST).sum() if short else ""))
        # the grid is the restated one, at the case's resolution
        assert geo["g"] == np.float32(S["eg_g"]) and geo["dim"].tolist() == S["eg_dim"].tolist() and geo["ncells"] == S["eg_ncells"]
        np.testing.assert_array_equal(geo["mn"], S["eg_min"])
        assert S["n_crop"] == len(G["crop_idx"])
        if name == "fine_cell_doubles":
            assert geo["cells_at_resolution"] > ec.EG_CAP and np.float32(S["eg_g"]) == np.float32(0.0022) * np.float32(2.0)
        else:
            assert np.float32(S["eg_g"]) == np.float32(2.0 * case["res"])
        if name.startswith("coarse_cell"):
            assert S["eg_ncells"] == 1 and S["eg_dim"].tolist() == [1, 1, 1]
        if name.startswith("fine_cell") and name != "fine_cell_doubles":
            assert b["slabs"] > 64
        # the queries outside the grid: as many as the host model counts, none in the cases that are not built for them
        if name.startswith("top_query"):
            ref = ec.xyz_of(case["model"])
            np.testing.assert_array_equal(G["bbox"], np.stack([ref.min(0), ref.max(0)], 1).ravel())
            assert outside >= len(case["particles"])
        else:
            assert outside == 0
        if path == "sorted":
            assert S["outside"] == outside and S["lik_outside"] == 0 and S["inline_shell"] >= outside
        else:
            assert S["lik_outside"] == outside and S["outside"] == 0 and S["lik_shell"] >= outside
        assert_route_totals(S, "per_query" if path == "shells" else path, n)
        if path == "shells":
            assert S["ec_nslots"] == 0 and S["lik_shell"] == S["lik_queries"] == n
            continue
        # (a query within rounding of a cell face may be counted on the other side, except under the identity)
        hit = len(np.unique(qcell[qcell >= 0]))
        assert abs(S["ec_nslots"] - hit) <= (0 if name.startswith("top_query") else 8)
        assert S["ec_nslots"] <= S["ec_slots_cap"]
        assert_list_ranges(S)
        # every cell has its list and only the queries outside the grid take the shell search: on the first evaluation
        # wherever the fresh pool cannot be short, and on the second in every case
        if not short or number == len(evs) - 1:
            assert S["ec_pool_used"] <= S["ec_pool_cap"] and not (S["ec_count"] == NOLIST).any()
            assert (S["inline_shell"] if path == "sorted" else S["lik_shell"]) == outside
    if name == "fine_cell_far_slabs" and path != "shells":
        # the lists that only the second round of segments can fill: one per site cell, none empty
        G, S = evs[-1]
        assert placed_lists(S).sum() >= 9
    # the three paths: the same bytes (each of the other two against the cell-sorted one)
    if path != "sorted":
        G, G0 = evs[-1][0], res_evaluate(gpu, orc, monkeypatch, name, "sorted")[1][-1][0]
        for k in ("raw", "nn_idx", "nn_d2", "crop_idx"):
            assert G[k].tobytes() == G0[k].tobytes(), k


@pytest.mark.parametrize("name", ["top_query_leaves_grid_g030", "odd_ratio_r037_gate030"])
def test_tracked_frames_at_other_resolutions(gpu, orc, monkeypatch, name):
    """compute() on the product (non-debug) kernels, two frames from the case's particles (setParticles: the first frame
    weighs the identity particles of the top_query case as they are), the pose within 1e-4 of the oracle's"""
    case = ec.build(name)
    S1, S2 = compute_pair(gpu, orc, monkeypatch, name, 2)
    for S in (S1, S2):
        assert np.float32(S["eg_g"]) == np.float32(2.0 * case["res"])
        assert not pool_may_be_short(S)  # (a few hundred cells hit: the fresh pool holds a chunk for each)
        assert not (S["ec_count"] == NOLIST).any() and S["ec_nslots"] > 0
        assert_list_ranges(S)
    if name.startswith("top_query"):
        # the first frame's box is the reference's own: the grid of the case, whose top queries leave it
        ref = ec.xyz_of(case["model"])
        geo = ec.grid_geometry(np.stack([ref.min(0), ref.max(0)], 1).ravel(), case["res"])
        assert geo["dim"].tolist() == S1["eg_dim"].tolist() and (ec.query_cell(geo, ref) < 0).any()
        # the cells hit are those of the queries inside the grid alone
        assert S1["ec_nslots"] == len(np.unique(ec.query_cell(geo, ref)[ec.query_cell(geo, ref) >= 0]))


def test_state_readback_refuses_other_handles(gpu):
    from pcl_tracking_amd._lib import PftError

    g = gpu.make_reference_tracker(particle_num=8)
    g.setReferenceCloud(scene.make_model(64))
    g.setInputCloud(scene.make_model(64))
    with pytest.raises(PftError):
        g.debugExactState()
    with pytest.raises(PftError):
        g.debugSetExactLimits(100)
    case = ec.build("grid_doubles")
    e = gpu.ParticleFilterTracker(seed=1)
    e.setParticleNum(8)
    e.setCloudCoherence(coherence(gpu, 0.1))
    e.setReferenceCloud(case["model"])
    e.setInputCloud(case["cloud"])
    with pytest.raises(PftError):
        e.debugSetExactLimits(ec.EC_SLOTS + 1)  # never above the allocation
    e.debugSetExactLimits(ec.EC_SLOTS)

"""Inputs of the exact nearest-neighbour route tests (tests/test_gpu_exact_routes.py): for every capacity fallback of
pcl_tracking_amd/csrc/pft_exact_nn.hip a deterministic reference cloud, input cloud, particle set and gate that crosses the
capacity, and a numpy float32 restatement of the parts of the device code that decide the route -- the grid geometry
(k_eg_setup), the cell of a point and of a query, the per-cell candidate list length (k_ec_build) and the workgroup's LDS
count table (eq_hash / eq_insert).  tests/test_exact_cases_host.py proves with the oracle alone, on the CPU, that each case
crosses its capacity with a margin of at least 2x, so float differences between this model and the device cannot flip a route.

The capacities below restate pft_internal.h / pft_exact_nn.hip; the GPU tests compare them with what the library reports
(debugExactState) so that a change there cannot go unnoticed here.

RES_NAMES are cases at other octree resolutions than 0.01, where the grid cell is not 2 cm (NAMES all keep RES): the query
that leaves the grid at the box's maximum, one cell for the whole crop, millimetre cells under a 10 cm gate (densely, and with every neighbour in the slabs that only
the second round of wave_segments_points delivers), a doubling from
a millimetre cell, everyday scenes at non-dyadic cell / gate ratios and isolated pairs just inside the gate.  For those the
search bounds (Kmax, R) and the two searches themselves (shell_search, list_search) are restated as well, so that the
host tests can show what a reach one cell short would lose.
"""
import functools

import numpy as np

from pcl_tracking_amd import scene

RES = 0.01            # octree resolution of the handles (the grid cell is two leaves)
EG_CAP = 1 << 21      # PFT_EG_CAP: grid cells
EC_SLOTS = 1 << 19    # PFT_EC_SLOTS: candidate lists per iteration
EC_POOL = 1 << 24     # PFT_EC_POOL: candidate entries, upper limit
EC_POOL_MIN = 1 << 20  # PFT_EC_POOL_MIN: first allocation
EC_STAGE = 448        # staged candidates per wave of k_ec_build; a longer list is walked twice
EC_CHUNK = 512        # pool entries a wave takes at a time; a list above half of it gets a piece of its own
EQ_TAB = 8192         # entries of the LDS count table of a tile of particles
EQ_PROBES = 48        # its probe window
NUM_CUS = 256         # MI355X: a tile holds ceil(P / NUM_CUS) particles, at most 32
SLOTS_LOWERED = 40  # the slot limit of the slots_capped case

f32 = np.float32
POSE = ("x", "y", "z", "roll", "pitch", "yaw")


def particles_around(pose, n, seed, sig_t, sig_r):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    for k, name in enumerate(POSE):
        p[name] = pose[k] + rng.normal(0, sig_t if k < 3 else sig_r, n)
    p["w"] = 1.0
    p["weight"] = 1.0 / n
    return p


def coloured(xyz, seed):
    rng = np.random.default_rng(seed)
    return scene.make_points(np.asarray(xyz, np.float32), rng.integers(0, 256, (len(xyz), 3)))


def ball(n, centre, radius, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= (radius * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    return v + np.asarray(centre)[None, :]


def cube(n, centre, side, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-side / 2.0, side / 2.0, (n, 3)) + np.asarray(centre)[None, :]


def tile_particles(P, num_cus=NUM_CUS):
    """ppw of pftk_likelihood_exact"""
    return min(max(-(-P // num_cus), 1), 32)


CUBE_CENTRE = (0.0, 0.0, 1.5)
NAMES = ("long_lists", "pool_at_ceiling", "grid_doubles", "window_full", "window_full_partial", "slots_capped")
# cases at other octree resolutions than RES (the grid cell is 2 * res): name -> (resolution, gate)
RES_CASES = {
    "top_query_leaves_grid_g030": (0.015, 0.1),
    "top_query_leaves_grid_g025": (0.0125, 0.03),
    "coarse_cell_g050": (0.25, 0.1),
    "coarse_cell_g100": (0.5, 0.1),
    "fine_cell": (0.0015, 0.1),
    "fine_cell_far_slabs": (0.0015, 0.1),
    "fine_cell_doubles": (0.0011, 0.1),
    "odd_ratio_r007_gate100": (0.007, 0.1),
    "odd_ratio_r013_gate030": (0.013, 0.03),
    "odd_ratio_r037_gate100": (0.037, 0.1),
    "odd_ratio_r037_gate030": (0.037, 0.03),
    "last_ring_g030": (0.015, 0.1),
    "last_ring_g003": (0.0015, 0.02),
}
RES_NAMES = tuple(RES_CASES)
LAST_RING_INSIDE = 1.0e-4   # a last_ring pair is this far inside the gate, its partner on the other side as far outside
LAST_RING_SHIFT = 3.0e-5    # the largest translation of a last_ring particle, per axis


@functools.lru_cache(maxsize=None)
def build(name, num_cus=NUM_CUS):
    """-> dict(model, cloud, particles, gate, res, slots): slots is the lowered slot limit or None.  long_lists is the input
    of the pool_grows test as well (two evaluations on one handle)."""
    if name in RES_CASES:
        return build_res_case(name)
    return dict(_build(name, num_cus), res=RES)


def _build(name, num_cus):
    gt = scene.model_gt_pose()
    if name in ("long_lists", "pool_at_ceiling"):
        # a dense ball inside a wide gate: every hit cell's list holds a large part of the ball
        n = 3000 if name == "long_lists" else 20000
        return dict(model=scene.make_model(256), cloud=coloured(ball(n, gt[:3], 0.05, 41), 42),
                    particles=particles_around(gt, 64, 43, 0.15, 0.5), gate=0.5, slots=None)
    if name in ("grid_doubles", "slots_capped"):
        # a crop box of several metres: more 2 cm cells than the cell arrays hold
        xyz = cube(6000, gt[:3], 4.0, 51)
        cloud = np.concatenate([scene.make_scene(50000), coloured(xyz, 52)])
        # two particles near every corner of a 3 m cube, so that the box does not hang on one outlier (a resample of a
        # tracked frame keeps its extent)
        p = particles_around(gt, 16, 53, 0.05, 0.5)
        for k, name_ in enumerate(("x", "y", "z")):
            p[name_] += np.where((np.arange(16) >> k) & 1, 1.5, -1.5).astype(np.float32)
        return dict(model=scene.make_model(128), cloud=cloud, particles=p, gate=0.1,
                    slots=SLOTS_LOWERED if name == "slots_capped" else None)
    if name == "window_full":
        # one particle per tile whose reference points alone fall into far more cells than the table has entries;
        # M is no multiple of 512 (the last block of reference points of a particle is partial)
        return dict(model=coloured(cube(24001, (0, 0, 0), 1.0, 61), 62), cloud=coloured(cube(5000, CUBE_CENTRE, 1.0, 63), 64),
                    particles=particles_around(CUBE_CENTRE + (0.0, 0.0, 0.0), 4, 65, 0.15, 0.5), gate=0.1, slots=None)
    if name == "window_full_partial":
        # two particles per tile and a last tile of one
        P = num_cus + 1
        return dict(model=coloured(cube(10001, (0, 0, 0), 1.0, 71), 72), cloud=coloured(cube(150, CUBE_CENTRE, 1.0, 73), 74),
                    particles=particles_around(CUBE_CENTRE + (0.0, 0.0, 0.0), P, 75, 0.15, 0.5), gate=0.1, slots=None)
    raise KeyError(name)


def identity_particles(n):
    """roll = pitch = yaw = 0 and no translation: the matrix is exactly the identity, a query is its reference point"""
    p = np.zeros(n, scene.PARTICLE_DTYPE)
    p["w"] = 1.0
    p["weight"] = 1.0 / n
    return p


def leaving_extents(res, cells=range(2, 80)):
    """[(k, E)]: float32 extents E of a box axis, one per cell count k where one exists, for which the grid has k cells
    (floor(fl(E / g)) + 1, the division of k_eg_setup) while the query at the box's maximum computes cell k
    (floor(fl(E * fl(1 / g))), the multiplication of eg_query_cell): that query leaves the grid.  E lies a few float32
    steps below k * g, which are all tried."""
    g = f32(2.0 * res)
    inv_g = f32(1.0) / g
    out = []
    for k in cells:
        e = np.nextafter(np.nextafter(f32(k) * g, f32(np.inf)), f32(np.inf))
        for _ in range(12):
            if int(np.floor(e / g)) + 1 == int(np.floor(e * inv_g)) == k:
                out.append((k, e))
                break
            e = np.nextafter(e, f32(-np.inf))
    return out


def top_query_case(res, gate, seed=81):
    """The reference cloud spans [0, E] on every axis under identity particles, so the crop box is [0, E] and the reference
    points on a maximal face are queries at the box's maximum.  E is a leaving extent (above) on as many axes as the
    resolution has three different ones for, else an ordinary 5.5 cells.  -> the case and `leaving`: per axis, whether E
    is a leaving extent"""
    rng = np.random.default_rng(seed)
    g = f32(2.0 * res)
    found = leaving_extents(res, range(5, 80))[:3]
    E = np.array([e for _, e in found] + [f32(5.5) * g] * (3 - len(found)), np.float32)
    leaving = np.array([True] * len(found) + [False] * (3 - len(found)))

    def inside(xyz):  # float32 and inside the box, faces included
        return np.clip(np.asarray(xyz, np.float64), 0.0, E.astype(np.float64)[None, :]).astype(np.float32)

    corners = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)], np.float32) * E[None, :]
    on_face = []  # 12 reference points on every maximal face, an edge point among them
    for a in range(3):
        pts = rng.uniform(0.0, 1.0, (12, 3)) * E[None, :]
        pts[:, a] = E[a]
        pts[0, (a + 1) % 3] = E[(a + 1) % 3]
        on_face.append(pts)
    on_face = inside(np.concatenate(on_face))
    ref = np.concatenate([corners, on_face, inside(rng.uniform(0.0, 1.0, (120, 3)) * E[None, :])])
    top = np.concatenate([corners[1:], on_face])  # every reference point with a maximal coordinate
    # the cloud: the maximal corner itself (clamped into cell dim - 1), points within one cell of it, points more than one
    # cell below it, for every reference point on a maximal face a partner inside the gate, and a filling
    near = E[None, :] - rng.uniform(0.0, 1.0, (6, 3)) * g
    below = E[None, :] - rng.uniform(1.2, 3.0, (6, 3)) * g
    v = np.abs(rng.normal(size=(len(top), 3)))
    partner = top - v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.2, 0.8, (len(top), 1)) * gate
    fill = rng.uniform(0.0, 1.0, (1500, 3)) * E[None, :]
    cloud = inside(np.concatenate([E[None, :], near, below, partner, fill]))
    return dict(model=coloured(ref, seed + 1), cloud=coloured(cloud, seed + 2), particles=identity_particles(4), gate=gate,
                res=res, slots=None, leaving=leaving, extent=E)


LAST_RING_DIRECTIONS = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)],
                                np.float64)  # both directions of 3 axes, 6 face diagonals and 4 space diagonals


def last_ring_case(res, gate, seed=91):
    """Isolated pairs.  78 reference points on a lattice of 3 gates (no cloud point of one site within the gate of
    another), each moved by less than a cell so that it lies 0.1, 0.5 or 0.9 of a cell above a cell face on every axis;
    site k has ONE cloud point inside the gate, LAST_RING_INSIDE short of it along direction k % 26, and one on the
    other side as far outside it.  The last two lattice sites are lone pairs, towards -y from 0.1 and towards +z from 0.9
    of a cell, without the point on the other side: nothing else lies near their cells, so k_ec_build finds their only
    point in its widest cube or not at all.  Eight reference points without neighbours span the crop box.  The
    particles are translations by at most LAST_RING_SHIFT per axis, so every pair stays inside the gate and every
    partner outside.  Reference points: the 8 of the box, the 78 sites, the 2 lone ones; cloud: the 78 inside points in
    the order of their sites, the 78 partners, the 2 lone points."""
    rng = np.random.default_rng(seed)
    g = float(f32(2.0 * res))
    lat = np.array([(x, y, z) for x in range(5) for y in range(4) for z in range(4)], np.float64) * 3.0 * gate
    lo = -1.5 * gate  # the box's minimal corner: the origin of the grid
    frac = np.concatenate([np.array([0.1, 0.5, 0.9])[np.arange(78) // 26], [0.1, 0.9]])
    sites = lo + (np.floor((lat - lo) / g) + frac[:, None]) * g
    u = np.concatenate([LAST_RING_DIRECTIONS[np.arange(78) % 26], [(0.0, -1.0, 0.0), (0.0, 0.0, 1.0)]])
    u = u / np.linalg.norm(u, axis=1)[:, None]
    inside = sites + u * (gate - LAST_RING_INSIDE)
    cloud = np.concatenate([inside[:78], (sites - u * (gate + LAST_RING_INSIDE))[:78], inside[78:]])
    hi = lat.max(0) + 1.5 * gate
    span = np.array([[(lo, hi[a])[(c >> a) & 1] for a in range(3)] for c in range(8)])
    p = identity_particles(8)
    for name_ in ("x", "y", "z"):
        p[name_][1:] = rng.uniform(-LAST_RING_SHIFT, LAST_RING_SHIFT, 7)
    return dict(model=coloured(np.concatenate([span, sites]), seed + 1), cloud=coloured(cloud, seed + 2), particles=p,
                gate=gate, res=res, slots=None)


FAR_SLABS_DIRECTIONS = ((0.0, 0.0, 1.0, 0.1), (0.0, 0.0, 1.0, 0.5), (0.0, 0.0, 1.0, 0.9), (0.3, 0.0, 1.0, 0.9), (-0.3, 0.0, 1.0, 0.9),
                        (0.0, 0.3, 1.0, 0.9), (0.0, -0.3, 1.0, 0.9), (0.0, 0.0, 1.0, 0.7), (0.2, 0.2, 1.0, 0.9))  # x, y, z, cell fraction


def far_slabs_case(res, gate, seed=121):
    """3 mm cells under a 10 cm gate with every in-gate neighbour of a site some 32 to 34 cells ABOVE its query's cell in
    z: the slabs of the Kmax cube and of the list pass that hold it are numbers 64 and up, the second round of
    wave_segments_points.  Nine reference points in one z layer, 9 cm apart, each on the given fraction of a cell on
    every axis; each has one cloud point LAST_RING_INSIDE short of the gate straight or slightly tilted upwards, and
    (but for the last two, which stay alone) one as far beyond the gate in the same direction.  Every cloud point lies
    in the upper layer, so the nearest point to a hit cell's centre is itself only found in those slabs.  The crop box
    (24 x 24 x 14 cm, spanned by eight more reference points) keeps the 3 mm cell; particles as in last_ring_case."""
    rng = np.random.default_rng(seed)
    g = float(f32(2.0 * res))
    d = np.array(FAR_SLABS_DIRECTIONS)
    lat = np.array([(x, y, 0.02) for x in (0.03, 0.12, 0.21) for y in (0.03, 0.12, 0.21)])
    sites = (np.floor(lat / g) + d[:, 3:4]) * g
    u = d[:, :3] / np.linalg.norm(d[:, :3], axis=1)[:, None]
    cloud = np.concatenate([sites + u * (gate - LAST_RING_INSIDE), (sites + u * (gate + LAST_RING_INSIDE))[:7]])
    span = np.array([[(0.0, (0.24, 0.24, 0.14)[a])[(c >> a) & 1] for a in range(3)] for c in range(8)])
    p = identity_particles(8)
    for name_ in ("x", "y", "z"):
        p[name_][1:] = rng.uniform(-LAST_RING_SHIFT, LAST_RING_SHIFT, 7)
    return dict(model=coloured(np.concatenate([span, sites]), seed + 1), cloud=coloured(cloud, seed + 2), particles=p,
                gate=gate, res=res, slots=None)


@functools.lru_cache(maxsize=None)
def _everyday_clouds():
    """the scene and model of the other tests, 16 particles around the ground truth; of the scene the 6 000 points
    nearest the object, in their order"""
    gt = scene.model_gt_pose()
    cloud = scene.make_scene(50000)
    near = np.sort(np.argsort(((xyz_of(cloud).astype(np.float64) - np.array(gt[:3])[None, :]) ** 2).sum(1), kind="stable")[:6000])
    return dict(model=scene.make_model(256), cloud=cloud[near], particles=particles_around(gt, 16, 101, 0.02, 0.3))


def build_res_case(name):
    """the cases of RES_NAMES: small (model <= 300 points, cloud <= 6 000, <= 16 particles)"""
    res, gate = RES_CASES[name]
    if name.startswith("top_query"):
        return top_query_case(res, gate)
    if name.startswith("last_ring"):
        return last_ring_case(res, gate)
    if name == "fine_cell_far_slabs":
        return far_slabs_case(res, gate)
    if name.startswith("odd_ratio"):
        return dict(_everyday_clouds(), gate=gate, res=res, slots=None)
    # a cube of reference points turning about CUBE_CENTRE, a ball of cloud points on one side of it: queries on the other
    # side find nothing inside the gate
    side, n, radius = {"coarse_cell_g050": (0.15, 3000, 0.08), "coarse_cell_g100": (0.15, 3000, 0.08),
                       "fine_cell": (0.12, 2000, 0.05), "fine_cell_doubles": (0.28, 2000, 0.15)}[name]
    centre = np.array(CUBE_CENTRE)
    sig_r = 0.1 if name == "fine_cell_doubles" else 0.3
    return dict(model=coloured(cube(200, (0, 0, 0), side, 111), 112), cloud=coloured(ball(n, centre + (radius, 0.0, 0.0), radius, 113), 114),
                particles=particles_around(tuple(centre) + (0.0, 0.0, 0.0), 16, 115, 0.02, sig_r), gate=gate, res=res, slots=None)


def xyz_of(cloud):
    return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(np.float32)


# ---- the device code that decides the route, restated in numpy float32 ----
def grid_geometry(bbox, res=RES, cap=EG_CAP):
    """k_eg_setup: the cell doubles until the grid fits `cap` cells"""
    b = np.asarray(bbox, np.float32)
    g = f32(2.0 * res)
    while True:
        dim = []
        for a in range(3):
            q = np.floor(f32(b[2 * a + 1] - b[2 * a]) / g)
            q = f32(0.0) if not q >= 0.0 else min(q, f32(4.0e6))
            dim.append(int(q) + 1)
        if dim[0] * dim[1] * dim[2] <= cap:
            break
        g = f32(g * f32(2.0))
    return dict(g=g, inv_g=f32(1.0) / g, dim=np.array(dim, np.int64), mn=b[0::2].copy(), ncells=dim[0] * dim[1] * dim[2],
                cells_at_resolution=int(np.prod([int(np.floor((b[2 * a + 1] - b[2 * a]) / f32(2.0 * res))) + 1 for a in range(3)])))


def _coords(geo, xyz):
    return np.floor((np.asarray(xyz, np.float32) - geo["mn"][None, :]) * geo["inv_g"]).astype(np.int64)


cell_coords = _coords  # eg_query_cell's unclamped coordinates


def cell_of(geo, xyz):
    """eg_cell_of: the (clamped) cell of a cropped point"""
    c = np.clip(_coords(geo, xyz), 0, geo["dim"][None, :] - 1)
    return (c[:, 2] * geo["dim"][1] + c[:, 1]) * geo["dim"][0] + c[:, 0]


def query_cell(geo, xyz):
    """eg_query_cell: the cell of a query, -1 outside the grid"""
    c = _coords(geo, xyz)
    inside = ((c >= 0) & (c < geo["dim"][None, :])).all(1)
    return np.where(inside, (c[:, 2] * geo["dim"][1] + c[:, 1]) * geo["dim"][0] + c[:, 0], -1)


def list_lengths(geo, cells, crop_xyz, gate):
    """k_ec_build's rule for the cells given: D = distance from the cell centre to the nearest cropped point; no candidates if
    D - r > gate, else the points within min(D + 2r, gate + r) + 1e-4 of the centre, r = g * sqrt(3) / 2 + 1e-4"""
    g, dim = geo["g"], geo["dim"]
    cells = np.asarray(cells, np.int64)
    cx, cy, cz = cells % dim[0], (cells // dim[0]) % dim[1], cells // (dim[0] * dim[1])
    ctr = geo["mn"][None, :] + (np.stack([cx, cy, cz], 1).astype(np.float32) + f32(0.5)) * g
    r = f32(0.5) * g * f32(1.7320508) + f32(1.0e-4)
    gate = f32(np.sqrt(f32(gate * gate)))
    pts = np.asarray(crop_xyz, np.float32)
    out = np.zeros(len(cells), np.int64)
    step = max(1, (1 << 24) // max(len(pts), 1))
    for lo in range(0, len(cells), step):
        c = ctr[lo:lo + step]
        d2 = ((c[:, None, :] - pts[None, :, :]) ** 2).sum(2)
        D = np.sqrt(d2.min(1))
        T = np.minimum(D + f32(2.0) * r, gate + r) + f32(1.0e-4)
        out[lo:lo + step] = np.where(D - r <= gate, (d2 <= (T * T)[:, None]).sum(1), 0)
    return out


def pool_demand(lengths):
    """entries k_ec_build asks of the pool at least: a list above EC_CHUNK / 2 takes exactly its length, the shorter ones
    share chunks (at least their lengths, rounded up to whole chunks in all)"""
    lengths = np.asarray(lengths, np.int64)
    return int(lengths[lengths > EC_CHUNK // 2].sum() + lengths[lengths <= EC_CHUNK // 2].sum())


def eq_hash(c):
    return ((np.asarray(c, np.uint64) * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(19)


def tile_table(cells):
    """the LDS count table of one tile, its queries' cells (>= 0) inserted one after the other (eq_insert; on the device the
    order among the lanes is arbitrary, so the SET of cells that finds its window full varies, their number hardly does):
    -> (distinct cells, cells that did not enter, queries of those cells)"""
    cells = np.asarray(cells, np.int64)
    uniq, counts = np.unique(cells[cells >= 0], return_counts=True)
    first = np.unique(cells[cells >= 0], return_index=True)[1]
    order = np.argsort(first, kind="stable")  # first occurrence: the order a sequential pass meets the cells in
    key = np.full(EQ_TAB, -1, np.int64)
    out_cells = out_queries = 0
    hashes = eq_hash(uniq).astype(np.int64)
    for k in order:
        h = hashes[k]
        for _ in range(EQ_PROBES):
            if key[h] < 0:
                key[h] = uniq[k]
                break
            h = (h + 1) & (EQ_TAB - 1)
        else:
            out_cells += 1
            out_queries += int(counts[k])
    return len(uniq), out_cells, out_queries


def placed_bounds(lengths, cap):
    """whatever order the waves reach the pool in: (lists placed at least, lists refused at least).  Only the lists that take a
    piece of their own (above EC_CHUNK / 2) are counted: the pool's counter only grows, so such a list is placed iff the
    entries asked for before it plus its own fit `cap`; a shorter one may still find room in its wave's chunk"""
    s = np.sort(np.asarray(lengths, np.int64))
    s = s[s > EC_CHUNK // 2]
    fits_small_first = int(np.searchsorted(np.cumsum(s), cap, side="right"))  # the most lists that can ever fit
    # the first list refused finds more than cap - (its length) entries taken, by lists no longer than the longest
    return int((cap - s[-1]) // s[-1]), len(s) - fits_small_first


# ---- the search bounds and the two searches, restated (tests/test_exact_cases_host.py: what an off-by-one would lose) ----
def search_bounds(geo, gate):
    """Kmax of k_ec_build, R of k_eq_scatter / k_likelihood_exact, the slabs of the widest cube (the segments of
    wave_segments_points) and `last`: the largest Chebyshev cell distance an in-gate neighbour can have, ceil(gate / g)"""
    g, inv_g = geo["g"], geo["inv_g"]
    hh = f32(0.5) * g
    r = hh * f32(1.7320508) + f32(1.0e-4)
    gate_ = np.sqrt(f32(gate * gate))
    Kmax = int(np.ceil((gate_ + r) * inv_g)) + 1
    # (KT of the list pass is at most that of the widest list, T = gate + r + 1e-4)
    KTmax = int(np.ceil((gate_ + r + f32(1.0e-4) + hh) * inv_g))
    return dict(KTmax=KTmax, Kmax=Kmax, R=int(np.ceil(gate_ * inv_g)) + 1, slabs=2 * Kmax + 1, last=int(np.ceil(gate_ * inv_g)), r=r, hh=hh,
                gate=gate_)


def _sq_dist(a, b):
    """pointSquaredDist in float32, the device's order of the sum: (n, 3) x (m, 3) -> (n, m)"""
    e = a[:, None, :] - b[None, :, :]
    return e[..., 0] * e[..., 0] + (e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2])


def _gated(best, idx, gate):
    return np.where(np.isfinite(best) & (best.astype(np.float64) < gate * gate), idx, -1)


def shell_search(geo, q, crop_xyz, gate, rings=None):
    """eg_shell_search: rings of Chebyshev radius 0 .. `rings` (default: R) around the query's unclamped cell, over the
    clamped cells of the cropped points, left as soon as everything closer than the best has been seen.  The device
    skips rows that cannot hold anything closer (not restated: it changes no result).  -> the neighbour's position in
    the crop, -1 without one inside the gate; equal distances: the lowest position"""
    q, pts = np.asarray(q, np.float32), np.asarray(crop_xyz, np.float32)
    R = search_bounds(geo, gate)["R"] if rings is None else rings
    gg = geo["g"] * f32(0.9999)
    gate_f = f32(gate * gate) * f32(1.0001)
    cp = np.clip(_coords(geo, pts), 0, geo["dim"][None, :] - 1)
    out = np.full(len(q), -1, np.int64)
    step = max(1, (1 << 22) // max(len(pts), 1))
    for lo in range(0, len(q), step):
        qq = q[lo:lo + step]
        cheb = np.abs(_coords(geo, qq)[:, None, :] - cp[None, :, :]).max(2)
        d2 = _sq_dist(qq, pts)
        best = np.full(len(qq), np.inf, np.float32)
        idx = np.full(len(qq), -1, np.int64)
        live = np.ones(len(qq), bool)
        for rr in range(R + 1):
            seen = np.where(cheb <= rr, d2, f32(np.inf))
            k = seen.argmin(1)
            b = seen[np.arange(len(qq)), k]
            idx = np.where(live & np.isfinite(b), k, idx)
            best = np.where(live, b, best)
            reach = f32(rr) * gg
            live &= ~((best < reach * reach) | (reach * reach > gate_f))
            if not live.any():
                break
        out[lo:lo + step] = _gated(best, idx, gate)
    return out


def list_search(geo, q, crop_xyz, gate, kmax=None, segs=None):
    """k_ec_build + the list walk for the queries inside the grid (those outside it: -2).  Per hit cell: D from the cubes
    of min(2, Kmax), min(4, Kmax), Kmax cells -- slabs over every x, so a cube is bounded in y and z alone --, no list
    unless the nearest point is inside a cube's reach and D - r <= gate, else the points within T of the centre (the
    device collects them from slabs that contain that ball); a query takes the nearest of its cell's list.  `kmax`
    replaces Kmax.  `segs`: only the first `segs` slabs of a cube (z offsets -K .. segs - 1 - K) and of the list pass
    (-KT .. segs - 1 - KT) deliver points: what wave_segments_points would see of a walk of more than EC_SEGS segments
    if it stopped after its first round."""
    q, pts = np.asarray(q, np.float32), np.asarray(crop_xyz, np.float32)
    b = search_bounds(geo, gate)
    Kmax = b["Kmax"] if kmax is None else kmax
    g, dim, r, hh, gate_ = geo["g"], geo["dim"], b["r"], b["hh"], b["gate"]
    qc = query_cell(geo, q)
    out = np.where(qc >= 0, -1, -2).astype(np.int64)
    cp = np.clip(_coords(geo, pts), 0, dim[None, :] - 1)
    for c in np.unique(qc[qc >= 0]):
        cc = np.array([c % dim[0], (c // dim[0]) % dim[1], c // (dim[0] * dim[1])])
        m = geo["mn"] + (cc.astype(np.float32) + f32(0.5)) * g
        dd = _sq_dist(m[None, :], pts)[0]
        cheb_yz = np.abs(cp[:, 1:] - cc[None, 1:]).max(1)
        dz = cp[:, 2] - cc[2]
        K, found, best = min(2, Kmax), False, f32(np.inf)
        while True:
            inside = dd[(cheb_yz <= K) & (True if segs is None else dz < segs - K)]
            best = inside.min() if len(inside) else f32(np.inf)
            reach = f32(K) * g + hh
            found = bool(best <= reach * reach * f32(0.999))
            if found or K >= Kmax:
                break
            K = min(4, Kmax) if K < 4 else Kmax
        D = np.sqrt(best)
        if not found or not D - r <= gate_:
            continue
        T = min(D + f32(2.0) * r, gate_ + r) + f32(1.0e-4)
        KT = int(np.ceil((T + hh) * geo["inv_g"]))
        members = np.flatnonzero((dd <= T * T) & (True if segs is None else dz < segs - KT))
        mine = np.flatnonzero(qc == c)
        d2 = _sq_dist(q[mine], pts[members])
        k = d2.argmin(1)
        out[mine] = _gated(d2[np.arange(len(mine)), k], members[k], gate)
    return out

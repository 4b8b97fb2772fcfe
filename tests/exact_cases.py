"""Inputs of the exact nearest-neighbour route tests (tests/test_gpu_exact_routes.py): for every capacity fallback of
pcl_tracking_amd/csrc/pft_exact_nn.hip a deterministic reference cloud, input cloud, particle set and gate that crosses the
capacity, and a numpy float32 restatement of the parts of the device code that decide the route -- the grid geometry
(k_eg_setup), the cell of a point and of a query, the per-cell candidate list length (k_ec_build) and the workgroup's LDS
count table (eq_hash / eq_insert).  tests/test_exact_cases_host.py proves with the oracle alone, on the CPU, that each case
crosses its capacity with a margin of at least 2x, so float differences between this model and the device cannot flip a route.

The capacities below restate pft_internal.h / pft_exact_nn.hip; the GPU tests compare them with what the library reports
(debugExactState) so that a change there cannot go unnoticed here.
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


@functools.lru_cache(maxsize=None)
def build(name, num_cus=NUM_CUS):
    """-> dict(model, cloud, particles, gate, slots): slots is the lowered slot limit or None.  long_lists is the input of the
    pool_grows test as well (two evaluations on one handle)."""
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

"""Named clouds for the input filters (csrc/pft_filters.hip) at the places where the kernels can
go wrong without the ordinary clouds noticing: long voxels across the 1024-point tiles of VoxelGrid's emit, points on
cell faces, cell indices past 2^24, keys that use the fourth radix byte, the INT32_MAX cell-product limit, huge and
infinite coordinates, PassThrough limits hit exactly, every history-table size.  Plain module, no GPU:
tests/test_filter_cases_host.py holds the model (tests/filters_model.py) against the C oracle on every case and checks
the structural condition each case exists for, tests/test_gpu_filters_edges.py runs them on the device.

A case is a `Case`: the cloud (read-only scene.POINT_DTYPE array) and the filter settings.  `expected(impl, case)`
runs the chain PassThrough -> grid with `impl` = the oracle module or the model module (same three function names) and
returns what the device has to report.  The key emulation below (`exact_keys`, `sorted_heads`) is a third, vectorised
statement of VoxelGrid's index, used only for the structural conditions."""
import collections

import numpy as np

from pcl_tracking_amd import scene

F = np.float32
FLT_MAX = float(np.finfo(F).max)
TILE = 1024   # points per workgroup of k_f_emit_exact / k_fa_emit_tile
CHUNK = 256   # points per round of their continuation loops

# mode: "pass" (PassThrough alone), "approx", "exact";  pass_: None or (field, lo, hi, negative)
Case = collections.namedtuple("Case", "name cloud mode leaf hist pass_")


def case(name, cloud, mode, leaf=0.01, hist=512, pass_=None):
    cloud = np.ascontiguousarray(cloud)
    assert cloud.dtype == scene.POINT_DTYPE
    cloud.setflags(write=False)
    return Case(name, cloud, mode, leaf, hist, pass_)


Expected = collections.namedtuple("Expected", "out n_pass pass_idx handed_through")


def expected(impl, c):
    """what PCL's chain gives: PassThrough (when set) feeds the grid; VoxelGrid hands ITS input through when the leaf
    is too small for it.  n_pass / pass_idx: the points that entered the grid (VoxelGrid skips non-finite points, so
    without a PassThrough they are the finite ones; ApproximateVoxelGrid takes every point)."""
    cloud = c.cloud
    idx = None
    if c.pass_ is not None:
        field, lo, hi, neg = c.pass_
        idx = impl.pass_through(cloud, field, lo, hi, negative=neg)
        cloud = cloud[idx]
    if c.mode == "pass":
        return Expected(cloud, len(idx), idx, False)
    if c.mode == "approx":
        return Expected(impl.approx_voxel_grid(cloud, c.leaf, c.hist), len(cloud), idx, False)
    out = impl.voxel_grid(cloud, c.leaf)
    if idx is None:
        idx = np.flatnonzero(finite_mask(cloud)).astype(np.int32)
    return Expected(cloud if out is None else out, len(idx), idx, out is None)


# ---- small tools ---------------------------------------------------------------------------------------------------
def finite_mask(c):
    return np.isfinite(c["x"]) & np.isfinite(c["y"]) & np.isfinite(c["z"])


def make_cloud(x, y, z, rgba):
    c = np.zeros(len(x), scene.POINT_DTYPE)
    c["x"], c["y"], c["z"] = np.asarray(x, F), np.asarray(y, F), np.asarray(z, F)
    c["w"] = 1.0
    c["rgba"] = rgba
    return c


def random_rgba(rng, n):
    return rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)


def random_cloud(n, seed, span=0.3, nan_frac=0.0):
    """the cloud of tests/test_gpu_filters.py: uniform in +-span, z around 1"""
    rng = np.random.default_rng(seed)
    c = np.zeros(n, scene.POINT_DTYPE)
    for k in ("x", "y", "z"):
        c[k] = rng.uniform(-span, span, n).astype(F)
    c["z"] += F(1.0)
    c["w"] = 1.0
    c["rgba"] = random_rgba(rng, n)
    if nan_frac:
        bad = rng.random(n) < nan_frac
        for k in ("x", "y", "z"):
            c[k][bad] = np.nan
    return c


def leaf3(leaf):
    return np.asarray([leaf] * 3 if np.isscalar(leaf) else leaf, F)


def cell_index(v, leaf):
    """floor(v * (1 / leaf)) in float32, as float64 integers (no int conversion: finite inputs only)"""
    inv = F(1) / F(leaf)
    prod = np.asarray(v, F) * inv
    assert prod.dtype == F
    return np.floor(prod).astype(np.float64)


def exact_keys(cloud, leaf):
    """VoxelGrid's voxel index of every finite point, in input order (clouds whose grid fits: no overflow anywhere)"""
    lf = leaf3(leaf)
    fin = finite_mask(cloud)
    cells = np.stack([cell_index(cloud[k][fin], lf[a]) for a, k in enumerate("xyz")], 1)
    lo = cells.min(0)
    div = cells.max(0) - lo + 1
    rel = np.stack([(cells[:, a].astype(F) - F(lo[a])).astype(np.int64) for a in range(3)], 1)
    assert div.prod() <= 2**31 - 1
    return rel[:, 0] + rel[:, 1] * int(div[0]) + rel[:, 2] * int(div[0] * div[1])


def sorted_heads(cloud, leaf):
    """positions, in the sorted order of the kept points, at which a voxel begins;  and the number of kept points"""
    keys = np.sort(exact_keys(cloud, leaf))
    return np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]]), len(keys)


def scatter_nan(rng, cloud, k):
    """k all-NaN points inserted at scattered positions"""
    at = np.sort(rng.choice(len(cloud) + 1, k, replace=False))
    bad = np.zeros(k, scene.POINT_DTYPE)
    for f in ("x", "y", "z"):
        bad[f] = np.nan
    bad["w"] = 1.0
    bad["rgba"] = random_rgba(rng, k)
    return np.insert(cloud, at, bad)


# ---- VoxelGrid: long voxels ------------------------------------------------------------------------------------------
LONG_RUNS = [1024, 1, 1279, 5000, 3, 255, 257, 700, 2500, 1]
LONG_RUN_HEADS = [0, 1024, 1025, 2304, 7304, 7307, 7562, 7819, 8519, 11019]
LONG_RUNS_KEPT = 11020


def exact_long_runs(white=False):
    """One voxel per run, run r in z cell r (z is the slowest axis of the index, so the runs sort in this order), the
    whole cloud shuffled -- the radix sort has to bring every voxel's points back together AND keep them in input
    order -- and 37 NaN points scattered through it, whose dropped keys sort behind the last run.  `white`: every
    colour byte 255, the largest channel sums (5000 x 255 < 2^24, exact in float).
    In sorted order: a head on a tile start (1024); a run that ends one whole 256-point round past its tile (1025 ..
    2304); tiles 3, 4, 5, 6 and 9 without a head; a continuation of 17 rounds; a short last tile."""
    rng = np.random.default_rng(11)
    n = sum(LONG_RUNS)
    xy = rng.integers(0, 6, (len(LONG_RUNS), 2))
    cell = np.repeat(np.c_[xy, np.arange(len(LONG_RUNS))], LONG_RUNS, axis=0)
    jit = rng.uniform(0.05, 0.95, (n, 3))
    pos = ((cell + jit) * 0.01).astype(F)
    rgba = np.full(n, 0xFFFFFFFF, np.uint32) if white else random_rgba(rng, n)
    c = make_cloud(pos[:, 0], pos[:, 1], pos[:, 2], rgba)[rng.permutation(n)]
    c = scatter_nan(rng, c, 37)
    heads, kept = sorted_heads(c, 0.01)
    assert heads.tolist() == LONG_RUN_HEADS and kept == LONG_RUNS_KEPT and len(c) == kept + 37
    return case("exact_long_runs" + ("_white" if white else ""), c, "exact")


def long_run_structure(heads, kept):
    """the paths of k_f_emit_exact that a sorted layout reaches"""
    heads = np.asarray(heads)
    ends = np.r_[heads[1:], kept]
    ntiles = -(-kept // TILE)
    tiles_with_head = set((heads // TILE).tolist())
    past_tile = ends - (heads // TILE + 1) * TILE  # how far a run reaches past the end of the tile it starts in
    return dict(
        head_free_tiles=[t for t in range(ntiles) if t not in tiles_with_head],
        head_on_tile_start=[int(h) for h in heads if h and h % TILE == 0],
        whole_rounds_past_tile=[int(p) // CHUNK for p in past_tile if p >= CHUNK and p % CHUNK == 0],
        longest=int((ends - heads).max()),
        max_rounds=int(-(-past_tile.max() // CHUNK)),
        short_last_tile=kept % TILE != 0,
    )


def _one_voxel_cloud():
    c = random_cloud(20000, 5, span=0.004)
    c["x"] = np.abs(c["x"])
    c["y"] = np.abs(c["y"])
    c["z"] = F(1.001) + np.abs(c["z"] - 1) * F(0.5)
    return c


def exact_one_voxel(mode="exact"):
    """20 000 points of one voxel: 19 tiles without a head behind the first, one run of 75 rounds"""
    c = _one_voxel_cloud()
    assert len(np.unique(exact_keys(c, 0.01))) == 1
    return case("one_voxel_" + mode, c, mode)


def exact_one_voxel_behind_pass(mode="exact"):
    """the same points, 7 of them lifted over a PassThrough limit (still inside the voxel): the run ends at n_pass =
    19 993, inside the last tile, with the 7 dropped keys sorted behind it"""
    c = _one_voxel_cloud()
    c["z"][[3, 1024, 5000, 5001, 12287, 19000, 19999]] = F(1.0095)
    assert len(np.unique(exact_keys(c, 0.01))) == 1
    c = case("one_voxel_behind_pass_" + mode, c, mode, pass_=("z", 0.0, 1.005, False))
    assert int((c.cloud["z"] <= F(1.005)).sum()) == 20000 - 7
    return c


# ---- value-space edges -----------------------------------------------------------------------------------------------
FACE_K = np.arange(-60, 61)


def face_values(leaf):
    """float32(k) * float32(leaf), k = -60 .. 60: the cell faces as a float program would write them"""
    v = FACE_K.astype(F) * F(leaf)
    assert v.dtype == F
    return v


def face_landing(leaf):
    """how many of the 121 face floats land in cell k - 1, in cell k, elsewhere"""
    got = cell_index(face_values(leaf), leaf)
    below, at = int((got == FACE_K - 1).sum()), int((got == FACE_K).sum())
    return below, at, len(FACE_K) - below - at


def cell_faces(leaf, mode):
    """every face float and its two float neighbours on every axis, 11 times each, the axes shuffled independently"""
    lf = leaf3(leaf)
    rng = np.random.default_rng(21)
    cols = []
    for a in range(3):
        v = face_values(lf[a])
        vals = np.concatenate([v, np.nextafter(v, F(-np.inf)), np.nextafter(v, F(np.inf))])
        assert vals.dtype == F
        cols.append(rng.permutation(np.tile(vals, 11)))
    c = make_cloud(cols[0], cols[1], cols[2], random_rgba(rng, len(cols[0])))
    return case("cell_faces_%s_%s" % ("iso" if np.isscalar(leaf) else "aniso", mode), c, mode, leaf=leaf)


# three denormals whose product with 100 is a denormal too, the largest denormal, two tiny normal floats
DENORMALS = np.asarray([1, 71362, 0x7FFF, 0x7FFFFF, 0x800000, 0xA00000], np.uint32).view(F)


def denormal_cells(mode):
    """x and y are denormal floats (whose product with 100 still is) or tiny normal ones, of both signs, and the two
    zeros: a negative value, however small, lies in cell -1, and the sums of a voxel add denormals.  A device that
    flushed them to zero would merge the two cells and change the centroids."""
    rng = np.random.default_rng(25)
    n = 1200
    vals = np.concatenate([DENORMALS, -DENORMALS, np.asarray([0.0, -0.0], F)])
    i = np.arange(n)
    c = make_cloud(vals[i % len(vals)], vals[rng.integers(0, len(vals), n)], rng.uniform(-0.03, 0.03, n), random_rgba(rng, n))
    return case("denormal_cells_" + mode, c, mode)


def far_narrow(mode, mirror=False):
    """a 10 cm slab 2 km from the origin at leaf 1e-4: cell indices around 2e7, where floats are 2 apart, so
    floor(x * inv) - (float) min_b is taken between even numbers"""
    rng = np.random.default_rng(31)
    n = 3000
    x = rng.uniform(1999.95, 2000.05, n)
    c = make_cloud(-x if mirror else x, rng.uniform(-0.005, 0.005, n), rng.uniform(-0.005, 0.005, n), random_rgba(rng, n))
    return case("far_narrow_%s%s" % (mode, "_mirror" if mirror else ""), c, mode, leaf=1e-4)


def product_limit(cells):
    """600 points over a cube of (cells - 0.5) leaves, a point in each extreme corner: cells^3 voxels"""
    rng = np.random.default_rng(41)
    side = (cells - 0.5) * 0.01
    p = rng.uniform(0.0, side, (600, 3))
    p[17] = 0.0
    p[401] = side
    c = make_cloud(p[:, 0], p[:, 1], p[:, 2], random_rgba(rng, 600))
    return case("product_limit_%d" % cells, c, "exact")


def product_limit_two_factors():
    """50 000 x 50 000 x 1 cells: the first two factors alone exceed INT32_MAX (each stays below 2^31, and the
    product of the three below 2^63)"""
    rng = np.random.default_rng(42)
    p = rng.uniform(0.0, 499.995, (600, 3))
    p[:, 2] = rng.uniform(0.001, 0.009, 600)
    p[5, :2] = 0.0
    p[590, :2] = 499.995
    c = make_cloud(p[:, 0], p[:, 1], p[:, 2], random_rgba(rng, 600))
    return case("product_limit_two_factors", c, "exact")


def cell_extents(cloud, leaf):
    """(int64_t)((max - min) * inv) + 1 per axis, as Python ints"""
    lf = leaf3(leaf)
    fin = finite_mask(cloud)
    out = []
    for a, k in enumerate("xyz"):
        d = (cloud[k][fin].max() - cloud[k][fin].min()) * (F(1) / lf[a])
        assert d.dtype == F
        out.append(int(d) + 1)
    return out


def huge_and_inf(mode, behind_pass=False, big=(3e7, -4e8)):
    """2 000 points in +-0.3 with coordinates far outside the int range of cell indices (every 7th x = 3e7: 3e9 cells;
    a strided y = -4e8) and infinite ones (x = +inf, z = -inf): floor_to_int answers INT_MIN, sums turn inf or NaN.
    Behind a PassThrough the non-finite points drop out and the huge ones stay; VoxelGrid then finds its leaf too small
    and hands the PassThrough's output on.  For that case pass big = (3e6, -4e6): 3e8 x 4e8 x 61 cells, so the oracle's
    product of three int64 stays below 2^63 (with the defaults it would overflow, which C leaves undefined)."""
    rng = np.random.default_rng(51)
    n = 2000
    p = rng.uniform(-0.3, 0.3, (n, 3)).astype(F)
    i = np.arange(n)
    p[i % 7 == 0, 0] = big[0]
    p[i % 11 == 3, 1] = big[1]
    p[i % 53 == 5, 0] = np.inf
    p[i % 61 == 7, 2] = -np.inf
    p[1000:1020] = [big[0], big[1], -np.inf]  # twenty points of voxel (INT_MIN, INT_MIN, INT_MIN) ...
    p[1000:1020:2, 0] = np.inf                # ... whose x sum meets +inf and -inf: a NaN centroid
    p[1001:1020:2, 0] = -np.inf
    c = make_cloud(p[:, 0], p[:, 1], p[:, 2], random_rgba(rng, n))
    name = "huge_and_inf_%s%s" % (mode, "_behind_pass" if behind_pass else "")
    return case(name, c, mode, pass_=("z", -1.0, 1.0, False) if behind_pass else None)


def pass_edge_values(lo, hi):
    lo, hi = F(lo), F(hi)
    up, down = F(np.inf), F(-np.inf)
    tiny = np.asarray([1, 71362, 0x7FFFFF], np.uint32).view(F)  # smallest, a middle and the largest denormal
    with np.errstate(over="ignore"):  # the neighbour of FLT_MAX is inf: a non-finite field value, dropped
        near = [np.nextafter(lo, down), np.nextafter(lo, up), np.nextafter(hi, down), np.nextafter(hi, up)]
    v = [lo, hi] + near
    v += [F(0.0), F(-0.0), F(FLT_MAX), F(-FLT_MAX), F(np.finfo(F).tiny), -F(np.finfo(F).tiny), F(5.0), F(-5.0), F(10.5)]
    v += list(tiny) + list(-tiny)
    return np.asarray(v, F)


def pass_edges(field, lo, hi, negative):
    """1 500 points (tiles are partial) whose filter field cycles through the limits, their float neighbours, the two
    zeros, +-FLT_MAX, denormals and a few ordinary values; the second half repeats them with a NaN or an infinity in
    one of the OTHER two fields (such a point is dropped whatever the limits say), and a few field values are
    themselves non-finite"""
    rng = np.random.default_rng(61)
    n = 1500
    vals = pass_edge_values(lo, hi)
    cols = {k: rng.uniform(-1.0, 1.0, n).astype(F) for k in "xyz"}
    i = np.arange(n)
    cols[field] = vals[i % len(vals)]
    others = [k for k in "xyz" if k != field]
    half = np.flatnonzero(i >= n // 2)
    poison = np.asarray([np.nan, np.inf, -np.inf], F)
    for j in half[::2]:
        cols[others[(j // 2) % 2]][j] = poison[(j // 4) % 3]
    cols[field][[100, 613, 999]] = poison
    c = make_cloud(cols["x"], cols["y"], cols["z"], random_rgba(rng, n))
    name = "pass_edges_%s_%g_%g_%s" % (field, lo, hi, "neg" if negative else "pos")
    return case(name, c, "pass", pass_=(field, float(lo), float(hi), bool(negative)))


PASS_LIMITS = [(0.0, 10.0), (10.0, 0.0), (-FLT_MAX, FLT_MAX)]


# ---- ApproximateVoxelGrid: every table size -------------------------------------------------------------------------
HIST_SIZES = [1 << k for k in range(12)]


def long_runs_cloud(seed):
    """the cloud of test_approx_voxel_grid_long_runs_across_tiles (tests/test_gpu_filters.py): consecutive runs of one
    voxel, 1 .. 2500 points long, over few voxels, so that table entries collide and flush each other"""
    rng = np.random.default_rng(seed)
    lens = rng.choice([1, 2, 3, 7, 60, 255, 256, 257, 700, 1024, 2500], 120)
    vox = rng.integers(0, 40, (len(lens), 3))
    cell = np.repeat(vox, lens, axis=0)
    n = len(cell)
    c = np.zeros(n, scene.POINT_DTYPE)
    jit = rng.uniform(0.05, 0.95, (n, 3))
    for a, k in enumerate(("x", "y", "z")):
        c[k] = ((cell[:, a] + jit[:, a]) * 0.01).astype(F)
    c["w"] = 1.0
    c["rgba"] = random_rgba(rng, n)
    return c


def hist_sizes(hist):
    return case("hist_%d" % hist, long_runs_cloud(0), "approx", hist=hist)


# ---- PassThrough fused with either grid ------------------------------------------------------------------------------
PAIRING_PASSES = [("x", -0.1, 0.2, False), ("y", -0.25, 0.05, False), ("z", 0.9, 1.1, True)]


def pairings(pass_, mode):
    c = random_cloud(5000, 71, nan_frac=0.05)
    return case("pairing_%s%s_%s" % (pass_[0], "_neg" if pass_[3] else "", mode), c, mode, pass_=pass_)


def nan_cloud():
    """5 % NaN points in front of a VoxelGrid without PassThrough"""
    return case("exact_nan", random_cloud(5000, 81, nan_frac=0.05), "exact")


# ---- the lists the two test files run --------------------------------------------------------------------------------
def grid_cases():
    """every case that compares bit for bit (builders are called at collection: keep them cheap)"""
    out = [exact_long_runs(), exact_long_runs(white=True), nan_cloud()]
    for mode in ("exact", "approx"):
        out += [exact_one_voxel(mode), exact_one_voxel_behind_pass(mode)]
        out += [cell_faces(0.01, mode), cell_faces((0.05, 0.02, 0.1), mode)]
        out += [far_narrow(mode), far_narrow(mode, mirror=True), denormal_cells(mode)]
        out += [pairings(p, mode) for p in PAIRING_PASSES]
    out += [product_limit(1290), product_limit(1291), product_limit_two_factors()]
    out += [huge_and_inf("approx", behind_pass=True), huge_and_inf("exact", behind_pass=True, big=(3e6, -4e6))]
    out += [hist_sizes(h) for h in HIST_SIZES]
    return out


def pass_cases():
    return [pass_edges(f, lo, hi, neg) for f in "xyz" for lo, hi in PASS_LIMITS for neg in (False, True)]


REUSE_SIZES = [5000, 300, 20000, 1, 0, 1025, 11057]


def reuse_clouds():
    """clouds of very different sizes for one handle, in this order: the per-point state a longer cloud leaves behind
    (keys, heads, tile counts) lies under every shorter one that follows, and a handle created small has to grow twice"""
    out = [random_cloud(5000, 91, nan_frac=0.05), random_cloud(300, 92), _one_voxel_cloud(), random_cloud(1, 93),
           random_cloud(0, 94), random_cloud(1025, 95, nan_frac=0.05), exact_long_runs().cloud]
    assert [len(c) for c in out] == REUSE_SIZES
    return out


REUSE_MODES = {  # mode of the handle, PassThrough in front (a limit that drops part of every cloud above)
    "pass": ("pass", ("y", 0.002, 0.25, False)),
    "approx": ("approx", None),
    "exact": ("exact", None),
    "exact_pass": ("exact", ("y", 0.002, 0.25, False)),
}

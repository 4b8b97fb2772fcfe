"""Adversarial geometry for the Euclidean clustering stage of model creation (csrc/pft_segment.hip section 6, DESIGN.md
section 3.7) and a brute-force reference of RULE link / size / order that shares nothing with the device's cell grid or
with cKDTree.  Plain module, no GPU: tests/test_cluster_cases_host.py checks the builders and the reference,
tests/test_gpu_cluster_topology.py runs the cases on the device.

Every builder returns (cloud, tol, min_size, max_size, expected): `cloud` a read-only scene.POINT_DTYPE array, `expected`
the list of input-index arrays in cluster order, or None where the device has to refuse the cloud.  All real points lie
outside RULE zero's cube (z >= 1) and carry a distinct rgba; unless the case says otherwise about 2 % NaN points and a
few points inside the cube are interleaved, so survivor index != input index.  `info`, when a dict is passed, receives
what the builder verified about its own cloud.

The exact-arithmetic cases use tol = 0.25 and coordinates on a binary lattice (2^-6, or 2^-10 where a cell, which is
0.12890625 = 132 * 2^-10 wide, has to be addressed): differences, their squares and the sum are exact in float32, so
"just below" and "at" the tolerance are decidable."""
import functools

import numpy as np

from pcl_tracking_amd import scene

F = np.float32
CELL_SLACK = 1.03125     # cell side = tol / 2 * (1 + 2^-5), the documented cell rule above cell_coord
U = 2.0 ** -10           # lattice unit of the cell-addressed cases
CELL_U = 132             # one cell of tol = 0.25 in units of U
MAX_AXIS_CELLS = 1 << 17
MAX_GRID_CELLS = 2 ** 32 - 1   # grids of this many cells or more are refused


# ---- the reference ------------------------------------------------------------------------------------------------
def link_matrix_rows(xyz, i0, i1, tol2):
    """rows i0..i1 of RULE link over all points: ((dx dx + dy dy) + dz dz) < tol2, every product and sum rounded to
    float32, strict"""
    a = xyz[i0:i1]
    dx = a[:, None, 0] - xyz[None, :, 0]
    dy = a[:, None, 1] - xyz[None, :, 1]
    dz = a[:, None, 2] - xyz[None, :, 2]
    assert dx.dtype == F
    return ((dx * dx + dy * dy) + dz * dz) < tol2


def brute_clusters(xyz, tol, min_size, max_size, block=256):
    """RULE link / size / order by all pairs: -> list of ascending index arrays into xyz (finite float32 [n, 3]), kept
    iff min_size <= size <= max_size, by size descending, ties by smallest index.  Pairs are tested in row blocks, the
    components of the pair graph come from scipy.sparse.csgraph."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    xyz = np.ascontiguousarray(xyz, F)
    n = len(xyz)
    if n == 0:
        return []
    assert np.isfinite(xyz).all()
    tol2 = F(tol * tol)
    rows, cols = [], []
    for i0 in range(0, n, block):
        r, c = np.nonzero(link_matrix_rows(xyz, i0, min(i0 + block, n), tol2))
        r += i0
        keep = c > r
        rows.append(r[keep])
        cols.append(c[keep])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    _, lab = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n)), directed=False)
    return _order(lab, np.arange(n, dtype=np.int64), min_size, max_size)


def _order(label, index, min_size, max_size):
    """RULE size / order over points `index` (ascending) with component labels `label`"""
    if len(index) == 0:
        return []
    o = np.argsort(label, kind="stable")
    cut = np.flatnonzero(np.diff(label[o])) + 1
    groups = [g for g in np.split(index[o], cut) if min_size <= len(g) <= max_size]
    groups.sort(key=lambda g: (-len(g), int(g[0])))
    return groups


# ---- the documented cell rule, restated -------------------------------------------------------------------------------
def cell_coords(xyz, tol):
    """floor((v - min) * float32(2 / (tol * 1.03125))) per axis in float32, min over the points given (the survivors)"""
    xyz = np.asarray(xyz, F)
    inv = F(2.0 / (tol * CELL_SLACK))
    lo = xyz.min(axis=0)
    return np.floor(((xyz - lo).astype(F) * inv).astype(F)).astype(np.int64)


def grid_dims(xyz, tol):
    return cell_coords(xyz, tol).max(axis=0) + 1


def cell_sorted_keys(xyz, tol):
    """the cell keys ix + nx (iy + ny iz) in cell-sorted order"""
    c = cell_coords(xyz, tol)
    d = c.max(axis=0) + 1
    return np.sort(c[:, 0] + d[0] * (c[:, 1] + d[1] * c[:, 2]))


# ---- assembling a cloud ---------------------------------------------------------------------------------------------
def assemble(xyz, seed, drop=True):
    """-> (cloud, index): the real points `xyz` in the order given, with about 2 % NaN points (at least 4) and 3 points
    inside RULE zero's cube interleaved at seeded positions when `drop`; index[k] = input index of real point k.  Every
    point has a distinct rgba."""
    xyz = np.asarray(xyz, F)
    n = len(xyz)
    assert n == 0 or xyz[:, 2].min() >= 1.0
    rng = np.random.default_rng(seed)
    n_nan = max(4, n // 50) if drop else 0
    n_zero = 3 if drop else 0
    total = n + n_nan + n_zero
    where = np.sort(rng.choice(total, n_nan + n_zero, replace=False)) if drop else np.zeros(0, np.int64)
    real = np.ones(total, bool)
    real[where] = False
    index = np.flatnonzero(real)
    cloud = np.zeros(total, scene.POINT_DTYPE)
    cloud["w"] = 1.0
    cloud["rgba"] = (np.arange(total, dtype=np.uint64) * 2654435761 + 12345).astype(np.uint32)  # odd multiplier: distinct
    for k, a in enumerate("xyz"):
        cloud[a][index] = xyz[:, k]
    if drop:
        kind = rng.permutation(n_nan + n_zero) < n_zero  # which of the dropped points lie in the cube
        zero, nan = where[kind], where[~kind]
        for a in "xyz":
            cloud[a][zero] = rng.integers(-9, 10, len(zero)) * F(2.0 ** -10)   # |v| <= 0.0088 < 0.01
            cloud[a][nan] = rng.uniform(1.0, 2.0, len(nan)).astype(F)
        axis = rng.integers(0, 3, len(nan))
        for k, a in enumerate("xyz"):
            cloud[a][nan[axis == k]] = np.nan
    cloud.flags.writeable = False
    return cloud, index


def cloud_xyz(cloud):
    return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(F)


def _from_brute(xyz, index, tol, min_size, max_size):
    return [index[c] for c in brute_clusters(xyz, tol, min_size, max_size)]


def _from_groups(group, index, min_size, max_size):
    """analytic expectation: real point k belongs to component group[k]"""
    return _order(np.asarray(group, np.int64), index, min_size, max_size)


# ---- a. offsets ----------------------------------------------------------------------------------------------------------
OFFSETS = [(dx, dy, dz) for dz in range(-2, 3) for dy in range(-2, 3) for dx in range(-2, 3) if (dx, dy, dz) != (0, 0, 0)]
FAR_CELLS = 124000   # the far copy's anchor lies this many cells below the set on x


def offsets(far=False, info=None):
    """For each of the 124 non-zero offsets in {-2..2}^3 one pair whose cells differ by exactly that offset and whose
    distance is below tol = 0.25, and a control pair with the same cell offset at distance >= tol (exactly tol for the
    six axis offsets of one cell), every pair in a slot of its own, the slots 13 cells apart (at least 4 tol between two
    pairs).  In units of 2^-10 a cell is 132 wide: the linking pair sits at 128 / 4 / 66 of its cells on axes where the
    offset is positive / negative / zero and the mirrored position of the target cell (1.06 cells apart for an offset
    of 2: the corner pair is at 0.947 tol); the control pair at 4 / 128 / 66 and mirrored (1.94 cells).  The first slot's
    control pair has offset (-2, -2, -2), and its second point is moved 4 units further out: it alone is the minimum on
    every axis, at a cell
    corner, and every other point stays 4 units (0.03 cells) or more inside its cell, above the 0.012 cells the float
    roundings of the cell rule can move a point 124 000 cells out.
    far: the whole set is translated by 124 000 cells along x, to x ~ 15 985, and an anchor point at x ~ 0.5 (a
    singleton) takes over the cell corner: the x axis spans more than 120 000 of the 2^17 cells allowed.
    Expected, from brute force: 124 clusters of two and 248 single points (249 with the anchor), min_size 1."""
    slots = [((-2, -2, -2), True)] + [(o, False) for o in OFFSETS] + [(o, True) for o in OFFSETS if o != (-2, -2, -2)]
    pts, pair_of = [], []
    for s, (off, control) in enumerate(slots):
        base = np.array([s % 8, (s // 8) % 8, s // 64], np.int64) * (13 * CELL_U) + 2 * CELL_U
        a, b = base.copy(), base + np.array(off) * CELL_U
        for k in range(3):
            d = off[k]
            pa = 66 if d == 0 else ((128 if d > 0 else 4) if not control else (4 if d > 0 else 128))
            a[k] += pa
            b[k] += 66 if d == 0 else CELL_U - pa
        pts += [a, b]
        pair_of.append((len(pts) - 2, len(pts) - 1, off, control))
    pts = np.array(pts, np.int64)
    if far:
        pts = np.concatenate([pts, (pts[1] - 4 - [FAR_CELLS * CELL_U, 0, 0])[None]])
    else:
        pts[1] -= 4
    origin = np.array([512 + FAR_CELLS * CELL_U if far else 1024, 1024, 1024], np.int64)
    xyz = ((pts + origin) * U).astype(F)
    assert np.array_equal(xyz.astype(np.float64), (pts + origin) * U)  # exact in float32
    order = np.random.default_rng(31).permutation(len(xyz))
    inv = np.argsort(order)
    xyz = xyz[order]
    cloud, index = assemble(xyz, 32)
    tol = 0.25
    if info is not None:
        cells = cell_coords(xyz, tol)
        tol2 = F(tol * tol)
        link, ctrl = set(), set()
        for ia, ib, off, control in pair_of:
            ia, ib = inv[ia], inv[ib]
            got = tuple(int(v) for v in cells[ib] - cells[ia])
            d = (xyz[ia] - xyz[ib]).astype(F)
            below = bool(F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < tol2)
            if got == off and below and not control:
                link.add(got)
            if got == off and not below and control:
                ctrl.add(got)
        info.update(link_offsets=link, control_offsets=ctrl, dims=grid_dims(xyz, tol))
    return cloud, tol, 1, 100, _from_brute(xyz, index, tol, 1, 100)


# ---- b. chains -------------------------------------------------------------------------------------------------------
CHAIN_N = 20000
CHAIN_STEP = 0.25 - 2.0 ** -6


def _bit_reversed(n):
    bits = max(1, (n - 1).bit_length())
    i = np.arange(1 << bits)
    r = np.zeros_like(i)
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r[r < n]


def chain_order(name, n):
    if name == "ascending":
        return np.arange(n)
    if name == "descending":
        return np.arange(n)[::-1].copy()
    if name == "random":
        return np.random.default_rng(41).permutation(n)
    assert name == "bit_reversed"
    return _bit_reversed(n)


def chains(order="ascending", gap=False, info=None):
    """20 000 points at spacing 0.25 - 2^-6 along x (coordinates on the 2^-6 lattice), one point per cell over about
    36 000 cells; cloud position p holds chain element chain_order(order)[p].  One cluster of 20 000.
    gap: the step from element 9 999 to 10 000 is exactly 0.25: two clusters of 10 000, a tie in size, so the one that
    holds the smaller input index comes first."""
    k = np.arange(CHAIN_N)
    x = 1.0 + CHAIN_STEP * k + (2.0 ** -6 if gap else 0.0) * (k >= CHAIN_N // 2)
    o = chain_order(order, CHAIN_N)
    xyz = np.stack([x, np.full(CHAIN_N, 1.0), np.full(CHAIN_N, 2.0)], 1)[o].astype(F)
    cloud, index = assemble(xyz, 42)
    group = (o >= CHAIN_N // 2).astype(np.int64) if gap else np.zeros(CHAIN_N, np.int64)
    if info is not None:
        info.update(dims=grid_dims(xyz, 0.25), cells=len(np.unique(cell_sorted_keys(xyz, 0.25))))
    return cloud, 0.25, 1, 10 ** 6, _from_groups(group, index, 1, 10 ** 6)


def spiral(info=None):
    """a square spiral in the xy plane, step 0.25 - 2^-6, arms three steps apart (0.70 > tol), 19 927 points stored in a
    seeded random order: one cluster, and the grid has ny > 1"""
    p, pts, d = np.array([0, 0]), [np.array([0, 0])], 0
    dirs = [(1, 0), (0, 1), (-1, 0), (0, -1)]
    for arm in range(1, 82):
        for _ in range(2):
            for _ in range(3 * arm):
                p = p + dirs[d % 4]
                pts.append(p)
            d += 1
    pts = np.array(pts, np.float64) * CHAIN_STEP + 40.0
    xyz = np.c_[pts, np.full(len(pts), 2.0)].astype(F)
    xyz = xyz[np.random.default_rng(43).permutation(len(xyz))]
    cloud, index = assemble(xyz, 44)
    if info is not None:
        info.update(dims=grid_dims(xyz, 0.25), n=len(xyz))
    return cloud, 0.25, 1, 10 ** 6, _from_groups(np.zeros(len(xyz), np.int64), index, 1, 10 ** 6)


# ---- c. crowded cells -------------------------------------------------------------------------------------------------
def crowded_cells(info=None):
    """Two sets of two cells, 2 apart on x, 256 points in each cell.  In the first set the only pair below tol between
    the two cells is the pair of the highest survivor indices of both (the last pair the link kernel's loops reach):
    at 128 and 4 units of their cells on x, 1.06 cells apart, while the other 255 points of each cell stay within the 8
    units farthest from the other cell (>= 256 units = tol from every point of the other cell).  In the control set,
    12 cells up on y, the two last points stay back as well: no pair below tol.  The points of a cell link among
    themselves (the cell's diagonal is 0.893 tol): one cluster of 512, then two of 256 (a tie)."""
    g = np.array([(x, 16 * y, 16 * z) for z in range(4) for y in range(8) for x in range(8)], np.int64)[:255]
    sets = []
    for s in range(2):
        y0 = s * 12 * CELL_U
        a = g + [0, y0, 0]
        b = g + [2 * CELL_U + 124, y0, 0]
        la = np.array([128 if s == 0 else 8, y0 + 66, 33])
        lb = np.array([2 * CELL_U + (4 if s == 0 else 123), y0 + 66, 33])
        sets.append((a, b, la, lb))
    crowd = np.concatenate([np.concatenate([a, b]) for a, b, _, _ in sets])
    group = np.concatenate([np.full(510, 0), np.full(255, 1), np.full(255, 2)])
    o = np.random.default_rng(51).permutation(len(crowd))
    pts = np.concatenate([crowd[o], [sets[0][2], sets[0][3], sets[1][2], sets[1][3]]])
    group = np.concatenate([group[o], [0, 0, 1, 2]])
    xyz = ((pts + 1024) * U).astype(F)
    cloud, index = assemble(xyz, 52)
    if info is not None:
        tol2 = F(0.25 * 0.25)
        cells = cell_coords(xyz, 0.25)
        below = []
        for s in range(2):
            ia = np.flatnonzero((group == (0 if s == 0 else 1)) & (cells[:, 0] == 0))
            ib = np.flatnonzero((group == (0 if s == 0 else 2)) & (cells[:, 0] == 2))
            near = link_matrix_rows(np.concatenate([xyz[ia], xyz[ib]]), 0, len(ia), tol2)[:, len(ia):]
            below.append([(int(ia[r]), int(ib[c])) for r, c in zip(*np.nonzero(near))])
            info["cell_counts_%d" % s] = (len(ia), len(ib))
            info["last_%d" % s] = (int(ia.max()), int(ib.max()))
        info.update(below=below, cells=len(np.unique(cells, axis=0)))
    return cloud, 0.25, 1, 10 ** 6, _from_groups(group, index, 1, 10 ** 6)


# ---- d. size rule -----------------------------------------------------------------------------------------------------
BLOB_SIZES = (4, 5, 5, 17, 40, 40, 41)


def size_rule(min_size=5, max_size=40, info=None):
    """Tight blobs of 4, 5, 5, 17, 40, 40 and 41 points, each inside one cell, 12 cells apart on x, their members
    interleaved in index order by a seeded permutation.  min 5, max 40 keeps 40, 40, 17, 5, 5; min = max = 5 (no key
    bits in the order sort) keeps the two blobs of 5; min 1, max 10^6 keeps all seven."""
    pts, group = [], []
    for b, n in enumerate(BLOB_SIZES):
        k = np.arange(n)
        pts.append(np.stack([b * 12 * CELL_U + 8 * (k % 8), 8 * ((k // 8) % 8), 8 * (k // 64) + 0 * k], 1))
        group.append(np.full(n, b))
    pts, group = np.concatenate(pts), np.concatenate(group)
    o = np.random.default_rng(61).permutation(len(pts))
    pts, group = pts[o], group[o]
    xyz = ((pts + 1024) * U).astype(F)
    cloud, index = assemble(xyz, 62)
    if info is not None:
        cells = cell_coords(xyz, 0.25)
        info.update(cells_per_blob=[len(np.unique(cells[group == b], axis=0)) for b in range(len(BLOB_SIZES))])
    return cloud, 0.25, min_size, max_size, _from_groups(group, index, min_size, max_size)


def isolated(info=None):
    """30 000 points on a 100 x 100 x 3 lattice of pitch 0.5 = 2 tol, in a seeded random order, min = max = 1:
    30 000 clusters of one, in index order"""
    k = np.arange(30000)
    xyz = np.stack([1.0 + 0.5 * (k % 100), 1.0 + 0.5 * ((k // 100) % 100), 1.0 + 0.5 * (k // 10000)], 1).astype(F)
    xyz = xyz[np.random.default_rng(63).permutation(len(xyz))]
    cloud, index = assemble(xyz, 64)
    return cloud, 0.25, 1, 1, _from_groups(np.arange(len(xyz)), index, 1, 1)


# ---- e. tile edges ----------------------------------------------------------------------------------------------------
TILE = 1024
TILE_EDGE_M = (1, 2, 1023, 1024, 1025, 4095, 4097)


def tile_edges(m, info=None):
    """Seeded "blobs + dust" at tol = 0.02 with exactly m survivors: five Gaussian blobs (sigma 8 mm, 90 % of the points,
    the first blob half of them), a clump of six within a millimetre or two above everything else (the last cell of the
    cell-sorted order) and uniform dust in a 1 m cube, in a seeded random order.  Above 1 024 points one
    cell's run of points straddles position 1 024 of the cell-sorted order, and from 1 023 points on the largest cluster
    has members in every tile of 1 024 survivors; the builder checks both.  m = 1 is a single point, m = 2 a linked pair.
    min_size is 2 from 1 023 points on (the dust drops out), 1 below.  Expected from brute force."""
    tol = 0.02
    if m <= 2:
        xyz = np.array([[0.5, 0.25, 1.5], [0.5, 0.265, 1.5]], F)[:m]
        cloud, index = assemble(xyz, 70 + m)
        if info is not None:
            info.update(m=m, straddles=False, tiles=1)
        return cloud, tol, 1, 10 ** 6, _from_brute(xyz, index, tol, 1, 10 ** 6)
    for seed in range(700, 720):
        rng = np.random.default_rng(seed + m)
        nb = (m * 9) // 10
        sizes = [nb // 2] + [nb // 8] * 3
        sizes.append(nb - sum(sizes))
        parts = [rng.uniform(0.2, 0.8, 3) + [0, 0, 1] + rng.normal(0, 0.008, (s, 3)) for s in sizes]
        parts.append(np.r_[rng.uniform(0.2, 0.8, 2), 2.1] + rng.normal(0, 0.0005, (6, 3)))  # above all the rest
        parts.append(rng.uniform(0, 1, (m - nb - 6, 3)) + [0, 0, 1])
        xyz = np.concatenate(parts).astype(F)
        xyz[0] = np.median(parts[0], axis=0)  # the middle of the first blob is stored last: the last tile has a member
        xyz = xyz[np.r_[1 + rng.permutation(m - 1), 0]]
        keys = cell_sorted_keys(xyz, tol)
        if m <= TILE or keys[TILE - 1] == keys[TILE]:
            break
    else:
        raise AssertionError("no seed puts a cell across position 1024")
    assert len(xyz) == m
    cloud, index = assemble(xyz, 71 + m)
    expected = _from_brute(xyz, index, tol, 2, 10 ** 6)
    rank = np.searchsorted(index, expected[0])  # survivor indices of the largest cluster
    tiles = np.unique(rank // TILE)
    assert len(tiles) == (m + TILE - 1) // TILE, "the largest cluster misses a tile"
    if info is not None:
        info.update(m=m, straddles=bool(m > TILE and keys[TILE - 1] == keys[TILE]), tiles=len(tiles))
    return cloud, tol, 2, 10 ** 6, expected


# ---- f. near the full key range -------------------------------------------------------------------------------------
def near_full_grid(over=False, info=None):
    """Pairs at the corners of a flat box of 120 000 x 30 000 x 1 cells (3.6e9, below the 2^32 - 1 the host admits),
    coordinates in units of 2^-10 (exact up to 2^14 m): at every corner a pair 240 units (just below tol) apart along
    x, pointing inwards; at the far corner also a pair at exactly 256 units (no link) and a pair across a cell boundary
    on both axes (100, 200 units apart).  Expected from brute force.
    over: the box is 120 000 x 40 000 x 1 cells, 4.8e9: the device has to refuse it (expected is None)."""
    X = 119999 * CELL_U + 66
    Y = (39999 if over else 29999) * CELL_U + 66
    pts = []
    for cx, cy in ((0, 0), (X, 0), (0, Y), (X, Y)):
        sx = 1 if cx == 0 else -1
        pts += [(cx, cy), (cx + sx * 240, cy)]
    pts += [(X - 2048, Y - 2048), (X - 2048 - 256, Y - 2048)]        # exactly tol
    pts += [(X - 4096, Y), (X - 4096 - 100, Y - 200)]                # 223.6 units, cells differ on x and y
    pts = np.array(pts, np.int64)
    xyz64 = np.c_[(pts + 512) * U, np.full(len(pts), 2.0)]
    xyz = xyz64.astype(F)
    assert np.array_equal(xyz.astype(np.float64), xyz64)
    xyz = xyz[np.random.default_rng(81).permutation(len(xyz))]
    cloud, index = assemble(xyz, 82)
    dims = grid_dims(xyz, 0.25)
    cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    assert dims.max() <= MAX_AXIS_CELLS and (cells >= MAX_GRID_CELLS) == over
    if info is not None:
        info.update(dims=dims, cells=cells)
    return cloud, 0.25, 1, 100, None if over else _from_brute(xyz, index, 0.25, 1, 100)


# ---- g. more than 2^20 survivors --------------------------------------------------------------------------------------
def over_a_million(blocks=1100, info=None):
    """`blocks` blocks of a 10 x 10 x 10 lattice of spacing 2^-7 on a pitch of 0.125 (11 x 10 x ... blocks), tol = 2^-5:
    every block is one component (lattice neighbours are 0.0078 apart) and the gaps between blocks are 0.0547 > tol.
    Block b loses its last b % 7 points, so the sizes run from 1 000 down to 994 and tie; the whole cloud is shuffled by
    a seeded permutation and 2 % dropped points are interleaved.  With 1 100 blocks 1 096 703 points survive, more than
    the 1 048 576 one trip of the scan's carry loop covers.  The expectation is analytic: group by block, order by
    (-size, smallest index); min 1, max 1 000."""
    k = np.arange(1000)
    lat = np.stack([k % 10, (k // 10) % 10, k // 100], 1)
    b = np.arange(blocks)
    keep = (k[None, :] < (1000 - b % 7)[:, None]).ravel()
    base = np.stack([b % 11, (b // 11) % 10, b // 110], 1) * 16
    pts = (base[:, None, :] + lat[None, :, :]).reshape(-1, 3)[keep]
    group = np.repeat(b, 1000)[keep]
    o = np.random.default_rng(91).permutation(len(pts))
    pts, group = pts[o], group[o]
    xyz = (1.0 + pts * 2.0 ** -7).astype(F)
    cloud, index = assemble(xyz, 92)
    if blocks == 1100:
        assert len(index) == 1096703 and len(index) > TILE * TILE
    if info is not None:
        info.update(survivors=len(index), total=len(cloud))
    return cloud, 2.0 ** -5, 1, 1000, _from_groups(group, index, 1, 1000)


# ---- the registry: every case once per process -------------------------------------------------------------------------
CASES = {"offsets-near": (offsets, {}), "offsets-far": (offsets, {"far": True})}
CASES.update({"chains-%s" % o: (chains, {"order": o}) for o in ("ascending", "descending", "random", "bit_reversed")})
CASES.update({"chains-gap": (chains, {"order": "random", "gap": True}), "chains-spiral": (spiral, {}),
              "crowded_cells": (crowded_cells, {}),
              "size_rule-5-40": (size_rule, {}), "size_rule-5-5": (size_rule, {"min_size": 5, "max_size": 5}),
              "size_rule-1-1000000": (size_rule, {"min_size": 1, "max_size": 10 ** 6}), "size_rule-isolated": (isolated, {})})
CASES.update({"tile_edges-%d" % m: (tile_edges, {"m": m}) for m in TILE_EDGE_M})
CASES["near_full_grid"] = (near_full_grid, {})
SMALL_CASES = tuple(CASES)           # a .. f
CASES["over_a_million"] = (over_a_million, {})
REFUSED_CASE = "near_full_grid-over"
CASES[REFUSED_CASE] = (near_full_grid, {"over": True})
EXPECTED_CASES = tuple(c for c in CASES if c != REFUSED_CASE)


@functools.lru_cache(maxsize=None)
def get(name):
    """-> (cloud, tol, min_size, max_size, expected) of a registered case, built once; treat as read-only"""
    fn, kw = CASES[name]
    return fn(**kw)


@functools.lru_cache(maxsize=None)
def get_info(name):
    fn, kw = CASES[name]
    info = {}
    fn(info=info, **kw)
    return info

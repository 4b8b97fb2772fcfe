"""Constructions for the result-pose search of the pose evaluators (mt_min_child / mt_search in
pcl_tracking_amd/csrc/pft_match_search.h, called by k_match, k_reacquire_score and k_refine_pairs) -- host-run helper, numpy
and the oracle only.  tests/test_search_cases_host.py shows with the oracle alone that the constructions are what they claim;
tests/test_gpu_search_cases.py then runs them through the three kernels.

Every case is a cloud, a reference cloud ("model") of queries, and a few poses that are pure x translations; the expected
(record, squared distance) of a query holds at ONE of them, `expect_pose`: the model holds `query - translation`, and the
translations are multiples of U = 2^-17 m so small that `model + translation` gives the query back bit for bit.

* The leaf phase: leaf_cases.all_cases() unchanged (leaves of 1 to 9 records, the ties inside a leaf, the 10 cm gate pair, the
  one-point crop with its one-level tree, the empty crop, crops of 5 000 and 5 001 points), at resolution 0.01; the expected
  pose is the identity.
* `descent`, at resolution 2^-7: ties between the children of one node.  The first cloud point is an anchor at
  (0.25, 0.25, 0.5); PCL's box starts as two cells per axis that meet at the first point and here only grows upwards, so cell
  k of an axis spans min + k r .. min + (k + 1) r with min = anchor - r + (PCL's float epsilon), and the second cloud point, in
  cell 63 of every axis, fixes six levels.  Each tie lives in a block of 16^3 cells of its own; inside its parent node the
  only records are one per tied child, 1.5 cells below the tie plane in a lower child and 0.5 cells above it in an upper one:
  a search that takes a later child at equality returns another record AND another distance.  The query lies at the float
  midpoint of the two child centres, formed from the oracle's box exactly as the kernel forms them; r and the child sides are
  powers of two above the float spacing of the coordinates, so (float)(x + side) == (float)x + side, the midpoint is a float
  and both float differences are equal and opposite: an exact tie.  (At r = 0.01 only some midpoints are; hence 2^-7.)  A tie
  on two or three axes at once is exact for the same reason -- each axis contributes bit-equal squares to every child's
  X + (Y + Z) -- so the 4-way, 8-way and 7-way (child 0 missing) ties are built as well.  Beside every tie query lie its two
  float neighbours on the tie axis (on every tie axis at once for the multi-axis ties): one step up belongs to the upper
  child, one step down to the lower.  `only_farther`: the lower x child of a node is empty and the query lies deep inside
  it.  `outside`: queries 0.3 m below the box minimum and above its maximum on each axis.
* `gates`, at resolution 0.01: three lone records at x = 0, one per gate g that reaches mt_search's callers (max_distance
  0.1, inlier_distance 0.02, pair_distance 0.05), each with two queries at distances a- < a+ along x, neighbouring floats
  with (double)(float)(a- a-) < g g <= (double)(float)(a+ a+) (leaf_cases.GATE_UNDER / GATE_OVER for every g).
"""
import functools

import numpy as np

import leaf_cases
import oracle

F = np.float32
U = leaf_cases.U
RES = 2.0 ** -7
ANCHOR = (0.25, 0.25, 0.5)
SHIFT = 6 * U  # the x translation at which the expectations of `descent` and `gates` hold
GATES = (("max_distance", 0.1), ("inlier_distance", 0.02), ("pair_distance", 0.05))
RESOLUTIONS = (0.02, 0.005, 0.037, RES)  # the realistic frame: test_eval_weights_non_default_parameters' values and 2^-7
LEVELS = (1, 2, 3)  # tied children of side 2, 4 and 8 cells
BLOCK = 16


def d2_of(record, query):
    """pointSquaredDist in float: x2 + (y2 + z2), unfused"""
    d = np.asarray(record, F) - np.asarray(query, F)
    return F(d[0] * d[0] + F(d[1] * d[1] + d[2] * d[2]))


def translation(x):
    m = np.eye(4, dtype=F)
    m[0, 3] = F(x)
    return m


def particles_of(xs):
    p = np.zeros(len(xs), leaf_cases.scene.PARTICLE_DTYPE)
    p["x"] = np.asarray(xs, F)
    p["w"] = 1.0
    p["weight"] = 1.0 / len(xs)
    return p


def child_centres(omin, res, depth, level_side, key):
    """the float centres of children 2 key and 2 key + 1 of one axis, as mt_min_child forms them: key of the parent, side of
    a child in cells (vs = res * 2^(D - lvl - 1) in double, the sum in double, one cast)"""
    vs = float(res) * float(level_side)
    assert level_side & (level_side - 1) == 0 and level_side < (1 << depth)
    return F((float(2 * key) + 0.5) * vs + float(omin)), F((float(2 * key + 1) + 0.5) * vs + float(omin))


def gate_floats(g):
    """neighbouring floats a- < a+ with (double)(float)(a- a-) < g g <= (double)(float)(a+ a+)"""
    gg = np.float64(g) * np.float64(g)
    a = F(g)
    while np.float64(F(a * a)) >= gg:
        a = np.nextafter(a, F(0))
    while np.float64(F(a * a)) < gg:
        a = np.nextafter(a, F(1))
    under = np.nextafter(a, F(0))
    assert np.float64(F(under * under)) < gg <= np.float64(F(a * a))
    return under, a


class SearchCase:
    """cloud / model: point records; poses: x translations (float), expect_pose: the one the expectations hold at"""

    def __init__(self, name, resolution, cloud, model, poses, expect_pose=0, whole_crop=True):
        self.name, self.resolution, self.cloud, self.model = name, float(resolution), cloud, model
        self.poses, self.expect_pose, self.whole_crop = [float(F(x)) for x in poses], expect_pose, whole_crop
        self.expect = []   # (query index, cloud index, float squared distance) at the expected pose
        self.ties = []     # dict(query, level, axes, tied (cloud indices, ascending child index), up, down)
        self.leaf_ties = []  # (query index, cloud indices that tie inside one leaf): the earliest wins
        self.gate = []     # (query index, cloud index, gate name, g, inside)
        self.outside = []  # (query index, axis, +1 above max / -1 below min)
        self.only_farther = []  # (query index, cloud index)
        self.clusters = None
        assert len(self.poses) <= 16 and len(self.cloud) <= 5001

    @property
    def shift(self):
        return self.poses[self.expect_pose]

    def matrices(self):
        return np.stack([translation(x) for x in self.poses])

    def queries(self, pose=None):
        """the model moved by a pose, in float as the kernels move it"""
        x = self.shift if pose is None else self.poses[pose]
        q = np.stack([self.model["x"], self.model["y"], self.model["z"]], 1).astype(F)
        q[:, 0] = q[:, 0] + F(x)
        return q


def from_leaf_case(c):
    xs = [0.0] + sorted(set(float(v) for v in leaf_cases.particles(16)["x"]) - {0.0})
    s = SearchCase(c.name, 0.01, c.cloud, c.model, xs, 0, c.whole_crop)
    s.expect = list(c.expect)
    s.leaf_ties = list(c.ties)
    s.gate = [(qi, idx, "max_distance", 0.1, inside) for qi, idx, inside in c.gate]
    s.clusters = list(c.clusters)
    return s


def _corners(lo, hi, grow=0.45):
    lo, hi = np.asarray(lo, np.float64) - grow, np.asarray(hi, np.float64) + grow
    return [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]


def _finish(name, resolution, cloud_xyz, query_xyz, poses, expect_pose, pad_to=64):
    """the model holds query - translation of the expected pose (exact: see the module's text), the corners of the cloud's
    box grown by 0.45 m -- the crop of every pose is the whole cloud -- and filler queries beside the anchor"""
    cloud_xyz = np.asarray(cloud_xyz, np.float64).reshape(-1, 3)
    q = [tuple(v) for v in query_xyz] + _corners(cloud_xyz.min(0), cloud_xyz.max(0))
    k = 0
    while len(q) < pad_to:
        q.append((cloud_xyz[0][0] + 0.011 * k, cloud_xyz[0][1] + 0.007 * k, cloud_xyz[0][2] + 0.003 * k))
        k += 1
    q = np.asarray(q, np.float64).astype(F)
    m = q.copy()
    m[:, 0] = q[:, 0] - F(poses[expect_pose])
    n = len(query_xyz)  # (the corners and the filler are whatever float they become)
    assert ((m[:n, 0] + F(poses[expect_pose])) == q[:n, 0]).all(), "model + translation gives the query back"
    return SearchCase(name, resolution, leaf_cases._points(cloud_xyz, 2), leaf_cases._points(m, 1), poses, expect_pose)


def cell(k):
    """the dyadic middle of cell k (per axis) of the 2^-7 grid anchored at ANCHOR"""
    return tuple(ANCHOR[a] + (k[a] - 0.5) * RES for a in range(3))


# (name, level j: tied children of side 2^j cells, tie axes, children left out, block of 16^3 cells)
TIE_SITES = [("x%d" % j, j, (0,), (), (1, 0, j)) for j in LEVELS] + \
            [("y%d" % j, j, (1,), (), (0, 1, j)) for j in LEVELS] + \
            [("z%d" % j, j, (2,), (), (1, 1, j)) for j in LEVELS] + \
            [("xy", 2, (0, 1), (), (1, 0, 0)), ("xyz", 2, (0, 1, 2), (), (0, 1, 0)), ("xyz_no0", 1, (0, 1, 2), (0,), (0, 0, 1))]
FARTHER_BLOCK = (0, 0, 2)


def case_descent():
    # (PCL grows the box downwards on every axis whose upper bound a new point does not violate: the far corner comes
    # second and violates all three, every later point lies inside)
    cloud, sites = [ANCHOR, cell((63, 63, 63))], []
    for name, j, axes, missing, block in TIE_SITES:
        h, recs = 1 << j, []
        for c in range(8):  # child index 4 x + 2 y + z; children that differ on a tie axis only
            up = [(c >> (2 - a)) & 1 for a in range(3)]
            if any(up[a] and a not in axes for a in range(3)) or c in missing:
                continue
            k = [BLOCK * block[a] + ((h if up[a] else h - 2) if a in axes else 0) for a in range(3)]
            recs.append((c, len(cloud)))
            cloud.append(cell(k))
        sites.append((name, j, axes, block, recs))
    far_k = [BLOCK * FARTHER_BLOCK[a] + (8 if a == 0 else 0) for a in range(3)]  # the upper x child of a 16-cell node
    farther = len(cloud)
    cloud.append(cell(far_k))
    tree = oracle.Octree(leaf_cases._points(cloud, 2), RES)
    info, keys = tree.info(), tree.point_keys()
    D, omin = info["depth"], info["min"]

    queries, ties = [], []
    for name, j, axes, block, recs in sites:
        base = np.array(cloud[recs[0][1]], np.float64)  # the other axes: the records' own coordinates
        q, up, down = base.astype(F), base.astype(F), base.astype(F)
        for a in axes:
            parent = int(keys[recs[0][1]][a]) >> (j + 1)
            assert all(int(keys[i][a]) >> (j + 1) == parent for _, i in recs)
            lo, hi = child_centres(omin[a], RES, D, 1 << j, parent)
            q[a] = F((np.float64(lo) + np.float64(hi)) / 2.0)
            up[a], down[a] = np.nextafter(q[a], F(2)), np.nextafter(q[a], F(0))
        ties.append(dict(name=name, query=len(queries), level=j, axes=axes, tied=[i for _, i in recs],
                         children=[c for c, _ in recs], up=len(queries) + 1, down=len(queries) + 2))
        queries += [q, up, down]
    # deep inside the empty lower x child: two cells above the node's low corner on every axis
    only_farther = (len(queries), farther)
    queries.append(np.array(cell([BLOCK * FARTHER_BLOCK[a] + 2 for a in range(3)]), F))
    outside = []
    inside = np.array(cell((20, 20, 20)), np.float64)
    for a in range(3):
        for side, edge in ((-1, info["min"][a] - 0.3), (1, info["max"][a] + 0.3)):
            q = inside.copy()
            q[a] = edge
            outside.append((len(queries), a, side))
            queries.append(q.astype(F))

    s = _finish("descent", RES, cloud, queries, [SHIFT, 0.0, 2 * U, -6 * U], 0)
    s.ties, s.only_farther, s.outside, s.depth, s.omin, s.omax = ties, [only_farther], outside, D, omin, info["max"]
    xyz = np.asarray(cloud, np.float64).astype(F)
    Q = s.queries()
    for t in ties:  # the lowest existing child at the tie, the highest one step above it; one step below it child 0 if it
        # exists (without it the three children next to it are no exact tie: the oracle decides)
        t["winner"], t["winner_up"] = t["tied"][0], t["tied"][-1]
        want = [(t["query"], t["winner"]), (t["up"], t["winner_up"])] + ([(t["down"], t["winner"])] if t["children"][0] == 0 else [])
        for qi, idx in want:
            s.expect.append((qi, idx, d2_of(xyz[idx], Q[qi])))
    s.expect.append((only_farther[0], farther, d2_of(xyz[farther], Q[only_farther[0]])))
    return s


GATE_SITES = ((0.0, 0.25, 0.5), (0.0, 0.55, 0.5), (0.0, 0.25, 0.8))


def case_gates():
    cloud, queries, gate = [leaf_cases.ANCHOR], [], []
    for (name, g), at in zip(GATES, GATE_SITES):
        cloud.append(at)
        for a, inside in zip(gate_floats(g), (True, False)):
            gate.append((len(queries), len(cloud) - 1, name, g, inside, a))
            queries.append((at[0] - float(a), at[1], at[2]))
    s = _finish("gates", 0.01, cloud, queries, [SHIFT, 0.0, -4 * U, 2 * U], 0)
    Q = s.queries()
    for qi, idx, name, g, inside, a in gate:
        assert Q[qi][0] == F(cloud[idx][0]) - a
        s.gate.append((qi, idx, name, g, inside))
        s.expect.append((qi, idx, F(a * a)))
    return s


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple([from_leaf_case(c) for c in leaf_cases.all_cases()] + [case_descent(), case_gates()])


CASE_NAMES = leaf_cases.CASE_NAMES + ("descent", "gates")

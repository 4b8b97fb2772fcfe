"""Constructions for the leaf phase of the likelihood kernel (host-run helper, numpy only): input clouds whose octree
leaves hold a chosen number of records in a chosen order, with queries whose nearest record -- and every exact tie -- is
known beforehand.  tests/test_leaf_cases.py shows with the oracle alone that the constructions are what they claim;
tests/test_gpu_leaf_phase.py then runs them through the kernel in both leaf-record forms.

How a case is made.  All particles have zero rotation, so a query is a reference point plus the particle's translation;
particle 0 is the identity.  The records of one leaf ("cluster") differ in x alone, by multiples of U = 2^-17 m, and every
coordinate of a cluster record or of a query aimed at it is a multiple of U below 1 m: the float differences and their
squares are exact, so the squared distance of a query at offset q from a record at offset r is ((r - q) U)^2 exactly, equal
offsets give bit-equal distances, and the winner of "first strictly smaller" follows from the integers.  Cluster centres
lie on a lattice of pitch 13/256 m.  PCL's octree starts as two cells per axis that meet at the first point, and grows by
whole cells: the first cloud point of every case is an anchor record 5/1024 m below the lattice origin on every axis, so
the lattice sites with index <= 5 per axis lie at least 1.1 mm inside their 1 cm cells; a cluster spans at most 0.14 mm
around its site.
The reference cloud also holds the eight corners of a box 0.45 m around the lattice, which makes the crop the whole cloud.
"""
import numpy as np

from pcl_tracking_amd import scene

U = 2.0 ** -17
PITCH = 13.0 / 256.0
ORIGIN = (0.25, 0.25, 0.5)
ANCHOR = tuple(v - 5.0 / 1024.0 for v in ORIGIN)
GATE_XYZ = (0.0, 0.25, 0.5)  # the lone record of the gate queries, a quarter of a metre beside the lattice
GATE_UNDER = float(np.nextafter(np.float32(0.1), np.float32(0)))  # squared: 0.0099999988 < 0.1 * 0.1
GATE_OVER = float(np.float32(0.1))                                 # squared, rounded to float: 0.0100000007 > 0.1 * 0.1

# records of a cluster in insertion order (offsets in U, even) and queries at odd offsets (no ties) beside one query on
# every record
SIZES = {1: [0], 2: [0, 6], 3: [8, 0, 4], 4: [0, 4, 8, 12], 5: [16, 0, 12, 4, 8], 9: [0, 2, 4, 6, 8, 10, 12, 14, 16]}
# exact ties: (records, query offset, positions that tie, the earlier one wins)
TIES = [([-4, 4, 12, 16], 0, (0, 1)), ([12, -4, 4, 16], 0, (1, 2)), ([-4, 12, 16, 4], 0, (0, 3)),
        ([0, 0, 8], 0, (0, 1)), ([6, 2, 2, 2, 10], 2, (1, 2))]


def site(i, j, k):
    return (ORIGIN[0] + PITCH * i, ORIGIN[1] + PITCH * j, ORIGIN[2] + PITCH * k)


def _points(xyz, seed):
    rng = np.random.default_rng(seed)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return scene.make_points(xyz.astype(np.float32), rng.integers(0, 256, (len(xyz), 3)))


def particles(P):
    p = np.zeros(P, scene.PARTICLE_DTYPE)
    p["x"] = [((k * 5) % 7 - 3) * 2 * U if k else 0.0 for k in range(P)]  # particle 0: the identity
    p["w"] = 1.0
    p["weight"] = 1.0 / P
    return p


def winner(records, q):
    """position of the first record at the smallest |offset - q|, and that squared distance as the kernel's float"""
    d = [abs(r - q) for r in records]
    pos = d.index(min(d))
    return pos, np.float32((d[pos] * U) ** 2)


class Case:
    def __init__(self, name, P, anchor_queries=()):
        self.name, self.P = name, P
        self.cloud_xyz, self.query_xyz = [], []
        self.clusters = []  # (first cloud index, size)
        self.swept = []     # the clusters with a query on every record
        self.expect = []    # (query index, cloud index, squared distance) for particle 0
        self.ties = []      # (query index, cloud indices that tie)
        self.gate = []      # (query index, cloud index, inside the gate)
        self.end = None     # (first cloud index, size) of the leaf that ends the leaf arrays
        self.whole_crop = True
        self.cluster(ANCHOR, [0], anchor_queries)

    def cluster(self, at, records, queries):
        first = len(self.cloud_xyz)
        for r in records:
            self.cloud_xyz.append((at[0] + r * U, at[1], at[2]))
        self.clusters.append((first, len(records)))
        if set(records) <= set(queries):
            self.swept.append((first, len(records)))
        for q in queries:
            pos, d2 = winner(records, q)
            self.expect.append((len(self.query_xyz), first + pos, d2))
            tie = [first + i for i, r in enumerate(records) if abs(r - q) == abs(records[pos] - q)]
            if len(tie) > 1:
                self.ties.append((len(self.query_xyz), tie))
            self.query_xyz.append((at[0] + q * U, at[1], at[2]))
        return first

    def gate_record(self):
        first = self.cluster(GATE_XYZ, [0], [])
        for a, inside in ((GATE_UNDER, True), (GATE_OVER, False)):
            self.gate.append((len(self.query_xyz), first, inside))
            self.expect.append((len(self.query_xyz), first, np.float32(np.float32(a) * np.float32(a))))
            self.query_xyz.append((GATE_XYZ[0] - a, GATE_XYZ[1], GATE_XYZ[2]))

    def finish(self, pad_to=0, cloud_shift=(0.0, 0.0, 0.0)):
        lo, hi = np.array(site(0, 0, 0)) - 0.45, np.array(site(5, 3, 3)) + 0.45
        corners = [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
        q = self.query_xyz + corners
        k = 0
        while len(q) < pad_to:  # more queries, between the lattice sites: whatever leaf they reach, the oracle decides
            q.append((ORIGIN[0] + 0.011 * k, ORIGIN[1] + 0.007 * k, ORIGIN[2] + 0.003 * k))
            k += 1
        self.model = _points(q, 1)
        self.cloud = _points(np.asarray(self.cloud_xyz, np.float64).reshape(-1, 3) + np.asarray(cloud_shift), 2)
        self.particles = particles(self.P)
        return self


def _all_queries(records):
    return sorted(set(records)) + [r + 1 for r in sorted(set(records))] + [min(records) - 3]


def case_sizes(end_size, name):
    """leaves of 1, 2, 3, 4, 5 and 9 records with a query on every record (the winner at every position) and between
    them, the exact ties, the gate pair, and a last leaf of end_size records"""
    c = Case(name, 16, anchor_queries=[0])
    for n, (size, records) in enumerate(SIZES.items()):
        c.cluster(site(n, 0, 0), records, _all_queries(records))
    for n, (records, q, _) in enumerate(TIES):
        c.cluster(site(n, 1, 0), records, [q])
    c.gate_record()
    records = SIZES[end_size]
    c.end = (c.cluster(site(5, 3, 3), records, _all_queries(records)), end_size)
    return c.finish(pad_to=96)


def case_mixed_wave():
    """64 queries, one wave: leaves of 1 and of 5 records side by side, the divergent tail of the scan loop"""
    c = Case("mixed_wave", 4)
    for n in range(7):
        c.cluster(site(n % 6, 1 + n // 6, 1), SIZES[1], [0, 1, -1, 3])
        c.cluster(site(n % 6, 1 + n // 6, 2), SIZES[5], [4, 16, 9, 1])
    c.finish()
    assert len(c.model) == 64
    return c


def case_one_point():
    c = Case("one_point", 4, anchor_queries=[0, 1, -5, 40])
    return c.finish(pad_to=64)


def case_empty_crop():
    c = Case("empty_crop", 4)
    for n, records in enumerate(SIZES.values()):
        c.cluster(site(n, 0, 0), records, [0])
    c.expect, c.whole_crop = [], False
    return c.finish(pad_to=64, cloud_shift=(0.0, 0.0, 50.0))


def case_crop_of(n_total):
    """the sizes case (without the last-leaf property) inside a crop of n_total points: single records one per cell fill it
    up.  Up to 5 000 points the builder copies the leaf records itself; from 5 001 on a gather launch does, which also
    fills the ancestor table."""
    c = Case("crop_%d" % n_total, 4)
    for n, (size, records) in enumerate(SIZES.items()):
        c.cluster(site(n, 0, 0), records, _all_queries(records))
    for n, (records, q, _) in enumerate(TIES):
        c.cluster(site(n, 1, 0), records, [q])
    c.gate_record()
    k = 0
    while len(c.cloud_xyz) < n_total:  # cell centres (the first point is one) of a slab above the clusters
        a, b, z = k % 26, (k // 26) % 14, k // (26 * 14)
        at = (ORIGIN[0] + 0.01 * a, ORIGIN[1] + 0.01 * b, ORIGIN[2] + 0.3 + 0.01 * z)
        c.cloud_xyz.append(at)
        c.clusters.append((len(c.cloud_xyz) - 1, 1))
        if k % 97 == 0:
            c.query_xyz.append((at[0] + 0.001, at[1] - 0.002, at[2] + 0.0015))
        k += 1
    return c.finish(pad_to=128)


def all_cases():
    return [case_sizes(5, "sizes_end_odd"), case_sizes(4, "sizes_end_even"), case_mixed_wave(), case_one_point(),
            case_empty_crop(), case_crop_of(5000), case_crop_of(5001)]


CASE_NAMES = ("sizes_end_odd", "sizes_end_even", "mixed_wave", "one_point", "empty_crop", "crop_5000", "crop_5001")

"""Clouds for the plane refit (csrc/pft_segment.hip k_sg_refit / k_sg_refit_tiles / k_sg_refit_top and the one-lane tail
csrc/pft_segment_solve.h; DESIGN.md section 3.7 "refit routes").  NumPy only.  Two families:

SUM cases: a tilted plane with noise far below the threshold, shuffled, with strays at least 0.3 m off the plane mixed
in, so that the pre-refit inlier list is a gather of exactly m points and the nine float sums round at every add: the
PCL chain and the pair tree give different bits, and so would a term dropped or swapped at a stage edge.

SOLVE cases: clouds the whole pipeline turns into a covariance that takes one branch of the eigen solve.  Those whose
name starts with "found:" were found by a seeded search over the traced model (`search` below is the search that found
them); the others are constructed.

tests/test_refit_cases_host.py proves on the CPU, with the model alone, that every case is what it claims;
tests/test_gpu_segment_refit.py runs them on the device."""
import functools

import numpy as np

import segment_model as M
import segment_rounds_model as R
from pcl_tracking_amd import scene

F = np.float32

# inlier counts of the sum cases, per order: PCL order stages 4 096 points with 1 024 threads; tree
# order has 8 points per thread, 512 per wave, 2 048 per tile, 1 024 tiles per chunk of k_sg_refit_top
PCL_M = [3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 12289]
TREE_M = [3, 4, 5, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4097, 2097152, 2097153]
TREE_GRID_M = [m for m in TREE_M if m <= 4097]  # run under three grid sizes of the tile launch
SUM_KW = dict(max_iterations=50, threshold=0.02, tol=0.02, min_size=1, max_size=2500)
# seed per m where it is not 0: the first for which the model finds exactly m pre-refit inliers that are no prefix of the
# cloud, no point within 1e-4 of the threshold, PCL-order and tree-order means that differ and, past 4 096, PCL sums that change when terms 4 095
# and 4 096 are swapped (one seed in about twenty: mostly (s + a) + b == (s + b) + a).  tests/test_refit_cases_host.py
# asserts all of it
SUM_SEEDS = {4: 1, 5: 1, 4097: 3, 8192: 8, 8193: 16, 12289: 107}


def _points(xyz):
    xyz = np.asarray(xyz, F)
    return scene.make_points(xyz, np.zeros((len(xyz), 3)))


def sum_cloud(m, seed=0):
    """m points on the plane z = 1.2 + 0.21 x - 0.13 y over [-1, 1]^2 with noise 0.5 mm, a few strays 0.3 .. 0.9 m
    above it, shuffled"""
    rng = np.random.default_rng(7000 + 31 * m + seed)
    xy = rng.uniform(-1, 1, (m, 2))
    plane = np.c_[xy, 1.2 + 0.21 * xy[:, 0] - 0.13 * xy[:, 1] + rng.normal(0, 0.0005, m)]
    ns = 2 if m <= 5 else max(3, min(40, m // 8))
    sxy = rng.uniform(-1, 1, (ns, 2))
    stray = np.c_[sxy, 1.2 + 0.21 * sxy[:, 0] - 0.13 * sxy[:, 1] + rng.uniform(0.3, 0.9, ns) * 1.05]
    xyz = np.r_[plane, stray].astype(F)
    return _points(xyz[rng.permutation(len(xyz))])


def rounds_scene():
    """three tilted planes 0.45 m apart and strays, shuffled: with plane rounds, rounds 2 and 3 read the compacted
    ping-pong buffers"""
    rng = np.random.default_rng(4242)
    parts = []
    for k, n0 in enumerate((5000, 3100, 1900)):
        xy = rng.uniform(-1, 1, (n0, 2))
        tilt = ((0.21, -0.13), (-0.17, 0.08), (0.05, 0.26))[k]
        parts.append(np.c_[xy, 1.0 + 0.45 * k + xy @ np.array(tilt) + rng.normal(0, 0.0005, n0)])
    parts.append(rng.uniform(-1, 1, (60, 3)) * [1, 1, 0.1] + [0, 0, 3.0])
    xyz = np.concatenate(parts).astype(F)
    return _points(xyz[rng.permutation(len(xyz))])


ROUNDS_KW = dict(max_iterations=100, threshold=0.02, tol=0.02, min_size=1, max_size=2500)
ROUNDS = (16, 0.05)


# ---- solve cases ------------------------------------------------------------------------------------------------------
def _tilted(normal_axis, z0, n=3000, seed=0, noise=0.001):
    """a noisy plane whose normal is mostly along one axis, at offset z0 along it"""
    rng = np.random.default_rng(8100 + seed)
    uv = rng.uniform(-1, 1, (n, 2))
    w = z0 + 0.11 * uv[:, 0] - 0.07 * uv[:, 1] + rng.normal(0, noise, n)
    cols = {2: (uv[:, 0], uv[:, 1], w), 1: (uv[:, 0], w, uv[:, 1]), 0: (w, uv[:, 0], uv[:, 1])}[normal_axis]
    return _points(np.c_[cols])


def _flat_axis(n=500, seed=1):
    rng = np.random.default_rng(8200 + seed)
    return _points(np.c_[rng.uniform(-1, 1, (n, 2)), np.ones(n)])


def _flat_dyadic(seed=0, n=400):
    """z = 1 + x / 2 + y / 4 exactly: x, y multiples of 2^-6 (so z is a float exactly)"""
    rng = np.random.default_rng(8300 + seed)
    xy = rng.integers(-64, 65, (n, 2)) / 64.0
    return _points(np.c_[xy, 1.0 + xy[:, 0] / 2 + xy[:, 1] / 4])


def _lattice_slab():
    """a square dyadic lattice 8 x 8 of spacing 1/8, two layers 2^-7 apart, 128 points: every sum and every mean is
    exact in either order, cov_xx == cov_yy and cov_xy == 0: a double root"""
    g = (np.arange(8) - 3.5) / 8.0
    x, y, z = np.meshgrid(g, g, 1.0 + np.array([-1.0, 1.0]) / 256.0, indexing="ij")
    return _points(np.c_[x.ravel() + 0.5, y.ravel() + 0.25, z.ravel()])


def _strip(seed=0, n=2000):
    """long in x, 4 cm wide in y, 2 mm noise in z: (l1 - l0) / l2 about 4e-4"""
    rng = np.random.default_rng(8400 + seed)
    return _points(np.c_[rng.uniform(-1, 1, n), rng.uniform(-0.0203, 0.0203, n), 1.0 + rng.normal(0, 0.002, n)])


def _blob(seed=0, n=200):
    rng = np.random.default_rng(8500 + seed)
    return _points(np.array([0.4, -0.3, 1.1]) + rng.uniform(-0.004, 0.004, (n, 3)))


def cube():
    """the eight corners of a cube of half side 2^-8 around (1, 0.5, 1): every sum exact, covariance 2^-16 I, all three
    roots 1, M - r0 I the zero matrix, the normal 0 / 0"""
    h = 2.0 ** -8
    c = np.array([[sx, sy, sz] for sx in (-h, h) for sy in (-h, h) for sz in (-h, h)]) + [1.0, 0.5, 1.0]
    return _points(c)


def _iso_blob(seed, k=4, half=0.125):
    """a k x k x k lattice cube with a non-dyadic spacing at a non-dyadic centre: isotropic up to the rounding of the
    sums, so c1 - c2 * c2 / 3 is rounding noise of either sign"""
    rng = np.random.default_rng(8600 + seed)
    g = (np.arange(k) - (k - 1) / 2) * (2 * half / max(k - 1, 1))
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    c = np.c_[x.ravel(), y.ravel(), z.ravel()] + rng.uniform(0.3, 0.6, 3)
    return _points(c[rng.permutation(len(c))])


def _flat_iso(seed, n=16):
    """exactly flat (z = 1) and four-fold symmetric about a centre: cov_xx == cov_yy up to rounding, the discriminant of
    computeRoots2 is zero up to rounding"""
    rng = np.random.default_rng(8700 + seed)
    p = rng.uniform(0.05, 0.4, (n, 2))
    q = np.r_[p, np.c_[-p[:, 1], p[:, 0]], -p, np.c_[p[:, 1], -p[:, 0]]] + rng.uniform(0.2, 0.9, 2)
    return _points(np.c_[q[rng.permutation(len(q))], np.ones(len(q))])


def _flat_sloped(seed, n=300):
    """exactly on a dyadic-sloped plane through float points whose products round: c0 is rounding noise of either sign"""
    rng = np.random.default_rng(8800 + seed)
    xy = rng.integers(-2048, 2049, (n, 2)) / 2048.0
    return _points(np.c_[xy, 1.0 + xy[:, 0] / 2 + xy[:, 1] / 4])


def _far_speck(seed, n=4):
    """four points within 10 um of (1, 0.5, 30): the spread is a few ulps of the coordinates, so every entry of
    accu - mean * mean is the difference of two rounded numbers that may agree to the last bit"""
    rng = np.random.default_rng(seed)
    return _points(np.array([1.0, 0.5, 30.0]) + rng.uniform(-1e-5, 1e-5, (n, 3)))


# name -> (cloud builder, kwargs of the pipeline).  Every solve case runs in both orders as a single plane.
SOLVE_KW = dict(max_iterations=50, threshold=0.015, tol=0.02, min_size=1, max_size=2500)
SOLVE_CASES = {
    "normal z": (lambda: _tilted(2, 1.3), {}),
    "normal y": (lambda: _tilted(1, 1.3), {}),
    "normal x": (lambda: _tilted(0, 1.3), {}),
    "flat axis-aligned": (_flat_axis, {}),
    "flat dyadic slopes": (_flat_dyadic, {}),
    "lattice slab": (_lattice_slab, {}),
    "thin strip": (_strip, dict(threshold=0.05)),
    "blob": (_blob, {}),
    "cube": (cube, {}),
    "plane at z = 8": (lambda: _tilted(2, 8.0, seed=3), {}),
    "plane at z = 30": (lambda: _tilted(2, 30.0, seed=3), {}),
    # found by `search` (first seed that sets the bit in the named order; the other order is run all the same)
    "found: isotropic lattice, seed 0 (a_over_3 clamp, tree order)": (lambda: _iso_blob(0), dict(threshold=0.5)),
    "found: isotropic lattice, seed 3 (a_over_3 clamp, PCL order)": (lambda: _iso_blob(3), dict(threshold=0.5)),
    "found: flat four-fold, seed 1 (d < 0, PCL order)": (lambda: _flat_iso(1), {}),
    "found: flat four-fold, seed 6 (d < 0, tree order)": (lambda: _flat_iso(6), {}),
    "found: far speck, seed 109 (scale <= FLT_MIN)": (lambda: _far_speck(109), {}),
    "found: flat sloped, seed 1 (r0 <= 0)": (lambda: _flat_sloped(1), {}),
    "found: flat sloped, seed 3 (r0 <= 0, tree order)": (lambda: _flat_sloped(3), {}),
}


_A, _Q, _C0, _R0, _D, _Z = M.A_CLAMPED, M.Q_CLAMPED, M.C0_SMALL, M.R0_FALLBACK, M.D_NEGATIVE, M.ZERO_LENGTH
_S2, _S3 = M.SWAP_01 | M.SWAP_12, M.SWAP_01 | M.SWAP_12 | M.SWAP_01_AGAIN
# the branch bitmap the model takes, (PCL order, tree order).  The unsorted roots are (largest, smallest, middle) for
# theta within [0, pi / 3], so the first two swaps always happen and the third only at a double root.
EXPECTED = {
    "normal z": (_S2 | M.PICK_0, _S2 | M.PICK_0),
    "normal y": (_S2 | M.PICK_1, _S2 | M.PICK_1),
    "normal x": (_S2 | M.PICK_2, _S2 | M.PICK_2),
    "flat axis-aligned": (_C0 | M.PICK_0, _C0 | M.PICK_0),
    "flat dyadic slopes": (_S2 | _R0 | M.PICK_0, _S2 | M.PICK_0),
    "lattice slab": (_S2 | M.PICK_0, _S2 | M.PICK_0),  # (the trigonometric roots of an exact double root differ by 6e-4)
    "thin strip": (_C0 | M.PICK_0, _C0 | M.PICK_0),  # l0 l1 / l2^2 is about 2e-9: below FLT_EPSILON
    "blob": (_S2 | M.PICK_0, _S2 | M.PICK_0),
    "cube": (_S3 | M.PICK_0 | _Z, _S3 | M.PICK_0 | _Z),
    "plane at z = 8": (_S2 | M.PICK_0, _S2 | _R0 | M.PICK_0),
    "plane at z = 30": (_S2 | _R0 | M.PICK_0, _S2 | M.PICK_0),
    "found: isotropic lattice, seed 0 (a_over_3 clamp, tree order)": (_Q | _S3 | M.PICK_1, _A | _Q | _S3 | M.PICK_0),
    "found: isotropic lattice, seed 3 (a_over_3 clamp, PCL order)": (_A | _Q | _S3 | M.PICK_0, _Q | _S3 | M.PICK_0),
    "found: flat four-fold, seed 1 (d < 0, PCL order)": (_C0 | _D | M.PICK_0, _C0 | M.PICK_0),
    "found: flat four-fold, seed 6 (d < 0, tree order)": (_C0 | M.PICK_0, _C0 | _D | M.PICK_0),
    # every entry of accu - mean * mean cancels to 0 in both orders: scale = 1, the zero matrix, the normal 0 / 0.  (Most
    # seeds leave rounding junk instead, an indefinite matrix with entries of an ulp of the means: seed 109 is the first
    # of 0 .. 199 that cancels in both orders; one in about 300 does in one order)
    "found: far speck, seed 109 (scale <= FLT_MIN)": (M.SCALE_TINY | _C0 | M.PICK_0 | _Z, M.SCALE_TINY | _C0 | M.PICK_0 | _Z),
    "found: flat sloped, seed 1 (r0 <= 0)": (_S2 | _R0 | M.PICK_0, _S2 | M.PICK_0),
    "found: flat sloped, seed 3 (r0 <= 0, tree order)": (_S2 | M.PICK_0, _S2 | _R0 | M.PICK_0),
}
# every bit of the record is reached by a cloud
REACHABLE = (1 << 13) - 1
# (case, order) whose plane comes out 0 / 0: found with every point a pre-refit inlier, no final inlier, nothing removed
NAN_PLANES = (("cube", "pcl"), ("cube", "tree"), ("found: far speck, seed 109 (scale <= FLT_MIN)", "pcl"),
              ("found: far speck, seed 109 (scale <= FLT_MIN)", "tree"))
ORDERS = ("pcl", "tree")


def solve_kw(name):
    kw = dict(SOLVE_KW)
    kw.update(SOLVE_CASES[name][1])
    return kw


def direct_trace(cloud, order="pcl"):
    """the record of a cloud whose inlier list is the whole cloud in input order (search only: the host test runs the
    pipeline)"""
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(F)
    return M.refit_trace(xyz, None, order)


def search(builder, bit, seeds=range(400), order="pcl"):
    """first seed whose direct trace sets `bit`"""
    for s in seeds:
        if direct_trace(builder(s), order)["branches"] & bit:
            return s
    return None


@functools.lru_cache(maxsize=None)
def model(kind, key, order):
    """R.pipeline of a case: kind "sum" (key = m), "solve" (key = name), "rounds" """
    if kind == "sum":
        return R.pipeline(sum_cloud(key, SUM_SEEDS.get(key, 0)), max_planes=1, fraction=0.0, order=order, near_eps=1e-4,
                          **SUM_KW)
    if kind == "rounds":
        return R.pipeline(rounds_scene(), max_planes=ROUNDS[0], fraction=ROUNDS[1], order=order, near_eps=1e-4, **ROUNDS_KW)
    return R.pipeline(SOLVE_CASES[key][0](), max_planes=1, fraction=0.0, order=order, near_eps=1e-4, **solve_kw(key))


def model_trace(r, k, order, trig=None):
    """the record of round k of a model result (None: no plane, or fewer than 4 pre-refit inliers)"""
    rd = r["rounds"][k]
    if not rd["found"]:
        return None
    return M.refit_trace(r["xyz"][rd["ransac_inliers"]], rd["ransac_coefficients"], order, trig)


# ---- comparing a record (the device's, or the host tool's) with the model ------------------------------------------------
REC = np.dtype([("m", "u4"), ("branches", "u4"), ("accu", "f4", 9), ("cov", "f4", 6), ("scale", "f4"), ("trig_arg", "f4", 3),
                ("trig", "f4", 3), ("roots", "f4", 3), ("len", "f4", 3), ("coef", "f4", 4)])
FIELDS = ("accu", "cov", "scale", "trig_arg", "roots", "len", "coef")  # every float field but the three trig values
# conditions, not measurements: the OpenCL full-profile bounds, the loosest accuracy a conforming single-precision device
# library may have (atan2 6 ulp, cos and sin 4 ulp)
TRIG_CAPS_ULP = (6.0, 4.0, 4.0)


def trig_errors_ulp(rec):
    """|value - float64 function of the same float arguments| in ulps of the result, for (atan2f, cosf, sinf); None when
    the solve never called them (computeRoots2 came first)"""
    if int(rec["branches"]) & M.C0_SMALL:
        return None
    ay, hb, th = (float(v) for v in np.asarray(rec["trig_arg"], F))
    want = (np.arctan2(ay, hb), np.cos(th), np.sin(th))
    return tuple(abs(float(g) - w) / float(np.spacing(F(abs(w)))) for g, w in zip(np.asarray(rec["trig"], F), want))


def same_bits(a, b):
    """bit for bit, NaNs in the same places (the sign and payload of a NaN are not the library's to choose: x86 gives
    0 / 0 the sign bit, NumPy and the device may not)"""
    a, b = np.atleast_1d(np.asarray(a, F)), np.atleast_1d(np.asarray(b, F))
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool((na == nb).all()) and a[~na].tobytes() == b[~nb].tobytes()


def check_record(rec, accu, m, label):
    """`rec` (a mapping with REC's fields) against the model's solve of the nine means `accu` with rec's own three trig
    values substituted: every field bit for bit, NaNs in the same places; -> the trig errors in ulps (or None)"""
    t = M.solve_trace(accu, m, trig=np.asarray(rec["trig"], F))
    assert int(rec["m"]) == m, label
    assert int(rec["branches"]) == t["branches"], (label, M.branch_names(int(rec["branches"])), M.branch_names(t["branches"]))
    for k in FIELDS:
        assert same_bits(rec[k], t[k]), (label, k, rec[k], t[k])
    err = trig_errors_ulp(rec)
    if err is None:
        assert np.asarray(rec["trig"], F).tobytes() == np.zeros(3, F).tobytes(), label
    else:
        for e, cap, fn in zip(err, TRIG_CAPS_ULP, ("atan2f", "cosf", "sinf")):
            assert e <= cap, (label, fn, e)
    return err

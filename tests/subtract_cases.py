"""Inputs of the scene-subtraction tests, shared by the CPU checks (tests/test_subtract_host.py: the cases test what
they claim, by the model alone) and the GPU checks (tests/test_gpu_subtract.py: the device against the model)."""
import functools
import itertools

import numpy as np

from pcl_tracking_amd import scene

F = np.float32
R = 0.02  # the default radius
DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3)]  # 27, the zero direction included
# displacement lengths as factors of the radius: a few ulps of the radius to either side, and steps that are still a few
# ulps of the COORDINATE when the lattice sits 100 m from the origin (ulp(100) = 7.6e-6 = r * 2^-11.4)
LENGTH_FACTORS = [1.0] + [1.0 + s * 2.0 ** -k for k in (22, 21, 20, 16, 12, 10, 9, 8) for s in (-1.0, 1.0)]
OFFSETS = {"origin": (0.0, 0.0, 0.0), "far": (100.0, -80.0, 60.0)}


def records(xyz, seed=0):
    """32-byte records with the coordinates given and every other byte filled, so that a copy is seen byte for byte"""
    rng = np.random.default_rng(seed)
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    p = np.zeros(len(xyz), scene.POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["w"] = 1.0
    p["rgba"] = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint64).astype(np.uint32)
    p["pad"] = rng.integers(0, 2 ** 32, (len(xyz), 3), dtype=np.uint64).astype(np.uint32)
    return p


def matrix(offset=(0.0, 0.0, 0.0), rpy=None):
    """3x4 float32: identity rotation, or R = Rz(yaw) Ry(pitch) Rx(roll), and the translation"""
    m = np.zeros((3, 4), np.float64)
    m[:, :3] = np.eye(3) if rpy is None else scene.pose_matrix(0.0, 0.0, 0.0, *rpy)[:3, :3]
    m[:, 3] = offset
    return m.astype(F)


def lattice(pitch=R, n=5):
    g = np.arange(n, dtype=np.float64) * pitch
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)


@functools.lru_cache(maxsize=None)
def neighbour_case(where="origin", rotated=False):
    """One slot: a 5 x 5 x 5 lattice of pitch r under T.  Frame points: every moved lattice point displaced along each
    of the 27 directions (rotated with T) by lengths that straddle r.  -> dict(model, T, frame xyz, direction id of
    every frame point, outward: the lattice point lies on the lattice's boundary in that direction, so that no other
    lattice point is nearer than the one displaced)"""
    import subtract_model as sm

    T = matrix(OFFSETS[where], (1.1, -0.4, 0.7) if rotated else None)
    model = lattice()
    q = sm.xform(T, model).astype(np.float64)
    ijk = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    rot = T[:, :3].astype(np.float64)
    xs, dirs, outs = [], [], []
    for di, d in enumerate(DIRECTIONS):
        dv = np.array(d, np.float64)
        nrm = np.linalg.norm(dv)
        u = rot @ (dv / nrm) if nrm else np.zeros(3)
        outward = np.ones(len(ijk), bool)
        for a in range(3):
            if d[a] > 0:
                outward &= ijk[:, a] == 4
            elif d[a] < 0:
                outward &= ijk[:, a] == 0
        for f in (LENGTH_FACTORS if nrm else [0.0]):
            xs.append((q + u * (float(F(R)) * f)).astype(F))
            dirs.append(np.full(len(q), di))
            outs.append(outward & (nrm > 0))
    return dict(model=model, T=T, frame=np.concatenate(xs), direction=np.concatenate(dirs), outward=np.concatenate(outs))


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """slots: 0 a 30 m line of 3 000 points (cell side far above r), 5 one point 5 000 times (zero extent, one crowded
    cell), 9 a single point, 12 no point at all; frame points scattered within 1.5 r of samples of each, plus far ones"""
    rng = np.random.default_rng(7)
    t = np.linspace(0.0, 30.0, 3000)
    line = np.stack([t, 0.1 * np.sin(t), 1.0 + 0.0 * t], 1).astype(F)
    same = np.tile(np.array([[0.5, -0.25, 2.0]], F), (5000, 1))
    one = np.array([[-1.0, 0.75, 1.5]], F)
    none = np.zeros((0, 3), F)
    slots = {0: (line, matrix()), 5: (same, matrix((0.01, 0.0, 0.0))), 9: (one, matrix()), 12: (none, matrix())}
    base = np.concatenate([line[rng.choice(3000, 600)], same[:300], np.tile(one, (300, 1))]).astype(np.float64)
    v = rng.normal(size=base.shape)
    v /= np.linalg.norm(v, axis=1)[:, None]
    near = base + v * rng.uniform(0.0, 1.5 * R, (len(base), 1))
    far = rng.uniform(-2.0, 32.0, (500, 3))
    frame = np.concatenate([near, far]).astype(F)
    return dict(slots=slots, frame=frame[rng.permutation(len(frame))])


@functools.lru_cache(maxsize=None)
def many_slots_case(n_slots=64):
    """n_slots slots of 40 points each in overlapping boxes; slots 2k and 2k + 1 share one model point (identity
    matrices), so frame points near it are equally far from both: ties between slots"""
    rng = np.random.default_rng(11)
    slots = {}
    shared = []
    for s in range(n_slots):
        c = np.array([0.03 * (s // 2), 0.02 * (s % 4), 1.0])
        pts = (c + rng.uniform(-0.04, 0.04, (40, 3))).astype(F)
        if s % 2 == 1:
            pts[0] = slots[s - 1][0][0]
            shared.append(pts[0])
        slots[s] = (pts, matrix())
    allp = np.concatenate([m for m, _ in slots.values()]).astype(np.float64)
    v = rng.normal(size=(4000, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    near = allp[rng.choice(len(allp), 4000)] + v * rng.uniform(0.0, 1.4 * R, (4000, 1))
    sh = np.array(shared, np.float64)
    v2 = rng.normal(size=(len(sh) * 8, 3))
    v2 /= np.linalg.norm(v2, axis=1)[:, None]
    at_shared = np.repeat(sh, 8, 0) + v2 * rng.uniform(0.0, 0.2 * R, (len(sh) * 8, 1))
    frame = np.concatenate([near, at_shared, sh]).astype(F)
    return dict(slots=slots, frame=frame[rng.permutation(len(frame))])


@functools.lru_cache(maxsize=None)
def sized_frame(n, seed=3):
    """n frame points around one slot: a 12 x 12 x 3 slab of pitch 0.8 r; about half of the points within reach"""
    rng = np.random.default_rng(seed)
    g = [np.arange(k, dtype=np.float64) * 0.8 * R for k in (12, 12, 3)]
    slab = (np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3) + np.array([0.3, -0.1, 0.9])).astype(F)
    lo, hi = slab.min(0).astype(np.float64), slab.max(0).astype(np.float64)
    frame = rng.uniform(lo - 4 * R, hi + 4 * R, (n, 3)).astype(F)
    return dict(slots={3: (slab, matrix())}, frame=frame)


# ---- the end-to-end scene: the small scene of tests/test_gpu_match.py (a 300-point model, frames of 4 000 points) ----
@functools.lru_cache(maxsize=None)
def small_world():
    full = scene.make_scene(50000)
    gtp = scene.model_gt_pose()
    gt = np.array(gtp[:3])
    xyz = np.stack([full["x"], full["y"], full["z"]], 1)
    far = np.flatnonzero(np.linalg.norm(xyz - gt, axis=1) >= 0.6)
    dense = scene.make_model(2000)
    T = scene.pose_matrix(*gtp)
    moved = (np.stack([dense["x"], dense["y"], dense["z"]], 1).astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    obj = dense.copy()
    obj["x"], obj["y"], obj["z"] = moved[:, 0], moved[:, 1], moved[:, 2]
    return dict(full=full, far=far, obj=obj, gt=gt, trans=T.astype(F))


@functools.lru_cache(maxsize=None)
def small_frame(f, second=False):
    """1 500 points of the object at the ground-truth pose and 2 500 of the background, shuffled; second: also 600 points
    of a second object of the same shape half a metre to the side, which nothing tracks"""
    w = small_world()
    rng = np.random.default_rng(100 + f)
    o = w["obj"][rng.choice(2000, 1500, replace=False)]
    parts = [o, w["full"][rng.choice(w["far"], 2500, replace=False)]]
    if second:
        o2 = w["obj"][rng.choice(2000, 600, replace=False)].copy()
        o2["x"] += F(SECOND_OFFSET)
        parts.append(o2)
    c = np.concatenate(parts)
    return c[rng.permutation(len(c))]


SECOND_OFFSET = 0.5
JUMP = -0.5  # two_object_frame: where the first object goes, along y


@functools.lru_cache(maxsize=None)
def two_object_frame(f, jumped=False):
    """the driver's two-object scene: object A (1 500 points at the ground-truth pose, or JUMP further along y), object B
    (600 points of the same shape SECOND_OFFSET to the side, never moving) and 2 500 background points"""
    w = small_world()
    rng = np.random.default_rng(200 + f)
    a = w["obj"][rng.choice(2000, 1500, replace=False)].copy()
    if jumped:
        a["y"] += F(JUMP)
    b = w["obj"][rng.choice(2000, 600, replace=False)].copy()
    b["x"] += F(SECOND_OFFSET)
    c = np.concatenate([a, b, w["full"][rng.choice(w["far"], 2500, replace=False)]])
    return c[rng.permutation(len(c))]


def object_cluster(shift_x=0.0, n=300, seed=7):
    """a model as the model-creation nodes cut it out: n points of the object where it stands in the camera frame"""
    c = small_world()["obj"][np.random.default_rng(seed).choice(2000, n, replace=False)].copy()
    c["x"] += F(shift_x)
    return c


def write_pcd(path, cloud):
    """PCD v0.7 binary with FIELDS x y z rgba, as pcl::PCDWriter lays it out"""
    n = len(cloud)
    hdr = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgba\nSIZE 4 4 4 4\nTYPE F F F U\n"
           "COUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (n, n))
    rec = np.zeros(n, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")]))
    for k in ("x", "y", "z", "rgba"):
        rec[k] = cloud[k]
    with open(path, "wb") as f:
        f.write(hdr.encode())
        f.write(rec.tobytes())


SEGMENT = dict(tol=0.02, min_size=100, max_size=25000)  # the clustering of the end-to-end test (plane and box off)

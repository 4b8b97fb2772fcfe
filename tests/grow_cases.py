"""The inputs of the model-growth tests.  A case is a dict(cfg=<pft_grow_config fields>, ops=[...]) whose ops are
("model", cloud), ("planes", planes) and ("apply", cloud, matrix3x4) in order; tests/test_gpu_grow.py runs every case
through ModelGrowth and through the restatement (tests/grow_model.py) and compares after each apply;
tests/test_grow_host.py shows with the restatement alone that each case tests what it claims."""
import functools

import numpy as np

import grow_model as gm
from pcl_tracking_amd import scene

F = np.float32
LEAF = 0.01
IDENT = np.eye(4, dtype=F)[:3]
LIMIT = 1 << 20


def matrix(t=(0.0, 0.0, 0.0), rpy=(0.0, 0.0, 0.0)):
    return scene.pose_matrix(t[0], t[1], t[2], *rpy)[:3].astype(F)


def centre(k):
    """the centre of cell k at the default leaf: far enough from the faces that float rounding cannot move the key"""
    return ((np.asarray(k, np.float64).reshape(-1, 3) + 0.5) * LEAF).astype(F)


def records(xyz, seed=0):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    rng = np.random.default_rng(1000 + seed)
    p = np.zeros(len(xyz), scene.POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["w"] = 1.0
    p["rgba"] = rng.integers(0, 1 << 32, len(xyz), dtype=np.uint64).astype(np.uint32)
    p["pad"] = rng.integers(0, 1 << 32, (len(xyz), 3), dtype=np.uint64).astype(np.uint32)  # (must not be copied)
    return p


def run(case, grow=None):
    """the case through the restatement -> (the Grow, [states of every apply], [stats after every apply])"""
    g = grow or gm.Grow(**case["cfg"])
    states, stats = [], []
    for op in case["ops"]:
        if op[0] == "model":
            g.set_model(op[1])
        elif op[0] == "planes":
            g.set_planes(op[1])
        else:
            states.append(g.apply(op[1], op[2]).copy())
            stats.append(g.stats())
    return g, states, stats


# ---- keys ----
def fused_xform(T, pts):
    """the row expression as a compiler contracts it: fma(T2, z, fma(T1, y, T0 x)) + T3 (a float product is exact in
    double, so one rounding of the double sum to float is the fused result)"""
    T = np.asarray(T, F).reshape(3, 4).astype(np.float64)
    p = np.asarray(pts, F).astype(np.float64)
    out = np.empty((len(p), 3), F)
    for r in range(3):
        acc = (T[r, 0] * p[:, 0]).astype(F)
        acc = (T[r, 1] * p[:, 1] + acc.astype(np.float64)).astype(F)
        acc = (T[r, 2] * p[:, 2] + acc.astype(np.float64)).astype(F)
        out[:, r] = acc + F(T[r, 3])
    return out


@functools.lru_cache(maxsize=None)
def fused_case_point():
    """-> (T, E): a camera-frame point E whose x cell under Ti differs between the fused and the unfused xform"""
    T = matrix((0.3, -0.2, 1.1), (0.4, -0.3, 0.7))
    Ti = gm.inverse(T)
    inv = F(1.0) / F(LEAF)
    rng = np.random.default_rng(77)
    for _ in range(200):
        yo = rng.uniform(-0.2, 0.2, 3)
        x = (T[:, :3].astype(np.float64) @ yo + T[:, 3]).astype(F)
        y0 = gm.xform(Ti, x[None])[0, 0]
        j = np.round(float(y0) * 100.0)
        x0 = F(float(x[0]) + (j / 100.0 - float(y0)) / float(Ti[0, 0]))
        around = (x0.view(np.int32) + np.arange(-64, 65, dtype=np.int32)).view(F)
        pts = np.stack([around, np.full(129, x[1], F), np.full(129, x[2], F)], 1)
        ku = np.floor(gm.xform(Ti, pts) * inv)
        kf = np.floor(fused_xform(Ti, pts) * inv)
        hit = np.flatnonzero((ku != kf).any(axis=1))
        if len(hit):
            return T, pts[hit[0]]
    raise AssertionError("no such point found")


def keys_case():
    top = LIMIT - 1
    model = centre([(0, 0, 0), (-3, -3, -3), (10, 0, 0), (top - 2, 0, 0), (-(top - 2), 0, 0), (0, top - 2, 0), (0, 0, -(top - 2))])
    faces = np.array([[F(j * LEAF), 0.005, 0.005] for j in range(-3, 14)], F)  # exactly on cell faces of x
    frame1 = np.concatenate([
        centre([(-1, -2, -3)]),                                      # 0 negative coordinates
        np.array([[-0.0001, 0.0001, 0.0001]], F),                    # 1 floor, not truncation: key (-1, 0, 0)
        centre([(top, 0, 0), (top + 1, 0, 0), (-top, 0, 0), (-top - 1, 0, 0)]),  # 2..5 |k| = 2^20 - 1 and 2^20
        centre([(0, top, 0), (0, top + 1, 0), (0, 0, -top), (0, 0, -top - 1)]),  # 6..9
        faces,                                                       # 10..26
    ])
    T, E = fused_case_point()
    Ti = gm.inverse(T)
    ku = np.floor(gm.xform(Ti, E[None]) * (F(1.0) / F(LEAF)))[0].astype(int)
    # a second model whose voxel is E's unfused cell moved one step in y: E is a CANDIDATE of the unfused key
    model2 = centre([(ku[0], ku[1] + 1, ku[2])])
    return dict(cfg=dict(max_radius=20000.0, confirm=1),
                ops=[("model", records(model, 1)), ("apply", records(frame1, 2), IDENT),
                     ("model", records(model2, 3)), ("apply", records(E[None], 4), T)],
                E=E, T=T)


# ---- every state, first rule wins ----
def rules_case():
    T = matrix((0.0, 0.0, 1.0))
    model = centre([(5, 0, 100), (5, 0, 0), (6, 0, 0), (-30, 0, 0)])  # (5, 0, 100): camera z = 2.005, on plane A
    margin = F(0.015)
    up = np.nextafter
    frame = np.array([
        [np.nan, 0.0, 2.0],                 # 0 NONFINITE, would be on plane A
        [0.0, np.inf, 1.0],                 # 1 NONFINITE, would be on plane B
        [0.055, 0.005, 2.005],              # 2 PLANE (A), its voxel (5, 0, 100) is MODEL
        [margin, 0.3, 1.2],                 # 3 PLANE (B): fabsf(..) == plane_margin exactly
        [up(margin, F(1)), 0.3, 1.2],       # 4 not on B: one float above the margin -> UNREACHED
        [-margin, 0.3, 1.2],                # 5 PLANE (B), the other side
        [0.5, 0.0, 1.0],                    # 6 r2 == max_r2 exactly: not FAR -> UNREACHED
        [up(F(0.5), F(1)), 0.0, 1.0],       # 7 FAR
        [0.055, 0.005, 1.005],              # 8 KNOWN (5, 0, 0)
        [0.075, 0.005, 1.005],              # 9 CANDIDATE -> ADDED (7, 0, 0)
        [0.078, 0.008, 1.008],              # 10 CANDIDATE, same voxel, higher index: stays CANDIDATE
        [0.2, 0.2, 1.2],                    # 11 UNREACHED
        [0.3, 0.0, 9.0],                    # 12 FAR
    ], F)
    return dict(cfg=dict(confirm=1), ops=[("model", records(model, 5)), ("planes", [[0, 0, 1, -2], [1, 0, 0, 0]]),
                                          ("apply", records(frame, 6), T), ("apply", records(frame, 6), T)])


# ---- reach ----
DIRECTIONS = [(1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (0, -1, 1), (-1, 1, -1), (1, 1, 1)]


def reach_case(r):
    """a one-voxel model; along every direction a point at Chebyshev distance exactly r and one at r + 1; a mixed offset
    (r, r - 1, 1).  The frame is applied twice with confirm = 1: the voxel at r + 1 is adjacent only to a voxel that is
    confirmed in the same apply, so it is UNREACHED in the first apply and ADDED in the second"""
    ks = []
    for d in DIRECTIONS:
        ks.append(tuple(r * c for c in d))
        ks.append(tuple((r + 1) * c for c in d))
    ks.append((-r, r - 1, 1))
    frame = records(centre(ks), 10 + r)
    return dict(cfg=dict(reach=r, confirm=1, max_voxels=1024),
                ops=[("model", records(centre([(0, 0, 0)]), 7)), ("apply", frame, IDENT), ("apply", frame, IDENT)], keys=ks)


# ---- many points in one voxel ----
CROWDS = {"1_last_in_wave": (1, 63), "2_across_waves": (2, 63), "64_first_in_last_wave": (64, 2176), "65": (65, 127),
          "1000": (1000, 64)}


def crowd_case(name):
    """m candidates in the voxel (2, 0, 0), the lowest at index `first`, the rest scattered behind it; every other point
    of the 2 240 is UNREACHED.  Applied three times with confirm = 3"""
    m, first = CROWDS[name]
    n = 2240
    rng = np.random.default_rng(m)
    xyz = centre(rng.integers(20, 40, (n, 3)))
    where = np.sort(np.concatenate([[first], first + 1 + rng.choice(n - first - 1, m - 1, replace=False)])).astype(int)
    xyz[where] = (np.array([0.02, 0.0, 0.0]) + rng.uniform(0.001, 0.009, (m, 3))).astype(F)
    frame = records(xyz, 20 + m)
    return dict(cfg=dict(), ops=[("model", records(centre([(0, 0, 0)]), 8))] + [("apply", frame, IDENT)] * 3, where=where)


# ---- timing rules ----
def confirm_case(c):
    frame = records(centre([(1, 0, 0), (0, 2, 0)]), 30)
    return dict(cfg=dict(confirm=c), ops=[("model", records(centre([(0, 0, 0)]), 9))] + [("apply", frame, IDENT)] * 3)


def forget_case(f):
    """a voxel seen at applies 1, 2, 4, 5, 6 (apply 3 has no points) with confirm = 3"""
    frame = records(centre([(1, 0, 0)]), 31)
    none = frame[:0]
    seq = [frame, frame, none, frame, frame, frame]
    return dict(cfg=dict(confirm=3, forget=f), ops=[("model", records(centre([(0, 0, 0)]), 9))] + [("apply", s, IDENT) for s in seq])


# ---- frontier and plane ----
def box_face(axis, size=(8, 6, 5)):
    """the cells of the box's face where coordinate `axis` is 0"""
    r = [range(s) for s in size]
    r[axis] = range(1)
    return [(x, y, z) for x in r[0] for y in r[1] for z in r[2]]


def frontier_case(reach=2, confirm=3, applies=7):
    """a box of 8 x 6 x 5 cells: the face z = 0 is the model, the face y = 0 is in every frame"""
    frame = records(centre(box_face(1)), 40)
    return dict(cfg=dict(reach=reach, confirm=confirm),
                ops=[("model", records(centre(box_face(2)), 41))] + [("apply", frame, IDENT)] * applies)


PLANE_PATCH = [(x, y, -1) for x in range(-12, 20) for y in range(-13, 19)]  # the layer under the box


def plane_case(with_plane, applies=8):
    """the same box standing on a plane (the layer z = -1, camera plane z = -0.005).  plane_margin = 0.004 takes that
    layer and nothing of the box; max_radius = 0.1 ends the creep along the plane ten cells from the origin"""
    frame = records(np.concatenate([centre(box_face(1)), centre(PLANE_PATCH)]), 42)
    ops = [("model", records(centre(box_face(2)), 41))]
    if with_plane:
        ops.append(("planes", [[0, 0, 1, 0.005]]))
    return dict(cfg=dict(confirm=1, max_radius=0.1, plane_margin=0.004), ops=ops + [("apply", frame, IDENT)] * applies)


# ---- capacity ----
def near_cells(count, skip=0):
    """`count` distinct cells within Chebyshev distance 4 of the origin, the origin left out"""
    cells = [(x, y, z) for z in range(-4, 5) for y in range(-4, 5) for x in range(-4, 5) if (x, y, z) != (0, 0, 0)]
    return cells[skip:skip + count]


def capacity_case():
    """max_voxels = 64, a one-voxel model.  Apply 1: 63 new voxels, exactly full, accepted.  Apply 2: the same and one
    more: overflow.  Apply 3: the 63 again: it works, from hits = 1.  Applies 4, 5: they are confirmed"""
    full = records(centre(near_cells(63)), 50)
    more = records(centre(near_cells(64)), 51)
    return dict(cfg=dict(reach=4, max_voxels=64),
                ops=[("model", records(centre([(0, 0, 0)]), 9)), ("apply", full, IDENT), ("apply", more, IDENT),
                     ("apply", full, IDENT), ("apply", full, IDENT), ("apply", full, IDENT)])


def rebuild_case(max_voxels):
    """forget = 1: every apply brings 20 voxels never seen again and one that recurs (confirmed at apply 3).  At
    max_voxels = 64 the dying entries force a rebuild before most applies; at 2^16 none happens"""
    ops = [("model", records(centre([(0, 0, 0)]), 9))]
    for a in range(7):
        cells = near_cells(20, skip=1 + 20 * a) + near_cells(1, skip=0) + ([(0, 0, 1 + a)] if a >= 3 else [])
        ops.append(("apply", records(centre(cells), 60 + a), IDENT))
    return dict(cfg=dict(reach=4, forget=1, max_voxels=max_voxels), ops=ops)


def too_many_voxels_model(count):
    return records(centre([(x, 0, 0) for x in range(count)]), 52)


# ---- shapes ----
SIZES = [0, 1, 63, 64, 65, 257, 4099]
MODELS = ["one", "sixty_four", "one_view", "empty"]


@functools.lru_cache(maxsize=None)
def shape_model(name):
    if name == "one":
        return records(centre([(0, 0, 0)]), 70)
    if name == "sixty_four":  # 64 points in 16 voxels
        rng = np.random.default_rng(71)
        return records(centre(np.repeat(near_cells(16, skip=300), 4, axis=0)) + rng.uniform(-0.004, 0.004, (64, 3)).astype(F), 71)
    if name == "one_view":
        return scene.make_model()
    return records(np.zeros((0, 3), F), 72)


def shape_case(model_name, n):
    """n points scattered through the model's neighbourhood at an arbitrary pose, a few of them not finite; two applies"""
    model = shape_model(model_name)
    T = matrix((0.1, -0.05, 0.9), (0.2, -0.1, 0.4))
    rng = np.random.default_rng(100 + n)
    half = 0.05 if model_name in ("one", "empty") else 0.3
    yo = rng.uniform(-half, half, (n, 3))
    if len(model) and n:
        near = rng.random(n) < 0.5  # half of them right beside model points
        pick = rng.integers(0, len(model), n)
        mx = gm.xyz_of(model).astype(np.float64)
        yo[near] = mx[pick[near]] + rng.uniform(-0.02, 0.02, (int(near.sum()), 3))
    x = (yo @ T[:, :3].astype(np.float64).T + T[:, 3]).astype(F)
    x[::97, 1] = np.nan
    frame = records(x, 73 + n)
    return dict(cfg=dict(confirm=2), ops=[("model", model), ("apply", frame, T), ("apply", frame, T)])


# ---- the ghost ----
ROLLED_POSE = scene.GT_POSE[:3] + (scene.GT_POSE[3] + 0.5,) + scene.GT_POSE[4:]


@functools.lru_cache(maxsize=None)
def ghost_world():
    """the frame with the object rolled by +0.5 rad (faces 2 and 4 visible), the one-view model, its true pose, and which
    frame points lie on the object"""
    frame = scene.make_scene(50000, obj_pose=ROLLED_POSE)
    model = scene.make_model()
    T = scene.pose_matrix(*scene.model_gt_pose(ROLLED_POSE))[:3].astype(F)
    box = scene.pose_matrix(*ROLLED_POSE)
    local = (gm.xyz_of(frame).astype(np.float64) - box[:3, 3]) @ box[:3, :3]
    on_object = (np.abs(local) <= np.asarray(scene.MODEL_DIMS) / 2 + 0.01).all(axis=1)
    return dict(frame=frame, model=model, T=T, on_object=on_object)


@functools.lru_cache(maxsize=None)
def ghost_run():
    """confirm = 1, the frame applied until the restatement stops adding -> (the Grow, [states], [stats])"""
    w = ghost_world()
    g = gm.Grow(confirm=1)
    g.set_model(w["model"])
    states, stats = [], []
    while not stats or stats[-1]["n_added"]:
        states.append(g.apply(w["frame"], w["T"]).copy())
        stats.append(g.stats())
    return g, states, stats


@functools.lru_cache(maxsize=None)
def ghost_counts():
    """the object's frame points that a subtraction at the true pose leaves in the residual (2 cm or more from every
    model point, by the subtraction's own arithmetic): with the one-view model, and with the grown one"""
    import subtract_model as sm

    w = ghost_world()
    obj = sm.xyz_of(w["frame"])[w["on_object"]]

    def left(model):
        return sm.subtract(obj, {0: (sm.xyz_of(model), w["T"])}, 0.02)["n_residual"]

    return dict(object=int(w["on_object"].sum()), before=left(w["model"]), after=left(ghost_run()[0].cloud))


# ---- the driver's sequence ----
ROLL_STEP = 0.1
ROLLING_FLAGS = ["--box", "-10,10,-10,10,-10,10", "--tolerance", "0.02", "--min-size", "500"]


@functools.lru_cache(maxsize=None)
def rolling_sequence(n_frames=5):
    """[scene, frame 1 .. n_frames]: the box of scene.MODEL_DIMS one metre in front of the camera, before a wall at
    z = 1.6 (the plane --segment removes); only the faces turned towards the camera.  In the scene the box shows one
    face; it rolls by ROLL_STEP per frame, and from the second frame on a second face is in view"""
    rng = np.random.default_rng(2026)
    xyz, fid = scene._box_surface_lattice(scene.MODEL_DIMS, 0.008)
    g = np.meshgrid(np.arange(-0.8, 0.8, 0.012), np.arange(-0.6, 0.6, 0.012), indexing="ij")
    wall = np.stack([g[0].ravel(), g[1].ravel(), np.full(g[0].size, 1.6)], 1)
    out = []
    for f in range(n_frames + 1):
        pose = (0.0, 0.0, 1.0, ROLL_STEP * f, 0.0, 0.0)
        T = scene.pose_matrix(*pose)
        keep = np.isin(fid, scene._visible_faces(scene.MODEL_DIMS, pose))
        box = xyz[keep] @ T[:3, :3].T + T[:3, 3]
        pts = np.concatenate([box, wall]) + rng.uniform(-0.001, 0.001, (int(keep.sum()) + len(wall), 3))
        rgb = np.concatenate([scene.FACE_RGB[fid[keep]], np.tile([[170, 170, 165]], (len(wall), 1))])
        out.append(scene.make_points(pts.astype(F), rgb)[rng.permutation(len(pts))])
    return out


CASES = {"keys": keys_case, "rules": rules_case, "frontier": frontier_case, "capacity": capacity_case,
         "plane_set": lambda: plane_case(True), "plane_unset": lambda: plane_case(False),
         "rebuild_64": lambda: rebuild_case(64), "rebuild_65536": lambda: rebuild_case(1 << 16)}
CASES.update({"reach_%d" % r: functools.partial(reach_case, r) for r in (1, 2, 3, 4)})
CASES.update({"crowd_" + k: functools.partial(crowd_case, k) for k in CROWDS})
CASES.update({"confirm_%d" % c: functools.partial(confirm_case, c) for c in (1, 2, 3)})
CASES.update({"forget_%d" % f: functools.partial(forget_case, f) for f in (1, 2)})
CASES.update({"shape_%s_%d" % (m, n): functools.partial(shape_case, m, n) for m in MODELS for n in SIZES
              if m == "one_view" or n in (0, 65, 4099)})

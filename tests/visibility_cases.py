"""Shared case builders of the visibility tests: tests/test_visibility_host.py runs every case through the NumPy model alone
(each case must show the states it claims), tests/test_gpu_visibility.py runs the same cases on the device.

An explicit case is dict(cam, ref (M, 3), T (3, 4), frame (N, 3), claim) with claim a function of the model's output.  The
small camera has power-of-two intrinsics, so that the hand-made cases hit pixels, pixel borders and margins exactly."""
import functools

import numpy as np

import visibility_model as vm

F = np.float32
IDENTITY = np.eye(4, dtype=F)[:3]
MARGIN = 0.03125  # 2^-5: exact in float, so is 2 - MARGIN
SMALL = dict(width=16, height=12, fx=16.0, fy=16.0, cx=8.0, cy=6.0, z_near=0.25, splat=1, occlusion_margin=MARGIN,
             self_margin=MARGIN)


def small(**kw):
    c = dict(SMALL)
    c.update(kw)
    return c


def at_pixel(cam, u, v, z):
    """the point whose projection is exactly (u + 0.5, v + 0.5) at depth z (exact for the small camera and dyadic z)"""
    return [(u + 0.5 - cam["cx"]) / cam["fx"] * z, (v + 0.5 - cam["cy"]) / cam["fy"] * z, z]


def pts(rows):
    return np.asarray(rows, F).reshape(-1, 3)


def rotation(roll, pitch, yaw, t):
    from pcl_tracking_amd import scene

    return scene.pose_matrix(t[0], t[1], t[2], roll, pitch, yaw)[:3].astype(F)


# ---- hand-made cases (identity matrix; the expected arrays are worked out by hand) --------------------------------------
def occluder_3pt():
    """three model points at z = 2 in pixels (8, 6), (12, 6), (4, 8); one frame point at z = 1 in pixel (8, 6): its 3 x 3
    footprint covers the first model point only"""
    cam = small()
    return dict(cam=cam, ref=pts([[0, 0, 2], [0.5, 0, 2], [-0.5, 0.25, 2]]), T=IDENTITY, frame=pts([[0, 0, 1]]),
                state=[vm.OCCLUDED, vm.VISIBLE, vm.VISIBLE], scene_gap=[1.0, 0.0, 0.0], self_gap=[0.0, 0.0, 0.0])


def precedence():
    """two model points in one pixel, z = 2 and 3, behind a frame point at z = 1: the back one is SELF_OCCLUDED although the
    scene covers it too (self before scene), the front one OCCLUDED"""
    cam = small()
    return dict(cam=cam, ref=pts([[0, 0, 2], [0, 0, 3]]), T=IDENTITY, frame=pts([[0, 0, 1]]),
                state=[vm.OCCLUDED, vm.SELF_OCCLUDED], scene_gap=[1.0, 2.0], self_gap=[0.0, 1.0])


def border_clip():
    """model points in the corner pixels (0, 0) and (15, 11) and in the centre; frame points at z = 1 in pixels (1, 1) and
    (14, 10): their footprints reach the corners and are cut by the image border"""
    cam = small()
    return dict(cam=cam, ref=pts([at_pixel(cam, 0, 0, 2), at_pixel(cam, 15, 11, 2), at_pixel(cam, 8, 6, 2)]), T=IDENTITY,
                frame=pts([at_pixel(cam, 1, 1, 1), at_pixel(cam, 14, 10, 1)]),
                state=[vm.OCCLUDED, vm.OCCLUDED, vm.VISIBLE], scene_gap=[1.0, 1.0, 0.0], self_gap=[0.0, 0.0, 0.0])


def strict_gates():
    """gap == margin exactly is not occluded, for either test: pixels (4, 2) scene gap == margin, (12, 2) scene gap twice the
    margin, (4, 10) two model points whose self gap == margin, (12, 10) self gap twice the margin"""
    cam = small()
    m = MARGIN
    ref = [at_pixel(cam, 4, 2, 2.0), at_pixel(cam, 12, 2, 2.0), at_pixel(cam, 4, 10, 2.0), at_pixel(cam, 4, 10, 2.0 + m),
           at_pixel(cam, 12, 10, 2.0), at_pixel(cam, 12, 10, 2.0 + 2 * m)]
    frame = [at_pixel(cam, 4, 2, 2.0 - m), at_pixel(cam, 12, 2, 2.0 - 2 * m)]
    return dict(cam=cam, ref=pts(ref), T=IDENTITY, frame=pts(frame),
                state=[vm.VISIBLE, vm.OCCLUDED, vm.VISIBLE, vm.VISIBLE, vm.VISIBLE, vm.SELF_OCCLUDED],
                scene_gap=[m, 2 * m, 0, 0, 0, 0], self_gap=[0, 0, 0, m, 0, 2 * m])


HAND_MADE = dict(occluder_3pt=occluder_3pt, precedence=precedence, border_clip=border_clip, strict_gates=strict_gates)


# ---- adversarial cases with an explicit matrix (the claim is a predicate on the model's output) --------------------------
def depth_ties():
    """frame points at exactly the model's depth (gap 0), several frame points of one depth in one pixel, model points of
    one depth in one pixel"""
    cam = small()
    ref = [at_pixel(cam, 4, 4, 2.0), at_pixel(cam, 4, 4, 2.0), at_pixel(cam, 10, 4, 1.5), at_pixel(cam, 10, 8, 1.5)]
    frame = [at_pixel(cam, 4, 4, 2.0), at_pixel(cam, 4, 4, 2.0), at_pixel(cam, 10, 4, 1.5), at_pixel(cam, 10, 8, 1.0),
             at_pixel(cam, 10, 8, 1.0), at_pixel(cam, 10, 8, 1.0)]
    return dict(cam=cam, ref=pts(ref), T=IDENTITY, frame=pts(frame),
                claim=lambda o: o["state"].tolist() == [0, 0, 0, 1] and o["scene_gap"].tolist() == [0, 0, 0, 0.5])


def nonfinite_frame():
    """NaN, +-inf, z <= 0 and z == z_near in the frame: none of them covers anything; the one finite point does"""
    cam = small()
    n, i = np.nan, np.inf
    ref = [at_pixel(cam, 8, 6, 2.0), at_pixel(cam, 3, 3, 2.0)]
    frame = [[n, 0, 1], [0, n, 1], [0, 0, n], [i, 0, 1], [-i, 0, 1], [0, i, 1], [0, 0, i], [0, 0, -i], [i, i, i],
             [0, 0, 0], [0, 0, -1], [0, 0, cam["z_near"]], [-0.0, 0.0, -0.0], at_pixel(cam, 3, 3, 1.0)]
    return dict(cam=cam, ref=pts(ref), T=IDENTITY, frame=pts(frame),
                claim=lambda o: o["state"].tolist() == [vm.VISIBLE, vm.OCCLUDED])


def behind_camera():
    """the matrix turns the model so that one point lies behind the camera, one on the near plane, one beside the image"""
    cam = small()
    T = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 1.0]], F)  # z -> 1 - z
    ref = [[0, 0, 2.0], [0, 0, 0.75], [0, 0, -1.0], [5.0, 0, -1.0], [0.25, 0.125, -0.5]]
    return dict(cam=cam, ref=pts(ref), T=T, frame=pts([[0, 0, 0.5]]),
                claim=lambda o: o["state"].tolist() == [3, 3, vm.OCCLUDED, 3, vm.VISIBLE])


def no_overlap():
    """frame points in front of the model's depth but in other pixels, beside the image and behind the camera: the
    footprints never meet the model's pixels"""
    cam = small()
    rng = np.random.default_rng(5)
    ref = [at_pixel(cam, u, v, 2.0) for u in (2, 3, 4) for v in (2, 3)]
    frame = [at_pixel(cam, u, v, 1.0) for u in range(7, 16) for v in range(0, 12)]
    frame += [at_pixel(cam, u, v, 1.0) for u in range(0, 7) for v in range(6, 12)]
    frame += [[9.0, 0, 1], [0, -9.0, 1], [0, 0, -1]]
    frame = pts(frame)[rng.permutation(len(frame))]
    return dict(cam=cam, ref=pts(ref), T=IDENTITY, frame=frame,
                claim=lambda o: o["n_visible"] == 6 and not o["scene_gap"].any())


def pruning():
    """frame points in the model's own pixels, all farther than the largest moved z, and some nearer ones: the far ones
    leave every gap at 0"""
    cam = small()
    ref = [at_pixel(cam, u, 5, 1.0 + 0.125 * u) for u in range(2, 14, 3)]
    far = [at_pixel(cam, u, 5, 3.0 + 0.25 * k) for u in range(2, 14, 3) for k in range(3)]
    near = [at_pixel(cam, 2, 5, 0.5)]
    return dict(cam=cam, ref=pts(ref), T=IDENTITY, frame=pts(far + near),
                claim=lambda o: o["state"].tolist() == [1, 0, 0, 0] and o["scene_gap"].tolist() == [0.75, 0, 0, 0])


def one_point_frame():
    cam = vm.camera()
    return dict(cam=cam, ref=pts([[0.01 * k, 0, 1.0] for k in range(-3, 4)]), T=IDENTITY, frame=pts([[0, 0, 0.5]]),
                claim=lambda o: o["n_frame"] == 1 and 0 < o["n_occluded"] < 7 and o["n_visible"] > 0)


def one_point_model():
    cam = vm.camera()
    return dict(cam=cam, ref=pts([[0.02, 0.01, 0]]), T=rotation(0.3, -0.2, 0.5, (0.1, 0.0, 1.0)),
                frame=random_frame(7, 500), claim=lambda o: o["n_reference"] == 1)


def random_frame(seed, n, depth=(0.4, 1.6), spread=0.5):
    rng = np.random.default_rng(seed)
    z = rng.uniform(depth[0], depth[1], n)
    return np.stack([rng.uniform(-spread, spread, n) * z, rng.uniform(-spread, spread, n) * z, z], 1).astype(F)


ALL_STATES = ("n_visible", "n_occluded", "n_self", "n_out")


def random_case(seed, cam, M=300, N=2000, spread=0.5, need=ALL_STATES):
    """a tilted box surface of M points in the middle of a random frame: every state of `need` occurs (a coarse image
    folds a tilted face into few pixels, so nearly all of it is self-occluded there)"""
    rng = np.random.default_rng(seed)
    box = rng.uniform(-0.12, 0.12, (M, 3))
    a = rng.integers(0, 3, M)
    box[np.arange(M), a] = np.where(rng.random(M) < 0.5, -0.12, 0.12)  # on the faces: the far ones are self-occluded
    box[: M // 10] *= 12.0  # some points leave the image or pass the camera
    T = rotation(0.4, -0.3, 0.7, (0.03, -0.02, 1.0))
    return dict(cam=cam, ref=box.astype(F), T=T, frame=random_frame(seed + 1, N, spread=spread),
                claim=lambda o: all(o[k] > 0 for k in need))


ADVERSARIAL = dict(
    depth_ties=depth_ties, nonfinite_frame=nonfinite_frame, behind_camera=behind_camera, no_overlap=no_overlap,
    pruning=pruning, one_point_frame=one_point_frame, one_point_model=one_point_model,
    random_small=lambda: random_case(11, small(), need=("n_occluded", "n_self", "n_out")),
    random_default=lambda: random_case(12, vm.camera()),
    splat0=lambda: random_case(13, vm.camera(splat=0), spread=0.25),
    splat4=lambda: random_case(14, vm.camera(splat=4)),
    splat4_small=lambda: random_case(15, small(splat=4), M=37, N=301, need=("n_occluded", "n_self", "n_out")),
    wide_image=lambda: random_case(16, vm.camera(width=1024, height=3, fx=600.0, cx=511.5, cy=1.0), M=129, N=777,
                                   need=("n_visible", "n_occluded", "n_out")),
)


# ---- tracked scenes (the result pose): a flat patch of 300 points one metre in front of the camera -----------------------
PATCH_POSE = (0.05, -0.03, 1.0, 0.05, -0.1, 0.2)
RULE_THRESHOLD = (0.25, 0.5, 2)
# full: the patch and the wall; gone: the wall alone (all visible, nothing matched); hidden: a plate in front of all of it
RULE_SEQUENCE = ["full", "gone", "hidden", "gone", "full", "gone"]


def _lattice(nx, ny, step):
    x, y = np.meshgrid((np.arange(nx) - (nx - 1) / 2) * step, (np.arange(ny) - (ny - 1) / 2) * step, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], 1)


@functools.lru_cache(maxsize=None)
def patch_model():
    """20 x 15 points at 1 cm in the model's z = 0 plane, as a point cloud of the tracker's layout"""
    from pcl_tracking_amd import scene

    xyz = _lattice(20, 15, 0.01).astype(F)
    rgb = np.stack([120 + 6 * np.arange(len(xyz)) % 100, np.full(len(xyz), 90), np.full(len(xyz), 60)], 1)
    return scene.make_points(xyz, rgb)


def patch_trans():
    from pcl_tracking_amd import scene

    return scene.pose_matrix(*PATCH_POSE).astype(F)


def _move(xyz, T):
    return (xyz.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)).astype(F)


@functools.lru_cache(maxsize=None)
def patch_frame(kind, f=0):
    """frames of at most 2 000 points: "full" the patch (a 0.5 cm sample of its surface) and a wall 0.6 m behind it;
    "half" the x <= centre half of the patch hidden behind a plate 0.2 m in front; "hidden" all of it behind the plate;
    "gone" the wall alone"""
    from pcl_tracking_amd import scene

    rng = np.random.default_rng(300 + f)
    T = patch_trans()
    surf = _move(_lattice(40, 30, 0.005) + rng.uniform(-0.001, 0.001, (1200, 3)) * [1, 1, 0], T)
    wall = np.concatenate([_lattice(25, 20, 0.03)[:, :2] + PATCH_POSE[:2], np.full((500, 1), 1.6)], 1).astype(F)
    cx = PATCH_POSE[0]
    plate = _lattice(30, 24, 0.01)  # 0.30 x 0.24 at z = 0.8: covers the patch's lines of sight with room to spare
    plate = (plate + [cx * 0.8, PATCH_POSE[1] * 0.8, 0.8]).astype(F)
    if kind == "full":
        parts, cols = [surf, wall], [(150, 90, 60), (80, 80, 80)]
    elif kind == "gone":
        parts, cols = [wall], [(80, 80, 80)]
    elif kind == "hidden":
        parts, cols = [plate, wall], [(30, 30, 200), (80, 80, 80)]
    elif kind == "half":
        # the plate's right edge on the line of sight of the patch's centre; the sensor sees the other half only
        left = plate[plate[:, 0] <= cx * 0.8]
        parts, cols = [surf[surf[:, 0] / surf[:, 2] > cx / PATCH_POSE[2] + 0.01], left, wall], [(150, 90, 60), (30, 30, 200), (80, 80, 80)]
    else:
        raise KeyError(kind)
    xyz = np.concatenate(parts)
    rgb = np.concatenate([np.tile(np.array(c), (len(p), 1)) for p, c in zip(parts, cols)])
    order = rng.permutation(len(xyz))
    assert len(xyz) <= 2000
    return scene.make_points(xyz[order], rgb[order])


def cloud_xyz(cloud):
    return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(F)

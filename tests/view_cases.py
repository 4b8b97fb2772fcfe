"""Constructed inputs of the view-selection tests: tests/test_view_host.py runs every case through the NumPy model alone (a
case carries the answer worked out by hand as `state`, or a `claim` about the model's output), tests/test_gpu_view.py runs
the same cases on the device.

A case is dict(cam, xyz (N, 3) float32, T (3, 4), K) plus `state` and / or `claim`.  The small camera has power-of-two
intrinsics, so that the hand-made cases hit pixels, pixel borders and the margin exactly."""
import functools

import numpy as np

import view_model as wm
import visibility_model as vm
from visibility_cases import IDENTITY, MARGIN, at_pixel, pts, small

F = np.float32
K_, D_, S_, O_, N_ = wm.KEPT, wm.DECIMATED, wm.SELF_OCCLUDED, wm.OUT_OF_VIEW, wm.NONFINITE


def records(xyz):
    """the 32-byte records of the points: every byte behind xyz carries a pattern of the index, so that a copy that drops
    or mixes a field shows"""
    from pcl_tracking_amd.scene import POINT_DTYPE

    xyz = np.asarray(xyz, F).reshape(-1, 3)
    r = np.zeros(len(xyz), POINT_DTYPE)
    r["x"], r["y"], r["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    i = np.arange(len(xyz), dtype=np.uint32)
    r["w"] = (i % 251).astype(F)
    r["rgba"] = i * np.uint32(2654435761)
    r["pad"] = (i[:, None] * np.uint32(3) + np.arange(3, dtype=np.uint32)) ^ np.uint32(0xA5A5A5A5)
    return r


def case(cam, xyz, T=IDENTITY, K=0, **kw):
    return dict(cam=cam, xyz=pts(xyz), T=np.asarray(T, F), K=K, **kw)


# ---- hand-made cases ------------------------------------------------------------------------------------------------------
def two_plates():
    """two parallel 20 x 15 cm plates of a 1 cm lattice, 10 cm apart, seen head-on with the default camera: the back plate's
    points project inside the front plate's footprints, so the kept points are the front plate"""
    ax, ay = np.arange(-0.095, 0.1, 0.01), np.arange(-0.07, 0.075, 0.01)
    x, y = (a.ravel() for a in np.meshgrid(ax, ay, indexing="ij"))
    front = np.stack([x, y, np.full_like(x, 1.0)], 1)
    back = np.stack([x, y, np.full_like(x, 1.1)], 1)
    n = len(front)
    return case(vm.camera(), np.concatenate([front, back]), state=[K_] * n + [S_] * n,
                claim=lambda o: o["kept_index"].tolist() == list(range(n)))


def strict_gate():
    """pixel (4, 10): a second point exactly self_margin behind the first is kept (the comparison is strict); pixel
    (12, 10): one ulp further back it is occluded"""
    cam = small()
    beyond = np.nextafter(F(2.0 + MARGIN), F(3))
    xyz = [at_pixel(cam, 4, 10, 2.0), at_pixel(cam, 4, 10, 2.0 + MARGIN), at_pixel(cam, 12, 10, 2.0), at_pixel(cam, 12, 10, beyond)]
    return case(cam, xyz, state=[K_, K_, K_, S_], gap=[0, MARGIN, 0, beyond - F(2.0)])


def equal_z():
    """two points in one pixel at one depth: neither hides the other, both gaps are 0"""
    cam = small()
    return case(cam, [at_pixel(cam, 5, 5, 2.0), at_pixel(cam, 5, 5, 2.0)], state=[K_, K_], gap=[0, 0])


def border_clip():
    """far points (z = 2) in the four corner pixels and in the middle of the four border rows / columns; near points
    (z = 1) one pixel inside of (0, 0), (15, 11), (8, 0) and (0, 6).  Every footprint here is cut by a border or a corner;
    the near points cover their far neighbours, the other four far points stay"""
    cam = small()
    far = [(0, 0), (15, 0), (0, 11), (15, 11), (8, 0), (8, 11), (0, 6), (15, 6)]
    near = [(1, 1), (14, 10), (8, 1), (1, 6)]
    xyz = [at_pixel(cam, u, v, 2.0) for u, v in far] + [at_pixel(cam, u, v, 1.0) for u, v in near]
    return case(cam, xyz, state=[S_, K_, K_, S_, S_, K_, S_, K_] + [K_] * 4, gap=[1, 0, 0, 1, 1, 0, 1, 0] + [0] * 4)


def one_pixel_image():
    """a 1 x 1 image: every in-view point shares the pixel"""
    cam = small(width=1, height=1, fx=1.0, fy=1.0, cx=0.5, cy=0.5)
    return case(cam, [[0, 0, 2], [0.25, -0.25, 3], [2, 0, 2], [0, -2, 2]], state=[K_, S_, O_, O_], gap=[0, 1, 0, 0])


def z_near_plane():
    """z == z_near is behind the near plane (front = z > z_near); one ulp further it is in view"""
    cam = small()
    return case(cam, [[0, 0, cam["z_near"]], [0, 0, np.nextafter(F(cam["z_near"]), F(1))], [0, 0, -1.0]],
                state=[O_, K_, O_], gap=[0, 0, 0])


def nonfinite_records():
    """NaN, +inf and -inf in each coordinate of an otherwise visible record, and one clean record.  Record 7 is
    (0, 0, +inf): see test_view_host.py on what keeps it out"""
    bad = []
    for c in range(3):
        for val in (np.nan, np.inf, -np.inf):
            p = [0.0, 0.0, 2.0]
            p[c] = val
            bad.append(p)
    return case(small(), bad + [[0, 0, 2.0]], state=[N_] * 9 + [K_], gap=[0] * 10)


def overflowing_q():
    """finite records whose q overflows: qz = 2 * 3e38 = +inf with qx = qy = 0 (in_view holds for such a q, its footprint
    splats +inf and, with no other point over its pixel (8, 6), its gap is fmaxf(inf - inf, 0) = 0: the finiteness clause of
    rule 2 alone keeps it out), and qx = +inf.  The third record lands in pixel (12, 8)"""
    T = np.array([[2, 0, 0, 0], [0, 1, 0, 0], [0, 0, 2, 0]], F)
    return case(small(), [[0, 0, 3e38], [3e38, 0, 1.0], [0.25, 0.25, 1.0]], T=T, state=[O_, O_, K_], gap=[0, 0, 0])


DECIMATION_N = 12


def decimation(K):
    """twelve visible points in twelve pixels of one row; K in {1, 11, 12, 13, 5}"""
    cam = small(splat=0)
    return case(cam, [at_pixel(cam, 2 + i, 6, 2.0) for i in range(DECIMATION_N)], K=K)


DECIMATION_K = (1, DECIMATION_N - 1, DECIMATION_N, DECIMATION_N + 1, 5)


def all_visible():
    cam = small(splat=0)
    return case(cam, [at_pixel(cam, u, v, 2.0) for v in range(12) for u in range(16)], state=[K_] * 192)


def none_visible():
    """behind the camera, beside the image, and not finite"""
    return case(small(), [[0, 0, -1.0]] * 40 + [[100, 0, 1.0]] * 40 + [[np.nan, 0, 1.0]] * 20, state=[O_] * 80 + [N_] * 20)


def alternating():
    """pairs in one pixel, front then back, 80 pixels: kept, occluded, kept, occluded, ..."""
    cam = small(splat=0)
    xyz = []
    for i in range(80):
        xyz += [at_pixel(cam, i % 16, i // 16, 2.0), at_pixel(cam, i % 16, i // 16, 3.0)]
    return case(cam, xyz, state=[K_, S_] * 80)


HAND_MADE = dict(two_plates=two_plates, strict_gate=strict_gate, equal_z=equal_z, border_clip=border_clip,
                 one_pixel_image=one_pixel_image, z_near_plane=z_near_plane, nonfinite_records=nonfinite_records,
                 overflowing_q=overflowing_q, all_visible=all_visible, none_visible=none_visible, alternating=alternating)


# ---- sizes: a random two-face shell at 1 m, the default camera ------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 256, 257, 1023, 1025)
BIG = (1 << 18) + 3
SHELL_T = np.array([[1, 0, 0, 0.02], [0, 1, 0, -0.01], [0, 0, 1, 1.0]], F)


@functools.lru_cache(maxsize=None)
def shell(N, K=0):
    """N points of the two large faces of a 40 x 40 x 20 cm box shell (z = -0.1 or +0.1 at random, +- 5 mm), moved to 1 m:
    dense enough (at BIG) that the far face is occluded by the near one, so about half the points are visible; every 97th
    record is not finite, every 89th lies behind the camera"""
    rng = np.random.default_rng(1000 + N)
    xyz = rng.uniform(-0.2, 0.2, (N, 3))
    xyz[:, 2] = np.where(rng.random(N) < 0.5, -0.1, 0.1) + rng.uniform(-0.005, 0.005, N)
    xyz = xyz.astype(F)
    xyz[5::97, 1] = np.nan
    xyz[7::89, 2] = F(-3.0)
    return case(vm.camera(), xyz, T=SHELL_T, K=K)


def all_cases():
    """name -> builder of every case the device is compared on (BIG apart: it takes seconds on the host)"""
    out = dict(HAND_MADE)
    for K in DECIMATION_K:
        out["decimation_K%d" % K] = functools.partial(decimation, K)
    for N in SIZES:
        out["shell_%d" % N] = functools.partial(shell, N)
    out["shell_1025_K333"] = functools.partial(shell, 1025, 333)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's output of a case, computed once and shared (treat as read-only)"""
    c = all_cases()[name]() if name != "big" else shell(BIG, 50001)
    return c, wm.select(c["cam"], c["xyz"], c["T"], c["K"])

"""Inputs of the colour-path tests (tests/test_gpu_colour_path.py, the colour case of tests/test_gpu_match.py): colours that
reach every branch of the integer RGB2HSV and of HSVColorCoherence, and two rigs in which a particle's weight is ONE pair
value, so that a slip in one term is not hidden in a sum of M of them.  tests/test_colour_cases_host.py proves with the
oracle alone that these inputs are what they claim to be.

Colours are (r, g, b) triples; clouds carry them as PCL's rgba word (a << 24 | r << 16 | g << 8 | b) with random alpha
bytes, which RGB2HSV must ignore.
"""
import functools

import numpy as np

import oracle
from pcl_tracking_amd import scene

EDGES = [
    (0, 0, 0), (255, 255, 255), (1, 1, 1), (77, 77, 77), (254, 254, 254),  # v == 0; diff == 0: div_table(0), h = s = 0
    (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255),  # s == 255, every v == r / g / b case
    (255, 0, 1), (255, 1, 0), (255, 0, 17), (255, 17, 0),  # v == r with g < b or b < g: h < 0 before the wrap in one order
    (1, 0, 0), (0, 1, 0), (0, 0, 1),  # v == diff == 1: the largest table entries
    (254, 255, 255), (255, 254, 255), (255, 255, 254),  # diff == 1 under v == 255: s == 1
    (255, 230, 235), (200, 255, 210), (215, 220, 255),  # pastels: small s, large v
]
REF_HUES = (0, 1, 45, 89, 90, 91, 179)
N_TARGETS = 256


def rgba_of(colours, alpha):
    c = np.asarray(colours, np.uint32).reshape(-1, 3)
    return scene.pack_rgba(c[:, 0], c[:, 1], c[:, 2], np.asarray(alpha, np.uint32))


def hsv_of(colours, argorder=1):
    """(n, 3) ints h, s, v of the oracle's integer RGB2HSV"""
    k = oracle.hsv_pack_many(oracle.default_config(hsv_pcl180_argorder=argorder), rgba_of(colours, 0))
    return np.stack([k & 0xff, (k >> 8) & 0xff, (k >> 16) & 0xff], 1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def hues():
    """HUES: one colour for every hue 0 .. 179 of the default argument order (the other order mirrors the hue circle, so it
    sees every hue as well): the first of 8 192 seeded random colours with that hue, which varies s and v"""
    rng = np.random.default_rng(20261020)
    cand = rng.integers(0, 256, (8192, 3))
    h = hsv_of(cand)[:, 0]
    grey = (cand.max(1) == cand.min(1))
    out = []
    for want in range(180):
        k = np.flatnonzero((h == want) & ~grey)
        assert len(k), want
        out.append(tuple(int(x) for x in cand[k[0]]))
    return out


@functools.lru_cache(maxsize=None)
def targets():
    """TARGETS: EDGES + HUES + random colours up to 256 -> (colours (256, 3), rgba words with random alpha bytes)"""
    rng = np.random.default_rng(20261021)
    c = np.array(EDGES + hues(), np.int64)
    c = np.concatenate([c, rng.integers(0, 256, (N_TARGETS - len(c), 3))])
    return c, rgba_of(c, rng.integers(0, 256, N_TARGETS))


@functools.lru_cache(maxsize=None)
def refs():
    """REFS: EDGES and the HUES entries of REF_HUES -> (colours (n, 3), rgba words with random alpha bytes)"""
    rng = np.random.default_rng(20261022)
    c = np.array(EDGES + [hues()[h] for h in REF_HUES], np.int64)
    return c, rgba_of(c, rng.integers(0, 256, len(c)))


def hue_tie(a, b):
    """HSVColorCoherence's two hue differences of the float hues a / 180.0f (source) and b / 180.0f (target) are equal"""
    sh, th = np.float32(a) / np.float32(180.0), np.float32(b) / np.float32(180.0)
    one = np.float32(1.0)
    hd1 = np.abs(sh - th)
    hd2 = np.where(sh < th, np.abs((one + sh) - th), np.abs((one + th) - sh))
    return hd1 == hd2


def _two_point_model(ref_rgba):
    m = scene.make_points(np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.5]], np.float32), np.zeros((2, 3)))
    m["rgba"] = np.uint32(ref_rgba)
    return m


def _identity_particles(xyz):
    p = np.zeros(len(xyz), scene.PARTICLE_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["w"] = 1.0
    p["weight"] = 1.0 / len(xyz)
    return p


def pair_rig(ref_rgba, target_rgba, seed, amp):
    """One pair per particle.  Model: A at the origin with the reference colour, B at (0, 0, 0.5).  Cloud: 256 points on a
    16 x 16 grid of 0.25 m pitch at z = 1, jittered by +-5 cm, coloured by target_rgba.  Particle i: identity rotation,
    translated onto cloud point i plus a uniform offset of at most amp per axis; a quarter of the particles, among them
    those on the six extreme cloud points, get offset 0 (distance exactly 0; the crop box then holds the whole cloud).
    A then lies within amp * sqrt(3) of cloud point i and 0.15 m or more from every other one; B lies 0.4 m or more from
    every point, outside the gate of 0.1 m.  -> dict(model, cloud, particles, max_distance)"""
    rng = np.random.default_rng(1000 + seed)
    g = (np.arange(16) - 7.5) * 0.25
    xyz = np.stack([np.repeat(g, 16), np.tile(g, 16), np.ones(256)], 1) + rng.uniform(-0.05, 0.05, (256, 3))
    xyz = xyz.astype(np.float32)
    cloud = scene.make_points(xyz, np.zeros((256, 3)))
    cloud["rgba"] = np.asarray(target_rgba, np.uint32)
    zero = np.zeros(256, bool)
    zero[np.concatenate([xyz.argmin(0), xyz.argmax(0)])] = True
    rest = rng.permutation(np.flatnonzero(~zero))
    zero[rest[:64 - int(zero.sum())]] = True
    off = rng.uniform(-amp, amp, (256, 3)).astype(np.float32)
    off[zero] = 0.0
    return dict(model=_two_point_model(ref_rgba), cloud=cloud, particles=_identity_particles(xyz + off), max_distance=0.1,
                zero_offset=zero)


def gate_rig():
    """The gate at equality.  The same model; a 16 x 16 grid of 0.5 m pitch at z = 1 with exactly representable
    coordinates; max_distance = 0.125, so max_distance^2 = 0.015625 exactly in float and in double.  Particle i sits 0.125
    from cloud point i along direction (i // 3) % 6 of +x -x +y -y +z -z; kind i % 3: 0 exactly on the gate (squared
    distance == 0.015625: outside, the comparison is strict), 1 one float inside, 2 one float outside.
    -> dict(model, cloud, particles, max_distance, kind)"""
    g = (np.arange(16) - 8) * 0.5
    xyz = np.stack([np.repeat(g, 16), np.tile(g, 16), np.ones(256)], 1).astype(np.float32)
    c, rgba = targets()
    cloud = scene.make_points(xyz, np.zeros((256, 3)))
    cloud["rgba"] = rgba
    i = np.arange(256)
    kind, direction = i % 3, (i // 3) % 6
    axis, sign = direction // 2, np.where(direction % 2 == 0, 1.0, -1.0).astype(np.float32)
    pos = xyz.copy()
    on = (xyz[i, axis] + sign * np.float32(0.125)).astype(np.float32)
    inside = np.nextafter(on, xyz[i, axis])
    outside = np.nextafter(on, on + sign)
    pos[i, axis] = np.where(kind == 0, on, np.where(kind == 1, inside, outside))
    return dict(model=_two_point_model(refs()[1][5]), cloud=cloud, particles=_identity_particles(pos), max_distance=0.125,
                kind=kind)


def own_paired(O, n=256):
    """particles whose model point A is paired with the cloud point of the same index (nn_idx counts in the cropped cloud)"""
    idx = O["nn_idx"][:, 0]
    crop = np.asarray(O["crop_idx"])
    ok = (idx >= 0) & (idx < len(crop))
    own = np.zeros(len(idx), bool)
    own[ok] = crop[idx[ok]] == np.flatnonzero(ok)
    return own

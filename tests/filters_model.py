"""Plain model of the three input filters (include/pft_filters.h), written from the descriptions of the PCL 1.8.0
algorithms (passthrough.hpp, approximate_voxel_grid.hpp, voxel_grid.hpp) and not from oracle/pft_oracle_filters.c: a
second, independent statement that tests/test_filter_cases_host.py holds against the C oracle bit for bit.  numpy and
Python only; every arithmetic step on coordinates and sums is an np.float32 operation, integer steps use Python ints
(unbounded) and are reduced to 32 bits where PCL's `int` would wrap.  Sums are literal loops, one float add per point
and component, colour channels included.  Test infrastructure, no GPU."""
import numpy as np

from pcl_tracking_amd import scene

F = np.float32
INT_MIN = -(1 << 31)
INT32_MAX = (1 << 31) - 1


def floor_to_int(v):
    """static_cast<int>(floor(v)) as an x86-64 build evaluates it: the conversion instruction answers INT_MIN for NaN
    and for every value outside [-2^31, 2^31)"""
    f = np.floor(F(v))
    if f != f or f < F(-2147483648.0) or f >= F(2147483648.0):
        return INT_MIN
    return int(f)


def _leaf3(leaf):
    lf = [leaf] * 3 if np.isscalar(leaf) else list(leaf)
    return [F(v) for v in lf]


def _cells(cloud, inv):
    """floor_to_int(coord * inverse leaf) of every point, three Python-int lists"""
    out = []
    with np.errstate(all="ignore"):
        for k, a in enumerate(("x", "y", "z")):
            prod = cloud[a] * inv[k]
            assert prod.dtype == F
            out.append([floor_to_int(v) for v in prod])
    return out


def _channels(rgba):
    """alpha, red, green, blue of the packed colour as float32 columns"""
    rgba = rgba.astype(np.uint32)
    return [((rgba >> s) & np.uint32(255)).astype(F) for s in (24, 16, 8, 0)]


def pass_through(cloud, field="z", lo=0.0, hi=10.0, negative=False):
    """pcl::PassThrough with a field name, keep_organized = false: a point with a non-finite x, y or z is removed
    whatever the limits; of the rest, the points whose field lies in [lo, hi] (both ends included) are kept, or, with
    `negative`, exactly the others.  Order kept.  -> int32 indices"""
    lo, hi = F(lo), F(hi)
    keep = []
    for i in range(len(cloud)):
        x, y, z = cloud["x"][i], cloud["y"][i], cloud["z"][i]
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
            continue
        v = cloud[field][i]
        inside = bool(lo <= v <= hi)
        if inside != bool(negative):
            keep.append(i)
    return np.asarray(keep, np.int32)


def approx_voxel_grid(cloud, leaf=0.01, hist_size=512):
    """pcl::ApproximateVoxelGrid<PointXYZRGBA>, downsample_all_data: one open voxel per entry of a history table
    addressed by (ix 7171 + iy 3079 + iz 4231) mod hist_size.  A point of another voxel that lands on an occupied entry
    first sends that entry's centroid to the output; what is still open at the end leaves in entry order.  The centroid
    is the 7-vector [x, y, z, (float) rgba, r, g, b] summed in float in arrival order and divided by (float) count; the
    colour is the truncated r, g, b packed with alpha 0, data[3] is 1."""
    assert hist_size > 0 and hist_size & (hist_size - 1) == 0
    inv = [F(1) / v for v in _leaf3(leaf)]
    ix, iy, iz = _cells(cloud, inv)
    a, r, g, b = _channels(cloud["rgba"])
    vec = np.stack([cloud["x"], cloud["y"], cloud["z"], cloud["rgba"].astype(F), r, g, b], 1)
    assert vec.dtype == F
    table = {}  # entry -> [voxel, count, sums]
    out = []

    def flush(voxel, count, sums):
        with np.errstate(all="ignore"):
            c = sums / F(count)
        out.append((c[0], c[1], c[2], int(c[4]) << 16 | int(c[5]) << 8 | int(c[6])))

    with np.errstate(all="ignore"):
        for i in range(len(cloud)):
            voxel = (ix[i], iy[i], iz[i])
            entry = (ix[i] * 7171 + iy[i] * 3079 + iz[i] * 4231) & (hist_size - 1)
            slot = table.get(entry)
            if slot is not None and slot[0] != voxel:
                flush(*slot)
                slot = None
            if slot is None:
                slot = table[entry] = [voxel, 0, np.zeros(7, F)]
            slot[1] += 1
            slot[2] += vec[i]
    for entry in sorted(table):
        flush(*table[entry])
    return _cloud_of(out)


def voxel_grid(cloud, leaf=0.01):
    """pcl::VoxelGrid<PointXYZRGBA>, no filter field, downsample_all_data, no minimum count: bounds over the finite
    points; min_b = floor(min * inv), div_b = max_b - min_b + 1; when the product of the three truncated extents
    (max - min) * inv, each plus one, exceeds INT32_MAX PCL gives up (-> None: the caller hands the input through);
    idx = ijk0 + ijk1 div0 + ijk2 div0 div1 with ijk = (int)(floor(coord * inv) - (float) min_b), the subtraction in
    float; points ordered by idx, ties in input order; per voxel the float sums of x, y, z, a, r, g, b in that order,
    each divided by (float) n, the four colour averages truncated and packed."""
    inv = [F(1) / v for v in _leaf3(leaf)]
    xyz = [cloud[k] for k in ("x", "y", "z")]
    fin = np.flatnonzero(np.isfinite(xyz[0]) & np.isfinite(xyz[1]) & np.isfinite(xyz[2]))
    if len(fin) == 0:
        return _cloud_of([])
    mn = [c[fin].min() for c in xyz]
    mx = [c[fin].max() for c in xyz]
    extent = 1
    for k in range(3):
        d = (mx[k] - mn[k]) * inv[k]
        assert d.dtype == F
        extent *= int(d) + 1  # (int64_t) truncates; Python ints do not overflow
    if extent > INT32_MAX:
        return None
    min_b = [floor_to_int(mn[k] * inv[k]) for k in range(3)]
    div_b = [floor_to_int(mx[k] * inv[k]) - min_b[k] + 1 for k in range(3)]
    mul = [1, div_b[0], div_b[0] * div_b[1]]
    idx = np.zeros(len(fin), np.int64)
    for k in range(3):
        rel = np.floor(xyz[k][fin] * inv[k]) - F(min_b[k])
        assert rel.dtype == F
        idx += rel.astype(np.int64) * mul[k]
    idx &= 0xFFFFFFFF  # static_cast<unsigned int>(idx)
    order = np.argsort(idx, kind="stable")
    a, r, g, b = _channels(cloud["rgba"])
    vec = np.stack([xyz[0], xyz[1], xyz[2], a, r, g, b], 1)
    assert vec.dtype == F
    out = []
    j = 0
    while j < len(order):
        e = j
        sums = np.zeros(7, F)
        while e < len(order) and idx[order[e]] == idx[order[j]]:
            sums += vec[fin[order[e]]]
            e += 1
        c = sums / F(e - j)
        out.append((c[0], c[1], c[2], int(c[3]) << 24 | int(c[4]) << 16 | int(c[5]) << 8 | int(c[6])))
        j = e
    return _cloud_of(out)


def _cloud_of(rows):
    c = np.zeros(len(rows), scene.POINT_DTYPE)
    for i, (x, y, z, rgba) in enumerate(rows):
        c["x"][i], c["y"][i], c["z"][i], c["rgba"][i] = x, y, z, rgba
    c["w"] = 1.0
    return c

"""CPU checks of the object report (pft_report): the NumPy restatement (tests/report_model.py)
against float64 linear algebra, on synthetic boxes with known answers and through the degenerate branches; the ABI
struct, the new symbols and the C++ driver's --device-report flag.  The device is compared with the model bit for bit in
tests/test_gpu_report.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import report_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pft_set_report_cloud", "pft_report", "pft_get_report", "pft_get_tracked_cloud")
FIELD_SIZES = [("transform", 16), ("centroid", 4), ("covariance", 9), ("eigenvalues", 3), ("axes", 9), ("box_min", 3),
               ("box_max", 3), ("box_centre", 3), ("box_quat", 4), ("box_size", 3), ("n_points", 1), ("info", 1)]


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def quat_to_matrix(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ---- the model against float64 linear algebra -----------------------------------------------------------------------
@pytest.mark.parametrize("order", [rm.SUM_TREE, rm.SUM_PCL])
@pytest.mark.parametrize("seed", range(6))
def test_model_against_eigh(order, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(50, 3000))
    A = rng.normal(size=(3, 3)) * rng.uniform(0.02, 0.3, 3)
    xyz = (rng.normal(size=(n, 3)) @ A + rng.uniform(-1, 1, 3)).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = rotation(rng)
    T[:3, 3] = rng.uniform(-0.5, 0.5, 3)
    out, moved = rm.report(xyz, T, order)
    assert out["info"] == 0
    m64 = moved.astype(np.float64)
    np.testing.assert_allclose(out["centroid"][:3], m64.mean(axis=0), atol=1e-6)
    cov = np.cov(m64.T, bias=True)
    np.testing.assert_allclose(out["covariance"].reshape(3, 3), cov, rtol=1e-4, atol=1e-7 * np.abs(cov).max())
    w, v = np.linalg.eigh(out["covariance"].reshape(3, 3).astype(np.float64))
    np.testing.assert_allclose(out["eigenvalues"], w, rtol=1e-5, atol=1e-5 * w.max())
    axes = out["axes"].reshape(3, 3).astype(np.float64)
    for k in range(2):  # columns 0 and 1 are eigenvectors (up to sign); column 2 is their cross product
        assert min(np.abs(axes[:, k] - v[:, k]).max(), np.abs(axes[:, k] + v[:, k]).max()) < 1e-4
    assert abs(np.linalg.det(axes) - 1.0) < 1e-5
    np.testing.assert_allclose(axes.T @ axes, np.eye(3), atol=1e-5)
    assert np.all(np.diff(out["eigenvalues"]) >= 0)
    # the box holds every point in the principal frame; the quaternion is the axes' rotation
    u = (m64 - out["centroid"][:3]) @ axes
    assert np.all(u >= out["box_min"] - 1e-5) and np.all(u <= out["box_max"] + 1e-5)
    np.testing.assert_allclose(quat_to_matrix(out["box_quat"]), axes, atol=1e-5)
    np.testing.assert_allclose(np.linalg.norm(out["box_quat"].astype(np.float64)), 1.0, atol=1e-6)


@pytest.mark.parametrize("order", [rm.SUM_TREE, rm.SUM_PCL])
@pytest.mark.parametrize("seed", range(4))
def test_rotated_cuboid(order, seed):
    """a lattice filling a cuboid of distinct sides: the box recovers the sides and the cuboid's centre"""
    rng = np.random.default_rng(100 + seed)
    sides = np.sort(rng.uniform(0.05, 0.4, 3))[::-1] * np.array([1.0, 0.8, 0.6])
    g = [np.linspace(-s / 2, s / 2, k) for s, k in zip(sides, (13, 11, 9))]
    local = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3)
    R = rotation(rng)
    centre = rng.uniform(-0.5, 0.5, 3)
    xyz = (local @ R.T + centre).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    out, _ = rm.report(xyz, T, order)
    assert out["info"] == 0
    np.testing.assert_allclose(np.sort(out["box_size"]), np.sort(sides), atol=1e-5)
    np.testing.assert_allclose(out["box_centre"], centre, atol=1e-6)
    # the largest eigenvalue's axis is the longest side
    axes = out["axes"].reshape(3, 3)
    assert abs(abs(float(axes[:, 2] @ R[:, 0])) - 1.0) < 1e-5


# ---- degenerate clouds: the documented branches, no NaN -------------------------------------------------------------
def degenerate_clouds():
    rng = np.random.default_rng(7)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    plane = rng.normal(size=(200, 2)) @ rng.normal(size=(2, 3))
    return {
        "one": np.array([[0.1, -0.2, 0.7]]),
        "two": np.array([[0.1, -0.2, 0.7], [0.3, 0.1, 0.65]]),
        "three": np.array([[0.1, -0.2, 0.7], [0.3, 0.1, 0.65], [-0.05, 0.02, 0.8]]),
        "identical": np.tile([[0.25, 0.5, 1.0]], (100, 1)),
        "collinear": np.outer(np.linspace(-0.2, 0.3, 150), d) + [0.1, 0.0, 0.9],
        "coplanar": plane * 0.1 + [0.0, 0.1, 0.8],
        "diagonal": np.concatenate([np.diag([0.3, 0.2, 0.1]), -np.diag([0.3, 0.2, 0.1])]) + [0.0, 0.0, 1.0],
        "axis_aligned": np.stack(np.meshgrid(np.linspace(-0.1, 0.1, 5), np.linspace(-0.2, 0.2, 7), [0.0, 0.05],
                                             indexing="ij"), -1).reshape(-1, 3),
    }


@pytest.mark.parametrize("order", [rm.SUM_TREE, rm.SUM_PCL])
@pytest.mark.parametrize("name", sorted(degenerate_clouds()))
def test_degenerate_clouds(order, name):
    xyz = degenerate_clouds()[name].astype(np.float32)
    out, _ = rm.report(xyz, np.eye(4, dtype=np.float32), order)
    assert out["info"] == 0
    for k in rm_fields():
        assert np.all(np.isfinite(out[k])), k
    axes = out["axes"].reshape(3, 3).astype(np.float64)
    assert abs(np.linalg.det(axes) - 1.0) < 1e-5
    assert np.all(out["box_size"] >= 0)


def rm_fields():
    return [f for f, _ in FIELD_SIZES if f not in ("n_points", "info")]


def test_diagonal_covariance_takes_the_v1norm2_branch():
    """an already diagonal covariance: the tridiagonalisation keeps Q = I (v1norm2 <= FLT_MIN) and the axes are the
    coordinate axes, sorted by eigenvalue"""
    cov = [[np.float32(0.04), np.float32(0), np.float32(0)], [np.float32(0), np.float32(0.01), np.float32(0)],
           [np.float32(0), np.float32(0), np.float32(0.09)]]
    evals, Q, info = rm.solve(cov, [np.float32(0)] * 3)
    assert info == 0
    assert [float(e) for e in evals] == [float(np.float32(0.01)), float(np.float32(0.04)), float(np.float32(0.09))]
    np.testing.assert_array_equal(np.abs(np.array(Q, np.float32)), [[0, 1, 0], [1, 0, 0], [0, 0, 1]])


def test_tree_sum_does_not_depend_on_padding():
    rng = np.random.default_rng(3)
    v = rng.normal(size=1000).astype(np.float32)
    assert rm.tree_sum(v) == rm.tree_sum(np.concatenate([v, np.full(24, -0.0, np.float32)]))
    assert np.signbit(rm.tree_sum(np.array([-0.0], np.float32)))
    assert rm.chain_sum(v) == np.float32(sum_seq(v))


def sum_seq(v):
    s = np.float32(0)
    for x in v:
        s = np.float32(s + x)
    return s


def test_min_max_ties_take_the_later_point():
    v = np.array([0.0, -0.0, 1.0, -0.0, 0.5], np.float32)
    assert np.signbit(rm.min_last(v))  # the last of the three zeros
    w = np.array([2.0, -0.0, 0.0], np.float32)
    assert rm.max_last(w) == 2.0 and not np.signbit(rm.min_last(w))


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_report_struct_layout(tmp_path):
    """pft_object_report: 240 bytes, fields in order without gaps, the same in C (compiled here) and in ctypes"""
    from pcl_tracking_amd import _lib

    off, want = 0, {}
    for name, n in FIELD_SIZES:
        want[name] = off
        off += 4 * n
    assert off == 236
    assert C.sizeof(_lib.ObjectReport) == 240
    for name, _ in FIELD_SIZES:
        assert getattr(_lib.ObjectReport, name).offset == want[name], name
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"pft.h\"\nint main(void) {\n"
                   "  printf(\"size %zu\\n\", sizeof(pft_object_report));\n" +
                   "".join("  printf(\"%s %%zu\\n\", offsetof(pft_object_report, %s));\n" % (f, f) for f, _ in FIELD_SIZES) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == 240 and int(got["size"]) % 16 == 0
    for name, _ in FIELD_SIZES:
        assert int(got[name]) == want[name], name


def test_report_symbols_are_declared_exported_and_bound():
    from pcl_tracking_amd import _lib

    header = open(os.path.join(ROOT, "include", "pft.h")).read()
    L = _lib.load()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(L, name), name
        assert name in bound and bound[name][0] is C.c_int, name


def test_python_and_cpp_mirrors_have_the_report_calls():
    from pcl_tracking_amd import tracker

    for m in ("setReportCloud", "computeReport", "getReport", "getTrackedCloud"):
        assert callable(getattr(tracker.ParticleFilterTracker, m))
    hpp = open(os.path.join(ROOT, "pcl_tracking_amd", "include", "pft", "particle_filter_tracker.hpp")).read()
    for m in ("setReportCloud", "computeReport", "getReport", "getTrackedCloud"):
        assert re.search(r"\b%s\(" % m, hpp), m


def test_cpp_driver_compiles_with_the_device_report_flag():
    from pcl_tracking_amd import build

    exe = build.build_example()
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--device-report" in r.stderr
    src = open(os.path.join(ROOT, "pcl_tracking_amd", "examples", "auto_tracking_amd.cpp")).read()
    assert "computeReport()" in src and "getReport()" in src

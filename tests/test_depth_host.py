"""Host-side checks of the depth entrance (no GPU): the NumPy model of the specification against answers derived by
hand, the inverse camera against the visibility camera's forward projection, scene.make_depth_images against the rays it
was rounded from, the Python argument checks that raise before the library is loaded, and pft/pnm_io.hpp under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import depth_cases as dc
import depth_model as dm
from pcl_tracking_amd import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
QNAN = 0x7FC00000


# ---- the model -------------------------------------------------------------------------------------------------------
def test_known_answers_u16():
    """4 x 2 pixels, fx = 2, fy = 4, cx = 1, cy = 0.5, divisor 1000: every number below is exact in float32
    pixel (c, r): lx = (c - 1) / 2, ly = (r - 0.5) / 4"""
    depth = np.array([[2000, 0, 4000, 500], [1000, 8000, 0, 250]], np.uint16)
    bgr = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)  # pixel i: b = 3 i, g = 3 i + 1, r = 3 i + 2
    out = dm.deproject(depth, bgr, camera=(2.0, 4.0, 1.0, 0.5), depth_divisor=1000.0, color_format="bgr8")
    want_xyz = {0: (-1.0, -0.25, 2.0), 2: (2.0, -0.5, 4.0), 3: (0.5, -0.0625, 0.5),
                4: (-0.5, 0.125, 1.0), 5: (0.0, 1.0, 8.0), 7: (0.25, 0.03125, 0.25)}
    for i in range(8):
        p = out[i]
        assert p["w"] == 1.0
        if i in want_xyz:
            assert (float(p["x"]), float(p["y"]), float(p["z"])) == want_xyz[i], i
            assert int(p["rgba"]) == 0xFF000000 | (3 * i + 2) << 16 | (3 * i + 1) << 8 | 3 * i
        else:  # depth 0
            assert [int(p[k].view(np.uint32)) for k in ("x", "y", "z")] == [QNAN] * 3 and int(p["rgba"]) == 0
    raw = out.view(np.uint8).reshape(8, 32)
    assert not raw[:, 20:].any()  # the 12 padding bytes


def test_known_answers_formats():
    px = np.array([[[10, 20, 30, 40]]], np.uint8)
    d = np.array([[1000]], np.uint16)
    cam = (1.0, 1.0, 0.0, 0.0)
    assert int(dm.deproject(d, px[:, :, :3], cam, color_format="bgr8")["rgba"][0]) == 0xFF1E140A
    assert int(dm.deproject(d, px[:, :, :3], cam, color_format="rgb8")["rgba"][0]) == 0xFF0A141E
    assert int(dm.deproject(d, px, cam, color_format="bgra8")["rgba"][0]) == 0xFF1E140A  # the alpha byte 40 is ignored
    assert int(dm.deproject(d, px, cam, color_format="rgba8")["rgba"][0]) == 0xFF0A141E
    assert int(dm.deproject(d, None, cam)["rgba"][0]) == 0xFF000000


def test_known_answers_f32():
    c = dc.CASES["f32_edges"]
    out = dm.deproject(**dc.kwargs(c))
    valid = np.isfinite(out["z"])
    #        nan    inf    -inf   0      -0     -1     denormal 1e-3  1e4   1.5   0.75  2
    assert valid.tolist() == [False, False, False, False, False, False, True, True, True, True, True, True]
    assert (out["z"][valid] == c["depth"].ravel()[valid]).all()  # metres go through untouched
    assert (out["rgba"][~valid] == 0).all() and (out["rgba"][valid] >> 24 == 0xFF).all()


def test_division_is_not_a_multiply():
    """z = (float)d / 1000 is the correctly rounded quotient: it equals the float64 quotient rounded once, and differs from
    d * 0.001f on 38 850 of the 65 535 depths"""
    d = np.arange(1, 65536, dtype=np.uint32).reshape(1, -1).astype(np.uint16)
    z = dm.deproject(d, None)["z"]
    assert (z == (d.ravel().astype(np.float64) / 1000.0).astype(np.float32)).all()
    assert np.count_nonzero(z != d.ravel().astype(np.float32) * F32(0.001)) == 38850 == len(dc.division_differs())


def test_every_pixel_projects_back_to_itself():
    """the inverse camera against the forward one of include/pft_visibility.h:11-12, same intrinsics, literal float32:
    xn = x / z, yn = y / z, uf = fx xn + cx, vf = fy yn + cy round to the pixel the point came from, for every pixel of a
    960 x 540 frame at 1, 500, 4500 and 65535 mm"""
    fx, fy, cx, cy = (F32(v) for v in dc.QHD)
    c, r = np.meshgrid(np.arange(960), np.arange(540), indexing="xy")
    worst = 0.0
    for mm in (1, 500, 4500, 65535):
        out = dm.deproject(np.full((540, 960), mm, np.uint16), None, dc.QHD)
        x, y, z = out["x"], out["y"], out["z"]
        assert np.isfinite(z).all()
        uf = fx * (x / z) + cx
        vf = fy * (y / z) + cy
        assert uf.dtype == np.float32
        assert (np.rint(uf).astype(np.int64) == c.ravel()).all() and (np.rint(vf).astype(np.int64) == r.ravel()).all()
        worst = max(worst, float(np.abs(uf.astype(np.float64) - c.ravel()).max()), float(np.abs(vf.astype(np.float64) - r.ravel()).max()))
    print("largest deviation %.3g pixels" % worst)
    assert worst <= 4 * 2.0 ** -14  # four units in the last place of a float32 column index above 512; measured 6.1e-05 = one


# ---- the defaults ---------------------------------------------------------------------------------------------------
def test_defaults_are_six_times_the_visibility_camera():
    from pcl_tracking_amd import _lib

    L = _lib.load()
    d, v = _lib.DepthFrame(), _lib.VisibilityConfig()
    L.pft_depth_frame_default(C.byref(d))
    L.pft_visibility_config_default(C.byref(v))
    assert (d.width, d.height, d.fx, d.fy) == (6 * v.width, 6 * v.height, 6 * v.fx, 6 * v.fy)
    # pixel centres: (c + 0.5) scales, so cx = 6 (v.cx + 0.5) - 0.5
    assert (d.cx, d.cy) == (6 * (v.cx + 0.5) - 0.5, 6 * (v.cy + 0.5) - 0.5) == (479.5, 269.5)
    assert (d.depth_format, d.depth_divisor, d.color_format) == (_lib.DEPTH_U16, 1000.0, _lib.COLOR_BGR8)
    assert (d.depth_stride, d.color_stride, d.abi_version) == (0, 0, _lib.PFT_ABI_VERSION)


# ---- the scene generator ---------------------------------------------------------------------------------------------
def test_make_depth_images():
    W, H = 240, 135
    depth, bgr, camera, pts = scene.make_depth_images(W, H, return_points=True)
    assert depth.shape == (H, W) and depth.dtype == np.uint16 and bgr.shape == (H, W, 3) and bgr.dtype == np.uint8
    assert camera == (0.82 * W, 0.82 * W, (W - 1) / 2, (H - 1) / 2)
    again = scene.make_depth_images(W, H)
    assert again[0].tobytes() == depth.tobytes() and again[1].tobytes() == bgr.tobytes() and again[2] == camera
    valid = depth.ravel() != 0
    assert 0.03 < 1 - valid.mean() < 0.5  # the dropout and the rays that hit nothing
    assert (np.isnan(pts[:, 2]) == ~valid).all()
    assert depth.max() > 10000  # the far strip beyond PassThrough's 10 m is kept
    cloud = dm.deproject(depth, bgr, camera)
    assert (np.isnan(cloud["z"]) == ~valid).all() and (cloud["rgba"][~valid] == 0).all()
    # within the quantisation: z was rounded to the nearest millimetre, so the point moved along its ray by at most
    # 0.5 mm in z (float32 rounding on top: 1 / fx, the ray and the product are rounded once each,
    # 3 x 6e-8 of at most 12 m is below 3 um)
    lx = (np.arange(W) - camera[2]) / camera[0]
    ly = (np.arange(H) - camera[3]) / camera[1]
    LX, LY = [a.ravel()[valid] for a in np.meshgrid(lx, ly, indexing="xy")]
    dz = cloud["z"][valid].astype(np.float64) - pts[valid, 2]
    assert np.abs(dz).max() <= 0.0005 + 2e-6
    assert np.abs(cloud["x"][valid] - pts[valid, 0]).max() <= 0.0005 * np.abs(LX).max() + 5e-6
    assert np.abs(cloud["y"][valid] - pts[valid, 1]).max() <= 0.0005 * np.abs(LY).max() + 5e-6
    # the same frame as make_depth_frame: the same pixels are valid, the points agree within the quantisation
    frame = scene.make_depth_frame(W, H)
    assert (np.isfinite(frame["z"]) == valid).all()
    assert np.abs(frame["z"][valid] - cloud["z"][valid]).max() <= 0.0005 + 2e-6
    # colours: make_depth_frame's, as B, G, R bytes
    assert (frame["rgba"][valid] == cloud["rgba"][valid]).all()


# ---- the Python argument checks ---------------------------------------------------------------------------------------
def test_argument_checks_raise_before_the_library_is_loaded():
    code = r"""
import numpy as np, sys
from pcl_tracking_amd import filters, _lib
_lib.load = lambda: (_ for _ in ()).throw(AssertionError("the library was touched"))
f = filters.InputFilter.__new__(filters.InputFilter)
f._cloud = f._dev = f._depth = None
d = np.ones((4, 6), np.uint16); c = np.zeros((4, 6, 3), np.uint8)
bad = [
    dict(depth=d.astype(np.int16)), dict(depth=d.astype(np.float64)), dict(depth=d[0]), dict(depth=d[None]),
    dict(depth=[[1, 2]]), dict(depth=np.zeros((0, 4), np.uint16)), dict(depth=d[:, ::2]), dict(depth=d[::-1]),
    dict(depth=d.astype(">u2")), dict(depth=np.broadcast_to(d[0], (4, 6))),
    dict(depth=d, color=c[:, :5]), dict(depth=d, color=c.astype(np.uint16)), dict(depth=d, color=c[:, :, 0]),
    dict(depth=d, color=c, color_format="bgra8"), dict(depth=d, color=c, color_format="yuv"),
    dict(depth=d, color=c, color_format="none"),
    dict(depth=d, color=np.zeros((4, 6, 4), np.uint8)[:, :, :3]), dict(depth=d, color=np.zeros((4, 12, 3), np.uint8)[:, ::2]),
    dict(depth=d, camera=(540.0, 540.0, 1.0)), dict(depth=d, camera=(0.0, 540.0, 1.0, 1.0)),
    dict(depth=d, camera=(540.0, -1.0, 1.0, 1.0)), dict(depth=d, camera=(540.0, 540.0, float("nan"), 1.0)),
    dict(depth=d, camera=(540.0, 540.0, 1.0, float("inf"))), dict(depth=d, camera=None),
    dict(depth=d, depth_divisor=0.0), dict(depth=d, depth_divisor=-1.0), dict(depth=d, depth_divisor=float("nan")),
]
for k in bad:
    try:
        f.setInputDepth(**k)
    except ValueError:
        continue
    sys.exit("no ValueError for %r" % (sorted(k),))
# what is allowed: padded rows with packed pixels, either dtype, four channels, no colour
big = np.zeros((4, 10), np.uint16)
f.setInputDepth(big[:, :6], np.zeros((4, 8, 3), np.uint8)[:, :6])
assert (f._depth[0].depth_stride, f._depth[0].color_stride) == (20, 24)
f.setInputDepth(d.astype(np.float32), np.zeros((4, 6, 4), np.uint8), color_format="rgba8")
assert (f._depth[0].depth_format, f._depth[0].color_format, f._depth[0].depth_stride) == (_lib.DEPTH_F32, _lib.COLOR_RGBA8, 0)
f.setInputDepth(d)
assert f._depth[0].color_format == _lib.COLOR_NONE and (f._depth[0].width, f._depth[0].height) == (6, 4)
f.setInputDepth(d[:1, :1][::1])
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- pnm_io.hpp --------------------------------------------------------------------------------------------------------
def test_pnm_io_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed"
    exe = str(tmp_path / "pnm_io_tool")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pcl_tracking_amd", "include"),
           os.path.join(ROOT, "tests", "cpp", "pnm_io_tool.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-3000:]


def test_pnm_files_written_by_python_are_what_the_header_reads(tmp_path):
    """the test suite's own writer (depth_cases.write_pgm / write_ppm) produces the two formats byte for byte"""
    d = np.array([[0, 1, 0x1234]], np.uint16)
    dc.write_pgm(str(tmp_path / "a.pgm"), d)
    assert open(tmp_path / "a.pgm", "rb").read() == b"P5\n3 1\n65535\n" + bytes([0, 0, 0, 1, 0x12, 0x34])
    bgr = np.array([[[1, 2, 3], [4, 5, 6]]], np.uint8)
    dc.write_ppm(str(tmp_path / "a.ppm"), bgr)
    assert open(tmp_path / "a.ppm", "rb").read() == b"P6\n2 1\n255\n" + bytes([3, 2, 1, 6, 5, 4])  # R, G, B

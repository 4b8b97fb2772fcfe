"""NumPy restatement of the depth entrance's specification (include/pft_filters.h), literal
float32: every operation is one NumPy float32 operation, so every result is rounded once and nothing is fused.

    cloud = deproject(depth, color, camera=(fx, fy, cx, cy), depth_divisor=1000.0, color_format="bgr8")

depth: 2-D uint16 (divided by depth_divisor) or float32 (metres); color: H x W x 3|4 uint8 or None.  The arrays are read
through NumPy indexing, so row padding can never reach a result.  Returns W H records of POINT_DTYPE, record r W + c for
pixel (c, r)."""
import numpy as np

from pcl_tracking_amd.scene import POINT_DTYPE

QNAN = np.uint32(0x7FC00000)
CHANNELS = {"bgr8": (2, 1, 0), "rgb8": (0, 1, 2), "bgra8": (2, 1, 0), "rgba8": (0, 1, 2)}  # where r, g, b lie in a pixel


def deproject(depth, color=None, camera=(540.0, 540.0, 479.5, 269.5), depth_divisor=1000.0, color_format="bgr8"):
    f32 = np.float32
    H, W = depth.shape
    fx, fy, cx, cy = (f32(v) for v in camera)
    ifx, ify = f32(1.0) / fx, f32(1.0) / fy
    c = np.arange(W, dtype=np.float32)[None, :].repeat(H, 0)
    r = np.arange(H, dtype=np.float32)[:, None].repeat(W, 1)
    lx = (c - cx) * ifx
    ly = (r - cy) * ify
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if depth.dtype == np.uint16:
            valid = depth != 0
            z = depth.astype(np.float32) / f32(depth_divisor)
        else:
            assert depth.dtype == np.float32
            valid = np.isfinite(depth) & (depth > 0)
            z = depth.copy()
        x = lx * z
        y = ly * z
    assert x.dtype == np.float32 and y.dtype == np.float32 and z.dtype == np.float32
    out = np.zeros(H * W, POINT_DTYPE)
    v = valid.ravel()
    for name, a in (("x", x), ("y", y), ("z", z)):
        bits = a.ravel().view(np.uint32).copy()
        bits[~v] = QNAN
        out[name] = bits.view(np.float32)
    out["w"] = 1.0
    rgba = np.full(H * W, 0xFF000000, np.uint32)
    if color is not None:
        ir, ig, ib = CHANNELS[color_format]
        assert color.shape == (H, W, 3 if color_format in ("bgr8", "rgb8") else 4) and color.dtype == np.uint8
        px = color.reshape(H * W, -1).astype(np.uint32)
        rgba |= px[:, ir] << 16 | px[:, ig] << 8 | px[:, ib]
    out["rgba"] = np.where(v, rgba, np.uint32(0))
    return out

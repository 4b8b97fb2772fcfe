"""Python mirror of the PCL filter classes the reference runs in front of the tracker (same member names
as the calls at /root/reference/src/auto_tracking.cpp:536-575), over the C ABI of include/pft_filters.h.
All compute runs in the HIP library; nothing here computes on the CPU.

    pass_ = PassThrough(); pass_.setFilterFieldName("z"); pass_.setFilterLimits(0, 10)
    pass_.setInputCloud(cloud); kept = pass_.filter()
    grid = ApproximateVoxelGrid(); grid.setLeafSize(0.01, 0.01, 0.01); grid.setInputCloud(kept); out = grid.filter()

InputFilter fuses PassThrough + voxel grid into one device pipeline whose output stays in HBM
(`filterDevice` -> (device pointer, n), ready for ParticleFilterTracker.setInputCloudDevice)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import VOXEL_APPROX, VOXEL_EXACT, VOXEL_NONE, FilterConfig, PftError
from .scene import POINT_DTYPE

QHD_CAMERA = (540.0, 540.0, 479.5, 269.5)  # fx, fy, cx, cy of pft_depth_frame_default (Kinect2 qhd, 960 x 540)
COLOR_FORMATS = {"none": (_lib.COLOR_NONE, 0), "bgr8": (_lib.COLOR_BGR8, 3), "rgb8": (_lib.COLOR_RGB8, 3),
                 "bgra8": (_lib.COLOR_BGRA8, 4), "rgba8": (_lib.COLOR_RGBA8, 4)}


def _row_stride(a, row_bytes, what):
    """row stride in bytes of an image whose pixels are packed inside a row (0 = packed); ValueError otherwise"""
    if a.shape[0] == 1 or a.strides[0] == row_bytes:
        return 0
    if a.strides[0] < row_bytes or a.strides[0] > 0xFFFFFFFF:
        raise ValueError("%s: rows overlap, run backwards or lie too far apart (row stride %d bytes)" % (what, a.strides[0]))
    return int(a.strides[0])


def depth_description(depth, color=None, camera=QHD_CAMERA, depth_divisor=1000.0, color_format="bgr8"):
    """pft_depth_frame for a 2-D uint16 / float32 depth image and an optional H x W x 3|4 uint8 colour image, strides
    taken from the arrays.  Pure Python: every complaint is a ValueError raised before the library is touched."""
    if not isinstance(depth, np.ndarray) or depth.ndim != 2 or depth.dtype not in (np.uint16, np.float32):
        raise ValueError("depth: a 2-D uint16 or float32 array is needed")
    H, W = depth.shape
    if H < 1 or W < 1 or H > _lib.DEPTH_MAX_AXIS or W > _lib.DEPTH_MAX_AXIS:
        raise ValueError("depth: width and height must be 1 .. %d" % _lib.DEPTH_MAX_AXIS)
    if not depth.dtype.isnative:
        raise ValueError("depth: samples must be in host byte order")
    if W > 1 and depth.strides[1] != depth.itemsize:
        raise ValueError("depth: the pixels of a row must be packed (pixel step %d bytes)" % depth.strides[1])
    d = _lib.DepthFrame()
    d.abi_version = _lib.PFT_ABI_VERSION
    d.width, d.height = W, H
    d.depth_format = _lib.DEPTH_U16 if depth.dtype == np.uint16 else _lib.DEPTH_F32
    d.depth_stride = _row_stride(depth, W * depth.itemsize, "depth")
    try:
        cam = [float(v) for v in camera]
    except (TypeError, ValueError):
        raise ValueError("camera: (fx, fy, cx, cy) is needed")
    if len(cam) != 4 or not all(np.isfinite(cam)) or cam[0] <= 0 or cam[1] <= 0:
        raise ValueError("camera: (fx, fy, cx, cy), all finite, fx and fy > 0")
    d.fx, d.fy, d.cx, d.cy = cam
    depth_divisor = float(depth_divisor)
    if not (np.isfinite(depth_divisor) and depth_divisor > 0):
        raise ValueError("depth_divisor: finite and > 0")
    d.depth_divisor = depth_divisor
    if color is None:
        d.color_format = _lib.COLOR_NONE
        return d
    if color_format not in COLOR_FORMATS or color_format == "none":
        raise ValueError("color_format: one of bgr8, rgb8, bgra8, rgba8 (or color=None)")
    fmt, ch = COLOR_FORMATS[color_format]
    if not isinstance(color, np.ndarray) or color.dtype != np.uint8 or color.ndim != 3 or color.shape != (H, W, ch):
        raise ValueError("color: a %d x %d x %d uint8 array is needed for %s" % (H, W, ch, color_format))
    if color.strides[2] != 1 or (W > 1 and color.strides[1] != ch):
        raise ValueError("color: the pixels of a row must be packed")
    d.color_format = fmt
    d.color_stride = _row_stride(color, W * ch, "color")
    return d


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class InputFilter:
    """PassThrough and / or a voxel grid as one device pipeline (one handle of include/pft_filters.h)."""

    def __init__(self, device_id=0, stream=None):
        self._L = _lib.load()
        self._cfg = FilterConfig()
        self._L.pft_filter_default_config(C.byref(self._cfg))
        self._cfg.device_id = device_id
        if stream is not None:
            self._cfg.stream = stream
            self._cfg.stream_is_external = 1
        self._h = None
        self._cloud = None
        self._dev = None
        self._depth = None

    # -- configuration (handle is created lazily, re-created when the configuration changes) --
    def _set(self, **kw):
        for k, v in kw.items():
            setattr(self._cfg, k, v)
        self.close()

    def setPassThrough(self, field="z", lo=0.0, hi=10.0, negative=False, enable=True):
        self._set(pass_enable=int(enable), pass_field="xyz".index(field), pass_min=lo, pass_max=hi,
                  pass_negative=int(negative))

    def setVoxelMode(self, mode):
        self._set(voxel_mode=mode)

    def setLeafSize(self, lx, ly=None, lz=None):
        ly = lx if ly is None else ly
        lz = lx if lz is None else lz
        self._set(leaf_size=(C.c_float * 3)(lx, ly, lz))

    def setHistorySize(self, n):
        self._set(approx_hist_size=int(n))

    def _check(self, status):
        if status != 0:
            detail = self._L.pft_filter_last_error_string(self._h).decode() if self._h else ""
            raise PftError(status, detail)

    def _ensure(self):
        if self._h is None:
            h = C.c_void_p()
            st = self._L.pft_filter_create(C.byref(self._cfg), C.byref(h))
            if st != 0:
                raise PftError(st, "pft_filter_create")
            self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.pft_filter_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- PCL-style use --
    def setInputCloud(self, cloud):
        cloud = np.ascontiguousarray(cloud)
        assert cloud.dtype == POINT_DTYPE
        self._cloud, self._dev, self._depth = cloud, None, None

    def setInputCloudDevice(self, device_ptr, n, keepalive=None):
        self._cloud, self._dev, self._depth = None, (int(device_ptr), int(n), keepalive), None

    def setInputDepth(self, depth, color=None, camera=QHD_CAMERA, depth_divisor=1000.0, color_format="bgr8"):
        """the frame as the sensor delivers it: a registered depth image (2-D uint16, divided by depth_divisor, or float32
        metres) and an optional colour image (H x W x 3|4 uint8) in host memory, camera = (fx, fy, cx, cy).  The organised
        cloud of W x H records is formed on the device (include/pft_filters.h has the specification); filter(),
        filterDevice() and filterAsync() then work as on a cloud, and passIndices() are pixel indices r W + c.  Row strides
        come from the arrays: rows may be padded, the pixels of a row must be packed.  Views of depthHostBuffers() make
        filterAsync() wait for nothing."""
        desc = depth_description(depth, color, camera, depth_divisor, color_format)
        self._cloud, self._dev, self._depth = None, None, (desc, depth, color)

    def depthHostBuffers(self, slot, shape=(540, 960), depth_dtype=np.uint16, color_format="bgr8"):
        """(depth, colour) NumPy views of pinned slot `slot` (0 or 1) of the handle, packed, for images of `shape` = (H, W);
        colour is None for color_format "none".  Fill them and pass them to setInputDepth: filterAsync() then waits for
        nothing, and the slot is busy until depthSlotDone(slot) says its upload has finished -- write to it only then.  The
        views die with the handle (close(), or any change of the configuration)."""
        H, W = int(shape[0]), int(shape[1])
        dt = np.dtype(depth_dtype)
        if color_format not in COLOR_FORMATS:
            raise ValueError("color_format: one of none, bgr8, rgb8, bgra8, rgba8")
        fmt, ch = COLOR_FORMATS[color_format]
        desc = depth_description(np.empty((1, 1), dt))
        desc.width, desc.height, desc.color_format = W, H, fmt
        self._ensure()
        pd, pc = C.c_void_p(), C.c_void_p()
        self._check(self._L.pft_filter_depth_host_buffers(self._h, C.byref(desc), int(slot), C.byref(pd), C.byref(pc)))
        depth = np.frombuffer((C.c_uint8 * (H * W * dt.itemsize)).from_address(pd.value), dt).reshape(H, W)
        color = None
        if ch:
            color = np.frombuffer((C.c_uint8 * (H * W * ch)).from_address(pc.value), np.uint8).reshape(H, W, ch)
        return depth, color

    def depthSlotDone(self, slot, wait=False):
        """has the upload of the last apply from pinned slot `slot` finished (wait=True: waits for it)"""
        self._ensure()
        done = C.c_int()
        self._check(self._L.pft_filter_depth_slot_done(self._h, int(slot), int(bool(wait)), C.byref(done)))
        return bool(done.value)

    def inputCloud(self):
        """the input cloud of the last apply on the host where the handle owns it: the organised cloud a depth apply
        formed, the upload of a host cloud (PftError 7 after a device cloud)"""
        p, n = self.inputDevice()
        out = np.zeros(n, POINT_DTYPE)
        got = C.c_size_t()
        self._check(self._L.pft_filter_get_input(self._h, _ptr(out), n, C.byref(got)))
        return out

    def inputDevice(self):
        """(device pointer, n) of that cloud in HBM, valid until the next apply: what ModelSegmenter.applyDevice and
        SceneSubtraction take"""
        if self._h is None:
            raise PftError(7, "inputDevice() before filter()")
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.pft_filter_input_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def _apply(self, wait=True):
        self._ensure()
        L = self._L
        if self._dev is not None:
            f = L.pft_filter_apply_device if wait else L.pft_filter_apply_device_async
            self._check(f(self._h, C.c_void_p(self._dev[0]), self._dev[1]))
        elif self._cloud is not None:
            f = L.pft_filter_apply if wait else L.pft_filter_apply_async
            self._check(f(self._h, _ptr(self._cloud), len(self._cloud)))
        elif self._depth is not None:
            desc, depth, color = self._depth
            f = L.pft_filter_apply_depth if wait else L.pft_filter_apply_depth_async
            self._check(f(self._h, C.byref(desc), C.c_void_p(depth.ctypes.data),
                          None if color is None else C.c_void_p(color.ctypes.data)))
        else:
            raise PftError(2, "filter() without an input cloud")

    def filterAsync(self):
        """enqueue the pipeline and return without waiting for it.  counts(), passIndices(), lastMilliseconds() and
        output() wait for it when first asked; ParticleFilterTracker.setInputCloudFromFilter hands the output on
        without any wait.  A device input cloud is borrowed until the pipeline has run."""
        self._apply(wait=False)

    def output(self):
        """the output cloud of the last filter() / filterAsync() on the host"""
        _, n_out = self.counts()
        out = np.zeros(n_out, POINT_DTYPE)
        n = C.c_size_t()
        self._check(self._L.pft_filter_get_output(self._h, _ptr(out), n_out, C.byref(n)))
        return out

    def outputDevice(self):
        """(device pointer, n) of the output cloud of the last filter() / filterAsync() (waits for a pending one)"""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.pft_filter_output_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def counts(self):
        a, b = C.c_size_t(), C.c_size_t()
        self._check(self._L.pft_filter_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def filter(self):
        """run the pipeline, return the output cloud on the host"""
        self._apply()
        _, n_out = self.counts()
        out = np.zeros(n_out, POINT_DTYPE)
        n = C.c_size_t()
        self._check(self._L.pft_filter_get_output(self._h, _ptr(out), n_out, C.byref(n)))
        return out

    def filterDevice(self):
        """run the pipeline, return (device pointer, n) of the output cloud in HBM (valid until the next call)"""
        self._apply()
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.pft_filter_output_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def passIndices(self):
        """indices of the points PassThrough kept (after filter())"""
        n_pass, _ = self.counts()
        idx = np.zeros(n_pass, np.int32)
        n = C.c_size_t()
        self._check(self._L.pft_filter_get_pass_indices(self._h, _ptr(idx), n_pass, C.byref(n)))
        return idx

    def lastMilliseconds(self):
        ms = C.c_double()
        self._check(self._L.pft_filter_last_ms(self._h, C.byref(ms)))
        return ms.value


class PassThrough(InputFilter):
    """pcl::PassThrough<PointXYZRGBA> (auto_tracking.cpp:536-547)"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self._set(voxel_mode=VOXEL_NONE, pass_enable=1)
        self._lim = (0.0, 10.0)
        self._field = "z"
        self._neg = False

    def setFilterFieldName(self, name):
        self._field = name
        self.setPassThrough(self._field, self._lim[0], self._lim[1], self._neg)

    def setFilterLimits(self, lo, hi):
        self._lim = (float(lo), float(hi))
        self.setPassThrough(self._field, self._lim[0], self._lim[1], self._neg)

    def setFilterLimitsNegative(self, neg):
        self._neg = bool(neg)
        self.setPassThrough(self._field, self._lim[0], self._lim[1], self._neg)

    def setKeepOrganized(self, keep):
        if keep:
            raise NotImplementedError("keep_organized = true is not on the reference's path (auto_tracking.cpp:543)")


class ApproximateVoxelGrid(InputFilter):
    """pcl::ApproximateVoxelGrid<PointXYZRGBA> (auto_tracking.cpp:563-575)"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self._set(voxel_mode=VOXEL_APPROX, pass_enable=0)


class VoxelGrid(InputFilter):
    """pcl::VoxelGrid<PointXYZRGBA> (auto_tracking.cpp:549-561)"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self._set(voxel_mode=VOXEL_EXACT, pass_enable=0)


def make_reference_input_filter(**kw):
    """PassThrough z in [0, 10] + ApproximateVoxelGrid(0.01): the reference's per-frame front end
    (auto_tracking.cpp:637, 683), fused"""
    return InputFilter(**kw)

"""Python mirror of scene subtraction (include/pft_subtract.h): which points of a frame do the tracked objects at their
current poses explain, and the rest as a cloud.  All compute runs in the HIP library.

    sub = SceneSubtraction(radius=0.02)
    sub.bindTracker(0, tracker)             # the tracker's model at its current result pose, taken on the device
    sub.setObject(1, cloud, matrix3x4)      # or an explicit cloud and matrix
    sub.apply(frame)                        # enqueues and returns
    n_in, n_explained, n_residual = sub.counts()
    clusters = sub.segmentResidual(segmenter)   # [(indices into the frame, points)]: what no object accounts for
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PftError, SubtractConfig
from .scene import POINT_DTYPE

_CLOUDS = {"reference": _lib.SUBTRACT_REFERENCE_CLOUD, "report": _lib.SUBTRACT_REPORT_CLOUD}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class SceneSubtraction:
    """one pft_subtract handle.  A bound tracker is borrowed: this object keeps the Python tracker alive and binds
    again when the tracker re-created its handle, but a tracker that is closed by hand must be removed first."""

    def __init__(self, radius=0.02, cloud="reference", device_id=0):
        if cloud not in _CLOUDS:
            raise PftError(1, "cloud: 'reference' or 'report'")
        self._L = _lib.load()
        cfg = SubtractConfig()
        self._L.pft_subtract_default_config(C.byref(cfg))
        cfg.radius = float(radius)
        cfg.cloud = _CLOUDS[cloud]
        cfg.device_id = int(device_id)
        self._h = None
        h = C.c_void_p()
        st = self._L.pft_subtract_create(C.byref(cfg), C.byref(h))
        if st != 0:
            raise PftError(st, "pft_subtract_create")
        self._h = h
        self._bound = {}  # slot -> (tracker, the handle value that was bound)
        self._keep = None

    def _check(self, status):
        if status != 0:
            raise PftError(status, self._L.pft_subtract_last_error_string(self._h).decode() if self._h else "")

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.pft_subtract_destroy(self._h)
            self._h = None
            self._bound = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- slots --
    def setObject(self, slot, cloud, matrix):
        """explicit slot: a cloud (only x, y, z are read) and a 3x4 (or 4x4) matrix"""
        cloud = np.ascontiguousarray(cloud, POINT_DTYPE)
        m = np.ascontiguousarray(np.asarray(matrix, np.float32).reshape(-1)[:12])
        self._check(self._L.pft_subtract_set_object(self._h, int(slot), _ptr(cloud), len(cloud), _ptr(m)))
        self._bound.pop(int(slot), None)

    def setObjectMatrix(self, slot, matrix):
        m = np.ascontiguousarray(np.asarray(matrix, np.float32).reshape(-1)[:12])
        self._check(self._L.pft_subtract_set_object_matrix(self._h, int(slot), _ptr(m)))

    def bindTracker(self, slot, tracker):
        tracker._ensure()
        self._check(self._L.pft_subtract_bind_tracker(self._h, int(slot), tracker._h))
        self._bound[int(slot)] = (tracker, tracker._h.value)

    def removeObject(self, slot):
        self._check(self._L.pft_subtract_remove_object(self._h, int(slot)))
        self._bound.pop(int(slot), None)

    def clear(self):
        self._check(self._L.pft_subtract_clear(self._h))
        self._bound = {}

    def _rebind(self):
        for slot, (t, hv) in list(self._bound.items()):
            if t._h is None or t._h.value != hv:  # the tracker re-created its handle (a configuration change)
                self.bindTracker(slot, t)

    # -- apply --
    def apply(self, cloud):
        cloud = np.ascontiguousarray(cloud, POINT_DTYPE)
        self._rebind()
        self._keep = None
        self._check(self._L.pft_subtract_apply(self._h, _ptr(cloud), len(cloud)))

    def applyDevice(self, device_ptr, n, keepalive=None):
        """a frame already resident in HBM (PCL 32-byte layout); keepalive is held until the next apply"""
        self._rebind()
        self._keep = keepalive
        self._check(self._L.pft_subtract_apply_device(self._h, C.c_void_p(int(device_ptr)), int(n)))

    # -- results of the last apply (these wait for it) --
    def counts(self):
        """(n_in, n_explained, n_residual)"""
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self._L.pft_subtract_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def owners(self):
        out = np.zeros(self.counts()[0], np.int32)
        self._check(self._L.pft_subtract_get_owner(self._h, _ptr(out), len(out)))
        return out

    def sqDistances(self):
        out = np.zeros(self.counts()[0], np.float32)
        self._check(self._L.pft_subtract_get_sq_dist(self._h, _ptr(out), len(out)))
        return out

    def support(self):
        out = np.zeros(_lib.SUBTRACT_MAX_OBJECTS, np.uint32)
        self._check(self._L.pft_subtract_get_support(self._h, _ptr(out), len(out)))
        return out

    def residual(self):
        out = np.zeros(self.counts()[2], POINT_DTYPE)
        n = C.c_size_t()
        self._check(self._L.pft_subtract_get_residual(self._h, _ptr(out), len(out), C.byref(n)))
        return out

    def residualIndices(self):
        out = np.zeros(self.counts()[2], np.int32)
        n = C.c_size_t()
        self._check(self._L.pft_subtract_get_residual_indices(self._h, _ptr(out), len(out), C.byref(n)))
        return out

    def residualDevice(self):
        """(device pointer, n): the residual in HBM, valid until the next apply; the pointer is 0 for an empty residual"""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.pft_subtract_residual_device(self._h, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def object(self, slot):
        """(matrix float32[3, 4], moved points float32[n, 3]) the last apply used for the slot"""
        n = C.c_size_t()
        m = np.zeros(12, np.float32)
        self._check(self._L.pft_subtract_get_object(self._h, int(slot), _ptr(m), None, 0, C.byref(n)))
        pts = np.zeros((n.value, 3), np.float32)
        self._check(self._L.pft_subtract_get_object(self._h, int(slot), _ptr(m), _ptr(pts), n.value, C.byref(n)))
        return m.reshape(3, 4), pts

    def lastMilliseconds(self):
        ms = C.c_double()
        self._check(self._L.pft_subtract_last_ms(self._h, C.byref(ms)))
        return ms.value

    def segmentResidual(self, segmenter):
        """hand the residual to the ModelSegmenter device to device; -> its clusters as [(indices into the FRAME,
        points)], in the segmenter's cluster order"""
        p, n = self.residualDevice()
        if n == 0:
            return []
        idx = self.residualIndices()
        segmenter.setInputCloudDevice(p, n, keepalive=self)
        segmenter.apply()
        return [(idx[ci], pts) for ci, pts in segmenter.clusters()]

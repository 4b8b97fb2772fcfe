"""Python mirror of the model preparation (include/pft_model.h): the "set object to track" block of the reference's
cloud_cb (auto_tracking.cpp:643-677) -- removeZeroPoints, compute3DCentroid, the re-centring by trans.inverse() and
gridSample -- as one device pipeline per object.  All compute runs in the HIP library.

    mp = ModelPreparation()
    mp.prepareFromSegmenter(seg, j, leaf=0.01)         # cluster j, read where it lies in HBM
    tracker.setObjectFromModel(mp, report_cloud=True)  # setReferenceCloud + setTrans (+ setReportCloud)
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PftError
from .scene import POINT_DTYPE


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _as_cloud(cloud):
    """a contiguous 1-D array of 32-byte PCL points; anything else is refused before the library is called"""
    if not isinstance(cloud, np.ndarray) or cloud.dtype != POINT_DTYPE:
        raise PftError(1, "the cloud must be a NumPy array of scene.POINT_DTYPE (32-byte pcl::PointXYZRGBA records)")
    if cloud.ndim != 1:
        raise PftError(1, "the cloud must be one-dimensional, got shape %r" % (cloud.shape,))
    return np.ascontiguousarray(cloud)


class ModelPreparation:
    """one pft_model handle, created at the first prepare*()"""

    def __init__(self, device_id=0):
        self._L = _lib.load()
        self._device_id = int(device_id)
        self._h = None
        self._keep = None

    def _check(self, status):
        if status != 0:
            detail = self._L.pft_model_last_error_string(self._h).decode() if self._h else ""
            raise PftError(status, detail)

    def _ensure(self):
        if self._h is None:
            h = C.c_void_p()
            st = self._L.pft_model_create(self._device_id, C.byref(h))
            if st != 0:
                raise PftError(st, "pft_model_create")
            self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.pft_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the three entrances ----
    def prepare(self, cloud, leaf=0.01):
        """an object cluster in host memory; leaf: gridSample's VoxelGrid leaf, <= 0 keeps the re-centred cloud"""
        cloud = _as_cloud(cloud)
        self._ensure()
        self._check(self._L.pft_model_prepare(self._h, _ptr(cloud), len(cloud), float(leaf)))

    def prepareDevice(self, ptr, n, leaf=0.01):
        """n 32-byte points at the device pointer `ptr`, read during the call only"""
        n = int(n)
        if n < 0:
            raise PftError(1, "prepareDevice: negative point count")
        self._ensure()
        self._check(self._L.pft_model_prepare_device(self._h, C.c_void_p(int(ptr)), n, float(leaf)))

    def prepareFromSegmenter(self, seg, cluster, leaf=0.01):
        """cluster `cluster` of the last apply() of the ModelSegmenter `seg`, read where it lies in HBM"""
        cluster = int(cluster)
        if cluster < 0:
            raise PftError(1, "prepareFromSegmenter: negative cluster index")
        if seg._h is None:
            raise PftError(7, "prepareFromSegmenter: the segmenter has not been applied yet")
        self._ensure()
        self._check(self._L.pft_model_prepare_from_segment(self._h, seg._h, cluster, float(leaf)))

    # ---- results of the last prepare ----
    def counts(self):
        """(points given, points after removeZeroPoints, points of the reference cloud)"""
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self._L.pft_model_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def trans(self):
        """4x4 float32: the identity with the centroid in column 3 (what setTrans takes)"""
        t = np.zeros(16, np.float32)
        self._check(self._L.pft_model_get_trans(self._h, _ptr(t)))
        return t.reshape(4, 4)

    def _cloud(self, get, n):
        out = np.zeros(n, POINT_DTYPE)
        got = C.c_size_t()
        self._check(get(self._h, _ptr(out), n, C.byref(got)))
        return out

    def recentred(self):
        """transed_ref: the re-centred, full-resolution model (reference_dict[obj])"""
        return self._cloud(self._L.pft_model_get_recentred, self.counts()[1])

    def reference(self):
        """transed_ref_downsampled: the tracker's reference cloud"""
        return self._cloud(self._L.pft_model_get_reference, self.counts()[2])

    def outputDevice(self):
        """((device pointer, n) of the re-centred cloud, (device pointer, n) of the reference cloud), valid until the
        next prepare*()"""
        p1, p2 = C.c_void_p(), C.c_void_p()
        n1, n2 = C.c_size_t(), C.c_size_t()
        self._check(self._L.pft_model_output_device(self._h, C.byref(p1), C.byref(n1), C.byref(p2), C.byref(n2)))
        return (p1.value or 0, n1.value), (p2.value or 0, n2.value)

    def lastMilliseconds(self):
        """(total, {stage: ms}) GPU time of the last prepare"""
        ms = C.c_double()
        st = (C.c_double * len(_lib.MODEL_STAGES))()
        self._check(self._L.pft_model_last_ms(self._h, C.byref(ms), st))
        return ms.value, dict(zip(_lib.MODEL_STAGES, list(st)))

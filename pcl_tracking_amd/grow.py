"""Python mirror of model growth (include/pft_grow.h): fold surface that is seen next to an object's model, frame after
frame, into the model.  All compute runs in the HIP library.

    grow = ModelGrowth(confirm=3)
    grow.setModel(model)                    # object frame; its voxels are the MODEL set
    grow.setPlanes([table_abcd])            # camera frame: points on these planes never enter
    grow.applyResidual(sub, matrix3x4)      # the residual of a SceneSubtraction, device to device; enqueues and returns
    if grow.stats()["n_added"]:
        tracker.setReportCloud(grow.model())   # the report cloud and the subtraction take the grown model;
                                               # the tracker's REFERENCE cloud stays what the user gave
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GROW_STATES, GrowConfig, GrowStatsStruct, PftError
from .scene import POINT_DTYPE

_FIELDS = ("leaf", "reach", "confirm", "forget", "max_radius", "max_voxels", "plane_margin")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _m12(matrix):
    m = np.ascontiguousarray(np.asarray(matrix, np.float32).reshape(-1)[:12])
    if m.size != 12:
        raise PftError(1, "matrix: 3x4 or 4x4")
    return m


class ModelGrowth:
    """one pft_grow handle: one object.  Keyword arguments are the fields of pft_grow_config; what is not given keeps the
    library's default."""

    def __init__(self, device_id=0, **kw):
        self._L = _lib.load()
        cfg = GrowConfig()
        self._L.pft_grow_default_config(C.byref(cfg))
        cfg.device_id = int(device_id)
        for k, v in kw.items():
            if k not in _FIELDS:
                raise TypeError("ModelGrowth: unknown configuration field %r" % k)
            setattr(cfg, k, v)
        self.config = {k: getattr(cfg, k) for k in _FIELDS}
        self._h = None
        h = C.c_void_p()
        st = self._L.pft_grow_create(C.byref(cfg), C.byref(h))
        if st != 0:
            raise PftError(st, self._L.pft_grow_last_error_string(None).decode())
        self._h = h
        self._keep = None

    def _check(self, status):
        if status != 0:
            raise PftError(status, self._L.pft_grow_last_error_string(self._h).decode() if self._h else "")

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.pft_grow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- inputs --
    def setModel(self, cloud):
        cloud = np.ascontiguousarray(cloud, POINT_DTYPE)
        self._check(self._L.pft_grow_set_model(self._h, _ptr(cloud), len(cloud)))

    def setModelDevice(self, device_ptr, n):
        self._check(self._L.pft_grow_set_model_device(self._h, C.c_void_p(int(device_ptr)), int(n)))

    def setPlanes(self, planes):
        """0 .. 4 planes (a, b, c, d) in the camera frame"""
        p = np.ascontiguousarray(np.asarray(planes, np.float32).reshape(-1, 4))
        self._check(self._L.pft_grow_set_planes(self._h, _ptr(p), len(p)))

    def apply(self, cloud, matrix):
        cloud = np.ascontiguousarray(cloud, POINT_DTYPE)
        self._keep = None
        self._check(self._L.pft_grow_apply(self._h, _ptr(cloud), len(cloud), _ptr(_m12(matrix))))

    def applyDevice(self, device_ptr, n, matrix, keepalive=None):
        """a cloud already resident in HBM (PCL 32-byte layout); keepalive is held until the next apply"""
        self._keep = keepalive
        self._check(self._L.pft_grow_apply_device(self._h, C.c_void_p(int(device_ptr)), int(n), _ptr(_m12(matrix))))

    def applyResidual(self, sub, matrix):
        """the residual of a SceneSubtraction's last apply, device to device"""
        p, n = sub.residualDevice()
        self.applyDevice(p, n, matrix, keepalive=sub)

    def applyTracker(self, tracker, cloud_or_sub):
        """at the tracker's result pose (read on the host): a host cloud, or a SceneSubtraction's residual"""
        m = tracker.toEigenMatrix(tracker.getResult())
        if hasattr(cloud_or_sub, "residualDevice"):
            self.applyResidual(cloud_or_sub, m)
        else:
            self.apply(cloud_or_sub, m)

    # -- results (these wait for the last apply) --
    def stats(self):
        """the fields of pft_grow_stats as a dict, the states by name.  After an apply that overflowed the first
        synchronising call raises PftError(6) once; the statistics are there on the next call"""
        s = GrowStatsStruct()
        self._check(self._L.pft_grow_get_stats(self._h, C.byref(s)))
        out = {k: int(getattr(s, k)) for k, _ in GrowStatsStruct._fields_ if k not in ("n_state", "pad")}
        out["n_state"] = {name: int(s.n_state[i]) for i, name in enumerate(GROW_STATES)}
        return out

    def _n_in(self):
        s = GrowStatsStruct()
        self._check(self._L.pft_grow_get_stats(self._h, C.byref(s)))
        return s

    def states(self):
        out = np.zeros(self._n_in().n_in, np.uint8)
        self._check(self._L.pft_grow_get_states(self._h, _ptr(out), len(out)))
        return out

    def model(self):
        out = np.zeros(self._n_in().n_model_points, POINT_DTYPE)
        n = C.c_size_t()
        self._check(self._L.pft_grow_get_model(self._h, _ptr(out), len(out), C.byref(n)))
        return out

    def modelDevice(self):
        """(device pointer, n): the model in HBM, valid until the next apply or setModel"""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.pft_grow_model_device(self._h, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def transform(self):
        """the inverse matrix of the last apply, float32[3, 4]"""
        m = np.zeros(12, np.float32)
        self._check(self._L.pft_grow_get_transform(self._h, _ptr(m)))
        return m.reshape(3, 4)

    def lastMilliseconds(self):
        ms = C.c_double()
        self._check(self._L.pft_grow_last_ms(self._h, C.byref(ms)))
        return ms.value

    def debugTable(self):
        """every MODEL and live PENDING voxel, sorted by key: dict of keys int32[n, 3], kind, hits, last_seen uint32[n]"""
        n = C.c_size_t()
        self._check(self._L.pft_debug_grow_get_table(self._h, None, None, None, None, 0, C.byref(n)))
        keys = np.zeros((n.value, 3), np.int32)
        kind, hits, seen = (np.zeros(n.value, np.uint32) for _ in range(3))
        self._check(self._L.pft_debug_grow_get_table(self._h, _ptr(keys), _ptr(kind), _ptr(hits), _ptr(seen), n.value, C.byref(n)))
        return dict(keys=keys, kind=kind, hits=hits, last_seen=seen)

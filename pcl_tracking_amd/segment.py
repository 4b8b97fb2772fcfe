"""Python mirror of the PCL classes the reference's model-creation nodes run (create_model_planar_segmentation.cpp:131-203,
create_model.cpp:131-179), over the C ABI of include/pft_segment.h.  All compute runs in the HIP library.

    seg = SACSegmentation(); seg.setMaxIterations(1000); seg.setDistanceThreshold(0.015)
    seg.setInputCloud(cloud); inliers, coefficients = seg.segment()
    ec = EuclideanClusterExtraction(); ec.setClusterTolerance(0.02); ec.setMinClusterSize(500)
    ec.setMaxClusterSize(25000); ec.setInputCloud(cloud); clusters = ec.extract()

ModelSegmenter is the fused pipeline (transform, removeZeroPoints, plane, ExtractIndices negative, PassThrough box,
clustering) of one handle; `make_planar_segmenter` / `make_box_segmenter` configure it as the two reference nodes,
`make_scene_segmenter` as the plane-after-plane loop of test/cluster_euclid.cpp:59-85 and test/cluster_extraction.cpp."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PftError, SegmentConfig, SegmentPlane, SegmentRefitDebug
from .scene import POINT_DTYPE


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class ModelSegmenter:
    """one pft_segment handle; the handle is created lazily and re-created when the configuration changes"""

    def __init__(self, device_id=0, stream=None, **cfg):
        self._L = _lib.load()
        self._cfg = SegmentConfig()
        self._L.pft_segment_default_config(C.byref(self._cfg))
        self._cfg.device_id = device_id
        if stream is not None:
            self._cfg.stream = stream
            self._cfg.stream_is_external = 1
        self._h = None
        self._cloud = None
        self._dev = None
        self._rounds = (1, 0.0)  # pft_segment_set_plane_rounds / _set_refit_order: applied to every handle created
        self._refit_order = _lib.PFT_SUM_PCL
        self.configure(**cfg)

    def configure(self, transform=None, plane=None, max_iterations=None, distance_threshold=None, probability=None,
                  optimize=None, box=None, box_enable=None, tolerance=None, min_size=None, max_size=None,
                  plane_rounds=None, refit_order=None):
        """transform: 4x4 camera->base (None keeps, False disables); box: (xmin, xmax, ymin, ymax, zmin, zmax);
        box_enable: three flags; plane_rounds: (max_planes, min_remaining_fraction), planes are removed one after the
        other while more than the fraction of the points is left; refit_order: "pcl" (serial float sums) or "tree"
        (adjacent-pair trees over many workgroups)"""
        c = self._cfg
        if plane_rounds is not None:
            mx, frac = plane_rounds
            if not 1 <= int(mx) <= _lib.SEGMENT_MAX_PLANES or not 0.0 <= float(frac) <= 1.0:
                raise PftError(1, "plane_rounds: max_planes 1 .. %d, fraction within [0, 1]" % _lib.SEGMENT_MAX_PLANES)
            self._rounds = (int(mx), float(frac))
        if refit_order is not None:
            if refit_order not in ("pcl", "tree"):
                raise PftError(1, "refit_order: 'pcl' or 'tree'")
            self._refit_order = _lib.PFT_SUM_TREE if refit_order == "tree" else _lib.PFT_SUM_PCL
        if transform is not None:
            if transform is False:
                c.transform_enable = 0
            else:
                m = np.asarray(transform, np.float32).reshape(16)
                c.transform_enable = 1
                c.transform = (C.c_float * 16)(*m)
        if plane is not None:
            c.plane_enable = int(bool(plane))
        if max_iterations is not None:
            c.max_iterations = int(max_iterations)
        if distance_threshold is not None:
            c.distance_threshold = float(distance_threshold)
        if probability is not None:
            c.probability = float(probability)
        if optimize is not None:
            c.optimize_coefficients = int(bool(optimize))
        if box is not None:
            b = [float(v) for v in box]
            c.box_min = (C.c_float * 3)(b[0], b[2], b[4])
            c.box_max = (C.c_float * 3)(b[1], b[3], b[5])
        if box_enable is not None:
            c.box_enable = (C.c_int32 * 3)(*[int(bool(v)) for v in box_enable])
        if tolerance is not None:
            c.cluster_tolerance = float(tolerance)
        if min_size is not None:
            c.min_cluster_size = int(min_size)
        if max_size is not None:
            c.max_cluster_size = int(max_size)
        self.close()

    @property
    def config(self):
        return self._cfg

    def _check(self, status):
        if status != 0:
            detail = self._L.pft_segment_last_error_string(self._h).decode() if self._h else ""
            raise PftError(status, detail)

    def _ensure(self):
        if self._h is None:
            h = C.c_void_p()
            st = self._L.pft_segment_create(C.byref(self._cfg), C.byref(h))
            if st != 0:
                raise PftError(st, "pft_segment_create")
            self._h = h
            self._check(self._L.pft_segment_set_plane_rounds(h, self._rounds[0], self._rounds[1]))
            self._check(self._L.pft_segment_set_refit_order(h, self._refit_order))

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.pft_segment_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setInputCloud(self, cloud):
        cloud = np.ascontiguousarray(cloud)
        assert cloud.dtype == POINT_DTYPE
        self._cloud, self._dev = cloud, None

    def setInputCloudDevice(self, device_ptr, n, keepalive=None):
        self._cloud, self._dev = None, (int(device_ptr), int(n), keepalive)

    def apply(self):
        """run the pipeline over the input cloud (host or device)"""
        self._ensure()
        if self._dev is not None:
            self._check(self._L.pft_segment_apply_device(self._h, C.c_void_p(self._dev[0]), self._dev[1]))
        elif self._cloud is not None:
            self._check(self._L.pft_segment_apply(self._h, _ptr(self._cloud), len(self._cloud)))
        else:
            raise PftError(2, "apply() without an input cloud")

    def applyDevice(self, device_ptr, n, keepalive=None):
        """setInputCloudDevice + apply: applyDevice(*f.inputDevice()) runs over the cloud a filter's depth apply formed"""
        self.setInputCloudDevice(device_ptr, n, keepalive)
        self.apply()

    # -- results of the last apply --
    def planeCount(self):
        """planes the last apply removed"""
        n = C.c_size_t()
        self._check(self._L.pft_segment_plane_count(self._h, C.byref(n), None))
        return n.value

    def stoppedBy(self):
        """why the plane rounds ended: _lib.ROUNDS_STOP_FRACTION / _NO_PLANE / _MAX_PLANES"""
        why = C.c_int()
        self._check(self._L.pft_segment_plane_count(self._h, None, C.byref(why)))
        return why.value

    def plane(self, round=0):
        """the record of one round (n_valid = the round's cloud size, sample indexes the round's cloud)"""
        pl = SegmentPlane()
        self._check(self._L.pft_segment_get_plane_round(self._h, round, C.byref(pl)))
        return {
            "status": pl.status, "n_valid": pl.n_valid, "coefficients": np.array(pl.coefficients, np.float32),
            "ransac_coefficients": np.array(pl.ransac_coefficients, np.float32), "sample": list(pl.sample),
            "ransac_inliers": pl.ransac_inliers, "inliers": pl.inliers, "iterations": pl.iterations,
            "hypotheses_scored": pl.hypotheses_scored, "n_survivors": pl.n_survivors,
        }

    def planeInliers(self, which=0, round=0):
        """indices into the input cloud: which = 0 final inliers, 1 the best RANSAC hypothesis' inliers"""
        n = C.c_size_t()
        pl = self.plane(round)
        cnt = pl["inliers"] if which == 0 else pl["ransac_inliers"]
        if pl["status"] != _lib.PLANE_FOUND:
            cnt = 0
        idx = np.zeros(cnt, np.int32)
        self._check(self._L.pft_segment_get_plane_round_inliers(self._h, round, which, _ptr(idx), cnt, C.byref(n)))
        return idx[: n.value]

    def clusterSizes(self):
        n = C.c_size_t()
        self._check(self._L.pft_segment_cluster_count(self._h, C.byref(n)))
        sizes = np.zeros(n.value, np.uint32)
        self._check(self._L.pft_segment_cluster_sizes(self._h, _ptr(sizes), n.value))
        return sizes

    def clusters(self):
        """[(indices into the input, points of the input)] in cluster order"""
        sizes = self.clusterSizes()
        total = int(sizes.sum())
        idx = np.zeros(total, np.int32)
        pts = np.zeros(total, POINT_DTYPE)
        n = C.c_size_t()
        self._check(self._L.pft_segment_get_cluster_indices(self._h, _ptr(idx), total, C.byref(n)))
        self._check(self._L.pft_segment_get_cluster_points(self._h, _ptr(pts), total, C.byref(n)))
        out, o = [], 0
        for s in sizes:
            out.append((idx[o:o + int(s)], pts[o:o + int(s)]))
            o += int(s)
        return out

    def clustersDevice(self):
        """(device pointer, sizes): all cluster points one after the other in HBM, in cluster order -- cluster j starts
        32 * sizes[:j].sum() bytes in.  Valid until the next apply(); the pointer is 0 without clusters."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.pft_segment_clusters_device(self._h, C.byref(p), C.byref(n)))
        return p.value or 0, self.clusterSizes()

    def hypotheses(self, round=0):
        """(samples int32[n, 3], counts uint32[n]) in draw order, n = RANSAC iterations of the round"""
        n = C.c_size_t()
        st = self._L.pft_debug_segment_round_hypotheses(self._h, round, None, None, 0, C.byref(n))
        if st not in (0, 6):
            self._check(st)
        smp = np.zeros((n.value, 3), np.int32)
        cnt = np.zeros(n.value, np.uint32)
        self._check(self._L.pft_debug_segment_round_hypotheses(self._h, round, _ptr(smp), _ptr(cnt), n.value,
                                                               C.byref(n)))
        return smp, cnt

    def refitDebug(self, round=0):
        """what the one-lane tail of a round's refit did (pft_segment_refit_debug) as a dict of NumPy values; raises
        PftError when the round found no plane or no refit ran"""
        d = SegmentRefitDebug()
        self._check(self._L.pft_debug_segment_refit(self._h, round, C.byref(d)))
        out = {"m": d.m, "branches": d.branches, "scale": np.float32(d.scale)}
        for k in ("accu", "cov", "trig_arg", "trig", "roots", "len", "coef"):
            out[k] = np.array(getattr(d, k), np.float32)
        return out

    def lastMilliseconds(self):
        """(total, {stage: ms})"""
        ms = C.c_double()
        st = (C.c_double * len(_lib.SEGMENT_STAGES))()
        self._check(self._L.pft_segment_last_ms(self._h, C.byref(ms), st))
        return ms.value, dict(zip(_lib.SEGMENT_STAGES, list(st)))


def make_planar_segmenter(**kw):
    """create_model_planar_segmentation.cpp: plane on, PassThrough y then x"""
    s = ModelSegmenter(**kw)
    s.configure(plane=True, box_enable=(1, 1, 0))
    return s


def make_box_segmenter(**kw):
    """create_model.cpp: no plane, PassThrough z, y, x"""
    s = ModelSegmenter(**kw)
    s.configure(plane=False, box_enable=(1, 1, 1))
    return s


def make_scene_segmenter(**kw):
    """test/cluster_euclid.cpp:59-85 and test/cluster_extraction.cpp: planes (100 iterations, 0.02 m) are removed until
    at most 30 % of the points are left, no box, then clusters at 0.02 m with 10 .. 2 500 points.  The reference's loop
    has no cap on the rounds; here it is PFT_SEGMENT_MAX_PLANES, and stoppedBy() tells when it was reached."""
    s = ModelSegmenter(**kw)
    s.configure(plane=True, max_iterations=100, distance_threshold=0.02, plane_rounds=(_lib.SEGMENT_MAX_PLANES, 0.3),
                box_enable=(0, 0, 0), tolerance=0.02, min_size=10, max_size=2500)
    return s


class SACSegmentation:
    """pcl::SACSegmentation<PointXYZRGBA> with SACMODEL_PLANE / SAC_RANSAC (create_model_planar_segmentation.cpp:161-167);
    removeZeroPoints runs first, as the reference does before it"""

    def __init__(self, **kw):
        self._s = ModelSegmenter(**kw)
        self._s.configure(plane=True, box_enable=(0, 0, 0), min_size=2 ** 31 - 1, max_size=1)  # no clustering

    def setMaxIterations(self, n):
        self._s.configure(max_iterations=n)

    def setDistanceThreshold(self, t):
        self._s.configure(distance_threshold=t)

    def setProbability(self, p):
        self._s.configure(probability=p)

    def setOptimizeCoefficients(self, on):
        self._s.configure(optimize=on)

    def setInputCloud(self, cloud):
        self._s.setInputCloud(cloud)

    def segment(self):
        """-> (inlier indices into the input cloud, coefficients float32[4] or empty when no model was found)"""
        self._s.apply()
        pl = self._s.plane()
        if pl["status"] != _lib.PLANE_FOUND:
            return np.zeros(0, np.int32), np.zeros(0, np.float32)
        return self._s.planeInliers(0), pl["coefficients"]


class EuclideanClusterExtraction:
    """pcl::EuclideanClusterExtraction<PointXYZRGBA> (create_model_planar_segmentation.cpp:184-189): removeZeroPoints,
    then the clusters; -> list of index arrays into the input cloud, by size descending"""

    def __init__(self, **kw):
        self._s = ModelSegmenter(**kw)
        self._s.configure(plane=False, box_enable=(0, 0, 0))

    def setClusterTolerance(self, t):
        self._s.configure(tolerance=t)

    def setMinClusterSize(self, n):
        self._s.configure(min_size=n)

    def setMaxClusterSize(self, n):
        self._s.configure(max_size=n)

    def setInputCloud(self, cloud):
        self._s.setInputCloud(cloud)

    def extract(self):
        self._s.apply()
        return [idx for idx, _ in self._s.clusters()]

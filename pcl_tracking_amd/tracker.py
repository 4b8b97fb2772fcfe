"""Python mirror of the PCL tracker interface the reference drives (same member names and argument
meaning as the calls at /root/reference/src/auto_tracking.cpp:201-254, 270, 309-310, 673-676, 691-693),
implemented over the C ABI of include/pft.h.  All compute runs in the HIP library; nothing here
computes on the CPU."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import Config, PftError

SUM_ORDERS = {"tree": _lib.PFT_SUM_TREE, "pcl": _lib.PFT_SUM_PCL}
from .scene import PARTICLE_DTYPE, POINT_DTYPE


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


LIK_LAYOUTS = ("u16_leaf_starts", "u32_words", "branch_only", "hybrid")  # PftHeader::lik_layout bits 1-2
LIK_DESCENTS = ("fast", "table_generic", "no_table")  # bits 3-4


def decode_likelihood_layout(out4):
    """pft_debug_get_likelihood_layout's four words -> dict (valid False: no DEBUG_NN likelihood launch recorded)"""
    w = int(out4[0])
    return dict(valid=bool(w & 1), layout=LIK_LAYOUTS[(w >> 1) & 3], descent=LIK_DESCENTS[min((w >> 3) & 3, 2)],
                indirect=bool(w & 32), leaf_indirect=bool(w & 64), jump_dropped=bool(w & 128), J=(w >> 8) & 15,
                n_lds_words=int(out4[1]), lds_bytes=int(out4[2]), margin_cells=float(np.uint32(out4[3]).view(np.float32)))


@dataclass
class ObjectReport:
    """pft_object_report as NumPy arrays (float32): what drawResult and viz_cb compute from one result"""
    transform: np.ndarray    # 4x4, the pose's matrix with T[2][3] += -0.005f
    centroid: np.ndarray     # 4, [3] = 1
    covariance: np.ndarray   # 3x3
    eigenvalues: np.ndarray  # 3, ascending
    axes: np.ndarray         # 3x3, the eigenvectors as columns, col 2 = col 0 x col 1
    box_min: np.ndarray      # 3, in the principal frame
    box_max: np.ndarray
    box_centre: np.ndarray   # 3, viz_cb's tfinal
    box_quat: np.ndarray     # 4, viz_cb's qfinal as (x, y, z, w)
    box_size: np.ndarray     # 3
    n_points: int
    info: int                # 0 success, 1 the eigen solver did not converge

    FIELDS = ("transform", "centroid", "covariance", "eigenvalues", "axes", "box_min", "box_max", "box_centre", "box_quat",
              "box_size")

    @classmethod
    def from_struct(cls, r):
        shapes = {"transform": (4, 4), "covariance": (3, 3), "axes": (3, 3)}
        kw = {}
        for f in cls.FIELDS:
            a = np.array(getattr(r, f), dtype=np.float32)
            kw[f] = a.reshape(shapes[f]) if f in shapes else a
        return cls(n_points=int(r.n_points), info=int(r.info), **kw)


@dataclass
class MatchStats:
    """pft_match_stats: how well the frame's result pose fits the frame, and the lost rule's state"""
    transform: np.ndarray  # 3x4 float32, the T used: pose_to_matrix(result) on the device
    coherence: float       # sum over the matched pairs of DistanceCoherence x HSVColorCoherence
    sum_sq_dist: float     # sum over the matched pairs of the squared distance
    n_reference: int
    n_matched: int
    n_crop: int
    evaluated: bool        # False: the last iteration was skipped or failed; the other fields are the last evaluated frame's
    below: bool            # n_matched < min_ratio * n_reference
    streak: int            # evaluated frames in a row that were below
    lost: bool             # streak >= lost_after
    calls: int

    @property
    def ratio(self):
        """matched share of the reference cloud (0 for an empty reference)"""
        return self.n_matched / self.n_reference if self.n_reference else 0.0

    @property
    def rms_distance(self):
        """root mean square distance of the matched pairs (nan without one)"""
        return float(np.sqrt(self.sum_sq_dist / self.n_matched)) if self.n_matched else float("nan")

    @classmethod
    def from_struct(cls, r):
        return cls(transform=np.array(r.transform, dtype=np.float32).reshape(3, 4), coherence=float(r.coherence),
                   sum_sq_dist=float(r.sum_sq_dist), n_reference=int(r.n_reference), n_matched=int(r.n_matched),
                   n_crop=int(r.n_crop), evaluated=bool(r.evaluated), below=bool(r.below), streak=int(r.streak),
                   lost=bool(r.lost), calls=int(r.calls))


@dataclass
class VisibilityStats:
    """pft_visibility_stats: how much of the model the camera sees at a pose, and the occlusion-aware lost rule's state"""
    transform: np.ndarray  # 3x4 float32, the T used
    n_reference: int
    n_visible: int
    n_occluded: int        # covered by the scene: a frame point lies more than occlusion_margin in front
    n_self: int            # covered by the model itself
    n_out: int             # behind the near plane or outside the image
    n_frame: int
    has_match: bool        # the counts of a computeMatch() of the same frame were at hand
    n_visible_matched: int
    hidden: bool           # n_visible < min_visible_ratio * n_reference
    below: bool            # n_visible_matched < min_ratio * n_visible (never while hidden or without a match)
    streak: int
    lost: bool             # streak >= lost_after
    evaluated: bool
    calls: int

    @property
    def visible_ratio(self):
        return self.n_visible / self.n_reference if self.n_reference else 0.0

    @classmethod
    def from_struct(cls, r):
        kw = {f: int(getattr(r, f)) for f in ("n_reference", "n_visible", "n_occluded", "n_self", "n_out", "n_frame",
                                               "n_visible_matched", "streak", "calls")}
        kw.update({f: bool(getattr(r, f)) for f in ("has_match", "hidden", "below", "lost", "evaluated")})
        return cls(transform=np.array(r.transform, dtype=np.float32).reshape(3, 4), **kw)


@dataclass
class ViewStats:
    """pft_view_stats: the counts of one selectView()"""
    transform: np.ndarray  # 3x4 float32, the T used
    n_model: int
    n_state: tuple         # records per state: kept, decimated, self-occluded, out of view, non-finite
    n_visible: int
    n_kept: int
    evaluated: bool
    calls: int

    @classmethod
    def from_struct(cls, r):
        return cls(transform=np.array(r.transform, dtype=np.float32).reshape(3, 4), n_model=int(r.n_model),
                   n_state=tuple(int(v) for v in r.n_state), n_visible=int(r.n_visible), n_kept=int(r.n_kept),
                   evaluated=bool(r.evaluated), calls=int(r.calls))


@dataclass
class PopulationStats:
    """pft_population_stats: how sure the filter is about its pose"""
    sum_w: float           # the 29 tree sums in double: weights, squared weights,
    sum_w2: float
    s: np.ndarray          # 6, weighted offsets from the representative state,
    S: np.ndarray          # 21, weighted products of offsets (k <= l, row by row)
    n_eff: float           # effective sample size (sum_w)^2 / sum_w2
    mean: np.ndarray       # 6 float64: x, y, z, roll, pitch, yaw
    cov: np.ndarray        # 6x6 float64, symmetric
    rpy_sigma: np.ndarray  # 3 float64
    pos_sigma: np.ndarray  # 3 float32, ascending: the semi-axes of the position ellipsoid
    pos_axes: np.ndarray   # 3x3 float32, its axes as columns
    w_max: float
    n: int                 # particles reduced
    n_zero: int            # particles with weight 0 (no correspondence)
    i_max: int             # the first particle of weight w_max
    solve_info: int        # 0, or 1: the eigen solver did not converge
    evaluated: bool        # False: the last iteration failed on the device; the other fields are the last evaluated call's
    uncertain: bool        # pos_sigma[2] > max_pos_sigma or n_eff < min_n_eff
    streak: int            # evaluated calls in a row that were uncertain
    flagged: bool          # streak >= after
    calls: int

    @classmethod
    def from_struct(cls, r):
        return cls(sum_w=float(r.sum_w), sum_w2=float(r.sum_w2), s=np.array(r.s, dtype=np.float64),
                   S=np.array(r.S, dtype=np.float64), n_eff=float(r.n_eff), mean=np.array(r.mean, dtype=np.float64),
                   cov=np.array(r.cov, dtype=np.float64).reshape(6, 6), rpy_sigma=np.array(r.rpy_sigma, dtype=np.float64),
                   pos_sigma=np.array(r.pos_sigma, dtype=np.float32),
                   pos_axes=np.array(r.pos_axes, dtype=np.float32).reshape(3, 3), w_max=float(r.w_max), n=int(r.n),
                   n_zero=int(r.n_zero), i_max=int(r.i_max), solve_info=int(r.solve_info), evaluated=bool(r.evaluated),
                   uncertain=bool(r.uncertain), streak=int(r.streak), flagged=bool(r.flagged), calls=int(r.calls))


@dataclass
class ReacquireResult:
    """pft_reacquire_result: the candidate a re-acquisition call selected"""
    n_centres: int
    n_candidates: int
    n_reference: int
    n_crop: int
    best: int              # candidate index, -1 without candidates
    best_centre: int
    pose: np.ndarray       # PARTICLE_DTYPE record of the best candidate
    transform: np.ndarray  # 3x4 float32, the T it was scored with
    n_inliers: int
    n_matched: int
    accepted: bool
    applied: bool
    coherence: float
    sum_sq_dist: float
    inlier_sq_dist: float
    refined: object = None  # reacquire(refine=True): the RefineResult of the best candidate

    @property
    def trans(self):
        """the 4x4 that apply hands to setTrans: `transform` over the row (0, 0, 0, 1)"""
        m = np.eye(4, dtype=np.float32)
        m[:3] = self.transform
        return m

    @classmethod
    def from_struct(cls, r):
        pose = np.frombuffer(bytes(r.pose), PARTICLE_DTYPE)[0].copy()
        return cls(n_centres=int(r.n_centres), n_candidates=int(r.n_candidates), n_reference=int(r.n_reference),
                   n_crop=int(r.n_crop), best=int(r.best), best_centre=int(r.best_centre), pose=pose,
                   transform=np.array(r.transform, dtype=np.float32).reshape(3, 4), n_inliers=int(r.n_inliers),
                   n_matched=int(r.n_matched), accepted=bool(r.accepted), applied=bool(r.applied),
                   coherence=float(r.coherence), sum_sq_dist=float(r.sum_sq_dist), inlier_sq_dist=float(r.inlier_sq_dist))


@dataclass
class RefineResult:
    """pft_refine_result: what a refinement call did"""
    status: int            # index into _lib.REFINE_STATUS
    iterations: int        # solves taken
    n_reference: int
    n_crop: int
    bbox: np.ndarray       # float64 x_min, x_max, y_min, y_max, z_min, z_max of the crop
    start: np.ndarray      # 3x4 float32
    transform: np.ndarray  # 3x4 float32, the final T
    pose: np.ndarray       # PARTICLE_DTYPE record: toState of `transform`
    n_pairs_before: int
    n_inliers_before: int
    sum_sq_dist_before: float
    inlier_sq_dist_before: float
    n_pairs_after: int
    n_inliers_after: int
    sum_sq_dist_after: float
    inlier_sq_dist_after: float
    improved: bool
    applied: bool

    @property
    def status_name(self):
        return _lib.REFINE_STATUS[self.status]

    @property
    def trans(self):
        """the 4x4 that apply hands to setTrans: `transform` over the row (0, 0, 0, 1)"""
        m = np.eye(4, dtype=np.float32)
        m[:3] = self.transform
        return m

    @classmethod
    def from_struct(cls, r):
        pose = np.frombuffer(bytes(r.pose), PARTICLE_DTYPE)[0].copy()
        b, a = r.before, r.after
        return cls(status=int(r.status), iterations=int(r.iterations), n_reference=int(r.n_reference), n_crop=int(r.n_crop),
                   bbox=np.array(r.bbox, dtype=np.float64), start=np.array(r.start, dtype=np.float32).reshape(3, 4),
                   transform=np.array(r.transform, dtype=np.float32).reshape(3, 4), pose=pose,
                   n_pairs_before=int(b.n_pairs), n_inliers_before=int(b.n_inliers), sum_sq_dist_before=float(b.sum_sq_dist),
                   inlier_sq_dist_before=float(b.inlier_sq_dist), n_pairs_after=int(a.n_pairs), n_inliers_after=int(a.n_inliers),
                   sum_sq_dist_after=float(a.sum_sq_dist), inlier_sq_dist_after=float(a.inlier_sq_dist),
                   improved=bool(r.improved), applied=bool(r.applied))


class DistanceCoherence:
    """pcl::tracking::DistanceCoherence (auto_tracking.cpp:240-242)"""

    def __init__(self):
        self.weight = 1.0

    def setWeight(self, w):
        self.weight = float(w)


class HSVColorCoherence:
    """pcl::tracking::HSVColorCoherence (auto_tracking.cpp:244-247)"""

    def __init__(self):
        self.weight, self.h_weight, self.s_weight, self.v_weight = 1.0, 1.0, 1.0, 0.0

    def setWeight(self, w):
        self.weight = float(w)

    def setHWeight(self, w):
        self.h_weight = float(w)

    def setSWeight(self, w):
        self.s_weight = float(w)

    def setVWeight(self, w):
        self.v_weight = float(w)


class OctreeSearch:
    """pcl::search::Octree(resolution) (auto_tracking.cpp:250-252)"""

    def __init__(self, resolution):
        self.resolution = float(resolution)


class ApproxNearestPairPointCloudCoherence:
    """pcl::tracking::ApproxNearestPairPointCloudCoherence (auto_tracking.cpp:235-253).  As upstream,
    the class keeps its own search::Octree(0.01); setSearchMethod is accepted and only its resolution
    (which the reference sets to the same 0.01) is used."""

    def __init__(self):
        self.point_coherences = []
        self.maximum_distance = float("inf")
        self.resolution = 0.01

    def addPointCoherence(self, c):
        self.point_coherences.append(c)

    def setSearchMethod(self, search):
        self.resolution = search.resolution

    def setMaximumDistance(self, d):
        self.maximum_distance = float(d)


class NearestPairPointCloudCoherence(ApproxNearestPairPointCloudCoherence):
    """pcl::tracking::NearestPairPointCloudCoherence: the true nearest neighbour instead of the greedy octree
    descent -- the alternative auto_tracking.cpp keeps commented out (:237-238, :249)"""
    exact = True


class ParticleFilterTracker:
    """pcl::tracking::ParticleFilterOMPTracker<PointXYZRGBA, ParticleXYZRPY>, fixed particle number."""

    def __init__(self, threads=16, device_id=0, stream=None, seed=1, rank=0, world_size=1, sum_order="tree"):
        """sum_order: "tree" (the default: adjacent-pair trees, independent of how the population is split) or "pcl"
        (PCL's own order for normalizeWeight's weight sum and update()'s weighted mean; one workgroup runs the chains)"""
        self._L = _lib.load()
        self._cfg = Config()
        self._L.pft_config_default(C.byref(self._cfg))
        self._cfg.device_id = device_id
        self._cfg.stream = stream
        self._cfg.stream_is_external = 0 if stream is None else 1  # 0 is a valid handle: the default stream
        self._cfg.seed = seed
        self._cfg.rank = rank
        self._cfg.world_size = world_size
        self._h = None
        # ParticleFilterTracker's change detector: use, interval, min points, resolution (PCL's constructor defaults)
        self._cd = [False, 10, 10, 0.01]
        self._match_thr = (0.0, 1)  # pft_set_match_threshold: min_ratio, lost_after
        self._spread_thr = (float("inf"), 0.0, 1)  # pft_set_spread_threshold: max_pos_sigma, min_n_eff, after
        self._vis_cam = None  # pft_set_visibility_camera: a VisibilityConfig once set (None: the library's default)
        self._vis_thr = (0.25, 0.0, 1)  # pft_set_visibility_threshold: min_visible_ratio, min_ratio, lost_after
        self._rq_centres = 0  # centres of the last reacquire()
        self.setSumOrder(sum_order)
        self._trans = np.eye(4, dtype=np.float32)
        self._ref = None
        self._report_cloud = None
        self._keep = None
        self.threads = threads  # OpenMP thread count of the reference; meaningless on the GPU

    # ---- configuration (before the first compute) ----
    def _cfg_guard(self):
        if self._h is not None:
            raise PftError(7, "configuration is fixed once the handle exists")

    def setSumOrder(self, order):
        """"tree" or "pcl", or a PFT_SUM_* value (pft_create validates it); fixed once the handle exists"""
        self._cfg_guard()
        if isinstance(order, str):
            if order not in SUM_ORDERS:
                raise PftError(1, "sum_order must be one of %s" % sorted(SUM_ORDERS))
            order = SUM_ORDERS[order]
        self._cfg.sum_order = int(order)

    # ---- change detection (PCL allows these at any time: forwarded to the handle whenever it exists) ----
    def _forward_change_detector(self):
        if self._h is not None:
            use, interval, min_points, res = self._cd
            self._check(self._L.pft_set_change_detector(self._h, int(use), int(interval), int(min_points), float(res)))

    def _set_cd(self, k, v):
        old = list(self._cd)
        self._cd[k] = v
        try:
            self._forward_change_detector()
        except PftError:
            self._cd = old
            raise

    def setUseChangeDetector(self, use):
        self._set_cd(0, bool(use))

    def getUseChangeDetector(self):
        return self._cd[0]

    def setIntervalOfChangeDetection(self, interval):
        self._set_cd(1, int(interval))

    def getIntervalOfChangeDetection(self):
        return self._cd[1]

    def setMinPointsOfChangeDetection(self, n):
        self._set_cd(2, int(n))

    def getMinPointsOfChangeDetection(self):
        return self._cd[2]

    def setResolutionOfChangeDetection(self, res):
        """latched at the first compute(), as PCL creates its detector there"""
        self._set_cd(3, float(res))

    def getResolutionOfChangeDetection(self):
        return self._cd[3]

    def setTrans(self, m):
        self._trans = np.ascontiguousarray(m, np.float32).reshape(4, 4)
        if self._h is not None:
            self._check(self._L.pft_set_trans(self._h, _ptr(self._trans)))

    def setStepNoiseCovariance(self, cov):
        self._cfg_guard()
        for i in range(6):
            self._cfg.step_noise_cov[i] = float(cov[i])

    def setInitialNoiseCovariance(self, cov):
        self._cfg_guard()
        for i in range(6):
            self._cfg.initial_noise_cov[i] = float(cov[i])

    def setInitialNoiseMean(self, mean):
        self._cfg_guard()
        for i in range(6):
            self._cfg.initial_noise_mean[i] = float(mean[i])

    def setIterationNum(self, n):
        self._cfg_guard()
        self._cfg.iteration_num = int(n)

    def setParticleNum(self, n):
        self._cfg_guard()
        self._cfg.particle_num = int(n)

    def setResampleLikelihoodThr(self, v):
        self._cfg_guard()
        self._cfg.resample_likelihood_thr = float(v)

    def setUseNormal(self, b):
        self._cfg_guard()
        self._cfg.use_normal = 1 if b else 0

    def setAlpha(self, a):
        self._cfg_guard()
        self._cfg.alpha = float(a)

    def setMotionRatio(self, r):
        """the share of new particles that take the motion step (PCL's default 0.25; read by the KLD resample only)"""
        self._cfg_guard()
        self._cfg.motion_ratio = float(r)

    def getMotionRatio(self):
        return self._cfg.motion_ratio

    def setMinIndices(self, n):
        pass  # only read when use_normal_ is true (auto_tracking.cpp:676)

    def setCloudCoherence(self, coh):
        self._cfg_guard()
        self._cfg.max_distance = coh.maximum_distance
        self._cfg.octree_resolution = coh.resolution
        self._cfg.exact_nearest = 1 if getattr(coh, "exact", False) else 0
        kinds = [type(c) for c in coh.point_coherences]
        if kinds != [DistanceCoherence, HSVColorCoherence]:
            raise PftError(1, "supported point coherences: DistanceCoherence then HSVColorCoherence "
                              "(auto_tracking.cpp:240-247)")
        d, h = coh.point_coherences
        self._cfg.distance_weight = d.weight
        self._cfg.hsv_weight = h.weight
        self._cfg.h_weight, self._cfg.s_weight, self._cfg.v_weight = h.h_weight, h.s_weight, h.v_weight

    # ---- handle ----
    def _check(self, status):
        if status != 0:
            detail = self._L.pft_last_error_string(self._h).decode() if self._h else ""
            raise PftError(status, detail)

    def _ensure(self):
        if self._h is None:
            h = C.c_void_p()
            st = self._L.pft_create(C.byref(self._cfg), C.byref(h))
            if st != 0:
                raise PftError(st)
            self._h = h
            self._check(self._L.pft_set_trans(self._h, _ptr(self._trans)))
            if self._cd != [False, 10, 10, 0.01]:
                self._forward_change_detector()
            if self._match_thr != (0.0, 1):
                self._check(self._L.pft_set_match_threshold(self._h, *self._match_thr))
            if self._spread_thr != (float("inf"), 0.0, 1):
                self._check(self._L.pft_set_spread_threshold(self._h, *self._spread_thr))
            if self._vis_cam is not None:
                self._check(self._L.pft_set_visibility_camera(self._h, C.byref(self._vis_cam)))
            if self._vis_thr != (0.25, 0.0, 1):
                self._check(self._L.pft_set_visibility_threshold(self._h, *self._vis_thr))
            if self._ref is not None:
                self._check(self._L.pft_set_reference(self._h, _ptr(self._ref), len(self._ref)))
            if self._report_cloud is not None:
                self._check(self._L.pft_set_report_cloud(self._h, _ptr(self._report_cloud), len(self._report_cloud)))

    def close(self):
        if self._h is not None:
            self._L.pft_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- data ----
    def setReferenceCloud(self, cloud):
        self._ref = np.ascontiguousarray(cloud, POINT_DTYPE)
        if self._h is not None:
            self._check(self._L.pft_set_reference(self._h, _ptr(self._ref), len(self._ref)))

    def setObjectFromModel(self, mp, report_cloud=False):
        """setReferenceCloud + setTrans from the ModelPreparation `mp` (auto_tracking.cpp:673-675); report_cloud=True is
        also setReportCloud with its re-centred cloud, copied device to device.  The handle is created first, as
        setInputCloud does; a refusal leaves the tracker as it was."""
        if mp._h is None:
            raise PftError(7, "setObjectFromModel: the model has not been prepared")
        self._ensure()
        self._check(self._L.pft_set_object_from_model(self._h, mp._h, 1 if report_cloud else 0))
        # what a later close() and re-creation hands to the new handle
        self._ref = mp.reference()
        self._trans = mp.trans()
        if report_cloud:
            self._report_cloud = mp.recentred()

    def setInputCloud(self, cloud):
        self._ensure()
        cloud = np.ascontiguousarray(cloud, POINT_DTYPE)
        self._check(self._L.pft_set_input(self._h, _ptr(cloud), len(cloud)))

    def setInputCloudDevice(self, device_ptr, n, keepalive=None):
        """input cloud already resident in HBM (PCL 32-byte layout)"""
        self._ensure()
        self._keep = keepalive
        self._check(self._L.pft_set_input_device(self._h, C.c_void_p(device_ptr), n))

    def setInputCloudFromFilter(self, f, max_points=0):
        """input cloud = the output of the InputFilter `f`, whose filter() / filterAsync() may still be running: the
        cloud and its count are read on the device, nothing waits on the host.  max_points bounds the count (0: the
        size of the filter's input).  `f` is kept alive by this object until the next setInputCloud*."""
        self._ensure()
        if f._h is None:
            raise PftError(7, "setInputCloudFromFilter: the filter has not been applied yet")
        self._keep = f
        self._check(self._L.pft_set_input_from_filter(self._h, f._h, int(max_points)))

    def debugInputRecords(self, first, n):
        """the handle's 16-byte input records [first, first + n) as (n, 4) uint32 (test hook)"""
        out = np.zeros((n, 4), np.uint32)
        self._check(self._L.pft_debug_get_input_records(self._h, _ptr(out), first, n))
        return out

    def compute(self):
        self._ensure()
        self._check(self._L.pft_compute(self._h))

    def synchronize(self):
        self._check(self._L.pft_synchronize(self._h))

    def getResult(self):
        out = np.zeros(1, PARTICLE_DTYPE)
        self._check(self._L.pft_get_result(self._h, _ptr(out)))
        return out[0]

    def getParticles(self):
        n = C.c_size_t()
        self._check(self._L.pft_get_particles(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, PARTICLE_DTYPE)
        if n.value:
            self._check(self._L.pft_get_particles(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def toEigenMatrix(self, particle):
        p = np.ascontiguousarray(particle, PARTICLE_DTYPE).reshape(1)
        m = np.zeros(16, np.float32)
        self._L.pft_to_matrix(_ptr(p), _ptr(m))
        return m.reshape(4, 4)

    def getFitRatio(self):
        v = C.c_double()
        self._check(self._L.pft_get_fit_ratio(self._h, C.byref(v)))
        return v.value

    # ---- object report (drawResult + viz_cb on the device) ----
    def setReportCloud(self, cloud):
        """reference_dict[obj]: the re-centred, full-resolution model the result pose moves (copied; may be replaced)"""
        self._report_cloud = np.ascontiguousarray(cloud, POINT_DTYPE)
        if self._h is not None:
            self._check(self._L.pft_set_report_cloud(self._h, _ptr(self._report_cloud), len(self._report_cloud)))

    def computeReport(self):
        """enqueues the report of the last compute() on the tracker's stream; nothing waits"""
        if self._h is None:
            raise PftError(7, "computeReport before the first compute()")
        self._check(self._L.pft_report(self._h))

    def getReport(self):
        """waits for the last computeReport(); returns ObjectReport (float32 arrays: transform 4x4, centroid 4,
        covariance 3x3, eigenvalues 3, axes 3x3, box_min / box_max / box_centre / box_size 3, box_quat 4 (x, y, z, w))"""
        if self._h is None:
            raise PftError(7, "getReport before the first compute()")
        r = _lib.ObjectReport()
        self._check(self._L.pft_get_report(self._h, C.byref(r)))
        return ObjectReport.from_struct(r)

    def getTrackedCloud(self):
        """tracked_cloud_dict[obj]: the report cloud moved by the last report's transform"""
        if self._h is None:
            raise PftError(7, "getTrackedCloud before the first compute()")
        n = C.c_size_t()
        self._check(self._L.pft_get_tracked_cloud(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, POINT_DTYPE)
        self._check(self._L.pft_get_tracked_cloud(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    # ---- match statistics of the result pose, the lost rule, resetTracking ----
    def setMatchThreshold(self, min_ratio, lost_after=1):
        """the object counts as lost after `lost_after` evaluated frames in a row whose result matched fewer than
        min_ratio * (reference points) points of the frame; (0, 1), the default, never fires.  Callable at any time"""
        thr = (float(min_ratio), int(lost_after))
        if not (0.0 <= thr[0] <= 1.0) or thr[1] < 1:
            raise PftError(1, "setMatchThreshold: min_ratio in [0, 1], lost_after >= 1")
        if self._h is not None:
            self._check(self._L.pft_set_match_threshold(self._h, thr[0], thr[1]))
        self._match_thr = thr

    def getMatchThreshold(self):
        return self._match_thr

    def computeMatch(self):
        """enqueues the match statistics of the last compute() on the tracker's stream; nothing waits"""
        if self._h is None:
            raise PftError(7, "computeMatch before the first compute()")
        self._check(self._L.pft_match(self._h))

    def getMatch(self):
        """waits for the last computeMatch(); returns MatchStats"""
        if self._h is None:
            raise PftError(7, "getMatch before the first compute()")
        r = _lib.MatchStatsStruct()
        self._check(self._L.pft_get_match(self._h, C.byref(r)))
        return MatchStats.from_struct(r)

    def getMatchPairs(self):
        """the pairs of the last computeMatch(), per reference point in the order of setReferenceCloud: (input_idx int32 --
        the partner's index in the frame's input cloud, -1 if not matched --, sq_dist float32 -- the neighbour's squared
        distance whether matched or not, inf for an empty crop)"""
        if self._h is None:
            raise PftError(7, "getMatchPairs before the first compute()")
        n = C.c_size_t()
        self._check(self._L.pft_get_match_pairs(self._h, None, None, 0, C.byref(n)))
        idx = np.zeros(n.value, np.int32)
        d2 = np.zeros(n.value, np.float32)
        self._check(self._L.pft_get_match_pairs(self._h, _ptr(idx), _ptr(d2), n.value, C.byref(n)))
        return idx, d2

    def isLost(self):
        """the lost flag of the last computeMatch() (waits for it)"""
        return self.getMatch().lost

    def resetTracking(self):
        """pcl::tracking::ParticleFilterTracker::resetTracking(): the next compute() is a first frame around the trans
        in force then; the change detector keeps its state, the lost rule's streak is cleared"""
        if self._h is not None:
            self._check(self._L.pft_reset_tracking(self._h))

    # ---- population statistics and the spread rule ----
    def setSpreadThreshold(self, max_pos_sigma=float("inf"), min_n_eff=0.0, after=1):
        """the pose counts as uncertain after `after` evaluated computeSpread() calls in a row whose largest position sigma
        exceeded max_pos_sigma (metres) or whose effective sample size fell below min_n_eff; (inf, 0, 1), the default,
        never fires.  Callable at any time"""
        thr = (float(max_pos_sigma), float(min_n_eff), int(after))
        if not (thr[0] >= 0.0) or not (thr[1] >= 0.0) or thr[2] < 1:
            raise PftError(1, "setSpreadThreshold: max_pos_sigma >= 0, min_n_eff >= 0, after >= 1")
        if self._h is not None:
            self._check(self._L.pft_set_spread_threshold(self._h, thr[0], thr[1], thr[2]))
        self._spread_thr = thr

    def getSpreadThreshold(self):
        return self._spread_thr

    def computeSpread(self):
        """enqueues the statistics of the population compute() left on the device; nothing waits"""
        if self._h is None:
            raise PftError(7, "computeSpread before the first compute()")
        self._check(self._L.pft_spread(self._h))

    def getSpread(self):
        """waits for the last computeSpread(); returns PopulationStats"""
        if self._h is None:
            raise PftError(7, "getSpread before the first compute()")
        r = _lib.PopulationStatsStruct()
        self._check(self._L.pft_get_spread(self._h, C.byref(r)))
        return PopulationStats.from_struct(r)

    def isUncertain(self):
        """the flag of the spread rule after the last computeSpread() (waits for it)"""
        return self.getSpread().flagged

    # ---- visibility of the model at a pose, the occlusion-aware lost rule ----
    def setVisibilityCamera(self, width=160, height=90, fx=90.0, fy=90.0, cx=79.5, cy=44.5, z_near=0.05, splat=1,
                            occlusion_margin=0.03, self_margin=0.03):
        """the pinhole camera at the origin, looking along +z, that computeVisibility() renders its two depth images with
        (the default: a Kinect2 qhd camera divided by six), the splat half-width and the two depth margins in metres"""
        c = _lib.VisibilityConfig(int(width), int(height), float(fx), float(fy), float(cx), float(cy), float(z_near),
                                  int(splat), float(occlusion_margin), float(self_margin))
        if self._h is not None:
            self._check(self._L.pft_set_visibility_camera(self._h, C.byref(c)))
        else:  # (the library's refusals, before there is a handle to ask)
            ok = (1 <= c.width <= 1024 and 1 <= c.height <= 1024 and 0 <= c.splat <= 4 and
                  all(np.isfinite(v) for v in (c.fx, c.fy, c.cx, c.cy, c.z_near, c.occlusion_margin, c.self_margin)) and
                  c.fx > 0 and c.fy > 0 and c.z_near >= 0 and c.occlusion_margin >= 0 and c.self_margin >= 0)
            if not ok:
                raise PftError(1, "setVisibilityCamera: a value outside its range (include/pft_visibility.h)")
        self._vis_cam = c

    def getVisibilityCamera(self):
        """the camera in force as a dict of pft_visibility_config's fields"""
        c = _lib.VisibilityConfig()
        if self._h is not None:
            self._check(self._L.pft_get_visibility_camera(self._h, C.byref(c)))
        elif self._vis_cam is not None:
            c = self._vis_cam
        else:
            self._L.pft_visibility_config_default(C.byref(c))
        return {f: getattr(c, f) for f, _ in c._fields_}

    def setVisibilityThreshold(self, min_visible_ratio=0.25, min_ratio=0.0, lost_after=1):
        """the object counts as hidden while fewer than min_visible_ratio * (reference points) are visible, and as lost
        after `lost_after` evaluated, matched, not hidden frames in a row in which fewer than min_ratio * (visible points)
        of the visible points were matched; (0.25, 0, 1), the default, never fires.  Callable at any time"""
        thr = (float(min_visible_ratio), float(min_ratio), int(lost_after))
        if not (0.0 <= thr[0] <= 1.0) or not (0.0 <= thr[1] <= 1.0) or thr[2] < 1:
            raise PftError(1, "setVisibilityThreshold: min_visible_ratio and min_ratio in [0, 1], lost_after >= 1")
        if self._h is not None:
            self._check(self._L.pft_set_visibility_threshold(self._h, *thr))
        self._vis_thr = thr

    def getVisibilityThreshold(self):
        return self._vis_thr

    def computeVisibility(self, matrix=None):
        """enqueues the visibility of the reference cloud against the current input cloud on the tracker's stream; nothing
        waits.  matrix: a 3x4 (or 4x4) float transform; None: the result pose of the last compute()"""
        if matrix is None:
            if self._h is None:
                raise PftError(7, "computeVisibility before the first compute()")
            self._check(self._L.pft_visibility(self._h, None))
            return
        self._ensure()
        m = np.ascontiguousarray(np.asarray(matrix, np.float32).reshape(-1)[:12])
        if m.size != 12:
            raise PftError(1, "computeVisibility: the matrix must have 3x4 or 4x4 entries")
        self._check(self._L.pft_visibility(self._h, _ptr(m)))

    def getVisibility(self):
        """waits for the last computeVisibility(); returns VisibilityStats"""
        if self._h is None:
            raise PftError(7, "getVisibility before the first computeVisibility()")
        r = _lib.VisibilityStatsStruct()
        self._check(self._L.pft_get_visibility(self._h, C.byref(r)))
        return VisibilityStats.from_struct(r)

    def getVisibilityPoints(self):
        """per reference point in the order of setReferenceCloud: (state uint8 -- 0 visible, 1 occluded by the scene,
        2 occluded by the model itself, 3 out of view --, scene_gap float32, self_gap float32)"""
        if self._h is None:
            raise PftError(7, "getVisibilityPoints before the first computeVisibility()")
        n = C.c_size_t()
        self._check(self._L.pft_get_visibility_points(self._h, None, None, None, 0, C.byref(n)))
        st = np.zeros(n.value, np.uint8)
        sg = np.zeros(n.value, np.float32)
        mg = np.zeros(n.value, np.float32)
        self._check(self._L.pft_get_visibility_points(self._h, _ptr(st), _ptr(sg), _ptr(mg), n.value, C.byref(n)))
        return st, sg, mg

    def isOccluded(self):
        """the hidden flag of the last computeVisibility() (waits for it)"""
        return self.getVisibility().hidden

    def isLostVisible(self):
        """the lost flag of the occlusion-aware rule after the last computeVisibility() (waits for it)"""
        return self.getVisibility().lost

    # ---- the view-dependent reference: a full model's visible side as the reference cloud ----
    def selectView(self, model, matrix=None, max_points=0):
        """enqueues the selection of the points of `model` that the visibility camera sees at `matrix` (3x4 or 4x4; None:
        the result pose of the last compute()); nothing waits.  model: a host cloud, a (device pointer, count) pair, or a
        ModelGrowth (its grown model, device to device).  max_points: 0 = no limit"""
        if matrix is None:
            if self._h is None:
                raise PftError(7, "selectView without a matrix before the first compute()")
            m = None
        else:
            self._ensure()
            m = np.ascontiguousarray(np.asarray(matrix, np.float32).reshape(-1)[:12])
            if m.size != 12:
                raise PftError(1, "selectView: the matrix must have 3x4 or 4x4 entries")
        if hasattr(model, "modelDevice"):
            p, n = model.modelDevice()  # (waits for the growth handle's stream)
            self._view_keep = model
            self._check(self._L.pft_view_select_device(self._h, C.c_void_p(p), n, _ptr(m), int(max_points)))
        elif isinstance(model, tuple):
            p, n = model
            self._view_keep = None
            self._check(self._L.pft_view_select_device(self._h, C.c_void_p(int(p)), int(n), _ptr(m), int(max_points)))
        else:
            cloud = np.ascontiguousarray(model, POINT_DTYPE)
            self._view_keep = cloud
            self._check(self._L.pft_view_select(self._h, _ptr(cloud), len(cloud), _ptr(m), int(max_points)))

    def getView(self):
        """waits for the last selectView(); returns ViewStats"""
        if self._h is None:
            raise PftError(7, "getView before the first selectView()")
        r = _lib.ViewStatsStruct()
        self._check(self._L.pft_get_view(self._h, C.byref(r)))
        return ViewStats.from_struct(r)

    def getViewPoints(self):
        """per model record: (state uint8 -- 0 kept, 1 decimated, 2 occluded by the model itself, 3 out of view, 4 not
        finite --, self_gap float32)"""
        if self._h is None:
            raise PftError(7, "getViewPoints before the first selectView()")
        n = C.c_size_t()
        self._check(self._L.pft_get_view_points(self._h, None, None, 0, C.byref(n)))
        st = np.zeros(n.value, np.uint8)
        gap = np.zeros(n.value, np.float32)
        self._check(self._L.pft_get_view_points(self._h, _ptr(st), _ptr(gap), n.value, C.byref(n)))
        return st, gap

    def getViewIndices(self):
        """the kept records' indices into the model, ascending (uint32)"""
        if self._h is None:
            raise PftError(7, "getViewIndices before the first selectView()")
        n = C.c_size_t()
        self._check(self._L.pft_get_view_indices(self._h, None, 0, C.byref(n)))
        idx = np.zeros(n.value, np.uint32)
        self._check(self._L.pft_get_view_indices(self._h, _ptr(idx), n.value, C.byref(n)))
        return idx

    def getViewCloud(self):
        """the kept records, whole, in index order"""
        if self._h is None:
            raise PftError(7, "getViewCloud before the first selectView()")
        n = C.c_size_t()
        self._check(self._L.pft_get_view_cloud(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, POINT_DTYPE)
        self._check(self._L.pft_get_view_cloud(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def viewCloudDevice(self):
        """(device pointer, n): the view cloud in HBM, valid until the next selectView()"""
        if self._h is None:
            raise PftError(7, "viewCloudDevice before the first selectView()")
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.pft_view_cloud_device(self._h, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def setReferenceFromView(self, min_points=1):
        """the view cloud of the last selectView() becomes the reference cloud (waits).  The object is the same: the lost,
        visibility and spread rules keep their streaks.  PftError(7), the old reference still in force, when the view keeps
        fewer than max(min_points, 1) points, was not evaluated, or has been consumed already"""
        if self._h is None:
            raise PftError(7, "setReferenceFromView before the first selectView()")
        self._check(self._L.pft_set_reference_from_view(self._h, int(min_points)))
        self._ref = self.getViewCloud()  # what a later close() and re-creation hands to the new handle

    def debugSetViewGrid(self, blocks):
        """test hook: the workgroups of every pass of the selectView() calls that follow (0: the default)"""
        self._ensure()
        self._check(self._L.pft_debug_set_view_grid(self._h, int(blocks)))

    # ---- re-acquisition of a lost object ----
    def reacquire(self, centres=None, segmenter=None, n=(1, 1, 8), span=(0.0, 0.0, 2.0 * np.pi), base_rpy=None,
                  inlier_distance=0.02, accept_ratio=0.5, apply=True, refine=False):
        """scores every centre x every orientation of the lattice (n = steps of roll, pitch, yaw over `span` around
        base_rpy; None: the angles of the current trans) against the current input cloud and returns the best candidate as
        a ReacquireResult.  centres: (k, 3) positions; or segmenter: a ModelSegmenter that has been applied -- the centroids
        of its clusters, formed on the device.  apply=True and an accepted candidate: setTrans(result.trans) +
        resetTracking().  refine=True: the lattice call only selects; its best transform is refined (refine(), the
        defaults), and of an accepted candidate the refined pose is applied if the refinement improved it, else the
        candidate's own (result.refined holds the RefineResult).  Synchronous"""
        if (centres is None) == (segmenter is None):
            raise PftError(1, "reacquire: give either centres or a segmenter")
        self._ensure()
        cfg = _lib.ReacquireConfig()
        self._L.pft_reacquire_config_default(C.byref(cfg))
        cfg.n_roll, cfg.n_pitch, cfg.n_yaw = (int(v) for v in n)
        if base_rpy is None:
            st = np.zeros(1, PARTICLE_DTYPE)
            self._L.pft_to_state(_ptr(self._trans), _ptr(st))
            base_rpy = (st[0]["roll"], st[0]["pitch"], st[0]["yaw"])
        for a in range(3):
            cfg.base_rpy[a] = float(base_rpy[a])
            cfg.span_rpy[a] = float(span[a])
        cfg.inlier_distance = float(inlier_distance)
        cfg.accept_ratio = float(accept_ratio)
        cfg.apply = 1 if (apply and not refine) else 0
        r = _lib.ReacquireResultStruct()
        if segmenter is not None:
            if segmenter._h is None:
                raise PftError(7, "reacquire: the segmenter has not been applied yet")
            self._check(self._L.pft_reacquire_from_segmenter(self._h, segmenter._h, C.byref(cfg), C.byref(r)))
        else:
            c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
            self._check(self._L.pft_reacquire(self._h, _ptr(c), len(c), C.byref(cfg), C.byref(r)))
        res = ReacquireResult.from_struct(r)
        self._rq_centres = res.n_centres  # getReacquireScores sizes its centre array by it
        if refine and res.best >= 0:
            res.refined = self.refine(start=res.transform, apply=bool(apply and res.accepted))
            if apply and res.accepted:
                if not res.refined.applied:
                    self.setTrans(res.trans)
                    self.resetTracking()
                res.applied = True
                return res
        if res.applied:
            self._trans = res.trans  # what a later close() and re-creation hands to the new handle
        return res

    # ---- refinement of a pose against the frame ----
    def refine(self, start=None, max_iterations=16, pair_distance=None, inlier_distance=0.02, margin=None, trans_eps=1e-4,
               rot_eps=1e-3, min_pairs=3, apply=False):
        """point-to-point ICP from `start` (3x4 or 4x4; None: the last result pose) against the current input cloud, all
        iterations on the device; returns a RefineResult.  pair_distance None: the tracker's max_distance; margin None:
        pair_distance.  apply=True and an improved pose: setTrans(result.trans) + resetTracking().  Synchronous"""
        self._ensure()
        cfg = _lib.RefineConfig()
        self._L.pft_refine_config_default(C.byref(cfg))
        cfg.max_iterations, cfg.min_pairs = int(max_iterations), int(min_pairs)
        cfg.pair_distance = 0.0 if pair_distance is None else float(pair_distance)
        cfg.inlier_distance = float(inlier_distance)
        cfg.margin = 0.0 if margin is None else float(margin)
        cfg.trans_eps, cfg.rot_eps = float(trans_eps), float(rot_eps)
        cfg.apply = 1 if apply else 0
        s = None
        if start is not None:
            s = np.asarray(start, np.float32)
            if s.shape not in ((3, 4), (4, 4), (12,), (16,)):
                raise PftError(1, "refine: start must be a 3x4 or 4x4 matrix")
            s = np.ascontiguousarray(s.reshape(-1)[:12])
        r = _lib.RefineResultStruct()
        self._check(self._L.pft_refine(self._h, _ptr(s), C.byref(cfg), C.byref(r)))
        res = RefineResult.from_struct(r)
        if res.applied:
            self._trans = res.trans
        return res

    def getRefineTrace(self):
        """the passes of the last refine(): dict(transform (n, 3, 4) float32, n_pairs, n_inliers (uint32), sums (n, 17),
        step_t2, step_r2 (float64)), n = iterations + 1"""
        if self._h is None:
            raise PftError(7, "getRefineTrace before the first refine()")
        n = C.c_size_t()
        self._check(self._L.pft_get_refine_trace(self._h, None, 0, C.byref(n)))
        e = (_lib.RefineTraceEntry * max(n.value, 1))()
        self._check(self._L.pft_get_refine_trace(self._h, C.cast(e, C.c_void_p), n.value, C.byref(n)))
        e = e[:n.value]
        return dict(transform=np.array([list(x.transform) for x in e], np.float32).reshape(-1, 3, 4),
                    n_pairs=np.array([x.n_pairs for x in e], np.uint32), n_inliers=np.array([x.n_inliers for x in e], np.uint32),
                    sums=np.array([list(x.sums) for x in e], np.float64).reshape(-1, 17),
                    step_t2=np.array([x.step_t2 for x in e], np.float64), step_r2=np.array([x.step_r2 for x in e], np.float64))

    def getReacquireScores(self):
        """the candidates and scores of the last reacquire(), in candidate order: dict(candidates (PARTICLE_DTYPE), mats
        (K, 3, 4), n_inliers, n_matched (uint32), coherence, sum_sq_dist, inlier_sq_dist (float64), centres (k, 3))"""
        if self._h is None:
            raise PftError(7, "getReacquireScores before the first reacquire()")
        n = C.c_size_t()
        self._check(self._L.pft_get_reacquire_scores(self._h, None, None, None, None, None, None, None, None, 0, C.byref(n)))
        K = n.value
        out = dict(candidates=np.zeros(K, PARTICLE_DTYPE), mats=np.zeros((K, 3, 4), np.float32),
                   n_inliers=np.zeros(K, np.uint32), n_matched=np.zeros(K, np.uint32), coherence=np.zeros(K, np.float64),
                   sum_sq_dist=np.zeros(K, np.float64), inlier_sq_dist=np.zeros(K, np.float64))
        nc = self._rq_centres
        centres = np.zeros((max(nc, 1), 3), np.float32)
        self._check(self._L.pft_get_reacquire_scores(
            self._h, _ptr(out["candidates"]), _ptr(out["mats"]), _ptr(out["n_inliers"]), _ptr(out["n_matched"]),
            _ptr(out["coherence"]), _ptr(out["sum_sq_dist"]), _ptr(out["inlier_sq_dist"]), _ptr(centres), K, C.byref(n)))
        out["centres"] = centres[:nc].copy()
        return out

    # ---- test hooks (stage-level parity against the oracle) ----
    def setParticles(self, p):
        self._ensure()
        p = np.ascontiguousarray(p, PARTICLE_DTYPE)
        self._check(self._L.pft_set_particles(self._h, _ptr(p), len(p)))

    def evalWeights(self, particles, want_nn=False):
        self._ensure()
        p = np.ascontiguousarray(particles, PARTICLE_DTYPE)
        P, M = len(p), len(self._ref)
        raw = np.zeros(P, np.float32)
        nn_idx = np.zeros((P, M), np.int32) if want_nn else None
        nn_d2 = np.zeros((P, M), np.float32) if want_nn else None
        self._check(self._L.pft_eval_weights(self._h, _ptr(p), P, _ptr(raw), _ptr(nn_idx), _ptr(nn_d2)))
        bbox = np.zeros(6, np.float32)
        self._check(self._L.pft_debug_get_bbox(self._h, _ptr(bbox)))
        n = C.c_size_t()
        self._check(self._L.pft_debug_get_crop(self._h, None, 0, C.byref(n)))
        crop = np.zeros(n.value, np.int32)
        if n.value:
            self._check(self._L.pft_debug_get_crop(self._h, _ptr(crop), n.value, C.byref(n)))
        depth, nl, nn = C.c_int32(), C.c_uint32(), C.c_uint32()
        mn, mx = np.zeros(3), np.zeros(3)
        self._check(self._L.pft_debug_get_octree(self._h, C.byref(depth), _ptr(mn), _ptr(mx), C.byref(nl), C.byref(nn)))
        keys = np.zeros((n.value, 3), np.uint32)
        if n.value:
            self._check(self._L.pft_debug_get_point_keys(self._h, _ptr(keys), n.value))
        q, s = C.c_uint64(), C.c_uint64()
        self._check(self._L.pft_debug_get_scan_stats(self._h, C.byref(q), C.byref(s)))
        lay = np.zeros(4, np.uint32)
        self._check(self._L.pft_debug_get_likelihood_layout(self._h, _ptr(lay)))
        return dict(raw=raw, nn_idx=nn_idx, nn_d2=nn_d2, bbox=bbox, crop_idx=crop, octree_depth=depth.value,
                    octree_min=mn, octree_max=mx, n_leaves=nl.value, n_words=nn.value, point_keys=keys,
                    scan_queries=q.value, scan_points=s.value, lik_layout=decode_likelihood_layout(lay))

    def debugChangeState(self, which=0):
        """the change detector's state: dict(gate, counter, box (min xyz, max xyz), depth, ring (k, 5): tested, changed,
        new voxels, new points, counter after -- oldest first --, n_calls).  which=1: the instance of debugChangeDetect"""
        self._ensure()
        gate, counter, n_calls = C.c_uint32(), C.c_uint32(), C.c_uint32()
        depth = C.c_int32()
        box = np.zeros(6, np.float64)
        ring = np.zeros((_lib.PFT_CD_RING, 5), np.uint32)
        self._check(self._L.pft_debug_change_state(self._h, which, C.byref(gate), C.byref(counter), _ptr(box),
                                                   C.byref(depth), _ptr(ring), C.byref(n_calls)))
        k = min(n_calls.value, _lib.PFT_CD_RING)
        return dict(gate=gate.value, counter=counter.value, box=box, depth=depth.value, ring=ring[:k].copy(),
                    n_calls=n_calls.value)

    def debugChangeDetect(self, cloud, min_points, resolution, reset):
        """one change-detector test on an explicit cloud (an instance apart from the tracker's) -> indices of the points
        in new voxels of at least min_points points, ascending"""
        self._ensure()
        cloud = np.ascontiguousarray(cloud, POINT_DTYPE)
        out = np.zeros(max(len(cloud), 1), np.uint32)
        n = C.c_size_t()
        self._check(self._L.pft_debug_change_detect(self._h, _ptr(cloud), len(cloud), int(min_points), float(resolution),
                                                    int(bool(reset)), _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def debugSetLimits(self, max_words=0, sorted_npass=0):
        """error-path tests: lower the octree node capacity / fix the sorted builder's radix passes"""
        self._ensure()
        self._check(self._L.pft_debug_set_limits(self._h, int(max_words), int(sorted_npass)))

    def debugSetExactLimits(self, ec_slots):
        """NearestPairPointCloudCoherence handles: lower the candidate-list slots handed out per iteration (never above the
        allocation); cells beyond the limit take the shell search"""
        self._ensure()
        self._check(self._L.pft_debug_set_exact_limits(self._h, int(ec_slots)))

    def debugExactState(self):
        """the exact-NN search structure after the last iteration (pft_debug_get_exact_state): eg_g, eg_dim, eg_min, eg_ncells,
        n_crop, ec_nslots, ec_pool_used, ec_pool_cap, eq_queries / eq_blocks (the halves of eq_totals), the capacities in force
        (ec_slots_cap, eg_cap, eq_tiles_cap, eq_cap) and compiled in (EC_SLOTS, EC_POOL, EG_CAP, EC_POOL_MIN), num_cus; the
        route counters of the last evalWeights(want_nn=True) (window_full, inline_shell, inline_empty, lik_shell, outside,
        lik_queries, lik_listed, lik_outside); ec_cells / ec_count / ec_base per placed slot, eg_start [eg_ncells + 1],
        leaf_order [n_crop]"""
        self._ensure()
        info = np.zeros(_lib.PFT_EXACT_STATE_WORDS, np.uint32)
        ctr = np.zeros(8, np.uint64)
        self._check(self._L.pft_debug_get_exact_state(self._h, _ptr(info), _ptr(ctr), None, None, None, 0, None, 0, None, 0))
        n_crop, ncells = int(info[8]), int(info[7])
        ns = min(int(info[9]), int(info[14]))
        cells, count, base = (np.zeros(ns, np.uint32) for _ in range(3))
        start = np.zeros(ncells + 1 if n_crop else 0, np.uint32)
        order = np.zeros(n_crop, np.uint32)
        self._check(self._L.pft_debug_get_exact_state(self._h, _ptr(info), None, _ptr(cells), _ptr(count), _ptr(base), ns,
                                                      _ptr(start), len(start), _ptr(order), n_crop))
        names = ("window_full", "inline_shell", "inline_empty", "lik_shell", "outside", "lik_queries", "lik_listed", "lik_outside")
        out = {k: int(v) for k, v in zip(names, ctr)}
        out.update(eg_g=float(info[0:1].view(np.float32)[0]), eg_dim=info[1:4].astype(np.int64), eg_min=info[4:7].view(np.float32).copy(),
                   eg_ncells=ncells, n_crop=n_crop, ec_nslots=int(info[9]), ec_pool_used=int(info[10]), ec_pool_cap=int(info[11]),
                   eq_queries=int(info[12]), eq_blocks=int(info[13]), ec_slots_cap=int(info[14]), eg_cap=int(info[15]),
                   eq_tiles_cap=int(info[16]), eq_cap=int(info[17]), EC_SLOTS=int(info[18]), EC_POOL=int(info[19]),
                   EG_CAP=int(info[20]), EC_POOL_MIN=int(info[21]), num_cus=int(info[22]),
                   ec_cells=cells, ec_count=count, ec_base=base, eg_start=start, leaf_order=order)
        return out

    def debugGetTree(self):
        """the linearised octree of the last build (pft_debug_get_tree): the header fields as ints (margin_cells, inv_res
        and ominf as float bits), lvl_start [depth + 2], words [n_words], leaf_order [n_crop], leaf_pts and crop_pts
        (n_crop, 4) uint32 records, jump: the whole uint16 allocation"""
        self._ensure()
        info = np.zeros(_lib.PFT_TREE_INFO_WORDS, np.uint32)
        self._check(self._L.pft_debug_get_tree(self._h, _ptr(info), None, 0, None, 0, None, 0, None, 0, None, 0))
        n, n_words, n_jump = int(info[0]), int(info[4]), int(info[19])
        words = np.zeros(n_words, np.uint32)
        order = np.zeros(n, np.uint32)
        leaf_pts = np.zeros((n, 4), np.uint32)
        crop_pts = np.zeros((n, 4), np.uint32)
        jump = np.zeros(n_jump, np.uint16)
        self._check(self._L.pft_debug_get_tree(self._h, _ptr(info), _ptr(words), n_words, _ptr(order), n, _ptr(leaf_pts), n,
                                               _ptr(crop_pts), n, _ptr(jump), n_jump))
        names = ("n_crop", "error", "depth", "use_table", "n_words", "n_leaves", "leaf_start", "n_grow", "build_path",
                 "leaf_indirect", "jump_level", "margin_cells_bits", "inv_res_bits")
        out = {k: int(info[i]) for i, k in enumerate(names)}
        depth = out["depth"]
        out.update(ominf_bits=info[13:16].copy(), build_epoch=int(info[16]), build_variant=int(info[17]),
                   build_lds_bytes=int(info[18]), lvl_start=info[20:20 + depth + 2].copy() if depth > 0 else info[20:20].copy(),
                   words=words, leaf_order=order, leaf_pts=leaf_pts, crop_pts=crop_pts, jump=jump)
        return out

    def debugStateSave(self):
        """checkpoint of the filter state between two frames (HBM-resident)"""
        self._check(self._L.pft_debug_state_save(self._h))

    def debugStateRestore(self):
        """back to the checkpoint: one kernel on the handle's stream"""
        self._check(self._L.pft_debug_state_restore(self._h))

    def debugInjectError(self, bits):
        """error-path tests: OR `bits` into the device-side error flags right after the next crop launch"""
        self._ensure()
        self._check(self._L.pft_debug_inject_error(self._h, int(bits)))

    def debugHostStat(self):
        """the pinned status block: last crop size, last depth, flags of the last failed iteration, unreported flags"""
        self._ensure()
        out = np.zeros(4, np.uint32)
        self._check(self._L.pft_debug_get_host_stat(self._h, _ptr(out)))
        return out

    def debugAncestorLevel(self):
        """the ancestor table's level choice (pft_debug_get_ancestor_level): dict(status -- the pinned word of the last build --,
        bits_d1 / bits_d2 -- log2 cells of its window at depth - 1 / depth - 2, None: no window --, anc_up -- the level asked of
        the last build as depth - anc_up, 0: none --, instance -- ANC_UP of the last likelihood instance --, changes, graph_builds)"""
        self._ensure()
        o = np.zeros(5, np.uint32)
        self._check(self._L.pft_debug_get_ancestor_level(self._h, _ptr(o)))
        st = int(o[0])
        b1, b2 = st & 0xFF, (st >> 8) & 0xFF
        valid = bool(st >> 31)
        return dict(status=st, bits_d1=b1 if valid and b1 != 0xFF else None, bits_d2=b2 if valid and b2 != 0xFF else None,
                    anc_up=int(np.int32(o[1])), instance=int(np.int32(o[2])), changes=int(o[3]), graph_builds=int(o[4]))

    def debugNormalize(self, w):
        self._ensure()
        w = np.array(w, np.float32, copy=True)
        fr = C.c_double()
        self._check(self._L.pft_debug_normalize(self._h, _ptr(w), len(w), C.byref(fr)))
        return w, fr.value

    def debugNormalizePartials(self, partial):
        """test hook: normalizeWeight with the raw weights formed in the same launch from the (n, nchunk) likelihood
        partial sums -> (normalised weights, fit ratio)"""
        self._ensure()
        partial = np.ascontiguousarray(partial, np.float64)
        n, nchunk = partial.shape
        w = np.zeros(n, np.float32)
        fr = C.c_double()
        self._check(self._L.pft_debug_normalize_partials(self._h, _ptr(partial), nchunk, n, _ptr(w), C.byref(fr)))
        return w, fr.value

    def debugAlias(self, w):
        self._ensure()
        w = np.ascontiguousarray(w, np.float32)
        a = np.zeros(len(w), np.int32)
        q = np.zeros(len(w), np.float64)
        self._check(self._L.pft_debug_alias(self._h, _ptr(w), len(w), _ptr(a), _ptr(q)))
        return a, q

    def debugWeightedMean(self, p):
        self._ensure()
        p = np.ascontiguousarray(p, PARTICLE_DTYPE)
        out = np.zeros(1, PARTICLE_DTYPE)
        self._check(self._L.pft_debug_weighted_mean(self._h, _ptr(p), len(p), _ptr(out)))
        return out[0]

    def debugInitParticles(self, rep, id_offset, n_local):
        self._ensure()
        rep = np.ascontiguousarray(rep, PARTICLE_DTYPE).reshape(1)
        out = np.zeros(n_local, PARTICLE_DTYPE)
        self._check(self._L.pft_debug_init_particles(self._h, _ptr(rep), id_offset, n_local, _ptr(out)))
        return out

    def debugResample(self, old, a, q, rep, epoch, id_offset=0, n_local=None):
        self._ensure()
        old = np.ascontiguousarray(old, PARTICLE_DTYPE)
        a = np.ascontiguousarray(a, np.int32)
        q = np.ascontiguousarray(q, np.float64)
        rep = np.ascontiguousarray(rep, PARTICLE_DTYPE).reshape(1)
        n_local = len(old) if n_local is None else n_local
        out = np.zeros(n_local, PARTICLE_DTYPE)
        self._check(self._L.pft_debug_resample(self._h, _ptr(old), len(old), _ptr(a), _ptr(q), _ptr(rep), epoch,
                                               id_offset, n_local, _ptr(out)))
        return out

    def debugResamplePrefix(self, old, rep, epoch, id_offset=0, n_local=None, instance=1, want_mats=False):
        """test hook: the product resample instances (no explicit table: the prefix-sum form is built from old's weights
        as given).  instance 0 = one lane per particle, 1 = four lanes, 2 = four lanes fused with the bounding box (needs
        a reference cloud).  -> particles, or (particles, matrices (n_local, 3, 4)) with want_mats"""
        self._ensure()
        old = np.ascontiguousarray(old, PARTICLE_DTYPE)
        rep = np.ascontiguousarray(rep, PARTICLE_DTYPE).reshape(1)
        n_local = len(old) if n_local is None else n_local
        out = np.zeros(n_local, PARTICLE_DTYPE)
        m = np.zeros((n_local, 12), np.float32) if want_mats else None
        self._check(self._L.pft_debug_resample_prefix(self._h, _ptr(old), len(old), _ptr(rep), epoch, id_offset, n_local,
                                                      int(instance), _ptr(out), _ptr(m) if want_mats else None))
        return (out, m.reshape(n_local, 3, 4)) if want_mats else out

    def debugPoseToMatrix(self, p):
        self._ensure()
        p = np.ascontiguousarray(p, PARTICLE_DTYPE)
        m = np.zeros((len(p), 12), np.float32)
        self._check(self._L.pft_debug_pose_to_matrix(self._h, _ptr(p), len(p), _ptr(m)))
        return m.reshape(len(p), 3, 4)

    def debugPackReference(self, cloud):
        """test hook: the reference side's colour conversion (k_pack_reference, the handle's argument order) on an explicit
        cloud -> (n, 4) float32 records h / 180, s / 255, v / 255, 0.  The handle's reference cloud is not touched"""
        self._ensure()
        cloud = np.ascontiguousarray(cloud, POINT_DTYPE)
        out = np.zeros((len(cloud), 4), np.float32)
        self._check(self._L.pft_debug_pack_reference(self._h, _ptr(cloud), len(cloud), _ptr(out)))
        return out

    # ---- per-kernel HIP-event timing ----
    def profileEnable(self, on=True):
        self._ensure()
        self._check(self._L.pft_profile_enable(self._h, 1 if on else 0))

    def profileReset(self):
        self._check(self._L.pft_profile_reset(self._h))

    def profileGet(self):
        out = {}
        for k in range(_lib.K_COUNT):
            ms, n = C.c_double(), C.c_uint64()
            self._check(self._L.pft_profile_get(self._h, k, C.byref(ms), C.byref(n)))
            out[self._L.pft_kernel_name(k).decode()] = (ms.value, n.value)
        return out


class KLDAdaptiveParticleFilterOMPTracker(ParticleFilterTracker):
    """pcl::tracking::KLDAdaptiveParticleFilterOMPTracker<PointXYZRGBA, ParticleXYZRPY>: what auto_tracking.cpp runs
    unless use_fixed is set (:207-222, :821).  setParticleNum is the initial count; every resample draws until the
    KL bound is met (at most setMaximumParticleNum)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._cfg.kld_adaptive = 1

    def setMaximumParticleNum(self, n):
        self._cfg_guard()
        self._cfg.maximum_particle_num = int(n)

    def setDelta(self, d):
        self._cfg_guard()
        self._cfg.kld_delta = float(d)

    def setEpsilon(self, e):
        self._cfg_guard()
        self._cfg.kld_epsilon = float(e)

    def setBinSize(self, bin_size):
        """bin_size: the six pose steps (x, y, z, roll, pitch, yaw), a ParticleXYZRPY upstream"""
        self._cfg_guard()
        if hasattr(bin_size, "dtype") and bin_size.dtype == PARTICLE_DTYPE:
            bin_size = [float(np.asarray(bin_size).reshape(-1)[0][k]) for k in ("x", "y", "z", "roll", "pitch", "yaw")]
        for i in range(6):
            self._cfg.kld_bin_size[i] = float(bin_size[i])

    def debugKldResample(self, old, a, q, motion, epoch, want_mats=False):
        """test hook: the KLD resample alone, with an explicit alias table -> (particles, bins (n,6), k); a = q = None:
        the product instance, on the prefix-sum form built from old's weights as given.  want_mats: the launch also
        writes the matrices, as under compute() -> (particles, bins, k, matrices (n, 3, 4))"""
        self._ensure()
        old = np.ascontiguousarray(old, PARTICLE_DTYPE)
        if (a is None) != (q is None):
            raise PftError(1, "debugKldResample: a and q are given together or not at all")
        if a is not None:
            a = np.ascontiguousarray(a, np.int32)
            q = np.ascontiguousarray(q, np.float64)
        motion = np.ascontiguousarray(motion, PARTICLE_DTYPE).reshape(1)
        cap = self._cfg.maximum_particle_num
        out = np.zeros(cap, PARTICLE_DTYPE)
        bins = np.zeros((cap, 6), np.int32)
        n, k = C.c_uint32(), C.c_uint32()
        if want_mats:
            m = np.zeros((cap, 12), np.float32)
            self._check(self._L.pft_debug_kld_resample_mats(self._h, _ptr(old), len(old), _ptr(a), _ptr(q), _ptr(motion),
                                                            epoch, _ptr(out), _ptr(bins), C.byref(n), C.byref(k), _ptr(m)))
            return out[:n.value].copy(), bins[:n.value].copy(), k.value, m[:n.value].reshape(n.value, 3, 4).copy()
        self._check(self._L.pft_debug_kld_resample(self._h, _ptr(old), len(old), _ptr(a), _ptr(q), _ptr(motion), epoch,
                                                   _ptr(out), _ptr(bins), C.byref(n), C.byref(k)))
        return out[:n.value].copy(), bins[:n.value].copy(), k.value


def make_reference_tracker(particle_num=400, seed=1, kld=False, change_detector=None, **kw):
    """A tracker configured exactly as /root/reference/src/auto_tracking.cpp:187-254 does; kld=True takes the
    use_fixed == false branch (:207-222), the reference's runtime default.  change_detector=(interval, min_points,
    resolution) also turns PCL's change detector on (the reference leaves it off)."""
    if kld:
        t = KLDAdaptiveParticleFilterOMPTracker(threads=16, seed=seed, **kw)
        t.setMaximumParticleNum(500)
        t.setDelta(0.99)
        t.setEpsilon(0.2)
        t.setBinSize([0.1] * 6)
    else:
        t = ParticleFilterTracker(threads=16, seed=seed, **kw)
    step = [0.015 * 0.015] * 6
    step[3] *= 40.0
    step[4] *= 40.0
    step[5] *= 40.0
    t.setTrans(np.eye(4, dtype=np.float32))
    t.setStepNoiseCovariance(step)
    t.setInitialNoiseCovariance([0.00001] * 6)
    t.setInitialNoiseMean([0.0] * 6)
    t.setIterationNum(2)
    t.setParticleNum(particle_num)
    t.setResampleLikelihoodThr(0.00)
    t.setUseNormal(False)
    coherence = ApproxNearestPairPointCloudCoherence()
    coherence.addPointCoherence(DistanceCoherence())
    color = HSVColorCoherence()
    color.setWeight(0.1)
    coherence.addPointCoherence(color)
    coherence.setSearchMethod(OctreeSearch(0.01))
    coherence.setMaximumDistance(0.1)
    t.setCloudCoherence(coherence)
    if change_detector is not None:
        interval, min_points, resolution = change_detector
        t.setIntervalOfChangeDetection(interval)
        t.setMinPointsOfChangeDetection(min_points)
        t.setResolutionOfChangeDetection(resolution)
        t.setUseChangeDetector(True)
    return t

/*
 * pft.h -- C ABI of the MI355X-native particle-filter point-cloud tracker.
 *
 * Drop-in boundary for the ONE hot path of cmaestre/pcl_tracking: the
 *   pcl::tracking::ParticleFilter(OMP)Tracker<pcl::PointXYZRGBA, pcl::tracking::ParticleXYZRPY>
 * object that /root/reference/src/auto_tracking.cpp builds at :201-206, configures at :225-254,
 * feeds at :673-676 (setReferenceCloud / setTrans) and :691 (setInputCloud) and runs at :693
 * (compute()), reading the pose back at :309-310 (getResult / toEigenMatrix) and :270 (getParticles).
 * The reference has no FFI for this path (it calls the PCL C++ classes directly); each entry point
 * below names the PCL member call it replaces.  The header-only C++ mirror of those classes over
 * this ABI is pcl_tracking_amd/include/pft/particle_filter_tracker.hpp; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Plain C: POD structs in PCL's memory layout, raw pointers and sizes, int status codes.
 * Nothing throws across this boundary.  A handle is not re-entrant (the reference serialises its
 * callback under a mutex, auto_tracking.cpp:604).  All compute runs as HIP kernels on gfx950; there
 * is no CPU fallback: without a usable GPU pft_create() fails with PFT_ERR_NO_DEVICE.
 */
#ifndef PFT_H
#define PFT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFT_ABI_VERSION 5

/* pcl::PointXYZRGBA (32 B, 16-aligned): x,y,z,1.0f | rgba (bytes b,g,r,a) | 12 B pad */
typedef struct pft_point_xyzrgba {
  float x, y, z, w;
  uint32_t rgba;
  uint32_t pad[3];
} pft_point_xyzrgba;

/* pcl::tracking::ParticleXYZRPY (32 B, 16-aligned): x,y,z,1.0f | roll,pitch,yaw,weight */
typedef struct pft_particle {
  float x, y, z, w;
  float roll, pitch, yaw, weight;
} pft_particle;

typedef enum pft_status {
  PFT_OK = 0,
  PFT_ERR_INVALID_ARG = 1,
  PFT_ERR_NO_INPUT = 2,     /* compute() without an input cloud: PCL prints PCL_ERROR and returns */
  PFT_ERR_NO_REFERENCE = 3, /* compute() before setReferenceCloud */
  PFT_ERR_NO_DEVICE = 4,    /* no gfx950 GPU / HIP runtime unusable: there is no CPU fallback */
  PFT_ERR_HIP = 5,          /* a HIP call failed; see pft_last_error_string */
  PFT_ERR_CAPACITY = 6,     /* a size exceeds what the handle was created for */
  PFT_ERR_STATE = 7,        /* call not valid in the current state */
  PFT_ERR_LOST = 8          /* "object not recognized": the lost rule of pft_match fired (thrown by the C++ mirror's compute()
                               for the reference's catch (int), auto_tracking.cpp:692-696; no C entry point returns it) */
} pft_status;

/* One POD holding every parameter the reference sets (auto_tracking.cpp:187-253) plus PCL's
 * constructor defaults it relies on.  pft_config_default() fills the reference's values. */
typedef struct pft_config {
  uint32_t abi_version;        /* PFT_ABI_VERSION */
  int32_t device_id;           /* HIP device ordinal */
  void* stream;                /* hipStream_t to enqueue on (used when stream_is_external != 0; the null
                                  handle then means HIP's default stream) */
  int32_t stream_is_external;  /* 0: the handle creates its own non-blocking stream */
  int32_t particle_num;        /* setParticleNum            :231   400 */
  int32_t iteration_num;       /* setIterationNum           :229   2 */
  double step_noise_cov[6];    /* setStepNoiseCovariance    :226   0.015^2 (x40 for r,p,y) */
  double initial_noise_cov[6]; /* setInitialNoiseCovariance :227   1e-5 */
  double initial_noise_mean[6];/* setInitialNoiseMean       :228   0 */
  double alpha;                /* ParticleFilterTracker ctor default 15.0 */
  double resample_likelihood_thr; /* setResampleLikelihoodThr :232 (inert upstream; kept for API parity) */
  double max_distance;         /* coherence->setMaximumDistance :253  0.1 */
  double octree_resolution;    /* search::Octree(0.01)      :251 */
  double distance_weight;      /* DistanceCoherence default weight 1.0 */
  double hsv_weight;           /* HSVColorCoherence::setWeight :246  0.1 */
  double h_weight, s_weight, v_weight; /* HSVColorCoherence ctor defaults 1, 1, 0 */
  int32_t hsv_pcl180_argorder; /* 1 = RGB2HSV(Red, Blue, Green) as written in PCL 1.8.0 */
  int32_t use_normal;          /* setUseNormal :233; only 0 is supported */
  uint64_t seed;               /* key of the counter-based RNG (PCL's engines are time(0)-seeded) */
  /* multi-GPU sharding: this handle owns global particle ids [rank*P/world, (rank+1)*P/world) */
  int32_t rank, world_size;
  /* capacities (0 = grow on demand at set_reference / set_input) */
  uint32_t max_reference_points, max_input_points;
  /* KLDAdaptiveParticleFilterOMPTracker, the tracker auto_tracking.cpp runs unless use_fixed is set (:207-222, :821):
   * particle_num is then only the initial count; every resample draws until the KL bound is met */
  int32_t kld_adaptive;          /* 0: ParticleFilterOMPTracker (:203-204)   1: KLD-adaptive (:207-208) */
  int32_t maximum_particle_num;  /* setMaximumParticleNum :209   500 */
  double kld_delta;              /* setDelta              :210   0.99 */
  double kld_epsilon;            /* setEpsilon            :211   0.2 */
  double kld_bin_size[6];        /* setBinSize            :212-219  0.1 each */
  double motion_ratio;           /* ParticleFilterTracker ctor default 0.25 (used by the KLD resample only) */
  /* NearestPairPointCloudCoherence (true nearest neighbour) instead of ApproxNearestPair...: the alternative the
   * reference keeps commented out at auto_tracking.cpp:237-238, :249 */
  int32_t exact_nearest;
  /* order of the two population sums (normalizeWeight's weight sum, update()'s weighted mean):
   *   PFT_SUM_TREE  adjacent-pair trees in double: independent of how the population is split, fast at any size
   *   PFT_SUM_PCL   PCL's own order: index order, weights in double, pose components in float (one workgroup runs
   *                 the dependent chains; the poses then follow PCL's tracker bit for bit where the trig agrees) */
  int32_t sum_order;
} pft_config;

#define PFT_SUM_TREE 0
#define PFT_SUM_PCL 1

typedef struct pft_tracker pft_tracker;

void pft_config_default(pft_config* cfg);
const char* pft_status_string(int status);

/* new ParticleFilterOMPTracker<...>(threads) + the setters of :225-254 */
int pft_create(const pft_config* cfg, pft_tracker** out);
void pft_destroy(pft_tracker* t);
const char* pft_last_error_string(const pft_tracker* t);

/* tracker_->setReferenceCloud(cloud) :673 -- host pointer, PCL layout, copied */
int pft_set_reference(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n);
/* tracker_->setTrans(Eigen::Affine3f) :225, :674 -- row-major 4x4 */
int pft_set_trans(pft_tracker* t, const float m[16]);
/* tracker_->setInputCloud(cloud) :691 -- host pointer, copied to HBM before the call returns */
int pft_set_input(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n);
/* same, for a cloud already resident in HBM (device pointer, PCL layout; borrowed until the next
 * pft_set_input* call) */
int pft_set_input_device(pft_tracker* t, const void* device_pts, size_t n);
/* same, for the output of an input filter (pft_filters.h) whose apply may still be running: the tracker borrows the
 * filter's output cloud and the DEVICE word that holds its count, and its stream waits for the apply with an event --
 * no host count, no host wait.  Works after pft_filter_apply* and pft_filter_apply*_async alike.
 *   max_points bounds the count: buffers and the grids of the launches that follow the input size (the crop, the
 *   leaf gather of the octree builder, the exact-NN grid, the sorted builder) are sized by it.  0 = the size of the
 *   apply's input, which the output can never exceed.
 *   A device count above the bound: the first crop reads max_points points only, and the next call that synchronises
 *   returns PFT_ERR_CAPACITY (pft_last_error_string names pft_set_input_from_filter).  A device count of zero: the
 *   iterations run as with an empty crop, and the next call that synchronises returns PFT_ERR_NO_INPUT.
 *   The filter's output is read by the first crop of the frame only (pft_compute or pft_eval_weights), which copies what
 *   later crops need; the filter's next apply waits (on the device) for that crop of every tracker that borrowed the
 *   output.  An apply issued BEFORE that crop was enqueued invalidates the hand-off: the compute then returns
 *   PFT_ERR_NO_INPUT.  Either handle may be destroyed first.
 *   PFT_ERR_INVALID_ARG with a text: a sharded handle (world_size > 1), a filter on another device.  PFT_ERR_STATE: the
 *   filter has not been applied yet.  With PFT_GRAPH=1 such a frame is launched directly. */
struct pft_filter;
int pft_set_input_from_filter(pft_tracker* t, struct pft_filter* f, size_t max_points);
/* tracker_->compute() :693 -- first call runs initParticles; then iteration_num x
 * [resample, weight, update].  Asynchronous on the handle's stream. */
int pft_compute(pft_tracker* t);
/* tracker_->getResult() :309 -- synchronises the stream.  Like every call that synchronises (pft_get_particles,
 * pft_get_fit_ratio, pft_synchronize, pft_eval_weights) it also reports device-side failures of the iterations run
 * since the last such call: PFT_ERR_CAPACITY (octree node capacity, depth or bounding-box growth steps exceeded) or
 * PFT_ERR_HIP (the one-pass crop gave up waiting), pft_last_error_string naming the flag; after
 * pft_set_input_from_filter also PFT_ERR_CAPACITY / PFT_ERR_NO_INPUT for a device-side input count above its bound / of zero.  The affected iteration ran
 * without a target cloud (all likelihoods zero), so the pose returned with the error is the unweighted particle mean;
 * the flags are per iteration and the next pft_compute starts clean.  (PCL's compute() is void; the reference's caller
 * wraps it in try / catch, auto_tracking.cpp:692-696.) */
int pft_get_result(pft_tracker* t, pft_particle* out);
/* tracker_->getParticles() :270 -- copy-out of all particle_num particles (all ranks' shards) */
int pft_get_particles(pft_tracker* t, pft_particle* out, size_t cap, size_t* n);
/* tracker_->toEigenMatrix(result) :310 == pcl::getTransformation; host-side helper, row-major 4x4 */
void pft_to_matrix(const pft_particle* p, float m[16]);
/* ParticleXYZRPY::toState(Affine3f) */
void pft_to_state(const float m[16], pft_particle* out);
/* fit_ratio_ diagnostic (w_min of the last normalizeWeight) */
int pft_get_fit_ratio(pft_tracker* t, double* out);
int pft_synchronize(pft_tracker* t);

/* ---- change detection (ParticleFilterTracker::setUseChangeDetector, setIntervalOfChangeDetection,
 *      setMinPointsOfChangeDetection, setResolutionOfChangeDetection; PCL defaults 0, 10, 10, 0.01) ----
 * Callable at any time.  An iteration whose counter has run out tests the cropped cloud against the one tested last
 * (OctreePointCloudChangeDetector, double-buffered); a test that finds no new voxel with at least min_points points skips
 * the octree build, the likelihood, update() and the next resample, and only renormalises the weights it holds.  The
 * skip is decided on the device: pft_compute stays asynchronous.  The resolution is latched at the first pft_compute, as
 * PCL creates its detector there.  Single-GPU handles with the approximate coherence only: a sharded handle or the
 * exact-NN mode returns PFT_ERR_INVALID_ARG for use != 0. */
int pft_set_change_detector(pft_tracker* t, int use, int interval, int min_points, double resolution);
int pft_get_change_detector(pft_tracker* t, int* use, int* interval, int* min_points, double* resolution);
#define PFT_CD_RING 32
/* detector state (synchronises).  which = 0: the tracker's detector, 1: the instance of pft_debug_change_detect.
 * gate = changed_, box = {min xyz, max xyz} in double; ring receives up to PFT_CD_RING decisions, oldest first, 5 words each
 * {tested, changed, new voxels, new points, counter after}; *n_calls = decisions made in all (0 before the first) */
int pft_debug_change_state(pft_tracker* t, int which, uint32_t* gate, uint32_t* counter, double box[6], int32_t* depth,
                           uint32_t* ring, uint32_t* n_calls);
/* one test on an explicit cloud with a detector of its own (never the tracker's); reset != 0 starts that detector afresh
 * at `resolution` (otherwise the resolution of its last reset holds).  new_idx receives up to cap indices of the points
 * that lie in new voxels of at least min_points points, ascending; *n_new their number */
int pft_debug_change_detect(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n, int min_points, double resolution,
                            int reset, uint32_t* new_idx, size_t cap, size_t* n_new);

/* ---- object report (drawResult + viz_cb, auto_tracking.cpp:301-326, :432-470): the full-resolution model moved by the
 *      result pose, its centroid (the position the node publishes) and its principal-axis box (viz.addCube) ----
 * Opt-in per handle and computed on the device, after pft_compute, on the handle's stream:
 *   transform   pose_to_matrix(representative state) on the device (double cos / sin rounded to float), T[2][3] += -0.005f
 *   tracked     ((T0 x + T1 y) + T2 z) + T3 per row for every report point; the other fields are copied
 *   centroid    compute3DCentroid of the tracked cloud ([3] = 1)
 *   covariance  computeCovarianceMatrixNormalized (row-major, symmetric)
 *   eigenvalues SelfAdjointEigenSolver<Matrix3f>, ascending; axes = its eigenvectors with col 2 = col 0 x col 1 (row-major)
 *   box_*       getMinMax3D of the tracked cloud in the principal frame (p2w = [axes^T | -(axes^T centroid)]);
 *               box_centre = axes * (max + min) / 2 + centroid, box_quat = Quaternion(axes) {x, y, z, w}, box_size = max - min
 * The sums follow pft_config::sum_order: PFT_SUM_TREE adjacent-pair trees in float, PFT_SUM_PCL index-order float chains
 * (the centroid is then PCL's bit for bit whenever the transform is). */
typedef struct pft_object_report {
  float transform[16];   /* row-major 4x4, the offset included */
  float centroid[4];
  float covariance[9];
  float eigenvalues[3];
  float axes[9];
  float box_min[3], box_max[3], box_centre[3];
  float box_quat[4];
  float box_size[3];
  uint32_t n_points;
  uint32_t info;         /* 0 success, 1 the eigen solver did not converge within 90 iterations */
  uint32_t pad[1];
} pft_object_report;     /* 240 B */

/* reference_dict[obj] (:675): host pointer, copied; may be called again at any time.  PFT_ERR_INVALID_ARG for n == 0, a
 * non-finite coordinate, or a sharded handle (world_size > 1) */
int pft_set_report_cloud(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n);
/* :673-675 from a model-preparation handle (pft_model.h) whose last prepare succeeded: pft_set_reference with its
 * downsampled cloud and pft_set_trans with its trans; with set_report_cloud != 0 also pft_set_report_cloud with its
 * re-centred cloud, copied device to device.  The tracker is left exactly as those calls leave it when given the same
 * clouds from the host.  The refusals of pft_set_report_cloud hold, with its texts, and are decided before anything is
 * applied; PFT_ERR_STATE for a model not prepared, PFT_ERR_INVALID_ARG for a model on another device */
struct pft_model;
int pft_set_object_from_model(pft_tracker* t, struct pft_model* m, int set_report_cloud);
/* enqueues the report on the handle's stream (never synchronises); it reads the representative state on the device, so
 * it follows the pft_compute calls before it in stream order.  PFT_ERR_STATE before the first pft_compute or without a
 * report cloud */
int pft_report(pft_tracker* t);
/* synchronises and copies the last report out; device-side failures are reported as by pft_get_result */
int pft_get_report(pft_tracker* t, pft_object_report* out);
/* tracked_cloud_dict[obj] (:325): the report cloud moved by the last report's transform; *n = its size, up to cap copied */
int pft_get_tracked_cloud(pft_tracker* t, pft_point_xyzrgba* out, size_t cap, size_t* n);

/* ---- match statistics of the result pose, the lost rule, resetTracking ----
 * What a caller cannot learn from pft_get_fit_ratio (PCL's w_min of the best PARTICLE): how much of the model, moved by the
 * frame's RESULT, finds a partner in the frame.  Opt-in, one extra launch on the handle's stream after pft_compute; it reads
 * the representative state and the last iteration's tree on the device, so nothing synchronises.  For every reference point
 * p_j:  q = T p_j with T = pose_to_matrix(result) on the device (double cos / sin rounded to float, no -5 mm offset) and the
 * likelihood's float expression; (partner, d2) = approxNearestSearch of q in the tree the frame's last iteration built;
 * matched_j = (double)d2 < max_distance^2, the likelihood's gate; the pair's value DistanceCoherence x HSVColorCoherence.
 *   n_matched    sum of matched_j
 *   coherence    sum of matched_j x pair value   } adjacent-pair trees in double over the handle's stored order of the
 *   sum_sq_dist  sum of matched_j x (double)d2   } reference points, padded with +0.0: independent of the launch shape
 *   n_crop       points of the crop searched;  evaluated  1, or 0 when there was nothing to evaluate: the last iteration was
 *                skipped by the change detector or raised a device-side failure ("no target").  The other fields then keep
 *                the values of the last evaluated frame, the streak included.  An empty crop is evaluated: 0 matched.
 *   below        (double)n_matched < min_ratio * (double)n_reference
 *   streak       below ? streak + 1 : 0;   lost  streak >= lost_after;   calls  pft_match launches so far
 * The streak is cleared by pft_reset_tracking and pft_set_reference. */
typedef struct pft_match_stats {
  float    transform[12];                        /* row-major 3x4, the T used */
  double   coherence, sum_sq_dist;
  uint32_t n_reference, n_matched, n_crop, evaluated;
  uint32_t below, streak, lost, calls;
} pft_match_stats;                               /* 96 B */

/* min_ratio in [0, 1] (default 0: never below), lost_after >= 1 (default 1); read by the pft_match calls that follow */
int pft_set_match_threshold(pft_tracker* t, double min_ratio, int lost_after);
int pft_get_match_threshold(pft_tracker* t, double* min_ratio, int* lost_after);
/* enqueues the match of the last pft_compute (never synchronises).  PFT_ERR_INVALID_ARG with a text: a sharded handle
 * (world_size > 1), an exact-NN handle (that mode builds no octree).  PFT_ERR_STATE: before the first pft_compute, or after
 * anything that rebuilt the handle's tree for other particles since (pft_eval_weights, pft_set_particles,
 * pft_debug_state_restore, pft_set_reference, an input cloud that made the buffers grow) */
int pft_match(pft_tracker* t);
/* synchronises and copies the last match out; device-side failures are reported as by pft_get_result */
int pft_get_match(pft_tracker* t, pft_match_stats* out);
/* the pairs of the last match, per reference point in the CALLER's order: input_idx = index in the frame's input cloud of
 * the partner if matched, else -1; sq_dist = the neighbour's d2 whether matched or not (INFINITY for an empty crop).
 * Either array may be null; *n = the reference size, up to cap copied.  After an unevaluated match: the last evaluated one's
 * for this reference cloud (pft_set_reference forgets the pairs and the result fields of the block: until a match is
 * evaluated for the new cloud they read -1 / INFINITY and n_reference = its size, n_matched = 0).  PFT_ERR_STATE without a
 * pft_match since the reference cloud was last set */
int pft_get_match_pairs(pft_tracker* t, int32_t* input_idx, float* sq_dist, size_t cap, size_t* n);
/* ParticleFilterTracker::resetTracking(): the handle forgets its population.  The next pft_compute (pft_dist_begin_frame on
 * a sharded handle) is a first frame in every respect -- initParticles(true) around the trans in force then, the
 * first-frame schedule, motion zero, resample epoch 0, builder hints reset -- and the tracker then runs bit for bit like a
 * fresh handle with the same configuration, reference and trans on the same frames.  The change detector keeps its state,
 * as PCL keeps its detector.  One deliberate difference: PCL keeps changed_ and the stale motion_, and would resample the
 * fresh uniform population once before the first weight() */
int pft_reset_tracking(pft_tracker* t);

/* ---- re-acquisition of a lost object: candidate poses scored on the device ----
 * K = n_centres * n_roll * n_pitch * n_yaw candidate poses -- every centre (usually the cluster centroids of a fresh
 * segmentation of the current frame) with every orientation of a lattice -- are scored against the handle's current input
 * cloud, the best one is selected, and with `apply` the tracker is restarted there.  Synchronous, like model preparation:
 * re-acquisition is a rare event, not a per-frame cost.
 *   candidate k = ((c * n_roll + ir) * n_pitch + ip) * n_yaw + iy:  position = centre c, per axis
 *       angle = (float)((double)base + (double)span * (((double)i + 0.5) / (double)n - 0.5))
 *     (offset 0 for n = 1, symmetric otherwise, no duplicate at a full-circle span); T_k = pose_to_matrix on the device
 *   crop, tree  over the box of all K transformed reference clouds, by the handle's builders, as pft_eval_weights drives them
 *   per reference point p_j:  q = T_k p_j, (partner, d2) = the search of pft_match;
 *       matched_j = (double)d2 < max_distance^2,   inlier_j = (double)d2 < inlier_distance^2
 *   n_matched, n_inliers  integers;  coherence, sum_sq_dist  as pft_match forms them (the same bits for the same T and
 *       tree);  inlier_sq_dist = sum of inlier_j x (double)d2, the same adjacent-pair tree in double
 *   best      the largest n_inliers; ties: the smaller inlier_sq_dist (in double), then the lowest k
 *   accepted  K > 0 && n_inliers >= 1 && !((double)n_inliers < accept_ratio * (double)n_reference)
 * With apply != 0 and accepted: pft_set_trans(the 4x4 of `transform`) + pft_reset_tracking -- the handle is exactly what those
 * two calls leave.  Otherwise the population, the weights, the resample epoch and the match streak are left alone; like
 * pft_eval_weights the call rebuilds the handle's tree, so a pft_match before the next pft_compute returns PFT_ERR_STATE.
 * Device-side builder failures are reported as by pft_get_result; nothing is applied then.  Zero centres (or a segmenter
 * without clusters): PFT_OK with n_candidates = 0, best = -1, accepted = 0.
 * PFT_ERR_INVALID_ARG with a text: a sharded handle, an exact-NN handle, a bad configuration value, a non-finite centre, a
 * segmenter on another device.  PFT_ERR_CAPACITY: K above PFT_REACQUIRE_MAX_CANDIDATES.  PFT_ERR_STATE: a segmenter that was
 * never applied.  PFT_ERR_NO_INPUT / PFT_ERR_NO_REFERENCE as pft_compute. */
#define PFT_REACQUIRE_MAX_CANDIDATES 65536
typedef struct pft_reacquire_config {
  int32_t n_roll, n_pitch, n_yaw;           /* >= 1 each */
  float base_rpy[3], span_rpy[3];           /* finite, span >= 0 */
  double inlier_distance;                   /* 0 < . <= max_distance; default 0.02 */
  double accept_ratio;                      /* [0, 1]; default 0.5 */
  int32_t apply;                            /* accepted: pft_set_trans(best) + pft_reset_tracking */
} pft_reacquire_config;                     /* 64 B */

typedef struct pft_reacquire_result {
  uint32_t n_centres, n_candidates, n_reference, n_crop;
  int32_t best, best_centre;                /* -1 when K == 0 */
  pft_particle pose; float transform[12];   /* the best candidate and the T it was scored with (row-major 3x4) */
  uint32_t n_inliers, n_matched, accepted, applied;
  double coherence, sum_sq_dist, inlier_sq_dist;
} pft_reacquire_result;                     /* 144 B */

/* 1 x 1 x 8 orientations, base 0, span (0, 0, 2 pi): yaw over the full circle; 0.02, 0.5, apply = 1 */
void pft_reacquire_config_default(pft_reacquire_config* cfg);
/* centres_xyz: n_centres x 3 floats on the host */
int pft_reacquire(pft_tracker* t, const float* centres_xyz, size_t n_centres, const pft_reacquire_config* cfg,
                  pft_reacquire_result* out);
/* the centres are compute3DCentroid (PCL's serial float chains) of every cluster of the segmenter's last apply, formed on
 * the device from where the clusters lie in HBM, in cluster order */
struct pft_segment;
int pft_reacquire_from_segmenter(pft_tracker* t, struct pft_segment* s, const pft_reacquire_config* cfg,
                                 pft_reacquire_result* out);
/* the candidates and scores of the last re-acquisition call, in candidate order; every array is optional and receives
 * min(cap, K) elements (mats12: 12 floats each), centres_xyz all of the call's centres (3 floats each; room for them is the
 * caller's business: pft_reacquire_result::n_centres); *n = K.  PFT_ERR_STATE before the first call */
int pft_get_reacquire_scores(pft_tracker* t, pft_particle* cand, float* mats12, uint32_t* n_inliers, uint32_t* n_matched,
                             double* coherence, double* sum_sq_dist, double* inlier_sq_dist, float* centres_xyz,
                             size_t cap, size_t* n);

/* ---- refinement of a pose against the frame: iterated closest-point fit on the device ----
 * Point-to-point ICP from a start pose, against the handle's current input cloud, with the search of pft_match as the
 * pairing.  Opt-in and synchronous: all iterations are enqueued at once, the stop decision is taken on the device, the
 * host waits once.  Quaternions are {w, x, y, z}; all arithmetic is IEEE, unfused, left to right.
 *   state     a unit quaternion Q and a translation t, both double.  The start is a row-major 3x4 float matrix: Q by the
 *             Shoemake branches of Quaternion(Matrix3) evaluated in double, then normalised; t its last column.  NULL: the
 *             matrix of the last result pose, exactly the T pft_match stores (only after a pft_compute).
 *   T         pass 0 runs with the start matrix itself; after a solve T = ((float)R(Q), (float)t), R(Q) the usual
 *             polynomial (R00 = 1 - 2 (yy + zz), R01 = 2 (xy - wz), ...).  A solve whose step is exactly zero (dq the
 *             identity and t_new == c) leaves Q, t and T as they are.
 *   crop, tree  once per call, by the handle's builders as pft_reacquire drives them: the box of the reference cloud under
 *             the eight copies of the start shifted by (+-(float)margin, +-(float)margin, +-(float)margin); reported in `bbox`
 *   one pass, over the reference points p_j at positions 0 .. M-1 of the stored (Morton) order:
 *       q = T p_j;  (partner, d2) = the search of pft_match;  pair_j = (double)d2 < pair_distance^2,
 *       inlier_j = (double)d2 < inlier_distance^2;  pivot c = (double) of T's translation;  a = (double)q - c,
 *       b = (double)partner - c;  n_pairs, n_inliers integers;  17 sums, each the adjacent-pair tree in double over the
 *       positions padded with +0.0 (pft_match's tree; the terms are signed, a step is taken only inside the padded size):
 *       sums[0..2] = sum pair a_r,  [3..5] = sum pair b_r,  [6 + 3 r + c] = sum pair a_r b_c,  [15] = sum pair (double)d2,
 *       [16] = sum inlier (double)d2
 *   solve     am = A / n, bm = B / n, S = H - A B^T / n (S_rc = H_rc - A_r B_c / n), S divided by its largest absolute entry
 *             (1 if zero); Horn's symmetric 4x4 matrix of S; cyclic Jacobi sweeps over (0,1),(0,2),(0,3),(1,2),(1,3),(2,3),
 *             a pair whose off-diagonal entry is exactly 0 skipped, theta = (a_qq - a_pp) / (2 a_pq),
 *             t = +-1 / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c, until every off-diagonal entry is 0
 *             or 16 sweeps; dq = the normalised eigenvector of the largest diagonal entry (the first on ties) with w >= 0;
 *             Q <- normalise(dq (x) Q), t <- c + (bm - R(dq) am);  step_t2 = |t_new - c|^2, step_r2 = 4 (dq_x^2 + dq_y^2 +
 *             dq_z^2).  The quaternion form never returns a reflection
 *   loop      pass k evaluates T_k (k = 0: `before`).  n_pairs < min_pairs: TOO_FEW_PAIRS, nothing is solved, T is kept and
 *             this pass is also `after`.  Else solve (iterations = k + 1): CONVERGED when step_t2 < trans_eps^2 and
 *             step_r2 < rot_eps^2, else MAX_ITERATIONS at k + 1 == max_iterations; then one more pass gives `after`.
 *             The trace holds iterations + 1 entries, one per pass
 *   improved  after.n_inliers > before.n_inliers, or equal and after.inlier_sq_dist < before.inlier_sq_dist
 *   pose      pft_to_state of the final transform (its angles carry that function's float tolerance; `transform` is exact)
 * With apply != 0 and improved: pft_set_trans(the 4x4 of `transform`) + pft_reset_tracking, and nothing else.  Otherwise the
 * population, weights, epoch, change detector and streaks are left alone; like pft_reacquire the call rebuilds the handle's
 * tree, so a pft_match before the next pft_compute returns PFT_ERR_STATE.  Device-side builder failures are reported as by
 * pft_get_result; nothing is applied then.
 * PFT_ERR_INVALID_ARG with a text: a sharded handle, an exact-NN handle, a bad configuration value, a non-finite start.
 * PFT_ERR_STATE: a NULL start without a pft_compute.  PFT_ERR_NO_INPUT / PFT_ERR_NO_REFERENCE as pft_compute. */
#define PFT_REFINE_MAX_ITERATIONS 64
#define PFT_REFINE_N_SUMS 17
enum { PFT_REFINE_CONVERGED = 0, PFT_REFINE_MAX_ITERATIONS_REACHED = 1, PFT_REFINE_TOO_FEW_PAIRS = 2 };
typedef struct pft_refine_config {
  int32_t max_iterations;                   /* 1 .. PFT_REFINE_MAX_ITERATIONS; default 16 */
  int32_t min_pairs;                        /* >= 3; default 3 */
  double pair_distance;                     /* >= 0; 0 = the handle's max_distance */
  double inlier_distance;                   /* > 0; default 0.02 */
  double margin;                            /* >= 0; 0 = pair_distance */
  double trans_eps, rot_eps;                /* >= 0; defaults 1e-4 m, 1e-3 rad */
  int32_t apply;                            /* improved: pft_set_trans(final) + pft_reset_tracking; default 0 */
} pft_refine_config;                        /* 56 B */

typedef struct pft_refine_score {
  uint32_t n_pairs, n_inliers;
  double sum_sq_dist, inlier_sq_dist;
} pft_refine_score;                         /* 24 B */

typedef struct pft_refine_result {
  uint32_t status, iterations, n_reference, n_crop;
  double bbox[6];                           /* x_min, x_max, y_min, y_max, z_min, z_max of the crop */
  float start[12], transform[12];           /* the start and the final T (row-major 3x4) */
  pft_particle pose;
  pft_refine_score before, after;
  uint32_t improved, applied;
} pft_refine_result;                        /* 248 B */

typedef struct pft_refine_trace_entry {
  float transform[12];                      /* the T of the pass */
  uint32_t n_pairs, n_inliers;
  double sums[PFT_REFINE_N_SUMS];
  double step_t2, step_r2;                  /* of the solve that followed the pass; 0 when none did */
} pft_refine_trace_entry;                   /* 208 B */

/* 16, 3, 0, 0.02, 0, 1e-4, 1e-3, apply = 0 */
void pft_refine_config_default(pft_refine_config* cfg);
/* start12: row-major 3x4 floats on the host, or NULL for the matrix of the last result pose */
int pft_refine(pft_tracker* t, const float* start12, const pft_refine_config* cfg, pft_refine_result* out);
/* the passes of the last pft_refine call; receives min(cap, iterations + 1) entries, *n = iterations + 1.  PFT_ERR_STATE
 * before the first completed call */
int pft_get_refine_trace(pft_tracker* t, pft_refine_trace_entry* entries, size_t cap, size_t* n);

/* ---- population statistics: pose covariance, effective sample size, the spread rule ----
 * What neither the result pose nor its match statistics say: how sure the filter is.  Opt-in, enqueued on the handle's
 * stream after pft_compute, never synchronises; it reduces the population pft_get_particles would return (after the last
 * weight() / update() of the frame, weights normalised).  pft_compute itself is untouched.
 * Particles i = 0 .. n-1 (n = particle_num, or the device-side active count of a KLD handle; slots beyond it are not read),
 * w_i the float weight, p_ik the six float pose components x, y, z, roll, pitch, yaw, r the representative state in force
 * (what pft_get_result returns), the pivot that keeps the second moments from cancelling:  d_ik = (double)p_ik - (double)r_k.
 * All sums are adjacent-pair trees in double over the particle index 0 .. n-1 padded with +0.0 to a power of two (the tree
 * of update() in the default order), built from aligned subtrees only: the bits depend neither on the workgroup size nor
 * on the grid.  Unfused, as the library is built:
 *   sum_w   sum of (double)w_i               sum_w2  sum of (double)w_i * (double)w_i
 *   s[k]    sum of (double)w_i * d_ik        S[kl]   sum of ((double)w_i * d_ik) * d_il for k <= l, row by row (21 values)
 *   n, n_zero (particles with w_i == 0: PCL's "no correspondence"), w_max and i_max (the lowest index on a tie)
 * One lane then derives, in plain double arithmetic (+ - x / only):
 *   n_eff    sum_w2 > 0 ? (sum_w * sum_w) / sum_w2 : 0
 *   mean[k]  (double)r_k + m_k with m_k = s[k] / sum_w
 *   cov[kl]  S[kl] / sum_w - m_k * m_l, symmetric 6 x 6, row-major, all 36 stored
 *   (sum_w == 0: every derived field is 0 and evaluated is still 1)
 *   pos_sigma, pos_axes, solve_info   the 3 x 3 block cov[0..2][0..2] rounded to float through the eigen solver of the object
 *            report: pos_sigma[a] = sqrtf(max(eigenvalue_a, 0)), ascending; pos_axes its eigenvectors as columns (row-major,
 *            col 2 = col 0 x col 1); solve_info its return value (1: no convergence)
 *   rpy_sigma[a]  sqrt(max(cov[3+a][3+a], 0)) in double
 * Euler angles are treated linearly, as PCL's update() treats them: particles are never wrapped, so a population does not
 * straddle +-pi.  The summation order is the tree on every handle, PFT_SUM_PCL handles included: PCL has no such statistic
 * to follow.  `mean` is formed in double and is not claimed to equal pft_get_result.
 * The spread rule mirrors the lost rule:
 *   uncertain  (double)pos_sigma[2] > max_pos_sigma || n_eff < min_n_eff
 *   streak     uncertain ? streak + 1 : 0;   flagged  streak >= after;   calls  pft_spread launches so far
 * The streak is cleared by pft_reset_tracking and pft_set_reference.
 *   evaluated  1, or 0 when the last iteration of the last pft_compute raised a device-side failure: every other field
 *              except calls then keeps its last value, the streak included.  An iteration skipped by the change detector is
 *              evaluated: its weights were renormalised, the population is valid. */
typedef struct pft_population_stats {
  double   sum_w, sum_w2;
  double   s[6];
  double   S[21];
  double   n_eff;
  double   mean[6];
  double   cov[36];
  double   rpy_sigma[3];
  float    pos_sigma[3];
  float    pos_axes[9];
  float    w_max;
  uint32_t n, n_zero, i_max, solve_info;
  uint32_t evaluated, uncertain, streak, flagged, calls;
} pft_population_stats;                          /* 688 B */

/* max_pos_sigma >= 0 (default +inf), min_n_eff >= 0 (default 0), after >= 1 (default 1): the defaults never fire.  Read by
 * the pft_spread calls that follow.  PFT_ERR_INVALID_ARG for a NaN or negative threshold, or after < 1 */
int pft_set_spread_threshold(pft_tracker* t, double max_pos_sigma, double min_n_eff, int after);
int pft_get_spread_threshold(pft_tracker* t, double* max_pos_sigma, double* min_n_eff, int* after);
/* enqueues the statistics of the population on the device (never synchronises).  Allowed after pft_set_particles, on KLD and
 * exact-NN handles, and with PFT_GRAPH=1 (launched outside the captured frame).  PFT_ERR_INVALID_ARG with a text: a sharded
 * handle (world_size > 1).  PFT_ERR_STATE: before a population exists (the first pft_compute or pft_set_particles) */
int pft_spread(pft_tracker* t);
/* synchronises and copies the last statistics out; device-side failures are reported as by pft_get_result */
int pft_get_spread(pft_tracker* t, pft_population_stats* out);

/* ---- multi-GPU phase API (one handle per rank; the collectives between the phases are issued by
 *      the host layer on the same stream, see pcl_tracking_amd/dist.py and DESIGN.md) ----
 * The host layer owns three device buffers and binds them once:
 *   bbox6    6 floats {-xmin,-ymin,-zmin,xmax,ymax,zmax}: ONE max all-reduce gives the global AABB
 *   shard    P/world particles (32 B each) with the raw weight in .weight
 *   gathered P particles: the all-gather of every rank's shard, in rank order
 * iteration = phase_a -> [all-reduce(max) bbox6] -> phase_b -> [all-gather shard -> gathered] -> phase_c */
int pft_dist_bind(pft_tracker* t, void* bbox6_dev, void* shard_dev, void* gathered_dev);
int pft_dist_begin_frame(pft_tracker* t);          /* initParticles on the first frame */
int pft_dist_phase_a(pft_tracker* t, int iteration); /* resample shard, pose->matrix, local AABB */
int pft_dist_phase_b(pft_tracker* t);              /* crop, octree, likelihood, raw weights into shard */
int pft_dist_phase_c(pft_tracker* t);              /* normalise, update, alias table over all particles */

/* ---- test hooks (used by tests/ to compare every stage with the oracle) ---- */
int pft_set_particles(pft_tracker* t, const pft_particle* p, size_t n);
/* deterministic chain A1-A7 on explicit particles: raw_w[P] = -(float)sum; optional per-pair
 * approximate-NN index into the cropped cloud (nn_idx[P*M]) and squared distance (nn_d2[P*M]) */
int pft_eval_weights(pft_tracker* t, const pft_particle* particles, size_t P, float* raw_w, int32_t* nn_idx,
                     float* nn_d2);
int pft_debug_get_bbox(pft_tracker* t, float bbox[6]); /* x_min,x_max,y_min,y_max,z_min,z_max */
int pft_debug_get_crop(pft_tracker* t, int32_t* idx, size_t cap, size_t* n);
/* test hook: the handle's 16-byte input records [first, first + n) (x, y, z, rgba bits), as the first crop of a frame
 * forms them; PFT_ERR_CAPACITY past the handle's input capacity */
int pft_debug_get_input_records(pft_tracker* t, void* out, size_t first, size_t n);
int pft_debug_get_octree(pft_tracker* t, int32_t* depth, double min_xyz[3], double max_xyz[3], uint32_t* n_leaves,
                         uint32_t* n_nodes);
int pft_debug_get_point_keys(pft_tracker* t, uint32_t* keys3, size_t cap_points);
int pft_debug_get_scan_stats(pft_tracker* t, uint64_t* queries, uint64_t* scanned_points);
/* the linearised octree of the last build, whichever launch built it (pft_eval_weights, or the last evaluated iteration of
 * pft_compute): waits for the handle's stream and copies; launches nothing.  info receives PFT_TREE_INFO_WORDS words:
 * [0] n_crop, [1] error, [2] depth, [3] use_table, [4] n_words, [5] n_leaves, [6] leaf_start, [7] n_grow, [8] build_path,
 * [9] leaf_indirect, [10] jump_level, [11] margin_cells (float bits), [12] inv_res (float bits), [13..15] ominf (float
 * bits), [16] build_epoch, [17] build_variant (k_octree_build: bits 0-2 the per-point store -- 1 RegStore<4>, 2 RegStore<8>,
 * 3 RegStore<14>, 4 HybridStore<8>, 5 GlobStore --, bit 3 the node words ended in LDS, bit 4 the leaf scratch was in LDS,
 * bit 5 an LDS attempt was abandoned and the tree rebuilt in HBM, bit 6 dense top levels, bit 7 the rescue launch built the
 * tree, bits 8-9 who writes the leaf records: 0 k_leaf_gather, 1 the builder, 2 nobody; the sorted builder: 6 | radix
 * passes << 10), [18] the dynamic LDS bytes k_octree_build is launched with on this device, [19] entries of the jump
 * allocation, [20 .. 20 + depth + 1] lvl_start (the rest zero).
 * Every array is optional (null or capacity 0) and receives min(capacity, count) elements: words [n_words] (0 after a
 * build error), leaf_order [n_crop], leaf_pts and crop_pts [n_crop] 16-byte records, jump [info[19]]: the whole allocation,
 * so entries beyond 8^jump_level can be looked at as well.  PFT_ERR_INVALID_ARG on sharded and exact_nearest handles (no
 * octree), PFT_ERR_STATE before the first input cloud */
#define PFT_TREE_INFO_WORDS 64
int pft_debug_get_tree(pft_tracker* t, uint32_t* info, uint32_t* words, size_t words_cap, uint32_t* leaf_order,
                       size_t leaf_order_cap, void* leaf_pts, size_t leaf_pts_cap, void* crop_pts, size_t crop_pts_cap,
                       uint16_t* jump, size_t jump_cap);
/* limits for the error-path tests: max_words != 0 lowers the octree node capacity (never above the allocation),
 * sorted_npass != 0 fixes the radix passes of the sorted builder (0 = derived from the previous depth) */
int pft_debug_set_limits(pft_tracker* t, uint32_t max_words, int sorted_npass);
/* checkpoint of the filter state between two frames (population with weights, alias table, representative state,
 * motion, KLD particle count, resample epoch); restore is one kernel on the handle's stream.  bench.py replays the
 * same frame with it (stationary workload); tests use it to compare two schedules from the same state.  The change
 * detector's state is part of the checkpoint; restore returns PFT_ERR_STATE (and changes nothing) if the detector was
 * first enabled, or its buffers grew with the input, after the save. */
int pft_debug_state_save(pft_tracker* t);
int pft_debug_state_restore(pft_tracker* t);
/* OR `bits` into the device-side error flags right after the next crop launch (what a failing stage leaves behind) */
int pft_debug_inject_error(pft_tracker* t, uint32_t bits);
/* the pinned status block: [0] last crop size, [1] last depth, [2] flags of the last failed iteration, [3] unreported flags */
int pft_debug_get_host_stat(pft_tracker* t, uint32_t out4[4]);
/* wall-clock stamps (100 MHz ticks) taken at phase boundaries inside the single-workgroup kernels of the
 * last iteration: [0..15] octree build, [16..31] population.  The kernels take the stamps only in the diagnostic variant
 * library (-DPFT_DIAG); the product library returns zeros */
int pft_debug_get_ticks(pft_tracker* t, uint64_t* ticks32);
/* descent statistics of the last pft_eval_weights call that asked for the NN arrays: [0..10] queries by
 * number of generic levels, [11] queries that used the jump table, [12] wave iterations, [13..15] sums of
 * the per-wave maxima of generic levels / fast levels / leaf size, [16..26] wave iterations by max generic,
 * [27..29] zero, [30] reference points the particles' bounding box is taken over (the hull subset), [31] all reference
 * points (the exact-NN mode puts its own bookkeeping into [8..13]) */
int pft_debug_get_descent_stats(pft_tracker* t, uint64_t* dbg32);
/* NearestPairPointCloudCoherence handles (exact_nearest; PFT_ERR_INVALID_ARG on others, PFT_ERR_STATE before the first input
 * cloud): the search structure's state after the last iteration -- which of its capacity fallbacks were taken.
 * info [PFT_EXACT_STATE_WORDS]: [0] grid cell edge eg_g (float bits), [1..3] eg_dim, [4..6] eg_min (float bits), [7] eg_ncells,
 * [8] n_crop, [9] ec_nslots (cells hit by queries, may exceed the slot capacity), [10] ec_pool_used (candidate entries asked
 * for, may exceed the pool), [11] ec_pool_cap of that iteration, [12] queries and [13] 64-query blocks of the cell-sorted
 * search (the two halves of eq_totals), [14] slot capacity in force, [15] grid cell capacity, [16] per-tile count tables
 * allocated, [17] capacity of the cell-sorted query array, [18] PFT_EC_SLOTS, [19] PFT_EC_POOL, [20] PFT_EG_CAP,
 * [21] PFT_EC_POOL_MIN, [22] compute units (the tiles of the LDS-aggregated passes hold ceil(P / CUs) particles, at most 32).
 * counters [8] (optional), written only by the instantiations that also write the NN arrays, so valid after a
 * pft_eval_weights call that asked for them (which zeroes them first): words 24..28 of the header's debug block -- [0] queries
 * k_eq_scatter placed through the probe-window-full branch, [1] queries it answered inline by the shell search, [2] inline
 * as "empty list", [3] queries k_likelihood_exact sent to the shell search, [4] k_eq_scatter queries outside the grid --
 * then words 0, 1, 3 of k_likelihood_exact: [5] its queries, [6] those served by a list, [7] those outside the grid.
 * (Words 0..6 are read by tools/exact_nn_bench.py, 8..13 and 30..31 are overlaid by pft_debug_get_descent_stats, 16..20
 * belong to -DPFT_EC_TIMING.)
 * Per-slot arrays ec_cells / ec_count (0xffffffff: no list, the pool was full) / ec_base, each optional, receive
 * min(slots_cap, ec_nslots, slot capacity) entries; eg_start receives min(eg_start_cap, eg_ncells + 1) cell starts of the
 * counting sort and leaf_order min(leaf_order_cap, n_crop) crop positions in sorted order. */
#define PFT_EXACT_STATE_WORDS 32
int pft_debug_get_exact_state(pft_tracker* t, uint32_t* info, uint64_t* counters, uint32_t* ec_cells, uint32_t* ec_count,
                              uint32_t* ec_base, size_t slots_cap, uint32_t* eg_start, size_t eg_start_cap,
                              uint32_t* leaf_order, size_t leaf_order_cap);
/* exact_nearest handles: the candidate-list slots handed out per iteration, 1 .. PFT_EC_SLOTS (the allocation; above it
 * PFT_ERR_CAPACITY).  Cells beyond the limit get no list and no segment: their queries take the shell search */
int pft_debug_set_exact_limits(pft_tracker* t, uint32_t ec_slots);
/* the same call's queries by number of "hard" generic steps (the per-axis nearest child is absent): 0, 1, 2, 3, >= 4 */
int pft_debug_get_hard_steps(pft_tracker* t, uint64_t out5[5]);
/* what the likelihood kernel chose in the last pft_eval_weights call that asked for the NN arrays (zero otherwise):
 * out4[0] bit 0 valid, bits 1-2 LDS layout (0 node words + u16 leaf starts, 1 u32 node words, 2 branch levels only,
 * 3 hybrid: top words in LDS), bits 3-4 descent (0 fast, 1 table generic, 2 no centre tables), bit 5 the instance reads
 * leaf records through leaf_order, bit 6 the builder's leaf_indirect, bit 7 the fast descent's jump table was dropped to
 * make the node words fit, bits 8-11 jump level used (0: none);
 * out4[1] node words held in LDS by the hybrid layout, out4[2] the workgroup's LDS bytes, out4[3] the fast descent's
 * margin in leaf cells (float bits) */
int pft_debug_get_likelihood_layout(pft_tracker* t, uint32_t out4[4]);
/* the ancestor table of the fast descent for the last tree built: info10 = {usable (filled for this tree), level L,
 * window first cell x, y, z, log2 of the window's cells bx, by, bz (level-L cells), tree build epoch, epoch the table was
 * filled for}; table (nullable) receives min(cap, 2^(bx+by+bz)) entries, entry [x | y << bx | z << (bx + by)] =
 * (a << 27) | node: node is the deepest existing ancestor of window cell (x, y, z) at a level a <= L; L is the tree's
 * depth - 1 or depth - 2 (pft_debug_get_ancestor_level).
 * PFT_ANCESTOR_TABLE=0 at pft_create: no table, info10[0] = info10[1] = 0 */
int pft_debug_get_ancestor_table(pft_tracker* t, uint32_t info10[10], uint32_t* table, size_t cap);
/* the level of the ancestor table, chosen per build (synchronises the stream): out5 = {the pinned status word of the last
 * build -- 0x80000000 | log2 cells of the window at depth - 1 | the same at depth - 2 << 8, 0xff: no window --, the level
 * the last build was asked for as depth - out5[1] (0: no table; 0xffffffff: no build yet), the ANC_UP of the last
 * likelihood instance launched, how often the request changed from one build to the next, graph instantiations of a
 * PFT_GRAPH=1 handle}.  PFT_ANC_UP_FORCE=0|1|2 at pft_create fixes the request */
int pft_debug_get_ancestor_level(pft_tracker* t, uint32_t out5[5]);
/* host-only (no device needed): the positions of the reference points the bounding box of the particles' transformed
 * clouds is taken over (A3: calcBoundingBox of the tracker that /root/reference/src/auto_tracking.cpp:691-693 runs) -- the
 * convex hull's vertices plus the shell the float evaluation can reach; `keep` has room for n indices (ascending),
 * *n_keep receives their number (n itself for a degenerate cloud).  Same points, same order as the library uses for a
 * reference cloud handed to pft_set_reference in this order. */
int pft_debug_aabb_support_subset(const pft_point_xyzrgba* pts, size_t n, uint32_t* keep, size_t* n_keep);
#ifdef PFT_DIAG
/* diagnostic variant library only (tools/build_variant.py diag -DPFT_DIAG; never in libpft_hip.so): skip stages of the
 * handle's likelihood kernel for timing (bit0 generic levels, bit1 leaf scan, bit2 coherence); results are wrong while set */
void pft_debug_set_ablate(pft_tracker* t, int mask);
#endif
/* diagnostic: resident likelihood workgroups per CU according to the HIP occupancy API */
int pft_debug_likelihood_occupancy(void);
int pft_debug_normalize(pft_tracker* t, float* w_inout, size_t n, double* fit_ratio);
/* normalizeWeight with the raw weights formed in the same launch from n rows of nchunk likelihood partial sums (row-major) */
int pft_debug_normalize_partials(pft_tracker* t, const double* partial, size_t nchunk, size_t n, float* w_out,
                                 double* fit_ratio);
int pft_debug_alias(pft_tracker* t, const float* w, size_t n, int32_t* a, double* q);
int pft_debug_weighted_mean(pft_tracker* t, const pft_particle* p, size_t n, pft_particle* out);
int pft_debug_init_particles(pft_tracker* t, const pft_particle* rep, uint32_t id_offset, size_t n_local,
                             pft_particle* out);
int pft_debug_resample(pft_tracker* t, const pft_particle* old, size_t n_total, const int32_t* a, const double* q,
                       const pft_particle* rep, uint32_t epoch, uint32_t id_offset, size_t n_local,
                       pft_particle* out);
/* the product resample instances on explicit inputs: the prefix-sum form of the alias table is built on the device from
 * old's weights exactly as given (in the handle's summation order), then the instance is launched as pft_compute does:
 * 0 = one lane per particle, 1 = four lanes per particle, 2 = four lanes fused with the bounding box (PFT_ERR_STATE
 * without a reference cloud, or when its support subset is too large for the fused form).  mats12 (nullable) receives
 * the n_local 3x4 matrices the launch writes next to the particles.  The running filter is not touched. */
int pft_debug_resample_prefix(pft_tracker* t, const pft_particle* old, size_t n_total, const pft_particle* rep,
                              uint32_t epoch, uint32_t id_offset, size_t n_local, int instance, pft_particle* out,
                              float* mats12);
int pft_debug_pose_to_matrix(pft_tracker* t, const pft_particle* p, size_t n, float* m12);
/* the reference side's colour conversion alone: the kernel pft_set_reference packs its cloud with, in the handle's
 * hsv_pcl180_argorder, on buffers of its own (the handle's reference cloud stays as it is; no hull is taken).
 * hsv_out receives n float4 records {h / 180.0f, s / 255.0f, v / 255.0f, 0} */
int pft_debug_pack_reference(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n, float* hsv_out);
/* KLD resample alone: n_old particles + their explicit alias table (a, q) + motion -> the new particle set
 * (capacity maximum_particle_num), their 6-D bins, the new count and the number of distinct bins.  a == NULL and
 * q == NULL: no table -- the prefix-sum form is built from old's weights as given and the product instance is launched */
int pft_debug_kld_resample(pft_tracker* t, const pft_particle* old, size_t n_old, const int32_t* a, const double* q,
                           const pft_particle* motion, uint32_t epoch, pft_particle* out, int32_t* bins6,
                           uint32_t* n_out, uint32_t* k_out);
/* the same, and the launch also writes the 3x4 matrix of every candidate (the pose -> matrix step the kernel fuses, as
 * under pft_compute): mats12 (required, room for maximum_particle_num matrices) receives those of the n_out particles */
int pft_debug_kld_resample_mats(pft_tracker* t, const pft_particle* old, size_t n_old, const int32_t* a,
                                const double* q, const pft_particle* motion, uint32_t epoch, pft_particle* out,
                                int32_t* bins6, uint32_t* n_out, uint32_t* k_out, float* mats12);
/* host-side KLDAdaptiveParticleFilterTracker::normalQuantile / calcKLBound (what the resample kernel is given) */
double pft_kld_normal_quantile(double u);
double pft_kld_bound(int k, double delta, double epsilon);

/* ---- per-kernel HIP-event timing on the handle's stream ---- */
enum {
  PFT_K_RESAMPLE = 0, PFT_K_AABB = 1, PFT_K_CROP = 2, PFT_K_OCTREE = 3, PFT_K_LIKELIHOOD = 4,
  PFT_K_POPULATION = 5, PFT_K_PACK = 6, PFT_K_COUNT = 7
};
int pft_profile_enable(pft_tracker* t, int on);
int pft_profile_get(pft_tracker* t, int kernel_id, double* total_ms, uint64_t* launches);
int pft_profile_reset(pft_tracker* t);
const char* pft_kernel_name(int kernel_id);

#ifdef __cplusplus
}
#endif
#endif

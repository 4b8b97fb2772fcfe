// particle_filter_tracker.hpp -- header-only C++ mirror, over the C ABI of include/pft.h, of the PCL classes
// that /root/reference/src/auto_tracking.cpp instantiates and calls on its hot path:
//
//   pcl::tracking::ParticleFilterOMPTracker<RefPointType, ParticleT>      :203-204
//   pcl::tracking::KLDAdaptiveParticleFilterOMPTracker<...>               :207-222 (the runtime default, :821)
//   pcl::tracking::ParticleFilterTracker<RefPointType, ParticleT>         :153 (base type of tracker_dict)
//   pcl::tracking::ApproxNearestPairPointCloudCoherence<RefPointType>     :235-236
//   pcl::tracking::DistanceCoherence / HSVColorCoherence                  :240-247
//   pcl::search::Octree<RefPointType>                                     :250
//   pcl::tracking::ParticleXYZRPY, pcl::PointXYZRGBA, pcl::PointCloud<T>
//
// Same member names, argument meaning and error behaviour (compute() never throws; a missing input cloud
// is reported on stderr and the call returns, as PCL's PCL_ERROR + early return does).  The types live in
// namespace pft so the header can sit next to a real PCL; on a machine that has PCL, the two lines of
// INTEGRATION.md switch auto_tracking.cpp over.  All compute happens in the HIP library.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "pft.h"
#include "pft_visibility.h"
#include "pft_view.h"

namespace pft {

struct PointXYZRGBA : pft_point_xyzrgba {  // layout of pcl::PointXYZRGBA
  PointXYZRGBA() {
    x = y = z = 0.0f;
    w = 1.0f;
    rgba = 0;
    pad[0] = pad[1] = pad[2] = 0;
  }
};
static_assert(sizeof(PointXYZRGBA) == 32, "pcl::PointXYZRGBA is 32 bytes");

struct ParticleXYZRPY : pft_particle {  // layout of pcl::tracking::ParticleXYZRPY
  ParticleXYZRPY() {
    x = y = z = roll = pitch = yaw = 0.0f;
    w = 1.0f;
    weight = 0.0f;
  }
  static int stateDimension() { return 6; }
  float operator[](unsigned i) const {
    switch (i) {
      case 0: return x;
      case 1: return y;
      case 2: return z;
      case 3: return roll;
      case 4: return pitch;
      case 5: return yaw;
      default: return 0.0f;
    }
  }
};
static_assert(sizeof(ParticleXYZRPY) == 32, "pcl::tracking::ParticleXYZRPY is 32 bytes");

// the part of Eigen::Affine3f the driver uses: a row-major 4x4
struct Affine3f {
  float m[16];
  Affine3f() { *this = Identity(); }
  static Affine3f Identity() {
    Affine3f a(0);
    for (int i = 0; i < 4; i++) a.m[5 * i] = 1.0f;
    return a;
  }
  float& operator()(int r, int c) { return m[4 * r + c]; }
  float operator()(int r, int c) const { return m[4 * r + c]; }

 private:
  explicit Affine3f(int) { std::memset(m, 0, sizeof(m)); }
};

template <typename PointT>
struct PointCloud {
  typedef std::shared_ptr<PointCloud<PointT>> Ptr;
  typedef std::shared_ptr<const PointCloud<PointT>> ConstPtr;
  std::vector<PointT> points;
  uint32_t width = 0, height = 1;
  bool is_dense = true;
  size_t size() const { return points.size(); }
  bool empty() const { return points.empty(); }
};

namespace search {
template <typename PointT>
class Octree {
 public:
  explicit Octree(double resolution) : resolution_(resolution) {}
  double getResolution() const { return resolution_; }

 private:
  double resolution_;
};
}  // namespace search

namespace tracking {

template <typename PointInT>
class PointCoherence {
 public:
  virtual ~PointCoherence() {}
  enum Kind { DISTANCE, HSV };
  virtual Kind kind() const = 0;
};

template <typename PointInT>
class DistanceCoherence : public PointCoherence<PointInT> {
 public:
  DistanceCoherence() : weight_(1.0) {}
  void setWeight(double w) { weight_ = w; }
  double getWeight() const { return weight_; }
  typename PointCoherence<PointInT>::Kind kind() const override { return PointCoherence<PointInT>::DISTANCE; }

 private:
  double weight_;
};

template <typename PointInT>
class HSVColorCoherence : public PointCoherence<PointInT> {
 public:
  HSVColorCoherence() : weight_(1.0), h_weight_(1.0), s_weight_(1.0), v_weight_(0.0) {}
  void setWeight(double w) { weight_ = w; }
  double getWeight() const { return weight_; }
  void setHWeight(double w) { h_weight_ = w; }
  void setSWeight(double w) { s_weight_ = w; }
  void setVWeight(double w) { v_weight_ = w; }
  double getHWeight() const { return h_weight_; }
  double getSWeight() const { return s_weight_; }
  double getVWeight() const { return v_weight_; }
  typename PointCoherence<PointInT>::Kind kind() const override { return PointCoherence<PointInT>::HSV; }

 private:
  double weight_, h_weight_, s_weight_, v_weight_;
};

template <typename PointInT>
class ApproxNearestPairPointCloudCoherence {
 public:
  typedef std::shared_ptr<ApproxNearestPairPointCloudCoherence<PointInT>> Ptr;
  typedef std::shared_ptr<PointCoherence<PointInT>> PointCoherencePtr;
  ApproxNearestPairPointCloudCoherence() : maximum_distance_(1e30), resolution_(0.01) {}
  virtual ~ApproxNearestPairPointCloudCoherence() {}
  virtual bool exactNearest() const { return false; }
  void addPointCoherence(const PointCoherencePtr& c) { point_coherences_.push_back(c); }
  // upstream keeps its own search::Octree(0.01) and ignores the object passed here; the reference passes
  // the same 0.01 (auto_tracking.cpp:250), so the resolution is taken from it
  void setSearchMethod(const std::shared_ptr<search::Octree<PointInT>>& s) {
    if (s) resolution_ = s->getResolution();
  }
  void setMaximumDistance(double d) { maximum_distance_ = d; }
  double getMaximumDistance() const { return maximum_distance_; }
  double getResolution() const { return resolution_; }
  const std::vector<PointCoherencePtr>& getPointCoherences() const { return point_coherences_; }

 private:
  std::vector<PointCoherencePtr> point_coherences_;
  double maximum_distance_, resolution_;
};

// pcl::tracking::NearestPairPointCloudCoherence: the true nearest neighbour instead of the greedy octree descent
// (the alternative auto_tracking.cpp keeps commented out at :237-238, :249); same setters
template <typename PointInT>
class NearestPairPointCloudCoherence : public ApproxNearestPairPointCloudCoherence<PointInT> {
 public:
  bool exactNearest() const override { return true; }
};

template <typename PointInT, typename StateT>
class ParticleFilterTracker {
 public:
  typedef PointCloud<PointInT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudInConstPtr;
  typedef PointCloud<StateT> PointCloudState;
  typedef typename PointCloudState::Ptr PointCloudStatePtr;
  typedef ApproxNearestPairPointCloudCoherence<PointInT> CloudCoherence;
  typedef typename CloudCoherence::Ptr CoherencePtr;

  ParticleFilterTracker() : handle_(nullptr) {
    pft_config_default(&cfg_);
    trans_ = Affine3f::Identity();
  }
  virtual ~ParticleFilterTracker() {
    if (handle_) pft_destroy(handle_);
  }
  ParticleFilterTracker(const ParticleFilterTracker&) = delete;
  ParticleFilterTracker& operator=(const ParticleFilterTracker&) = delete;

  // ---- setters used at auto_tracking.cpp:225-254 ----
  void setTrans(const Affine3f& trans) {
    trans_ = trans;
    if (handle_) pft_set_trans(handle_, trans_.m);
  }
  void setStepNoiseCovariance(const std::vector<double>& cov) { copy6(cov, cfg_.step_noise_cov); }
  void setInitialNoiseCovariance(const std::vector<double>& cov) { copy6(cov, cfg_.initial_noise_cov); }
  void setInitialNoiseMean(const std::vector<double>& mean) { copy6(mean, cfg_.initial_noise_mean); }
  void setIterationNum(int n) { guard(); cfg_.iteration_num = n; }
  void setParticleNum(int n) { guard(); cfg_.particle_num = n; }
  void setResampleLikelihoodThr(double v) { guard(); cfg_.resample_likelihood_thr = v; }
  void setUseNormal(bool b) { guard(); cfg_.use_normal = b ? 1 : 0; }
  void setAlpha(double a) { guard(); cfg_.alpha = a; }
  // the share of new particles that take the motion step (PCL's ctor default 0.25; read by the KLD resample only)
  void setMotionRatio(double r) { guard(); cfg_.motion_ratio = r; }
  double getMotionRatio() const { return cfg_.motion_ratio; }
  void setMinIndices(int) {}  // read only when use_normal_ is true
  void setSeed(uint64_t s) { guard(); cfg_.seed = s; }      // PCL's engines are time(0)-seeded
  // PFT_SUM_TREE (default) or PFT_SUM_PCL: the order of normalizeWeight's and update()'s population sums (pft.h)
  void setSumOrder(int order) { guard(); cfg_.sum_order = order; }
  // ParticleFilterTracker's change detector (PCL defaults: off, 10, 10, 0.01).  Not guarded: PCL allows them between
  // frames; they reach the handle whenever it exists.  The resolution is latched at the first compute().
  // (a setting the handle refuses -- e.g. the detector on an exact-NN handle -- is reported and not kept)
  void setUseChangeDetector(bool use) { setChangeDetector(use, cd_interval_, cd_min_points_, cd_resolution_); }
  bool getUseChangeDetector() const { return use_cd_; }
  void setIntervalOfChangeDetection(unsigned int interval) { setChangeDetector(use_cd_, interval, cd_min_points_, cd_resolution_); }
  unsigned int getIntervalOfChangeDetection() const { return cd_interval_; }
  void setMinPointsOfChangeDetection(unsigned int n) { setChangeDetector(use_cd_, cd_interval_, n, cd_resolution_); }
  unsigned int getMinPointsOfChangeDetection() const { return cd_min_points_; }
  void setResolutionOfChangeDetection(double res) { setChangeDetector(use_cd_, cd_interval_, cd_min_points_, res); }
  double getResolutionOfChangeDetection() const { return cd_resolution_; }
  void setDevice(int id) { guard(); cfg_.device_id = id; }
  // enqueue on the caller's HIP stream (hipStream_t; nullptr = the default stream) instead of a stream of the handle's own
  void setStream(void* hip_stream) { guard(); cfg_.stream = hip_stream; cfg_.stream_is_external = 1; }
  // particle sharding over the GPUs of a node (one process per GPU): this handle owns the global particle ids
  // [rank * N / world, (rank + 1) * N / world); such a handle is driven through the pft_dist_* phases of pft.h with the
  // two collectives in between (examples/dist_tracking_amd.cpp), not through compute()
  void setShard(int rank, int world_size) { guard(); cfg_.rank = rank; cfg_.world_size = world_size; }
  // compute() is asynchronous and PCL's returns void.  The reference wraps it in try / catch (int)
  // (auto_tracking.cpp:692-696): with this switch on, compute() waits for the frame and throws the pft_status (an int)
  // if the device reported a failure for it (octree capacity / depth, crop time-out: pft.h).  With a match threshold
  // whose min_ratio is above 0 (setMatchThreshold) it also enqueues the match behind the frame, and throws
  // (int)PFT_ERR_LOST when the lost rule fired: the reference's handler then prints its "Object not recognized".
  // That match is the frame's: getMatch() / getMatchPairs() return it, and a computeMatch() of the caller's own on the same
  // frame would be a second one and advance the streak twice.  Handles that cannot match (exact-NN coherence, a shard)
  // get no implicit match: compute() reports their device failures only
  void setThrowOnFailure(bool b) { throw_on_failure_ = b; }
  // the handle exists from the first compute() on; create() makes it now (for callers of the C ABI's phase API)
  bool create() { return ensure(); }
  void setCloudCoherence(const CoherencePtr& c) {
    guard();
    coherence_ = c;
    cfg_.max_distance = c->getMaximumDistance();
    cfg_.octree_resolution = c->getResolution();
    cfg_.exact_nearest = c->exactNearest() ? 1 : 0;
    const auto& pcs = c->getPointCoherences();
    if (pcs.size() != 2 || pcs[0]->kind() != PointCoherence<PointInT>::DISTANCE ||
        pcs[1]->kind() != PointCoherence<PointInT>::HSV)
      throw std::invalid_argument("supported point coherences: DistanceCoherence then HSVColorCoherence");
    auto* d = static_cast<DistanceCoherence<PointInT>*>(pcs[0].get());
    auto* h = static_cast<HSVColorCoherence<PointInT>*>(pcs[1].get());
    cfg_.distance_weight = d->getWeight();
    cfg_.hsv_weight = h->getWeight();
    cfg_.h_weight = h->getHWeight();
    cfg_.s_weight = h->getSWeight();
    cfg_.v_weight = h->getVWeight();
  }

  // ---- data, auto_tracking.cpp:673, 691 ----
  void setReferenceCloud(const PointCloudInConstPtr& ref) {
    ref_ = ref;
    if (handle_ && ref_) check(pft_set_reference(handle_, ref_->points.data(), ref_->points.size()), "setReferenceCloud");
  }
  PointCloudInConstPtr getReferenceCloud() const { return ref_; }
  void setInputCloud(const PointCloudInConstPtr& cloud) {
    input_ = cloud;
    dev_input_ = nullptr;
    filter_input_ = nullptr;
  }
  // a cloud already in HBM (n 32-byte points), e.g. the output of pft::InputFilter::filterDevice
  void setInputCloudDevice(const pft_point_xyzrgba* device_points, size_t n) {
    input_.reset();
    dev_input_ = device_points;
    dev_n_ = n;
    filter_input_ = nullptr;
  }
  // the output of a pft::InputFilter whose filter() / filterAsync() may still be running: cloud and count are read on the
  // device, nothing waits on the host.  max_points bounds the count (0: the size of the filter's input).  The filter object
  // must have been applied, and must not be applied again before this tracker's compute()
  template <class Filter>
  void setInputCloudFromFilter(Filter& f, size_t max_points = 0) {
    input_.reset();
    dev_input_ = nullptr;
    filter_input_ = f.nativeHandle();
    filter_max_ = max_points;
  }

  // ---- auto_tracking.cpp:693 ----
  void compute() {
    if (filter_input_) {
      if (!ensure()) return;
      if (check(pft_set_input_from_filter(handle_, filter_input_, filter_max_), "setInputCloudFromFilter") != PFT_OK) return;
      finish(check(pft_compute(handle_), "compute"));
      return;
    }
    if (dev_input_ && dev_n_) {
      if (!ensure()) return;
      if (check(pft_set_input_device(handle_, dev_input_, dev_n_), "setInputCloudDevice") != PFT_OK) return;
      finish(check(pft_compute(handle_), "compute"));
      return;
    }
    if (!input_ || input_->points.empty()) {
      std::fprintf(stderr, "[pft::ParticleFilterTracker::compute] input cloud is empty or not set\n");
      return;  // PCL: PCL_ERROR + early return, no exception
    }
    if (!ensure()) return;
    if (check(pft_set_input(handle_, input_->points.data(), input_->points.size()), "setInputCloud") != PFT_OK) return;
    finish(check(pft_compute(handle_), "compute"));
  }

  // ---- auto_tracking.cpp:309-310, 270 ----
  StateT getResult() const {
    StateT r;
    if (handle_) check(pft_get_result(handle_, &r), "getResult");  // also reports device-side failures of the frame
    return r;
  }
  Affine3f toEigenMatrix(const StateT& particle) const {
    Affine3f a;
    pft_to_matrix(&particle, a.m);
    return a;
  }
  PointCloudStatePtr getParticles() const {
    PointCloudStatePtr out(new PointCloudState());
    if (!handle_) return out;
    size_t n = 0;
    pft_get_particles(handle_, nullptr, 0, &n);
    out->points.resize(n);
    if (n) check(pft_get_particles(handle_, out->points.data(), n, &n), "getParticles");
    out->width = (uint32_t)n;
    return out;
  }
  double getFitRatio() const {
    double v = 0.0;
    if (handle_) check(pft_get_fit_ratio(handle_, &v), "getFitRatio");
    return v;
  }
  // ---- object report (drawResult :301-326 + viz_cb :432-470, on the device) ----
  // reference_dict[obj]: the re-centred, full-resolution model the result pose moves; may be replaced at any time
  int setReportCloud(const PointCloudInConstPtr& cloud) {
    report_cloud_ = cloud;
    if (!handle_ || !report_cloud_) return PFT_OK;
    return check(pft_set_report_cloud(handle_, report_cloud_->points.data(), report_cloud_->points.size()), "setReportCloud");
  }
  // setReferenceCloud + setTrans (+ setReportCloud) from a pft::ModelPreparation that has been prepared (:673-675): the
  // report cloud goes device to device.  The handle is created first, as compute() would.
  template <class Model>
  int setObjectFromModel(Model& mp, bool with_report_cloud = false) {
    if (!ensure()) return PFT_ERR_NO_DEVICE;
    const int st = check(pft_set_object_from_model(handle_, mp.nativeHandle(), with_report_cloud ? 1 : 0), "setObjectFromModel");
    if (st != PFT_OK) return st;
    trans_ = mp.getTrans();
    std::shared_ptr<PointCloudIn> ref(new PointCloudIn());
    mp.getReference(*ref);
    ref_ = ref;
    if (with_report_cloud) report_cloud_.reset();  // the handle holds it; the host copy is not needed again
    return PFT_OK;
  }
  // enqueues the report of the last compute() on the tracker's stream; nothing waits
  int computeReport() {
    if (!handle_) return check(PFT_ERR_STATE, "computeReport");
    return check(pft_report(handle_), "computeReport");
  }
  // waits for the last computeReport(): transform, centroid, covariance, axes and the principal-axis box
  pft_object_report getReport() const {
    pft_object_report r;
    std::memset(&r, 0, sizeof(r));
    if (handle_) check(pft_get_report(handle_, &r), "getReport");
    return r;
  }
  // tracked_cloud_dict[obj] (:325): the report cloud moved by the last report's transform
  void getTrackedCloud(PointCloudIn& cloud) const {
    cloud.points.clear();
    size_t n = 0;
    if (handle_ && check(pft_get_tracked_cloud(handle_, nullptr, 0, &n), "getTrackedCloud") == PFT_OK && n) {
      cloud.points.resize(n);
      check(pft_get_tracked_cloud(handle_, cloud.points.data(), n, &n), "getTrackedCloud");
    }
    cloud.width = (uint32_t)cloud.points.size();
    cloud.height = 1;
  }

  // ---- match statistics of the result pose, the lost rule, resetTracking (pft.h) ----
  // lost after `lost_after` evaluated frames in a row with fewer than min_ratio * (reference points) matched points
  int setMatchThreshold(double min_ratio, int lost_after = 1) {
    if (!(min_ratio >= 0.0 && min_ratio <= 1.0) || lost_after < 1) return check(PFT_ERR_INVALID_ARG, "setMatchThreshold");
    if (handle_) {
      const int st = check(pft_set_match_threshold(handle_, min_ratio, lost_after), "setMatchThreshold");
      if (st != PFT_OK) return st;
    }
    match_min_ratio_ = min_ratio;
    match_lost_after_ = lost_after;
    return PFT_OK;
  }
  // enqueues the match of the last compute() on the tracker's stream; nothing waits.  Every call is one step of the lost
  // rule: not to be called for a frame whose compute() already matched (setThrowOnFailure(true) with min_ratio > 0)
  int computeMatch() {
    if (!handle_) return check(PFT_ERR_STATE, "computeMatch");
    return check(pft_match(handle_), "computeMatch");
  }
  // waits for the last computeMatch()
  pft_match_stats getMatch() const {
    pft_match_stats m;
    std::memset(&m, 0, sizeof(m));
    if (handle_) check(pft_get_match(handle_, &m), "getMatch");
    return m;
  }
  // per reference point, in the order of setReferenceCloud: the partner's index in the input cloud (-1: not matched) and
  // the neighbour's squared distance
  void getMatchPairs(std::vector<int32_t>& input_idx, std::vector<float>& sq_dist) const {
    input_idx.clear();
    sq_dist.clear();
    size_t n = 0;
    if (handle_ && check(pft_get_match_pairs(handle_, nullptr, nullptr, 0, &n), "getMatchPairs") == PFT_OK && n) {
      input_idx.resize(n);
      sq_dist.resize(n);
      check(pft_get_match_pairs(handle_, input_idx.data(), sq_dist.data(), n, &n), "getMatchPairs");
    }
  }
  bool isLost() const { return handle_ && getMatch().lost != 0; }
  // pcl::tracking::ParticleFilterTracker::resetTracking(): the next compute() is a first frame around the trans in force
  // then; the change detector keeps its state, the lost rule's streak is cleared
  void resetTracking() {
    if (handle_) check(pft_reset_tracking(handle_), "resetTracking");
  }

  // ---- population statistics and the spread rule (pft.h, pft_spread) ----
  // uncertain after `after` evaluated computeSpread() calls in a row whose largest position sigma exceeded max_pos_sigma or
  // whose effective sample size fell below min_n_eff; the defaults never fire
  int setSpreadThreshold(double max_pos_sigma, double min_n_eff = 0.0, int after = 1) {
    if (!(max_pos_sigma >= 0.0) || !(min_n_eff >= 0.0) || after < 1) return check(PFT_ERR_INVALID_ARG, "setSpreadThreshold");
    if (handle_) {
      const int st = check(pft_set_spread_threshold(handle_, max_pos_sigma, min_n_eff, after), "setSpreadThreshold");
      if (st != PFT_OK) return st;
    }
    spread_max_pos_sigma_ = max_pos_sigma;
    spread_min_n_eff_ = min_n_eff;
    spread_after_ = after;
    return PFT_OK;
  }
  // enqueues the statistics of the population the last compute() left on the device; nothing waits
  int computeSpread() {
    if (!handle_) return check(PFT_ERR_STATE, "computeSpread");
    return check(pft_spread(handle_), "computeSpread");
  }
  // waits for the last computeSpread()
  pft_population_stats getSpread() const {
    pft_population_stats p;
    std::memset(&p, 0, sizeof(p));
    if (handle_) check(pft_get_spread(handle_, &p), "getSpread");
    return p;
  }
  bool isUncertain() const { return handle_ && getSpread().flagged != 0; }

  // ---- visibility of the model at a pose, the occlusion-aware lost rule (pft_visibility.h) ----
  // the pinhole camera at the origin, looking along +z, of the computeVisibility() calls that follow; a value outside its
  // range is reported and not kept
  int setVisibilityCamera(const pft_visibility_config& cam) {
    if (handle_) {
      const int st = check(pft_set_visibility_camera(handle_, &cam), "setVisibilityCamera");
      if (st != PFT_OK) return st;
    }
    vis_cam_ = cam;
    vis_cam_set_ = true;
    return PFT_OK;
  }
  pft_visibility_config getVisibilityCamera() const {
    pft_visibility_config c;
    if (handle_ && pft_get_visibility_camera(handle_, &c) == PFT_OK) return c;
    if (vis_cam_set_) return vis_cam_;
    pft_visibility_config_default(&c);
    return c;
  }
  // hidden while fewer than min_visible_ratio * (reference points) are visible; lost after `lost_after` evaluated, matched,
  // not hidden frames in a row with fewer than min_ratio * (visible points) of the visible points matched
  int setVisibilityThreshold(double min_visible_ratio, double min_ratio = 0.0, int lost_after = 1) {
    if (!(min_visible_ratio >= 0.0 && min_visible_ratio <= 1.0) || !(min_ratio >= 0.0 && min_ratio <= 1.0) || lost_after < 1)
      return check(PFT_ERR_INVALID_ARG, "setVisibilityThreshold");
    if (handle_) {
      const int st = check(pft_set_visibility_threshold(handle_, min_visible_ratio, min_ratio, lost_after), "setVisibilityThreshold");
      if (st != PFT_OK) return st;
    }
    vis_min_visible_ratio_ = min_visible_ratio;
    vis_min_ratio_ = min_ratio;
    vis_lost_after_ = lost_after;
    return PFT_OK;
  }
  // enqueues the visibility of the reference cloud against the input cloud the handle holds (the one of the last
  // compute()) on the tracker's stream; nothing waits.  m12: a row-major 3x4 matrix; nullptr: the last result pose
  int computeVisibility(const float* m12 = nullptr) {
    if (!handle_) return check(PFT_ERR_STATE, "computeVisibility");
    return check(pft_visibility(handle_, m12), "computeVisibility");
  }
  // waits for the last computeVisibility()
  pft_visibility_stats getVisibility() const {
    pft_visibility_stats v;
    std::memset(&v, 0, sizeof(v));
    if (handle_) check(pft_get_visibility(handle_, &v), "getVisibility");
    return v;
  }
  // per reference point, in the order of setReferenceCloud: PFT_VIS_* and the two depth gaps
  void getVisibilityPoints(std::vector<uint8_t>& state, std::vector<float>& scene_gap, std::vector<float>& self_gap) const {
    state.clear();
    scene_gap.clear();
    self_gap.clear();
    size_t n = 0;
    if (handle_ && check(pft_get_visibility_points(handle_, nullptr, nullptr, nullptr, 0, &n), "getVisibilityPoints") == PFT_OK && n) {
      state.resize(n);
      scene_gap.resize(n);
      self_gap.resize(n);
      check(pft_get_visibility_points(handle_, state.data(), scene_gap.data(), self_gap.data(), n, &n), "getVisibilityPoints");
    }
  }
  bool isOccluded() const { return handle_ && getVisibility().hidden != 0; }
  bool isLostVisible() const { return handle_ && getVisibility().lost != 0; }

  // ---- the view-dependent reference (pft_view.h): a full model's visible side as the reference cloud ----
  // enqueues the selection of the records of `model` that the visibility camera sees at m12 (row-major 3x4; nullptr: the
  // last result pose) on the tracker's stream; nothing waits.  max_points: 0 = no limit
  int selectView(const PointCloudIn& model, const float* m12 = nullptr, uint32_t max_points = 0) {
    if (m12 ? !ensure() : !handle_) return check(m12 ? PFT_ERR_NO_DEVICE : PFT_ERR_STATE, "selectView");
    return check(pft_view_select(handle_, model.points.data(), model.points.size(), m12, max_points), "selectView");
  }
  // ... of n records in this device's HBM (16-byte aligned), written in the order of the tracker's stream or before
  int selectView(const pft_point_xyzrgba* device_points, size_t n, const float* m12 = nullptr, uint32_t max_points = 0) {
    if (m12 ? !ensure() : !handle_) return check(m12 ? PFT_ERR_NO_DEVICE : PFT_ERR_STATE, "selectView");
    return check(pft_view_select_device(handle_, device_points, n, m12, max_points), "selectView");
  }
  // ... of the grown model of a pft::ModelGrowth, device to device (modelDevice() waits for that handle's stream)
  template <class Growth, class = decltype(&Growth::modelDevice)>
  int selectView(Growth& grow, const float* m12 = nullptr, uint32_t max_points = 0) {
    const pft_point_xyzrgba* p = nullptr;
    size_t n = 0;
    grow.modelDevice(&p, &n);
    return selectView(p, n, m12, max_points);
  }
  // waits for the last selectView()
  pft_view_stats getView() const {
    pft_view_stats v;
    std::memset(&v, 0, sizeof(v));
    if (handle_) check(pft_get_view(handle_, &v), "getView");
    return v;
  }
  // per model record: PFT_VIEW_* and the self gap
  void getViewPoints(std::vector<uint8_t>& state, std::vector<float>& self_gap) const {
    state.clear();
    self_gap.clear();
    size_t n = 0;
    if (handle_ && check(pft_get_view_points(handle_, nullptr, nullptr, 0, &n), "getViewPoints") == PFT_OK && n) {
      state.resize(n);
      self_gap.resize(n);
      check(pft_get_view_points(handle_, state.data(), self_gap.data(), n, &n), "getViewPoints");
    }
  }
  // the kept records' indices into the model, ascending
  void getViewIndices(std::vector<uint32_t>& idx) const {
    idx.clear();
    size_t n = 0;
    if (handle_ && check(pft_get_view_indices(handle_, nullptr, 0, &n), "getViewIndices") == PFT_OK && n) {
      idx.resize(n);
      check(pft_get_view_indices(handle_, idx.data(), n, &n), "getViewIndices");
    }
  }
  // the kept records, whole, in index order
  void getViewCloud(PointCloudIn& out) const {
    out.points.clear();
    size_t n = 0;
    if (handle_ && check(pft_get_view_cloud(handle_, nullptr, 0, &n), "getViewCloud") == PFT_OK && n) {
      out.points.resize(n);
      check(pft_get_view_cloud(handle_, out.points.data(), n, &n), "getViewCloud");
    }
    out.width = (uint32_t)out.points.size();
    out.height = 1;
  }
  // the view cloud of the last selectView() becomes the reference cloud (waits).  The object is the same: the lost, the
  // visibility and the spread rule keep their streaks.  A refusal (PFT_ERR_STATE: fewer than max(min_points, 1) points
  // kept, a select that was not evaluated or is consumed already) prints its text and leaves the old reference in force
  int setReferenceFromView(uint32_t min_points = 1) {
    if (!handle_) return check(PFT_ERR_STATE, "setReferenceFromView");
    const int st = check(pft_set_reference_from_view(handle_, min_points), "setReferenceFromView");
    if (st != PFT_OK) return st;
    std::shared_ptr<PointCloudIn> ref(new PointCloudIn());
    getViewCloud(*ref);
    ref_ = ref;
    return PFT_OK;
  }

  // ---- re-acquisition of a lost object (pft.h, pft_reacquire) ----
  // every centre (n_centres x 3 floats) with every orientation of cfg's lattice is scored against the input cloud the handle
  // holds -- the one of the last compute() --; with cfg.apply and an accepted candidate the tracker is restarted at it:
  // setTrans(the candidate's matrix) + resetTracking().  Synchronous.  Returns the pft_status
  int reacquire(const float* centres_xyz, size_t n_centres, const pft_reacquire_config& cfg, pft_reacquire_result& out) {
    std::memset(&out, 0, sizeof(out));
    out.best = out.best_centre = -1;
    int st = handInput("reacquire");
    if (st != PFT_OK) return st;
    st = check(pft_reacquire(handle_, centres_xyz, n_centres, &cfg, &out), "reacquire");
    if (st == PFT_OK) applied(out);
    return st;
  }
  // the same with the cluster centroids of a pft::ModelSegmenter's last apply as centres, formed on the device
  template <class Segmenter>
  int reacquireFromSegmenter(Segmenter& seg, const pft_reacquire_config& cfg, pft_reacquire_result& out) {
    std::memset(&out, 0, sizeof(out));
    out.best = out.best_centre = -1;
    int st = handInput("reacquireFromSegmenter");
    if (st != PFT_OK) return st;
    st = check(pft_reacquire_from_segmenter(handle_, seg.nativeHandle(), &cfg, &out), "reacquireFromSegmenter");
    if (st == PFT_OK) applied(out);
    return st;
  }
  // pft_reacquire_config_default with the angles of the current trans as the lattice's base
  pft_reacquire_config reacquireConfig() const {
    pft_reacquire_config c;
    pft_reacquire_config_default(&c);
    StateT s;
    pft_to_state(trans_.m, &s);
    c.base_rpy[0] = s.roll;
    c.base_rpy[1] = s.pitch;
    c.base_rpy[2] = s.yaw;
    return c;
  }

  // ---- refinement of a pose against the frame (pft.h, pft_refine) ----
  // point-to-point ICP from start12 (row-major 3x4; nullptr: the last result pose) against the input cloud the handle holds,
  // all iterations on the device; with cfg.apply and an improved pose the tracker is restarted at it: setTrans(the final
  // matrix) + resetTracking().  Synchronous.  Returns the pft_status
  int refine(const float* start12 /*nullptr: the result*/, const pft_refine_config& cfg, pft_refine_result& out) {
    std::memset(&out, 0, sizeof(out));
    int st = handInput("refine");
    if (st != PFT_OK) return st;
    st = check(pft_refine(handle_, start12, &cfg, &out), "refine");
    if (st == PFT_OK && out.applied) {
      trans_ = Affine3f::Identity();
      std::memcpy(trans_.m, out.transform, sizeof(float) * 12);
    }
    return st;
  }
  pft_refine_config refineConfig() const {
    pft_refine_config c;
    pft_refine_config_default(&c);
    return c;
  }

  int getIterationNum() const { return cfg_.iteration_num; }
  int getParticleNum() const { return cfg_.particle_num; }
  pft_tracker* nativeHandle() { return handle_; }

 protected:
  void guard() const {
    if (handle_) throw std::logic_error("tracker parameters are fixed after the first compute()");
  }
  void copy6(const std::vector<double>& v, double* dst) {
    guard();
    for (size_t i = 0; i < 6 && i < v.size(); i++) dst[i] = v[i];
  }
  void setChangeDetector(bool use, unsigned int interval, unsigned int min_points, double res) {
    const bool u0 = use_cd_;
    const unsigned int i0 = cd_interval_, m0 = cd_min_points_;
    const double r0 = cd_resolution_;
    use_cd_ = use;
    cd_interval_ = interval;
    cd_min_points_ = min_points;
    cd_resolution_ = res;
    if (forwardChangeDetector() != PFT_OK) {
      use_cd_ = u0;
      cd_interval_ = i0;
      cd_min_points_ = m0;
      cd_resolution_ = r0;
    }
  }
  int forwardChangeDetector() {
    if (!handle_) return PFT_OK;
    return check(pft_set_change_detector(handle_, use_cd_ ? 1 : 0, (int)cd_interval_, (int)cd_min_points_, cd_resolution_),
                 "setUseChangeDetector");
  }
  int check(int st, const char* what) const {
    if (st != PFT_OK)
      std::fprintf(stderr, "[pft::ParticleFilterTracker::%s] %s: %s\n", what, pft_status_string(st),
                   handle_ ? pft_last_error_string(handle_) : "");
    return st;
  }
  // re-acquisition scores against the input cloud the handle holds: the one of the last compute()
  int handInput(const char* what) {
    if (!ensure()) return check(PFT_ERR_NO_DEVICE, what);
    return PFT_OK;
  }
  void applied(const pft_reacquire_result& r) {
    if (!r.applied) return;
    trans_ = Affine3f::Identity();  // what the handle now holds: the candidate's 3x4 over (0, 0, 0, 1)
    std::memcpy(trans_.m, r.transform, sizeof(float) * 12);
  }
  void finish(int st) {
    if (!throw_on_failure_) return;
    const bool match = st == PFT_OK && match_min_ratio_ > 0.0 && !cfg_.exact_nearest && cfg_.world_size == 1;
    if (match) st = check(pft_match(handle_), "compute");
    if (st == PFT_OK) st = check(pft_synchronize(handle_), "compute");
    if (st != PFT_OK) throw st;
    if (match) {
      pft_match_stats m;
      std::memset(&m, 0, sizeof(m));
      st = check(pft_get_match(handle_, &m), "compute");
      if (st != PFT_OK) throw st;
      if (m.lost) throw (int)PFT_ERR_LOST;
    }
  }
  bool ensure() {
    if (handle_) return true;
    int st = pft_create(&cfg_, &handle_);
    if (st != PFT_OK) {
      check(st, "create");
      handle_ = nullptr;
      return false;
    }
    pft_set_trans(handle_, trans_.m);
    if (use_cd_ || cd_interval_ != 10 || cd_min_points_ != 10 || cd_resolution_ != 0.01) forwardChangeDetector();
    if (match_min_ratio_ != 0.0 || match_lost_after_ != 1)
      check(pft_set_match_threshold(handle_, match_min_ratio_, match_lost_after_), "setMatchThreshold");
    if (spread_max_pos_sigma_ != HUGE_VAL || spread_min_n_eff_ != 0.0 || spread_after_ != 1)
      check(pft_set_spread_threshold(handle_, spread_max_pos_sigma_, spread_min_n_eff_, spread_after_), "setSpreadThreshold");
    if (vis_cam_set_) check(pft_set_visibility_camera(handle_, &vis_cam_), "setVisibilityCamera");
    if (vis_min_visible_ratio_ != 0.25 || vis_min_ratio_ != 0.0 || vis_lost_after_ != 1)
      check(pft_set_visibility_threshold(handle_, vis_min_visible_ratio_, vis_min_ratio_, vis_lost_after_), "setVisibilityThreshold");
    if (ref_) check(pft_set_reference(handle_, ref_->points.data(), ref_->points.size()), "setReferenceCloud");
    if (report_cloud_)
      check(pft_set_report_cloud(handle_, report_cloud_->points.data(), report_cloud_->points.size()), "setReportCloud");
    return true;
  }

  pft_config cfg_;
  pft_tracker* handle_;
  Affine3f trans_;
  PointCloudInConstPtr ref_, input_, report_cloud_;
  const pft_point_xyzrgba* dev_input_ = nullptr;
  size_t dev_n_ = 0;
  pft_filter* filter_input_ = nullptr;  // setInputCloudFromFilter
  size_t filter_max_ = 0;
  bool throw_on_failure_ = false;
  CoherencePtr coherence_;
  bool use_cd_ = false;
  unsigned int cd_interval_ = 10, cd_min_points_ = 10;
  double cd_resolution_ = 0.01;
  double match_min_ratio_ = 0.0;  // setMatchThreshold
  int match_lost_after_ = 1;
  double spread_max_pos_sigma_ = HUGE_VAL, spread_min_n_eff_ = 0.0;  // setSpreadThreshold
  int spread_after_ = 1;
  pft_visibility_config vis_cam_ = {};  // setVisibilityCamera
  bool vis_cam_set_ = false;
  double vis_min_visible_ratio_ = 0.25, vis_min_ratio_ = 0.0;  // setVisibilityThreshold
  int vis_lost_after_ = 1;
};

// the class the reference actually news (auto_tracking.cpp:203-204); the thread count is the OpenMP team
// size of PCL's CPU loops and has no meaning here
template <typename PointInT, typename StateT>
class ParticleFilterOMPTracker : public ParticleFilterTracker<PointInT, StateT> {
 public:
  explicit ParticleFilterOMPTracker(unsigned int nr_threads = 0) : threads_(nr_threads) {}
  unsigned int getNumberOfThreads() const { return threads_; }

 private:
  unsigned int threads_;
};

// the class the reference news unless use_fixed is set (auto_tracking.cpp:207-222, default :821): particle_num is
// the initial count, every resample draws until the KL bound is met (at most setMaximumParticleNum)
template <typename PointInT, typename StateT>
class KLDAdaptiveParticleFilterOMPTracker : public ParticleFilterTracker<PointInT, StateT> {
 public:
  explicit KLDAdaptiveParticleFilterOMPTracker(unsigned int nr_threads = 0) : threads_(nr_threads) {
    this->cfg_.kld_adaptive = 1;
  }
  void setMaximumParticleNum(unsigned int nr) { this->guard(); this->cfg_.maximum_particle_num = (int)nr; }
  void setDelta(double delta) { this->guard(); this->cfg_.kld_delta = delta; }
  void setEpsilon(double eps) { this->guard(); this->cfg_.kld_epsilon = eps; }
  void setBinSize(const StateT& bin_size) {
    this->guard();
    for (unsigned i = 0; i < 6; i++) this->cfg_.kld_bin_size[i] = bin_size[i];
  }
  unsigned int getNumberOfThreads() const { return threads_; }

 private:
  unsigned int threads_;
};

}  // namespace tracking
}  // namespace pft

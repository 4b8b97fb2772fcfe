// tracking_app.hpp -- what /root/reference/src/auto_tracking.cpp's OpenNISegmentTracking does around its trackers, without
// ROS / VTK, for any number of objects (shared by auto_tracking_amd.cpp and dist_tracking_amd.cpp):
//
//   buildTrackers()      one tracker per object, configured as initialize_trackers() does        :181-259
//   setObjectsToTrack()  the frame-#2 step: removeZeroPoints, centroid, re-centre, gridSample,
//                        setReferenceCloud / setTrans / setMinIndices                            :577-595, :646-677
//   objectPosition()     drawResult + viz_cb: the full-resolution model moved by the result pose
//                        (5 mm towards the camera "for better visualization") and its centroid,
//                        which the node publishes as the object's position                       :300-326, :432-466
//   setObjectsToTrackOnDevice()  the same step as one device pipeline per object (pft::ModelPreparation), from the model
//                        clouds or straight from a segmenter's clusters in HBM                  :646-677, :749-772
//   --device-report      the same on the device (pft_report), with viz_cb's principal-axis box       :432-466
//   --match              the match statistics of every result (pft_match) and the lost rule that makes the
//                        reference's "Object not recognized" handler fire; --reset-on-loss: resetTracking() then  :692-696
//   --spread             the population statistics behind every result (pft_spread): effective sample size, position
//                        ellipsoid, angle sigmas and the spread rule
//   --reacquire          a lost object is looked for among the cluster centroids of a segmentation of the frame
//                        (reacquire) and restarted where it is found
//   --refine             the pose found by --reacquire is refined against the frame (refine) before the restart
//   --discover           the frame minus the objects that are tracked (pft::SceneSubtraction) goes through the segmenter;
//                        every cluster of that residual becomes a new object
//   --reacquire-residual the segmentation that serves the lost objects runs on the residual of the objects still tracked
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "pft/common.hpp"
#include "pft/filters.hpp"
#include "pft/model_growth.hpp"
#include "pft/model_preparation.hpp"
#include "pft/pcd_io.hpp"
#include "pft/particle_filter_tracker.hpp"
#include "pft/scene_subtraction.hpp"

namespace app {

using namespace pft;
using namespace pft::tracking;

typedef PointXYZRGBA RefPointType;
typedef ParticleXYZRPY ParticleT;
typedef PointCloud<RefPointType> Cloud;
typedef ParticleFilterTracker<RefPointType, ParticleT> ParticleFilter;

struct Options {
  int particles = 400;                  // :231
  uint64_t seed = 1;                    // PCL's engines are time(0)-seeded; object k uses seed + k
  bool use_fixed = true;                // the reference's main() passes false (:821): the KLD-adaptive tracker
  double downsampling_grid_size = 0.01; // :824; 0 = the model is used as given
  unsigned threads = 16;                // :845, meaningless on the GPU
  bool pcl_sums = false;                // PCL's summation order for normalizeWeight / update (pft_config::sum_order)
  bool change_detector = false;         // PCL's change detector (setUseChangeDetector) with the three settings below
  unsigned int cd_interval = 10, cd_min_points = 10;
  double cd_resolution = 0.01;
  bool device_report = false;           // drawResult + viz_cb on the device: setReportCloud / computeReport / getReport
  bool match = false;                   // match statistics of every result: setMatchThreshold / computeMatch / getMatch
  double match_min_ratio = 0.0;         // lost after match_lost_after frames in a row below this matched share
  int match_lost_after = 1;
  bool reset_on_loss = false;           // resetTracking() on a lost object
  bool spread = false;                  // population statistics of every frame: setSpreadThreshold / computeSpread / getSpread
  double spread_max_pos_sigma = HUGE_VAL;  // uncertain after spread_after calls in a row above this position sigma
  double spread_min_n_eff = 0.0;        // or below this effective sample size
  int spread_after = 1;
  bool visibility = false;              // --visibility: setVisibilityCamera / computeVisibility / getVisibility per frame
  double vis_min_visible_ratio = 0.25;  // hidden below this visible share of the model
  double vis_occlusion_margin = 0.03;
  bool reacquire = false;               // a lost object is looked for among the clusters of the frame (pft_reacquire)
  bool refine = false;                  // --refine: the best candidate of a re-acquisition is refined (pft_refine)
  int rf_max_iterations = 16;
  double rf_pair_distance = 0.0;        // 0: the tracker's max_distance
  int rq_n_yaw = 8;                     // yaw steps over the full circle around the object's initial orientation
  double rq_accept_ratio = 0.5;         // inliers / model points a candidate needs
  double rq_inlier_distance = 0.02;
  bool discover = false;                // --discover: clusters of the frame that no tracked object explains become objects
  int discover_every = 1;               // every n-th frame
  double discover_radius = 0.02;        // the subtraction's radius (also --reacquire-residual's)
  bool grow_models = false;             // --grow-models: every bound object grows on the residual at its result pose
  int grow_confirm = 3, grow_reach = 2;  // pft_grow_config::confirm / reach
  double grow_max_radius = 0.5;         // pft_grow_config::max_radius
  bool reacquire_residual = false;      // --reacquire-residual: lost objects are looked for in the residual only
  bool view_reference = false;          // --view-reference: the reference cloud follows the visible side of a full model
  double view_angle = 0.2;              // re-selected once the result has turned this far (rad) from the last selection
  unsigned view_min_points = 1, view_max_points = 0;  // setReferenceFromView's floor, selectView's limit (0: none)
};

// *.pcd = PCD v0.7 with fields x y z rgba (create_model.cpp:219-222 writes them, :741 once loaded them);
// anything else = a raw array of 32-byte pcl::PointXYZRGBA records
inline Cloud::Ptr loadCloud(const char* path) {
  Cloud::Ptr c(new Cloud());
  const size_t len = std::strlen(path);
  if (len > 4 && !std::strcmp(path + len - 4, ".pcd")) {
    if (pft::io::loadPCDFile(path, *c) == -1) {
      std::fprintf(stderr, "pcd file not found or not readable: %s\n", path);
      c->points.clear();
    }
    return c;
  }
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    return c;
  }
  std::fseek(f, 0, SEEK_END);
  const long sz = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  c->points.resize((size_t)sz / sizeof(RefPointType));
  if (std::fread(c->points.data(), sizeof(RefPointType), c->points.size(), f) != c->points.size()) c->points.clear();
  std::fclose(f);
  c->width = (uint32_t)c->points.size();
  return c;
}

// keeps the points that are neither NaN nor within 1 cm of the sensor origin on all three axes (:577-595)
inline void removeZeroPoints(const Cloud& cloud, Cloud& result) {
  result.points.clear();
  for (const RefPointType& p : cloud.points) {
    const bool at_origin = std::fabs(p.x) < 0.01 && std::fabs(p.y) < 0.01 && std::fabs(p.z) < 0.01;
    if (!at_origin && !std::isnan(p.x) && !std::isnan(p.y) && !std::isnan(p.z)) result.points.push_back(p);
  }
  result.width = (uint32_t)result.points.size();
  result.height = 1;
  result.is_dense = true;
}

class TrackingApp {
 public:
  explicit TrackingApp(const Options& o) : opt_(o) {}

  std::map<int, std::shared_ptr<ParticleFilter>> tracker_dict;   // :153
  std::map<int, Cloud::Ptr> ref_cloud_dict;                      // the segmented object clusters, camera frame
  std::map<int, Cloud::Ptr> reference_dict;                      // re-centred, full resolution (:675)
  std::map<int, Cloud::Ptr> tracked_cloud_dict;                  // :325

  // one tracker per object, parameters of auto_tracking.cpp:187-254; `configure` lets a caller add what the reference
  // has no notion of (device, stream, shard) before the handle exists
  template <class F>
  void buildTrackers(int nb_objects, F&& configure) {
    for (int obj_id = 0; obj_id < nb_objects; obj_id++) addTracker(obj_id, configure);
  }
  // one more tracker with the same parameters (--discover adds objects while the frames run)
  template <class F>
  void addTracker(int obj_id, F&& configure) {
    std::vector<double> step_cov(6, 0.015 * 0.015);
    for (int k = 3; k < 6; k++) step_cov[k] *= 40.0;
    const std::vector<double> init_cov(6, 0.00001), init_mean(6, 0.0);
    {
      std::shared_ptr<ParticleFilter> tr;
      if (opt_.use_fixed) {
        tr.reset(new ParticleFilterOMPTracker<RefPointType, ParticleT>(opt_.threads));
      } else {
        auto* kld = new KLDAdaptiveParticleFilterOMPTracker<RefPointType, ParticleT>(opt_.threads);
        kld->setMaximumParticleNum(500);
        kld->setDelta(0.99);
        kld->setEpsilon(0.2);
        ParticleT bin;
        bin.x = bin.y = bin.z = bin.roll = bin.pitch = bin.yaw = 0.1f;
        kld->setBinSize(bin);
        tr.reset(kld);
      }
      tr->setTrans(Affine3f::Identity());
      tr->setStepNoiseCovariance(step_cov);
      tr->setInitialNoiseCovariance(init_cov);
      tr->setInitialNoiseMean(init_mean);
      tr->setIterationNum(2);
      tr->setParticleNum(opt_.particles);
      tr->setResampleLikelihoodThr(0.00);
      tr->setUseNormal(false);
      tr->setSeed(opt_.seed + (uint64_t)obj_id);
      tr->setSumOrder(opt_.pcl_sums ? PFT_SUM_PCL : PFT_SUM_TREE);
      if (opt_.change_detector) {
        tr->setIntervalOfChangeDetection(opt_.cd_interval);
        tr->setMinPointsOfChangeDetection(opt_.cd_min_points);
        tr->setResolutionOfChangeDetection(opt_.cd_resolution);
        tr->setUseChangeDetector(true);
      }
      ApproxNearestPairPointCloudCoherence<RefPointType>::Ptr coherence(new ApproxNearestPairPointCloudCoherence<RefPointType>());
      coherence->addPointCoherence(std::make_shared<DistanceCoherence<RefPointType>>());
      auto color = std::make_shared<HSVColorCoherence<RefPointType>>();
      color->setWeight(0.1);
      coherence->addPointCoherence(color);
      coherence->setSearchMethod(std::make_shared<search::Octree<RefPointType>>(0.01));
      coherence->setMaximumDistance(0.1);
      tr->setCloudCoherence(coherence);
      if (opt_.match) tr->setMatchThreshold(opt_.match_min_ratio, opt_.match_lost_after);
      if (opt_.spread) tr->setSpreadThreshold(opt_.spread_max_pos_sigma, opt_.spread_min_n_eff, opt_.spread_after);
      if (opt_.visibility) {  // the occlusion-aware rule takes over the match's thresholds
        pft_visibility_config cam;
        pft_visibility_config_default(&cam);
        cam.occlusion_margin = opt_.vis_occlusion_margin;
        tr->setVisibilityCamera(cam);
        tr->setVisibilityThreshold(opt_.vis_min_visible_ratio, opt_.match_min_ratio, opt_.match_lost_after);
      }
      configure(*tr, obj_id);
      tracker_dict[obj_id] = tr;
    }
  }

  // returns false if an object's model is empty
  bool setObjectsToTrack() {
    for (auto& kv : tracker_dict) {
      const int obj_id = kv.first;
      const Cloud::Ptr ref_cloud = ref_cloud_dict[obj_id];
      Cloud::Ptr nonzero_ref(new Cloud());
      removeZeroPoints(*ref_cloud, *nonzero_ref);
      if (nonzero_ref->empty()) {
        std::fprintf(stderr, "object %d: empty model\n", obj_id);
        return false;
      }
      float c[4] = {0, 0, 0, 1};
      compute3DCentroid(*nonzero_ref, c);  // the object's initial position
      Affine3f trans = Affine3f::Identity();
      trans(0, 3) = c[0];
      trans(1, 3) = c[1];
      trans(2, 3) = c[2];
      Cloud::Ptr transed_ref(new Cloud());
      transformPointCloud(*nonzero_ref, *transed_ref, inverseOfTranslation(trans));
      Cloud::Ptr transed_ref_downsampled(new Cloud());
      if (opt_.downsampling_grid_size > 0) {  // gridSample (:549-561): pcl::VoxelGrid, on the device
        pft::VoxelGrid grid;
        const float leaf = (float)opt_.downsampling_grid_size;
        grid.setLeafSize(leaf, leaf, leaf);
        grid.setInputCloud(transed_ref);
        grid.filter(*transed_ref_downsampled);
      } else {
        *transed_ref_downsampled = *transed_ref;
      }
      std::fprintf(stderr, "object %d ref_cloud: %zu data points, nonzero_ref: %zu, downsampled: %zu\n", obj_id,
                   ref_cloud->points.size(), nonzero_ref->points.size(), transed_ref_downsampled->points.size());
      kv.second->setReferenceCloud(transed_ref_downsampled);
      kv.second->setTrans(trans);
      recentre_dict_[obj_id] = trans;
      reference_dict[obj_id] = transed_ref;
      if (opt_.device_report) kv.second->setReportCloud(transed_ref);
      kv.second->setMinIndices((int)ref_cloud->points.size() / 2);
    }
    return true;
  }

  // setObjectsToTrack() on the device: every object's model goes through one pft::ModelPreparation pipeline
  // (removeZeroPoints, centroid, re-centring, gridSample) and reaches its tracker with setObjectFromModel, the
  // full-resolution cloud device to device.  Same prints, same return value.  reference_dict is filled only when the
  // host-side consumer asks for it (referenceCloud).
  bool setObjectsToTrackOnDevice() { return prepareOnDevice(nullptr); }
  // the same with the clusters of a segmenter's last apply as ref_cloud_dict, read where they lie in HBM: cluster j is
  // object j (the reference's service call, :749-772)
  bool setObjectsToTrackOnDevice(pft::ModelSegmenter& seg) { return prepareOnDevice(&seg); }

  // reference_dict[obj_id], fetched from the object's model preparation the first time it is asked for
  Cloud::Ptr referenceCloud(int obj_id) {
    auto it = reference_dict.find(obj_id);
    if (it != reference_dict.end() && it->second) return it->second;
    Cloud::Ptr c(new Cloud());
    auto mp = model_dict_.find(obj_id);
    if (mp != model_dict_.end()) mp->second->getRecentred(*c);
    reference_dict[obj_id] = c;
    return c;
  }

  // the tracked cloud of an object (drawResult) and its centroid (viz_cb), from a result pose
  void objectPosition(int obj_id, const ParticleT& result, float centroid[4]) {
    Affine3f transformation = tracker_dict[obj_id]->toEigenMatrix(result);
    transformation(2, 3) += -0.005f;  // "move a little bit for better visualization": the published centroid carries it
    Cloud::Ptr result_cloud(new Cloud());
    transformPointCloud(*referenceCloud(obj_id), *result_cloud, transformation);
    tracked_cloud_dict[obj_id] = result_cloud;
    centroid[0] = centroid[1] = centroid[2] = 0.0f;
    centroid[3] = 1.0f;
    compute3DCentroid(*result_cloud, centroid);
  }

  // the match hook of one object and frame, after its computeMatch(): prints the `match` line; a lost object gets the
  // reference's message (:695) and, with --reset-on-loss, a resetTracking() -- unless the caller deals with the loss itself
  // (reset = false: --reacquire).  With --visibility the loss is the occlusion-aware rule's, and a hidden object gets
  // `Object occluded` instead.  Returns true when the object is lost
  bool reportMatch(size_t frame, int obj_id, bool reset = true) {
    ParticleFilter& tr = *tracker_dict[obj_id];
    const pft_match_stats m = tr.getMatch();
    const double ratio = m.n_reference ? (double)m.n_matched / (double)m.n_reference : 0.0;
    std::printf("frame %zu object %d match %u / %u ratio %.6f coherence %.9g rms %.9g crop %u evaluated %u below %u streak %u lost %u\n",
                frame, obj_id, m.n_matched, m.n_reference, ratio, m.coherence,
                m.n_matched ? std::sqrt(m.sum_sq_dist / (double)m.n_matched) : 0.0, m.n_crop, m.evaluated, m.below, m.streak,
                m.lost);
    bool lost = m.lost != 0;
    if (opt_.visibility) {  // the occlusion-aware rule decides: a hidden object is not lost, whatever its match says
      const pft_visibility_stats vis = tr.getVisibility();
      if (vis.hidden) {
        std::fprintf(stderr, "frame %zu object %d: Object occluded\n", frame, obj_id);
        return false;
      }
      lost = vis.lost != 0;
    }
    if (!lost) return false;
    std::fprintf(stderr, "frame %zu object %d: Object not recognized\n", frame, obj_id);
    if (reset && opt_.reset_on_loss) tr.resetTracking();
    return true;
  }

  // the visibility hook of one object and frame, after its computeVisibility(): prints the `visibility` line
  void reportVisibility(int obj_id) {
    const pft_visibility_stats vis = tracker_dict[obj_id]->getVisibility();
    std::printf("visibility obj %d visible %u/%u occluded %u self %u out %u\n", obj_id, vis.n_visible, vis.n_reference,
                vis.n_occluded, vis.n_self, vis.n_out);
  }

  // the spread hook of one object and frame, after its computeSpread(): prints the `spread` line (every value round-trips)
  void reportSpread(int obj_id) {
    const pft_population_stats p = tracker_dict[obj_id]->getSpread();
    std::printf("spread obj %d: n_eff %.17g n %u zero %u w_max %.9g pos_sigma %.9g %.9g %.9g rpy_sigma %.17g %.17g %.17g "
                "evaluated %u uncertain %u streak %u flagged %u\n",
                obj_id, p.n_eff, p.n, p.n_zero, (double)p.w_max, (double)p.pos_sigma[0], (double)p.pos_sigma[1],
                (double)p.pos_sigma[2], p.rpy_sigma[0], p.rpy_sigma[1], p.rpy_sigma[2], p.evaluated, p.uncertain, p.streak,
                p.flagged);
  }

  // --reacquire: the objects `lost` in this frame (ascending ids) against the clusters of `seg`, a segmentation of the frame.
  // The first object takes its centres from the segmenter on the device; a centre accepted by one object is dropped for
  // the others.  One line per object; an object that finds no place falls back to --reset-on-loss
  template <class Segmenter>
  void reacquireLost(const std::vector<int>& lost, Segmenter& seg) {
    std::vector<float> centres;
    std::vector<int> cluster_of;  // the segmenter's cluster index of every centre still to be had
    bool have_centres = false;
    for (const int obj_id : lost) {
      ParticleFilter& tr = *tracker_dict[obj_id];
      pft_reacquire_config cfg = tr.reacquireConfig();
      cfg.n_yaw = opt_.rq_n_yaw;
      cfg.accept_ratio = opt_.rq_accept_ratio;
      cfg.inlier_distance = opt_.rq_inlier_distance;
      cfg.apply = opt_.refine ? 0 : 1;  // --refine: the lattice call only selects
      pft_reacquire_result res;
      int st;
      if (!have_centres) {
        st = tr.reacquireFromSegmenter(seg, cfg, res);
        if (st == PFT_OK) {
          centres.assign((size_t)res.n_centres * 3u, 0.0f);
          size_t k = 0;
          pft_get_reacquire_scores(tr.nativeHandle(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   centres.data(), 0, &k);
          for (uint32_t c = 0; c < res.n_centres; c++) cluster_of.push_back((int)c);
          have_centres = true;
        }
      } else {
        st = tr.reacquire(centres.data(), cluster_of.size(), cfg, res);
      }
      const bool accepted = st == PFT_OK && res.accepted;
      const int centre = st == PFT_OK && res.best_centre >= 0 ? cluster_of[(size_t)res.best_centre] : -1;
      std::printf("reacquire obj %d: centre %d candidate %d inliers %u/%u accepted %d\n", obj_id, centre,
                  st == PFT_OK ? res.best : -1, res.n_inliers, res.n_reference, accepted ? 1 : 0);
      if (opt_.refine && st == PFT_OK && res.best >= 0) refineBest(obj_id, tr, res, accepted);
      if (accepted) {
        centres.erase(centres.begin() + 3 * res.best_centre, centres.begin() + 3 * res.best_centre + 3);
        cluster_of.erase(cluster_of.begin() + res.best_centre);
      } else if (opt_.reset_on_loss) {
        tr.resetTracking();
      }
    }
  }

  // --refine: the best candidate of a re-acquisition refined against the frame (refine).  Of an accepted candidate the
  // refined pose is applied if the refinement improved it, else the candidate's own
  void refineBest(int obj_id, ParticleFilter& tr, const pft_reacquire_result& res, bool accepted) {
    pft_refine_config cfg = tr.refineConfig();
    cfg.max_iterations = opt_.rf_max_iterations;
    cfg.pair_distance = opt_.rf_pair_distance;
    cfg.apply = accepted ? 1 : 0;
    pft_refine_result r;
    const int st = tr.refine(res.transform, cfg, r);
    static const char* const names[] = {"CONVERGED", "MAX_ITERATIONS", "TOO_FEW_PAIRS"};
    std::printf("refine obj %d: iterations %u status %s inliers %u -> %u/%u improved %d\n", obj_id, r.iterations,
                st == PFT_OK && r.status < 3u ? names[r.status] : "FAILED", r.before.n_inliers, r.after.n_inliers, res.n_reference,
                st == PFT_OK && r.improved ? 1 : 0);
    if (accepted && !(st == PFT_OK && r.applied)) {
      Affine3f m = Affine3f::Identity();
      std::memcpy(m.m, res.transform, sizeof(float) * 12);
      tr.setTrans(m);
      tr.resetTracking();
    }
  }

  // --discover / --reacquire-residual: the frame (in HBM when d_frame is given, else `frame`) minus every object that is
  // not in `lost`, bound at its current result pose.  Slot k holds the k-th object bound (boundIds()); at most
  // PFT_SUBTRACT_MAX_OBJECTS objects are bound.  The residual stays in the subtraction until its next apply
  pft::SceneSubtraction& subtractTracked(const Cloud& frame, const pft_point_xyzrgba* d_frame, size_t d_n,
                                         const std::vector<int>& lost) {
    if (!subtraction_) subtraction_.reset(new pft::SceneSubtraction((float)opt_.discover_radius));
    subtraction_->clear();
    bound_ids_.clear();
    for (auto& kv : tracker_dict) {
      bool is_lost = false;
      for (const int id : lost) is_lost = is_lost || id == kv.first;
      if (is_lost) continue;
      if ((int)bound_ids_.size() == PFT_SUBTRACT_MAX_OBJECTS) {
        std::fprintf(stderr, "subtraction: more than %d tracked objects, object %d and later ones are not subtracted\n",
                     (int)PFT_SUBTRACT_MAX_OBJECTS, kv.first);
        break;
      }
      auto grown = grown_dict_.find(kv.first);
      if (grown != grown_dict_.end()) {  // --grow-models: the grown model at the result pose, an explicit slot
        const Affine3f pose = kv.second->toEigenMatrix(kv.second->getResult());
        subtraction_->setObject((int)bound_ids_.size(), *grown->second, pose.m);
      } else {
        subtraction_->bindTracker((int)bound_ids_.size(), *kv.second);
      }
      bound_ids_.push_back(kv.first);
    }
    if (d_frame) subtraction_->applyDevice(d_frame, d_n);
    else subtraction_->apply(frame);
    return *subtraction_;
  }
  const std::vector<int>& boundIds() const { return bound_ids_; }

  // --grow-models: every object of the last subtractTracked() grows on its residual at its result pose (pft::ModelGrowth;
  // `plane`: the scene's plane {a, b, c, d} in the camera frame, or null).  One line per object.  A model that grew becomes
  // the tracker's report cloud and what subtractTracked() subtracts from then on; the REFERENCE cloud stays as it was
  void growModels(pft::SceneSubtraction& sub, const float* plane) {
    for (const int obj_id : bound_ids_) {
      ParticleFilter& tr = *tracker_dict[obj_id];
      std::shared_ptr<pft::ModelGrowth>& g = growth_dict_[obj_id];
      if (!g) {
        pft_grow_config cfg = pft::ModelGrowth::defaults();
        cfg.confirm = opt_.grow_confirm;
        cfg.reach = opt_.grow_reach;
        cfg.max_radius = (float)opt_.grow_max_radius;
        g.reset(new pft::ModelGrowth(cfg));
        g->setModel(*referenceCloud(obj_id));
        if (plane) g->setPlanes(plane, 1);
      }
      g->applyTracker(tr, sub);
      const pft_grow_stats s = g->stats();
      std::printf("grow obj %d: candidates %u added %u model %u\n", obj_id, s.n_state[PFT_GROW_CANDIDATE] + s.n_added, s.n_added,
                  s.n_model_points);
      if (!s.n_added) continue;
      Cloud::Ptr grown(new Cloud());
      g->model(*grown);
      grown_dict_[obj_id] = grown;
      reference_dict[obj_id] = grown;
      tr.setReportCloud(grown);
    }
  }

  // --view-model: an object's full-surface model, in the coordinates of its model file; it is moved by the re-centring
  // transform the object's model got.  False for an empty cloud or an unknown object
  bool setViewModel(int obj_id, const Cloud& full) {
    auto rc = recentre_dict_.find(obj_id);
    Cloud::Ptr nonzero(new Cloud()), moved(new Cloud());
    removeZeroPoints(full, *nonzero);
    if (rc == recentre_dict_.end() || nonzero->empty()) return false;
    transformPointCloud(*nonzero, *moved, inverseOfTranslation(rc->second));
    view_model_dict_[obj_id] = moved;
    return true;
  }

  // --view-reference, after a frame's result: once the result has turned more than view_angle away from the pose of the
  // object's last selection (the first result always selects), the visible side of the object's full model at the result
  // pose -- the grown model under --grow-models, else its --view-model -- becomes the reference cloud.  One line per
  // selection; a refusal prints its text and the tracking goes on with the old reference
  void updateViewReference(size_t frame, int obj_id, const ParticleT& result) {
    ParticleFilter& tr = *tracker_dict[obj_id];
    const Affine3f now = tr.toEigenMatrix(result);
    auto last = view_pose_dict_.find(obj_id);
    if (last != view_pose_dict_.end()) {
      double trace = 0.0;  // of R_last^T R_now
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) trace += (double)last->second(r, c) * (double)now(r, c);
      const double cosine = std::min(1.0, std::max(-1.0, (trace - 1.0) / 2.0));
      if (!(std::acos(cosine) > opt_.view_angle)) return;
    }
    int st = PFT_ERR_STATE;
    auto g = growth_dict_.find(obj_id);
    auto m = view_model_dict_.find(obj_id);
    if (opt_.grow_models && g != growth_dict_.end() && g->second) st = tr.selectView(*g->second, nullptr, opt_.view_max_points);
    else if (!opt_.grow_models && m != view_model_dict_.end()) st = tr.selectView(*m->second, nullptr, opt_.view_max_points);
    else return;  // no full model (yet)
    if (st != PFT_OK) return;
    const pft_view_stats v = tr.getView();
    if (!v.evaluated) return;
    std::printf("view obj %d frame %zu: model %u visible %u kept %u\n", obj_id, frame, v.n_model, v.n_visible, v.n_kept);
    if (tr.setReferenceFromView(opt_.view_min_points) == PFT_OK) view_pose_dict_[obj_id] = now;
  }

  // --discover: the clusters of `seg` (a segmentation of the residual) become objects with the next free ids, prepared on
  // the device from where the clusters lie (the --segment path).  One line per new object
  template <class F>
  void discoverObjects(size_t frame, pft::ModelSegmenter& seg, F&& configure) {
    const std::vector<uint32_t> sizes = seg.clusterSizes();
    for (size_t c = 0; c < sizes.size(); c++) {
      const int obj_id = tracker_dict.empty() ? 0 : tracker_dict.rbegin()->first + 1;
      addTracker(obj_id, configure);
      if (!prepareOne(obj_id, *tracker_dict[obj_id], &seg, c)) {
        tracker_dict.erase(obj_id);
        continue;
      }
      std::printf("discover frame %zu: cluster %zu -> obj %d (%u points)\n", frame, c, obj_id, sizes[c]);
    }
  }

  const Options& options() const { return opt_; }

 private:
  Options opt_;
  std::map<int, std::shared_ptr<pft::ModelPreparation>> model_dict_;  // the device-side models, one handle per object
  std::unique_ptr<pft::SceneSubtraction> subtraction_;                // created by the first subtractTracked()
  std::vector<int> bound_ids_;                                        // object of every slot of the last subtractTracked()
  std::map<int, std::shared_ptr<pft::ModelGrowth>> growth_dict_;      // --grow-models: one handle per object
  std::map<int, Cloud::Ptr> grown_dict_;                              // the objects whose model grew, and that model
  std::map<int, Affine3f> recentre_dict_;                             // the re-centring translation of every object's model
  std::map<int, Cloud::Ptr> view_model_dict_;                         // --view-model: the full model, re-centred
  std::map<int, Affine3f> view_pose_dict_;                            // --view-reference: the pose of the last selection

  bool prepareOnDevice(pft::ModelSegmenter* seg) {
    for (auto& kv : tracker_dict)
      if (!prepareOne(kv.first, *kv.second, seg, (size_t)kv.first)) return false;
    return true;
  }
  // one object's model from its model cloud, or from cluster `cluster` of a segmenter's last apply
  bool prepareOne(int obj_id, ParticleFilter& tracker, pft::ModelSegmenter* seg, size_t cluster) {
    {
      std::shared_ptr<pft::ModelPreparation> mp(new pft::ModelPreparation());
      if (seg) mp->setInputFromSegmenter(*seg, cluster);
      else mp->setInputCloud(ref_cloud_dict[obj_id]);
      mp->setLeafSize(opt_.downsampling_grid_size > 0 ? (float)opt_.downsampling_grid_size : 0.0f);
      if (!mp->prepare()) {
        std::fprintf(stderr, "object %d: empty model\n", obj_id);
        return false;
      }
      std::fprintf(stderr, "object %d ref_cloud: %zu data points, nonzero_ref: %zu, downsampled: %zu\n", obj_id,
                   mp->inputPoints(), mp->nonzeroPoints(), mp->referencePoints());
      if (tracker.setObjectFromModel(*mp, opt_.device_report) != PFT_OK) return false;
      model_dict_[obj_id] = mp;
      recentre_dict_[obj_id] = mp->getTrans();
      reference_dict.erase(obj_id);
      tracker.setMinIndices((int)mp->inputPoints() / 2);
    }
    return true;
  }
};

// pose and published position of one object for one frame; %.9g round-trips a float, so a test can feed the pose back to the oracle
inline void printObjectLine(size_t frame, int obj_id, const ParticleT& r, const float c[4]) {
  std::printf("frame %zu object %d pose %.9g %.9g %.9g %.9g %.9g %.9g  centroid %.9g %.9g %.9g\n", frame, obj_id, r.x, r.y, r.z,
              r.roll, r.pitch, r.yaw, c[0], c[1], c[2]);
}

// viz_cb's box (viz.addCube(tfinal, qfinal, size...)) from the device report: centre, quaternion {x, y, z, w}, size
inline void printBoxLine(size_t frame, int obj_id, const pft_object_report& r) {
  std::printf("frame %zu object %d box %.9g %.9g %.9g  quat %.9g %.9g %.9g %.9g  size %.9g %.9g %.9g\n", frame, obj_id,
              r.box_centre[0], r.box_centre[1], r.box_centre[2], r.box_quat[0], r.box_quat[1], r.box_quat[2], r.box_quat[3],
              r.box_size[0], r.box_size[1], r.box_size[2]);
}

}  // namespace app

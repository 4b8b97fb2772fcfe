// segmentation.hpp -- header-only C++ mirror, over the C ABI of include/pft_segment.h, of the PCL classes the
// reference's model-creation nodes run (create_model_planar_segmentation.cpp:131-203, create_model.cpp:131-179):
//
//   pcl::SACSegmentation<PointXYZRGBA>            setMaxIterations / setDistanceThreshold / segment
//   pcl::EuclideanClusterExtraction<PointXYZRGBA> setClusterTolerance / setMin/MaxClusterSize / extract
//
// pft::ModelSegmenter is the fused pipeline (transform, removeZeroPoints, plane, ExtractIndices negative, PassThrough
// box, clustering) of one device handle.  All compute happens in the HIP library; failures throw std::runtime_error.
// setPlaneRounds makes it the loop of test/cluster_euclid.cpp:59-85 and test/cluster_extraction.cpp: planes are removed
// one after the other while more than a fraction of the points is left.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "pft_segment.h"
#include "pft/particle_filter_tracker.hpp"

namespace pft {

struct PointIndices {
  std::vector<int> indices;
};

struct ModelCoefficients {
  std::vector<float> values;
};

class ModelSegmenter {
 public:
  explicit ModelSegmenter(int device_id = 0, void* hip_stream = nullptr) {
    pft_segment_default_config(&cfg_);
    cfg_.device_id = device_id;
    if (hip_stream) {
      cfg_.stream = hip_stream;
      cfg_.stream_is_external = 1;
    }
  }
  virtual ~ModelSegmenter() { close(); }
  ModelSegmenter(const ModelSegmenter&) = delete;
  ModelSegmenter& operator=(const ModelSegmenter&) = delete;

  pft_segment_config& config() {
    close();  // the next apply re-creates the handle with the changed configuration
    return cfg_;
  }
  // camera -> base, row-major (the tf lookup of :119)
  void setTransform(const float m[16]) {
    for (int k = 0; k < 16; k++) config().transform[k] = m[k];
    cfg_.transform_enable = 1;
  }
  void setPlane(bool on) { config().plane_enable = on ? 1 : 0; }
  // PassThrough limits, inclusive; axis 0 = x, 1 = y, 2 = z
  void setBox(int axis, bool enable, float lo, float hi) {
    config().box_enable[axis] = enable ? 1 : 0;
    cfg_.box_min[axis] = lo;
    cfg_.box_max[axis] = hi;
  }

  // planes are removed one after the other while (double)remaining > min_remaining_fraction * (double)n_valid and
  // fewer than max_planes (1 .. PFT_SEGMENT_MAX_PLANES) rounds ran: cluster_euclid.cpp runs (no cap, 0.3)
  void setPlaneRounds(int max_planes, double min_remaining_fraction) {
    if (max_planes < 1 || max_planes > PFT_SEGMENT_MAX_PLANES || !(min_remaining_fraction >= 0.0 && min_remaining_fraction <= 1.0))
      throw std::invalid_argument("setPlaneRounds: max_planes 1 .. 16, min_remaining_fraction within [0, 1]");
    max_planes_ = max_planes;
    min_fraction_ = min_remaining_fraction;
    if (h_) check(pft_segment_set_plane_rounds(h_, max_planes_, min_fraction_), "pft_segment_set_plane_rounds");
  }
  // PFT_SUM_PCL (default): the refit's serial float sums; PFT_SUM_TREE: pair trees over many workgroups
  void setRefitOrder(int order) {
    if (order != PFT_SUM_PCL && order != PFT_SUM_TREE) throw std::invalid_argument("setRefitOrder: PFT_SUM_PCL or PFT_SUM_TREE");
    refit_order_ = order;
    if (h_) check(pft_segment_set_refit_order(h_, refit_order_), "pft_segment_set_refit_order");
  }

  void setInputCloud(const PointCloud<PointXYZRGBA>::ConstPtr& cloud) {
    input_ = cloud;
    dev_in_ = nullptr;
  }
  void setInputCloudDevice(const pft_point_xyzrgba* device_points, size_t n) {
    input_.reset();
    dev_in_ = device_points;
    dev_n_ = n;
  }

  void apply() {
    if (!h_) {
      check(pft_segment_create(&cfg_, &h_), "pft_segment_create");
      check(pft_segment_set_plane_rounds(h_, max_planes_, min_fraction_), "pft_segment_set_plane_rounds");
      check(pft_segment_set_refit_order(h_, refit_order_), "pft_segment_set_refit_order");
    }
    if (dev_in_)
      check(pft_segment_apply_device(h_, dev_in_, dev_n_), "pft_segment_apply_device");
    else if (input_)
      check(pft_segment_apply(h_, input_->points.data(), input_->points.size()), "pft_segment_apply");
    else
      throw std::runtime_error("ModelSegmenter::apply without an input cloud");
  }

  pft_segment_plane plane() {
    pft_segment_plane p;
    check(pft_segment_get_plane(h_, &p), "pft_segment_get_plane");
    return p;
  }
  // planes the last apply removed / why the rounds ended (PFT_ROUNDS_STOP_*)
  size_t planeCount() {
    size_t n = 0;
    check(pft_segment_plane_count(h_, &n, nullptr), "pft_segment_plane_count");
    return n;
  }
  int stoppedBy() {
    int why = 0;
    check(pft_segment_plane_count(h_, nullptr, &why), "pft_segment_plane_count");
    return why;
  }
  // the record of one round: n_valid is the round's cloud size, sample indexes the round's cloud
  pft_segment_plane plane(size_t round) {
    pft_segment_plane p;
    check(pft_segment_get_plane_round(h_, round, &p), "pft_segment_get_plane_round");
    return p;
  }
  // a round's inliers, indices into the input cloud: which = 0 the final ones, 1 those of the best hypothesis
  void planeInliers(size_t round, PointIndices& inliers, int which = 0) {
    const pft_segment_plane p = plane(round);
    std::vector<int32_t> idx(p.status == PFT_PLANE_FOUND ? (which == 0 ? p.inliers : p.ransac_inliers) : 0);
    size_t n = 0;
    check(pft_segment_get_plane_round_inliers(h_, round, which, idx.data(), idx.size(), &n),
          "pft_segment_get_plane_round_inliers");
    inliers.indices.assign(idx.begin(), idx.begin() + n);
  }
  // the final plane inliers, indices into the input cloud
  void planeInliers(PointIndices& inliers) {
    const pft_segment_plane p = plane();
    std::vector<int32_t> idx(p.status == PFT_PLANE_FOUND ? p.inliers : 0);
    size_t n = 0;
    check(pft_segment_get_plane_inliers(h_, 0, idx.data(), idx.size(), &n), "pft_segment_get_plane_inliers");
    inliers.indices.assign(idx.begin(), idx.begin() + n);
  }
  // cluster_indices: indices into the input cloud; clouds (may be null): the input's points of every cluster
  void clusters(std::vector<PointIndices>& cluster_indices, std::vector<PointCloud<PointXYZRGBA>>* clouds = nullptr) {
    size_t nc = 0;
    check(pft_segment_cluster_count(h_, &nc), "pft_segment_cluster_count");
    std::vector<uint32_t> sizes(nc);
    check(pft_segment_cluster_sizes(h_, sizes.data(), nc), "pft_segment_cluster_sizes");
    size_t total = 0;
    for (uint32_t s : sizes) total += s;
    std::vector<int32_t> idx(total);
    std::vector<PointXYZRGBA> pts(total);
    size_t n = 0;
    check(pft_segment_get_cluster_indices(h_, idx.data(), total, &n), "pft_segment_get_cluster_indices");
    if (clouds) check(pft_segment_get_cluster_points(h_, pts.data(), total, &n), "pft_segment_get_cluster_points");
    cluster_indices.assign(nc, PointIndices());
    if (clouds) clouds->assign(nc, PointCloud<PointXYZRGBA>());
    size_t o = 0;
    for (size_t c = 0; c < nc; c++) {
      cluster_indices[c].indices.assign(idx.begin() + o, idx.begin() + o + sizes[c]);
      if (clouds) {
        PointCloud<PointXYZRGBA>& cl = (*clouds)[c];
        cl.points.assign(pts.begin() + o, pts.begin() + o + sizes[c]);
        cl.width = sizes[c];
        cl.height = 1;
        cl.is_dense = true;
      }
      o += sizes[c];
    }
  }
  // the clusters' sizes in cluster order, and all their points one after the other where they lie in HBM (valid until
  // the next apply): what pft::ModelPreparation::setInputFromSegmenter reads
  std::vector<uint32_t> clusterSizes() {
    size_t nc = 0;
    check(pft_segment_cluster_count(h_, &nc), "pft_segment_cluster_count");
    std::vector<uint32_t> sizes(nc);
    check(pft_segment_cluster_sizes(h_, sizes.data(), nc), "pft_segment_cluster_sizes");
    return sizes;
  }
  void clustersDevice(const pft_point_xyzrgba** device_points, size_t* n_total) {
    check(pft_segment_clusters_device(h_, device_points, n_total), "pft_segment_clusters_device");
  }
  pft_segment* nativeHandle() { return h_; }
  double lastMilliseconds() const {
    double ms = 0.0;
    if (h_) pft_segment_last_ms(h_, &ms, nullptr);
    return ms;
  }

 protected:
  pft_segment_config cfg_;
  void close() {
    if (h_) pft_segment_destroy(h_);
    h_ = nullptr;
  }

 private:
  pft_segment* h_ = nullptr;
  int max_planes_ = 1;  // handle settings: applied to every handle apply() creates
  double min_fraction_ = 0.0;
  int refit_order_ = PFT_SUM_PCL;
  PointCloud<PointXYZRGBA>::ConstPtr input_;
  const pft_point_xyzrgba* dev_in_ = nullptr;
  size_t dev_n_ = 0;

  void check(int st, const char* what) {
    if (st != PFT_OK)
      throw std::runtime_error(std::string(what) + ": " + pft_status_string(st) + " " +
                               (h_ ? pft_segment_last_error_string(h_) : ""));
  }
};

// pcl::SACSegmentation<PointXYZRGBA>, SACMODEL_PLANE / SAC_RANSAC; removeZeroPoints runs first, as in the reference
class SACSegmentation : public ModelSegmenter {
 public:
  SACSegmentation() {
    config().plane_enable = 1;
    for (int a = 0; a < 3; a++) cfg_.box_enable[a] = 0;
    cfg_.min_cluster_size = 0x7fffffff;  // min > max: no clusters wanted, the clustering is skipped
    cfg_.max_cluster_size = 1;
  }
  void setMaxIterations(int n) { config().max_iterations = n; }
  void setDistanceThreshold(double t) { config().distance_threshold = t; }
  void setProbability(double p) { config().probability = p; }
  void setOptimizeCoefficients(bool on) { config().optimize_coefficients = on ? 1 : 0; }
  void segment(PointIndices& inliers, ModelCoefficients& coefficients) {
    apply();
    const pft_segment_plane p = plane();
    coefficients.values.clear();
    inliers.indices.clear();
    if (p.status != PFT_PLANE_FOUND) return;  // "Error segmenting the model! No solution found."
    coefficients.values.assign(p.coefficients, p.coefficients + 4);
    planeInliers(inliers);
  }
};

// pcl::EuclideanClusterExtraction<PointXYZRGBA>; removeZeroPoints runs first
class EuclideanClusterExtraction : public ModelSegmenter {
 public:
  EuclideanClusterExtraction() {
    config().plane_enable = 0;
    for (int a = 0; a < 3; a++) cfg_.box_enable[a] = 0;
  }
  void setClusterTolerance(double t) { config().cluster_tolerance = t; }
  void setMinClusterSize(int n) { config().min_cluster_size = n; }
  void setMaxClusterSize(int n) { config().max_cluster_size = n; }
  void extract(std::vector<PointIndices>& cluster_indices) {
    apply();
    clusters(cluster_indices);
  }
};

}  // namespace pft

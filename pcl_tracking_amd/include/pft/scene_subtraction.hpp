// scene_subtraction.hpp -- header-only C++ mirror, over the C ABI of include/pft_subtract.h, of scene subtraction:
// which points of a frame do the tracked objects at their current poses explain, and the rest as a cloud.
//
//   pft::SceneSubtraction sub(0.02f);
//   sub.bindTracker(0, tracker);            // the tracker's model at its current result pose, taken on the device
//   sub.setObject(1, cloud, matrix3x4);     // or an explicit cloud and matrix
//   sub.applyDevice(frame_in_hbm, n);       // enqueues and returns
//   sub.segmentResidual(segmenter);         // the residual goes to the segmenter device to device
//
// RAII over the handle; all compute happens in the HIP library; failures throw std::runtime_error.  A bound tracker is
// borrowed: removeObject (or destroy this object) before the tracker goes away or re-creates its handle.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "pft_subtract.h"
#include "pft/particle_filter_tracker.hpp"
#include "pft/segmentation.hpp"

namespace pft {

class SceneSubtraction {
 public:
  explicit SceneSubtraction(float radius = 0.02f, int cloud = PFT_SUBTRACT_REFERENCE_CLOUD, int device_id = 0) {
    pft_subtract_config cfg;
    pft_subtract_default_config(&cfg);
    cfg.radius = radius;
    cfg.cloud = cloud;
    cfg.device_id = device_id;
    check(pft_subtract_create(&cfg, &h_), "pft_subtract_create");
  }
  ~SceneSubtraction() {
    if (h_) pft_subtract_destroy(h_);
  }
  SceneSubtraction(const SceneSubtraction&) = delete;
  SceneSubtraction& operator=(const SceneSubtraction&) = delete;

  // explicit slot: only x, y, z of the cloud are read; m12 is a row-major 3x4 matrix
  void setObject(int slot, const PointCloud<PointXYZRGBA>& cloud, const float m12[12]) {
    check(pft_subtract_set_object(h_, slot, cloud.points.data(), cloud.points.size(), m12), "pft_subtract_set_object");
  }
  void setObjectMatrix(int slot, const float m12[12]) {
    check(pft_subtract_set_object_matrix(h_, slot, m12), "pft_subtract_set_object_matrix");
  }
  // bound slot: every apply takes the tracker's model and its current result pose on the device
  template <typename PointInT, typename StateT>
  void bindTracker(int slot, tracking::ParticleFilterTracker<PointInT, StateT>& tracker) {
    if (!tracker.create()) throw std::runtime_error("SceneSubtraction::bindTracker: the tracker has no device handle");
    check(pft_subtract_bind_tracker(h_, slot, tracker.nativeHandle()), "pft_subtract_bind_tracker");
  }
  void removeObject(int slot) { check(pft_subtract_remove_object(h_, slot), "pft_subtract_remove_object"); }
  void clear() { check(pft_subtract_clear(h_), "pft_subtract_clear"); }

  void apply(const PointCloud<PointXYZRGBA>& frame) {
    check(pft_subtract_apply(h_, frame.points.data(), frame.points.size()), "pft_subtract_apply");
  }
  void applyDevice(const pft_point_xyzrgba* device_points, size_t n) {
    check(pft_subtract_apply_device(h_, device_points, n), "pft_subtract_apply_device");
  }

  // results of the last apply: these wait for it
  void counts(size_t* n_in, size_t* n_explained, size_t* n_residual) {
    check(pft_subtract_counts(h_, n_in, n_explained, n_residual), "pft_subtract_counts");
  }
  std::vector<int32_t> owners() {
    std::vector<int32_t> v(nIn());
    check(pft_subtract_get_owner(h_, v.data(), v.size()), "pft_subtract_get_owner");
    return v;
  }
  std::vector<float> sqDistances() {
    std::vector<float> v(nIn());
    check(pft_subtract_get_sq_dist(h_, v.data(), v.size()), "pft_subtract_get_sq_dist");
    return v;
  }
  std::vector<uint32_t> support() {
    std::vector<uint32_t> v(PFT_SUBTRACT_MAX_OBJECTS);
    check(pft_subtract_get_support(h_, v.data(), v.size()), "pft_subtract_get_support");
    return v;
  }
  void residual(PointCloud<PointXYZRGBA>& out) {
    size_t n = 0;
    counts(nullptr, nullptr, &n);
    out.points.resize(n);
    check(pft_subtract_get_residual(h_, out.points.data(), n, &n), "pft_subtract_get_residual");
    out.width = (uint32_t)n;
    out.height = 1;
    out.is_dense = false;
  }
  std::vector<int32_t> residualIndices() {
    size_t n = 0;
    counts(nullptr, nullptr, &n);
    std::vector<int32_t> v(n);
    check(pft_subtract_get_residual_indices(h_, v.data(), n, &n), "pft_subtract_get_residual_indices");
    return v;
  }
  void residualDevice(const pft_point_xyzrgba** device_points, size_t* n) {
    check(pft_subtract_residual_device(h_, device_points, n), "pft_subtract_residual_device");
  }
  // the matrix and the moved points (x, y, z each) the last apply used for a slot
  void object(int slot, float m12[12], std::vector<float>* moved_xyz = nullptr) {
    size_t n = 0;
    check(pft_subtract_get_object(h_, slot, m12, nullptr, 0, &n), "pft_subtract_get_object");
    if (!moved_xyz) return;
    moved_xyz->resize(3 * n);
    check(pft_subtract_get_object(h_, slot, m12, moved_xyz->data(), n, &n), "pft_subtract_get_object");
  }
  double lastMilliseconds() {
    double ms = 0.0;
    check(pft_subtract_last_ms(h_, &ms), "pft_subtract_last_ms");
    return ms;
  }

  // the residual goes to the segmenter where it lies in HBM and the segmenter runs; the clusters' indices then point
  // into the residual: toFrameIndices maps them to the frame.  Returns the residual's size (0: the segmenter did not run)
  size_t segmentResidual(ModelSegmenter& segmenter) {
    const pft_point_xyzrgba* d = nullptr;
    size_t n = 0;
    residualDevice(&d, &n);
    if (n == 0) return 0;
    segmenter.setInputCloudDevice(d, n);
    segmenter.apply();
    return n;
  }
  // a cluster's indices into the residual -> indices into the frame the residual was taken from
  void toFrameIndices(PointIndices& cluster) {
    const std::vector<int32_t> idx = residualIndices();
    for (int& i : cluster.indices) i = idx.at((size_t)i);
  }
  pft_subtract* nativeHandle() { return h_; }

 private:
  pft_subtract* h_ = nullptr;
  size_t nIn() {
    size_t n = 0;
    counts(&n, nullptr, nullptr);
    return n;
  }
  void check(int st, const char* what) {
    if (st != PFT_OK)
      throw std::runtime_error(std::string(what) + ": " + pft_status_string(st) + " " +
                               (h_ ? pft_subtract_last_error_string(h_) : ""));
  }
};

}  // namespace pft

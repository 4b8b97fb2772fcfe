// model_growth.hpp -- header-only C++ mirror, over the C ABI of include/pft_grow.h, of model growth: fold surface that is
// seen next to an object's model, frame after frame, into the model.
//
//   pft::ModelGrowth grow;                      // or ModelGrowth(cfg) from ModelGrowth::defaults()
//   grow.setModel(model);                       // object frame
//   grow.setPlanes(table_abcd, 1);              // camera frame: points on these planes never enter
//   grow.applyResidual(sub, m12);               // the residual of a SceneSubtraction, device to device
//   if (grow.stats().n_added) { grow.model(cloud); tracker.setReportCloud(cloud); }
//
// The grown model is for the report cloud and the scene subtraction; the tracker's REFERENCE cloud stays what the user gave.
// RAII over the handle; all compute happens in the HIP library; failures throw std::runtime_error.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "pft_grow.h"
#include "pft/particle_filter_tracker.hpp"
#include "pft/scene_subtraction.hpp"

namespace pft {

class ModelGrowth {
 public:
  static pft_grow_config defaults() {
    pft_grow_config cfg;
    pft_grow_default_config(&cfg);
    return cfg;
  }
  explicit ModelGrowth(const pft_grow_config& cfg = defaults()) { check(pft_grow_create(&cfg, &h_), "pft_grow_create"); }
  ~ModelGrowth() {
    if (h_) pft_grow_destroy(h_);
  }
  ModelGrowth(const ModelGrowth&) = delete;
  ModelGrowth& operator=(const ModelGrowth&) = delete;

  void setModel(const PointCloud<PointXYZRGBA>& cloud) {
    check(pft_grow_set_model(h_, cloud.points.data(), cloud.points.size()), "pft_grow_set_model");
  }
  void setModelDevice(const pft_point_xyzrgba* device_points, size_t n) {
    check(pft_grow_set_model_device(h_, device_points, n), "pft_grow_set_model_device");
  }
  // n_planes x {a, b, c, d} in the camera frame
  void setPlanes(const float* abcd, size_t n_planes) { check(pft_grow_set_planes(h_, abcd, n_planes), "pft_grow_set_planes"); }

  // m12: the object's pose, a row-major 3x4 matrix.  Enqueues and returns
  void apply(const PointCloud<PointXYZRGBA>& cloud, const float m12[12]) {
    check(pft_grow_apply(h_, cloud.points.data(), cloud.points.size(), m12), "pft_grow_apply");
  }
  void applyDevice(const pft_point_xyzrgba* device_points, size_t n, const float m12[12]) {
    check(pft_grow_apply_device(h_, device_points, n, m12), "pft_grow_apply_device");
  }
  // the residual of the subtraction's last apply, where it lies in HBM (valid until the subtraction's next apply)
  void applyResidual(SceneSubtraction& sub, const float m12[12]) {
    const pft_point_xyzrgba* d = nullptr;
    size_t n = 0;
    sub.residualDevice(&d, &n);
    applyDevice(d, n, m12);
  }
  // at the tracker's result pose, read on the host
  template <typename PointInT, typename StateT>
  void applyTracker(tracking::ParticleFilterTracker<PointInT, StateT>& tracker, SceneSubtraction& sub) {
    float m12[12];
    resultMatrix(tracker, m12);
    applyResidual(sub, m12);
  }
  template <typename PointInT, typename StateT>
  void applyTracker(tracking::ParticleFilterTracker<PointInT, StateT>& tracker, const PointCloud<PointXYZRGBA>& cloud) {
    float m12[12];
    resultMatrix(tracker, m12);
    apply(cloud, m12);
  }

  // results: these wait for the last apply
  pft_grow_stats stats() {
    pft_grow_stats s;
    check(pft_grow_get_stats(h_, &s), "pft_grow_get_stats");
    return s;
  }
  std::vector<uint8_t> states() {
    std::vector<uint8_t> v(stats().n_in);
    check(pft_grow_get_states(h_, v.data(), v.size()), "pft_grow_get_states");
    return v;
  }
  void model(PointCloud<PointXYZRGBA>& out) {
    size_t n = stats().n_model_points;
    out.points.resize(n);
    check(pft_grow_get_model(h_, out.points.data(), n, &n), "pft_grow_get_model");
    out.width = (uint32_t)n;
    out.height = 1;
    out.is_dense = true;
  }
  void modelDevice(const pft_point_xyzrgba** device_points, size_t* n) {
    check(pft_grow_model_device(h_, device_points, n), "pft_grow_model_device");
  }
  void transform(float ti12[12]) { check(pft_grow_get_transform(h_, ti12), "pft_grow_get_transform"); }
  double lastMilliseconds() {
    double ms = 0.0;
    check(pft_grow_last_ms(h_, &ms), "pft_grow_last_ms");
    return ms;
  }
  // every MODEL and live PENDING voxel, sorted by key
  struct Table {
    std::vector<int32_t> keys;  // three per entry
    std::vector<uint32_t> kind, hits, last_seen;
  };
  Table debugTable() {
    size_t n = 0;
    check(pft_debug_grow_get_table(h_, nullptr, nullptr, nullptr, nullptr, 0, &n), "pft_debug_grow_get_table");
    Table t;
    t.keys.resize(3 * n);
    t.kind.resize(n);
    t.hits.resize(n);
    t.last_seen.resize(n);
    check(pft_debug_grow_get_table(h_, t.keys.data(), t.kind.data(), t.hits.data(), t.last_seen.data(), n, &n),
          "pft_debug_grow_get_table");
    return t;
  }
  pft_grow* nativeHandle() { return h_; }

 private:
  pft_grow* h_ = nullptr;
  template <typename TrackerT>
  static void resultMatrix(TrackerT& tracker, float m12[12]) {
    const Affine3f a = tracker.toEigenMatrix(tracker.getResult());
    for (int k = 0; k < 12; k++) m12[k] = a.m[k];
  }
  void check(int st, const char* what) {
    if (st != PFT_OK)
      throw std::runtime_error(std::string(what) + ": " + pft_status_string(st) + " " + pft_grow_last_error_string(h_));
  }
};

}  // namespace pft

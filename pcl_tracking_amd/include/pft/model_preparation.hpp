// model_preparation.hpp -- header-only C++ mirror, over the C ABI of include/pft_model.h, of the "set object to track"
// block of the reference's cloud_cb (auto_tracking.cpp:643-677): removeZeroPoints, compute3DCentroid, the re-centring by
// trans.inverse() and gridSample, as one device pipeline.
//
//   pft::ModelPreparation mp;
//   mp.setInputFromSegmenter(seg, j);  mp.setLeafSize(0.01f);  mp.prepare();
//   tracker.setObjectFromModel(mp, /*with_report_cloud=*/true);          // :673-675
//
// All compute happens in the HIP library; failures throw std::runtime_error, except an empty model (no point left after
// removeZeroPoints), for which prepare() returns false as the reference's caller tests it.
#pragma once
#include <stdexcept>
#include <string>

#include "pft_model.h"
#include "pft/particle_filter_tracker.hpp"
#include "pft/segmentation.hpp"

namespace pft {

class ModelPreparation {
 public:
  explicit ModelPreparation(int device_id = 0) : device_id_(device_id) {}
  ~ModelPreparation() {
    if (h_) pft_model_destroy(h_);
  }
  ModelPreparation(const ModelPreparation&) = delete;
  ModelPreparation& operator=(const ModelPreparation&) = delete;

  void setInputCloud(const PointCloud<PointXYZRGBA>::ConstPtr& cloud) {
    clearInput();
    input_ = cloud;
  }
  void setInputCloudDevice(const pft_point_xyzrgba* device_points, size_t n) {
    clearInput();
    dev_in_ = device_points;
    dev_n_ = n;
  }
  // cluster j of the segmenter's last apply, read where it lies in HBM
  void setInputFromSegmenter(ModelSegmenter& seg, size_t j) {
    clearInput();
    seg_ = &seg;
    seg_j_ = j;
  }
  // gridSample's leaf (downsampling_grid_size_, 0.01); <= 0: the reference cloud is the re-centred cloud
  void setLeafSize(float leaf) { leaf_ = leaf; }

  // false: no point left after removeZeroPoints (the reference's empty model)
  bool prepare() {
    if (!h_) check(pft_model_create(device_id_, &h_), "pft_model_create");
    int st;
    if (seg_)
      st = pft_model_prepare_from_segment(h_, seg_->nativeHandle(), seg_j_, leaf_);
    else if (dev_in_)
      st = pft_model_prepare_device(h_, dev_in_, dev_n_, leaf_);
    else if (input_)
      st = pft_model_prepare(h_, input_->points.data(), input_->points.size(), leaf_);
    else
      throw std::runtime_error("ModelPreparation::prepare without an input");
    if (st == PFT_ERR_NO_INPUT) return false;
    check(st, "pft_model_prepare");
    return true;
  }

  size_t inputPoints() const { return count(0); }
  size_t nonzeroPoints() const { return count(1); }
  size_t referencePoints() const { return count(2); }

  Affine3f getTrans() const {
    Affine3f t;
    check(pft_model_get_trans(h_, t.m), "pft_model_get_trans");
    return t;
  }
  // transed_ref: the re-centred, full-resolution model (reference_dict[obj])
  void getRecentred(PointCloud<PointXYZRGBA>& cloud) { fetch(cloud, pft_model_get_recentred, nonzeroPoints()); }
  // transed_ref_downsampled: what the tracker takes as its reference cloud
  void getReference(PointCloud<PointXYZRGBA>& cloud) { fetch(cloud, pft_model_get_reference, referencePoints()); }
  double lastMilliseconds() const {
    double ms = 0.0;
    if (h_) pft_model_last_ms(h_, &ms, nullptr);
    return ms;
  }
  pft_model* nativeHandle() { return h_; }

 private:
  int device_id_;
  pft_model* h_ = nullptr;
  float leaf_ = 0.01f;
  PointCloud<PointXYZRGBA>::ConstPtr input_;
  const pft_point_xyzrgba* dev_in_ = nullptr;
  size_t dev_n_ = 0;
  ModelSegmenter* seg_ = nullptr;
  size_t seg_j_ = 0;

  void clearInput() {
    input_.reset();
    dev_in_ = nullptr;
    seg_ = nullptr;
  }
  size_t count(int which) const {
    size_t c[3] = {0, 0, 0};
    check(pft_model_counts(h_, &c[0], &c[1], &c[2]), "pft_model_counts");
    return c[which];
  }
  void fetch(PointCloud<PointXYZRGBA>& cloud, int (*get)(pft_model*, pft_point_xyzrgba*, size_t, size_t*), size_t n) {
    cloud.points.resize(n);
    size_t got = 0;
    check(get(h_, cloud.points.data(), n, &got), "pft_model_get_cloud");
    cloud.width = (uint32_t)n;
    cloud.height = 1;
    cloud.is_dense = true;
  }
  void check(int st, const char* what) const {
    if (st != PFT_OK)
      throw std::runtime_error(std::string(what) + ": " + pft_status_string(st) + " " +
                               (h_ ? pft_model_last_error_string(h_) : ""));
  }
};

}  // namespace pft

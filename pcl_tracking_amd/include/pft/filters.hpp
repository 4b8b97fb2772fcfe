// filters.hpp -- header-only C++ mirror, over the C ABI of include/pft_filters.h, of the PCL filter classes
// that /root/reference/src/auto_tracking.cpp runs in front of the tracker:
//
//   pcl::PassThrough<PointType>            filterPassThrough   :536-547
//   pcl::VoxelGrid<PointType>              gridSample          :549-561
//   pcl::ApproximateVoxelGrid<PointType>   gridSampleApprox    :563-575
//
// Same member names and argument meaning (setFilterFieldName / setFilterLimits / setKeepOrganized /
// setLeafSize / setInputCloud / filter).  pft::InputFilter is the fused form the MI355X path prefers:
// PassThrough + voxel grid in one device pipeline whose output cloud stays in HBM and is handed to
// ParticleFilterTracker::setInputCloudDevice without touching the host.  All compute happens in the HIP
// library; filter() throws std::runtime_error on a HIP failure, as a PCL filter never silently degrades.
#pragma once
#include <stdexcept>
#include <string>

#include "pft_filters.h"
#include "pft/particle_filter_tracker.hpp"

namespace pft {

// the pinhole camera of a depth frame; the defaults are pft_depth_frame_default's (Kinect2 qhd, 960 x 540)
struct DepthCamera {
  float fx = 540.0f, fy = 540.0f, cx = 479.5f, cy = 269.5f;
};

class InputFilter {
 public:
  explicit InputFilter(int device_id = 0, void* hip_stream = nullptr) {
    pft_filter_default_config(&cfg_);
    cfg_.device_id = device_id;
    if (hip_stream) {
      cfg_.stream = hip_stream;
      cfg_.stream_is_external = 1;
    }
  }
  virtual ~InputFilter() { close(); }
  InputFilter(const InputFilter&) = delete;
  InputFilter& operator=(const InputFilter&) = delete;

  void setPassThrough(const std::string& field, float lo, float hi, bool negative = false, bool enable = true) {
    cfg_.pass_enable = enable ? 1 : 0;
    cfg_.pass_field = field == "x" ? 0 : (field == "y" ? 1 : 2);
    cfg_.pass_min = lo;
    cfg_.pass_max = hi;
    cfg_.pass_negative = negative ? 1 : 0;
    close();
  }
  void setVoxelMode(int mode) {
    cfg_.voxel_mode = mode;
    close();
  }
  void setLeafSize(float lx, float ly, float lz) {
    cfg_.leaf_size[0] = lx;
    cfg_.leaf_size[1] = ly;
    cfg_.leaf_size[2] = lz;
    close();
  }
  void setHistorySize(unsigned n) {
    cfg_.approx_hist_size = n;
    close();
  }

  void setInputCloud(const PointCloud<PointXYZRGBA>::ConstPtr& cloud) {
    input_ = cloud;
    dev_in_ = nullptr;
    depth_ = nullptr;
  }
  // a cloud already in HBM (n 32-byte points)
  void setInputCloudDevice(const pft_point_xyzrgba* device_points, size_t n) {
    input_.reset();
    dev_in_ = device_points;
    dev_n_ = n;
    depth_ = nullptr;
  }
  // The frame as the sensor delivers it: a registered depth image and an optional colour image in host memory, described
  // by a pft_depth_frame (include/pft_filters.h has the specification).  The organised cloud of width x height records is
  // formed on the device; filter / filterDevice / filterAsync then work as on a cloud.  The images are borrowed until the
  // filter call returns; pointers of depthHostBuffers make filterAsync wait for nothing
  void setInputDepth(const pft_depth_frame& frame, const void* depth, const void* color) {
    input_.reset();
    dev_in_ = nullptr;
    frame_ = frame;
    depth_ = depth;
    color_ = color;
  }
  // 16-bit depth (divided by depth_divisor) + packed colour, both tightly packed
  void setInputDepth(const uint16_t* depth, const uint8_t* color, int width, int height, const DepthCamera& cam = DepthCamera(),
                     float depth_divisor = 1000.0f, int color_format = PFT_COLOR_BGR8) {
    setInputDepth(depthFrame(width, height, cam, PFT_DEPTH_U16, depth_divisor, color ? color_format : PFT_COLOR_NONE), depth, color);
  }
  static pft_depth_frame depthFrame(int width, int height, const DepthCamera& cam = DepthCamera(), int depth_format = PFT_DEPTH_U16,
                                    float depth_divisor = 1000.0f, int color_format = PFT_COLOR_BGR8) {
    pft_depth_frame d;
    pft_depth_frame_default(&d);
    d.width = width;
    d.height = height;
    d.fx = cam.fx;
    d.fy = cam.fy;
    d.cx = cam.cx;
    d.cy = cam.cy;
    d.depth_format = depth_format;
    d.depth_divisor = depth_divisor;
    d.color_format = color_format;
    return d;
  }
  // pinned slot `slot` (0 or 1) of the handle, sized for `frame`: fill it, pass its pointers to setInputDepth, and write
  // to it again only when depthSlotDone(slot) says its upload has finished.  The slots die with the handle (any set* call
  // that changes the configuration)
  void depthHostBuffers(int slot, const pft_depth_frame& frame, void** depth, void** color) {
    if (!h_) check(pft_filter_create(&cfg_, &h_), "pft_filter_create");
    check(pft_filter_depth_host_buffers(h_, &frame, slot, depth, color), "pft_filter_depth_host_buffers");
  }
  bool depthSlotDone(int slot, bool wait = false) {
    if (!h_) return true;
    int done = 0;
    check(pft_filter_depth_slot_done(h_, slot, wait ? 1 : 0, &done), "pft_filter_depth_slot_done");
    return done != 0;
  }
  // the input cloud of the last filter call where the handle owns it (the cloud a depth apply formed, the upload of a
  // host cloud), in HBM, valid until the next filter call: what ModelSegmenter / SceneSubtraction take
  void inputDevice(const pft_point_xyzrgba** device_points, size_t* n) {
    if (!h_) throw std::runtime_error("inputDevice() before filter()");
    check(pft_filter_input_device(h_, device_points, n), "pft_filter_input_device");
  }
  void inputCloud(PointCloud<PointXYZRGBA>& cloud) {
    const pft_point_xyzrgba* p = nullptr;
    size_t n = 0, got = 0;
    inputDevice(&p, &n);
    cloud.points.resize(n);
    check(pft_filter_get_input(h_, cloud.points.data(), n, &got), "pft_filter_get_input");
    const bool organised = depth_ && (size_t)frame_.width * (size_t)frame_.height == n;
    cloud.width = organised ? (uint32_t)frame_.width : (uint32_t)n;
    cloud.height = organised ? (uint32_t)frame_.height : 1;
    cloud.is_dense = false;
  }

  // pcl::Filter::filter(PointCloud& output)
  void filter(PointCloud<PointXYZRGBA>& output) {
    apply();
    size_t n_pass = 0, n_out = 0;
    check(pft_filter_counts(h_, &n_pass, &n_out), "pft_filter_counts");
    output.points.resize(n_out);
    size_t got = 0;
    check(pft_filter_get_output(h_, output.points.data(), n_out, &got), "pft_filter_get_output");
    output.width = static_cast<uint32_t>(n_out);
    output.height = 1;          // downsampling breaks the organised structure
    output.is_dense = cfg_.voxel_mode != PFT_VOXEL_APPROX;  // ApproximateVoxelGrid: false, PassThrough / VoxelGrid: true
  }
  // fused path: output stays in HBM (valid until the next filter call on this object)
  void filterDevice(const pft_point_xyzrgba** device_points, size_t* n_out) {
    apply();
    check(pft_filter_output_device(h_, device_points, n_out), "pft_filter_output_device");
  }
  // the same pipeline, enqueued without waiting for it: the host cloud may be reused at once, a device cloud is borrowed
  // until the pipeline has run.  passedPoints / outputPoints / lastMilliseconds wait for it when first asked;
  // ParticleFilterTracker::setInputCloudFromFilter hands the output on without any wait
  void filterAsync() { apply(false); }
  pft_filter* nativeHandle() { return h_; }
  size_t outputPoints() const {
    size_t n_pass = 0, n_out = 0;
    if (h_) pft_filter_counts(h_, &n_pass, &n_out);
    return n_out;
  }
  size_t passedPoints() const {
    size_t n_pass = 0, n_out = 0;
    if (h_) pft_filter_counts(h_, &n_pass, &n_out);
    return n_pass;
  }
  double lastMilliseconds() const {
    double ms = 0.0;
    if (h_) pft_filter_last_ms(h_, &ms);
    return ms;
  }

 protected:
  pft_filter_config cfg_;

  void close() {
    if (h_) pft_filter_destroy(h_);
    h_ = nullptr;
  }

 private:
  pft_filter* h_ = nullptr;
  PointCloud<PointXYZRGBA>::ConstPtr input_;
  const pft_point_xyzrgba* dev_in_ = nullptr;
  size_t dev_n_ = 0;
  pft_depth_frame frame_ = {};
  const void* depth_ = nullptr;
  const void* color_ = nullptr;

  void check(int st, const char* what) {
    if (st != PFT_OK)
      throw std::runtime_error(std::string(what) + ": " + pft_status_string(st) + " " +
                               (h_ ? pft_filter_last_error_string(h_) : ""));
  }
  void apply(bool wait = true) {
    if (!h_) check(pft_filter_create(&cfg_, &h_), "pft_filter_create");
    if (dev_in_)
      check((wait ? pft_filter_apply_device : pft_filter_apply_device_async)(h_, dev_in_, dev_n_), "pft_filter_apply_device");
    else if (input_)
      check((wait ? pft_filter_apply : pft_filter_apply_async)(h_, input_->points.data(), input_->points.size()),
            "pft_filter_apply");
    else if (depth_)
      check((wait ? pft_filter_apply_depth : pft_filter_apply_depth_async)(h_, &frame_, depth_, color_), "pft_filter_apply_depth");
    else
      throw std::runtime_error("filter() without an input cloud");
  }
};

// pcl::PassThrough<PointXYZRGBA> (auto_tracking.cpp:536-547)
class PassThrough : public InputFilter {
 public:
  explicit PassThrough(int device_id = 0, void* hip_stream = nullptr) : InputFilter(device_id, hip_stream) {
    cfg_.voxel_mode = PFT_VOXEL_NONE;
    cfg_.pass_enable = 1;
  }
  void setFilterFieldName(const std::string& name) {
    cfg_.pass_field = name == "x" ? 0 : (name == "y" ? 1 : 2);
    close();
  }
  void setFilterLimits(float lo, float hi) {
    cfg_.pass_min = lo;
    cfg_.pass_max = hi;
    close();
  }
  void setFilterLimitsNegative(bool negative) {
    cfg_.pass_negative = negative ? 1 : 0;
    close();
  }
  void setKeepOrganized(bool keep) {
    if (keep) throw std::invalid_argument("keep_organized = true is not on the reference's path (auto_tracking.cpp:543)");
  }
};

// pcl::ApproximateVoxelGrid<PointXYZRGBA> (auto_tracking.cpp:563-575)
class ApproximateVoxelGrid : public InputFilter {
 public:
  explicit ApproximateVoxelGrid(int device_id = 0, void* hip_stream = nullptr) : InputFilter(device_id, hip_stream) {
    cfg_.voxel_mode = PFT_VOXEL_APPROX;
    cfg_.pass_enable = 0;
  }
};

// pcl::VoxelGrid<PointXYZRGBA> (auto_tracking.cpp:549-561)
class VoxelGrid : public InputFilter {
 public:
  explicit VoxelGrid(int device_id = 0, void* hip_stream = nullptr) : InputFilter(device_id, hip_stream) {
    cfg_.voxel_mode = PFT_VOXEL_EXACT;
    cfg_.pass_enable = 0;
  }
};

}  // namespace pft

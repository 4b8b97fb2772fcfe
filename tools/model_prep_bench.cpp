// model_prep_bench.cpp -- "set object to track" (auto_tracking.cpp:643-677) from a cluster that lies in HBM to a tracker
// that is ready to compute, two ways (tools/model_prep_bench.py builds and runs this):
//
//   host    the cluster is copied to the host, then TrackingApp::setObjectsToTrack(): removeZeroPoints, compute3DCentroid
//           and the re-centring on one CPU thread, gridSample on the device, setReferenceCloud / setTrans (/ setReportCloud)
//   device  pft::ModelPreparation::prepare() on the cluster where it lies, then setObjectFromModel
//
//   model_prep_bench <points> <reps> <report 0|1>   ->  one JSON line; wall-clock milliseconds, median of the repetitions
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../pcl_tracking_amd/examples/tracking_app.hpp"

using namespace app;

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s <points> <reps> <report 0|1>\n", argv[0]);
    return 2;
  }
  const size_t n = (size_t)std::atol(argv[1]);
  const int reps = std::atoi(argv[2]);
  Options opt;
  opt.device_report = std::atoi(argv[3]) != 0;
  // an object cluster as the segmenter leaves it: a 0.3 m cube around (0.1, -0.1, 0.8), a few invalid points
  std::mt19937 rng(12345);
  std::uniform_real_distribution<float> u(-0.15f, 0.15f);
  Cloud::Ptr cluster(new Cloud());
  cluster->points.resize(n);
  for (size_t i = 0; i < n; i++) {
    RefPointType& p = cluster->points[i];
    p.x = 0.1f + u(rng);
    p.y = -0.1f + u(rng);
    p.z = 0.8f + u(rng);
    p.rgba = (uint32_t)rng();
    if (i % 97 == 5) p.x = p.y = p.z = 0.001f;
  }
  pft_point_xyzrgba* d_cluster = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d_cluster), n * sizeof(pft_point_xyzrgba)) != hipSuccess ||
      hipMemcpy(d_cluster, cluster->points.data(), n * sizeof(pft_point_xyzrgba), hipMemcpyHostToDevice) != hipSuccess) {
    std::fprintf(stderr, "no device memory for the cluster\n");
    return 1;
  }
  if (!std::freopen("/dev/null", "w", stderr)) return 1;  // setObjectsToTrack prints one line per call

  TrackingApp host(opt), dev(opt);
  host.buildTrackers(1, [](ParticleFilter& tr, int) { tr.create(); });
  dev.buildTrackers(1, [](ParticleFilter& tr, int) { tr.create(); });
  pft::ModelPreparation mp;
  std::vector<double> t_host, t_dev, stage[PFT_MODEL_STAGES];
  size_t n_ref[2] = {0, 0};
  for (int r = -3; r < reps; r++) {  // three warm-up rounds; the two paths alternate
    double t0 = now_ms();
    Cloud::Ptr c(new Cloud());
    c->points.resize(n);
    if (hipMemcpy(c->points.data(), d_cluster, n * sizeof(pft_point_xyzrgba), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    host.ref_cloud_dict[0] = c;
    if (!host.setObjectsToTrack()) return 1;
    double t1 = now_ms();
    mp.setInputCloudDevice(d_cluster, n);
    mp.setLeafSize((float)opt.downsampling_grid_size);
    if (!mp.prepare() || dev.tracker_dict[0]->setObjectFromModel(mp, opt.device_report) != PFT_OK) return 1;
    double t2 = now_ms();
    if (r < 0) continue;
    t_host.push_back(t1 - t0);
    t_dev.push_back(t2 - t1);
    double ms = 0.0, st[PFT_MODEL_STAGES];
    pft_model_last_ms(mp.nativeHandle(), &ms, st);
    for (int k = 0; k < PFT_MODEL_STAGES; k++) stage[k].push_back(st[k]);
    n_ref[0] = host.tracker_dict[0]->getReferenceCloud()->points.size();
    n_ref[1] = mp.referencePoints();
  }
  std::printf("{\"points\": %zu, \"reps\": %d, \"report_cloud\": %d, \"reference_points\": [%zu, %zu], "
              "\"host_ms\": %.4f, \"device_ms\": %.4f, \"gpu_stage_us\": {\"remove_zero_points\": %.1f, \"centroid\": %.1f, "
              "\"recentre\": %.1f, \"grid_sample\": %.1f}}\n",
              n, reps, opt.device_report ? 1 : 0, n_ref[0], n_ref[1], median(t_host), median(t_dev), 1e3 * median(stage[0]),
              1e3 * median(stage[1]), 1e3 * median(stage[2]), 1e3 * median(stage[3]));
  (void)hipFree(d_cluster);
  return 0;
}

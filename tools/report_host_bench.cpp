// report_host_bench.cpp -- the host path the object report replaces (examples/tracking_app.hpp objectPosition + viz_cb's
// box steps), timed on one CPU thread: per object and frame, drawResult's transformPointCloud and compute3DCentroid
// (pft/common.hpp, as the driver runs them), then the covariance loop, the eigen-decomposition (the same scalar code the
// device runs in one lane, csrc/pft_report_solve.h), p2w, getMinMax3D and the box.  Built and run by
// tools/report_bench.py --host.
//
//   report_host_bench <n_points> <reps>   -> one JSON line: median microseconds of the centroid part and of the box part
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../pcl_tracking_amd/csrc/pft_report_solve.h"
#include "pft/common.hpp"
#include "pft/particle_filter_tracker.hpp"

using namespace pft;

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? std::strtoul(argv[1], nullptr, 10) : 25000;
  const int reps = argc > 2 ? std::atoi(argv[2]) : 50;
  PointCloud<PointXYZRGBA> ref;
  ref.points.resize(n);
  std::mt19937 g(7);
  std::normal_distribution<float> d(0.0f, 1.0f);
  for (auto& p : ref.points) {
    p.x = 0.1f * d(g);
    p.y = 0.05f * d(g);
    p.z = 0.02f * d(g);
    p.w = 1.0f;
  }
  ref.width = (uint32_t)n;
  pft_particle pose = {0.05f, -0.02f, 0.8f, 1.0f, 0.1f, -0.2f, 0.3f, 0.0f};
  std::vector<double> t_centroid, t_box;
  volatile float sink = 0.0f;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    // objectPosition: toEigenMatrix + offset, transformPointCloud, compute3DCentroid
    Affine3f T;
    pft_to_matrix(&pose, T.m);
    T.m[11] += -0.005f;
    PointCloud<PointXYZRGBA> tracked;
    transformPointCloud(ref, tracked, T);
    float c[4] = {0, 0, 0, 1};
    compute3DCentroid(tracked, c);
    const auto t1 = std::chrono::steady_clock::now();
    // viz_cb: computeCovarianceMatrixNormalized
    float C11 = 0, C12 = 0, C22 = 0, C00 = 0, C01 = 0, C02 = 0;
    for (const auto& p : tracked.points) {
      float x = p.x - c[0], y = p.y - c[1], z = p.z - c[2];
      C11 += y * y;
      C12 += y * z;
      C22 += z * z;
      y *= x;
      z *= x;
      x *= x;
      C00 += x;
      C01 += y;
      C02 += z;
    }
    const float nf = (float)n;
    float cov[3][3] = {{C00 / nf, C01 / nf, C02 / nf}, {C01 / nf, C11 / nf, C12 / nf}, {C02 / nf, C12 / nf, C22 / nf}};
    float ev[3], ax[3][3], q[4];
    report_solve(cov, ev, ax);
    Affine3f P;
    for (int i = 0; i < 3; i++) {
      for (int k = 0; k < 3; k++) P.m[4 * i + k] = ax[k][i];
      P.m[4 * i + 3] = -(ax[0][i] * c[0] + (ax[1][i] * c[1] + ax[2][i] * c[2]));
    }
    PointCloud<PointXYZRGBA> cp;
    transformPointCloud(tracked, cp, P);
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (const auto& p : cp.points) {
      const float v[3] = {p.x, p.y, p.z};
      for (int k = 0; k < 3; k++) {
        mn[k] = mn[k] < v[k] ? mn[k] : v[k];
        mx[k] = mx[k] > v[k] ? mx[k] : v[k];
      }
    }
    float centre[3];
    for (int i = 0; i < 3; i++) {
      const float md0 = 0.5f * (mx[0] + mn[0]), md1 = 0.5f * (mx[1] + mn[1]), md2 = 0.5f * (mx[2] + mn[2]);
      centre[i] = (ax[i][0] * md0 + (ax[i][1] * md1 + ax[i][2] * md2)) + c[i];
    }
    rp_quaternion(ax, q);
    const auto t2 = std::chrono::steady_clock::now();
    sink = sink + centre[0] + q[3] + ev[2];
    t_centroid.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
    t_box.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
  }
  std::printf("{\"side\": \"host\", \"points\": %zu, \"reps\": %d, \"centroid_us_median\": %.2f, \"box_us_median\": %.2f, "
              "\"total_us_median\": %.2f}\n",
              n, reps, median(t_centroid), median(t_box), median(t_centroid) + median(t_box));
  return 0;
}

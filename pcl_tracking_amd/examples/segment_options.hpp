// segment_options.hpp -- the model-creation flags shared by create_model_amd (which writes the clusters to files) and
// auto_tracking_amd --segment (which hands them to the trackers on the device): one parser, one meaning.
//
//   [--no-plane] [--transform m00 m01 ... m33] [--box xmin,xmax,ymin,ymax,zmin,zmax] [--tolerance T] [--min-size N]
//   [--max-size N] [--planes MAX[,FRACTION]] [--tree-refit] [--sac ITER,THRESHOLD] [--voxel LEAF]
//
// create_model_amd.cpp explains each of them.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pft/filters.hpp"
#include "pft/segmentation.hpp"
#include "tracking_app.hpp"

// the usage text of the flags, in two parts (create_model_amd prints its own --ascii between them)
#define APP_SEGMENT_USAGE_1 \
  "[--no-plane] [--transform 16 floats] [--box xmin,xmax,ymin,ymax,zmin,zmax] [--tolerance T] [--min-size N] [--max-size N]"
#define APP_SEGMENT_USAGE_2 "[--planes MAX[,FRACTION]] [--tree-refit] [--sac ITER,THRESHOLD] [--voxel LEAF]"

namespace app {

struct SegmentOptions {
  bool plane = true;
  bool have_transform = false, have_box = false;
  float T[16];
  float box[6];
  double tol = -1.0;
  int min_size = -1, max_size = -1;
  int max_planes = 0, sac_iter = -1;
  double fraction = 0.3, sac_thr = -1.0;
  float leaf = 0.0f;
  bool tree_refit = false;
};

// argv[i]: 1 = a segmentation flag, consumed with its values (i on the last of them); 0 = not one of ours; -1 = one of
// ours with a bad value, the message printed
inline int parseSegmentFlag(SegmentOptions& o, int argc, char** argv, int& i) {
  if (!std::strcmp(argv[i], "--no-plane")) o.plane = false;
  else if (!std::strcmp(argv[i], "--transform") && i + 16 < argc) {
    for (int k = 0; k < 16; k++) o.T[k] = std::strtof(argv[++i], nullptr);
    o.have_transform = true;
  } else if (!std::strcmp(argv[i], "--box") && i + 1 < argc) {
    if (std::sscanf(argv[++i], "%f,%f,%f,%f,%f,%f", &o.box[0], &o.box[1], &o.box[2], &o.box[3], &o.box[4], &o.box[5]) != 6) {
      std::fprintf(stderr, "--box xmin,xmax,ymin,ymax,zmin,zmax\n");
      return -1;
    }
    o.have_box = true;
  } else if (!std::strcmp(argv[i], "--tolerance") && i + 1 < argc) o.tol = std::atof(argv[++i]);
  else if (!std::strcmp(argv[i], "--min-size") && i + 1 < argc) o.min_size = std::atoi(argv[++i]);
  else if (!std::strcmp(argv[i], "--max-size") && i + 1 < argc) o.max_size = std::atoi(argv[++i]);
  else if (!std::strcmp(argv[i], "--tree-refit")) o.tree_refit = true;
  else if (!std::strcmp(argv[i], "--voxel") && i + 1 < argc) o.leaf = std::strtof(argv[++i], nullptr);
  else if (!std::strcmp(argv[i], "--planes") && i + 1 < argc) {
    const int got = std::sscanf(argv[++i], "%d,%lf", &o.max_planes, &o.fraction);
    if (got < 1 || o.max_planes < 1 || o.max_planes > PFT_SEGMENT_MAX_PLANES || !(o.fraction >= 0.0 && o.fraction <= 1.0)) {
      std::fprintf(stderr, "--planes MAX[,FRACTION]: MAX 1 .. %d, FRACTION within [0, 1]\n", (int)PFT_SEGMENT_MAX_PLANES);
      return -1;
    }
  } else if (!std::strcmp(argv[i], "--sac") && i + 1 < argc) {
    if (std::sscanf(argv[++i], "%d,%lf", &o.sac_iter, &o.sac_thr) != 2 || o.sac_iter < 0 || !(o.sac_thr >= 0.0)) {
      std::fprintf(stderr, "--sac ITER,THRESHOLD\n");
      return -1;
    }
  } else {
    return 0;
  }
  return 1;
}

// the segmenter configured as the flags describe
inline void configureSegmenter(const SegmentOptions& o, pft::ModelSegmenter& seg) {
  seg.setPlane(o.plane);
  pft_segment_config& c = seg.config();
  if (!o.plane) c.box_enable[2] = 1;  // create_model.cpp: PassThrough z as well
  if (o.have_box)
    for (int a = 0; a < 3; a++) {
      c.box_min[a] = o.box[2 * a];
      c.box_max[a] = o.box[2 * a + 1];
    }
  if (o.have_transform) seg.setTransform(o.T);
  if (o.tol > 0.0) seg.config().cluster_tolerance = o.tol;
  if (o.min_size >= 0) seg.config().min_cluster_size = o.min_size;
  if (o.max_size >= 0) seg.config().max_cluster_size = o.max_size;
  if (o.sac_iter >= 0) {
    seg.config().max_iterations = o.sac_iter;
    seg.config().distance_threshold = o.sac_thr;
  }
  if (o.max_planes > 0) seg.setPlaneRounds(o.max_planes, o.fraction);
  if (o.tree_refit) seg.setRefitOrder(PFT_SUM_TREE);
}

// a cloud that lies in HBM (a subtraction's residual) through the same pipeline; with --voxel the clusters' indices point
// into the grid's output.  The cloud must stay valid until the call returns
inline void segmentDeviceCloud(const SegmentOptions& o, const pft_point_xyzrgba* d_cloud, size_t n, pft::VoxelGrid& grid,
                               pft::ModelSegmenter& seg) {
  configureSegmenter(o, seg);
  if (o.leaf > 0.0f) {
    grid.setLeafSize(o.leaf, o.leaf, o.leaf);
    grid.setInputCloudDevice(d_cloud, n);
    grid.filterDevice(&d_cloud, &n);
  }
  seg.setInputCloudDevice(d_cloud, n);
  seg.apply();
}

// the scene through the pipeline the flags describe: the optional VoxelGrid first (its output stays on the device, in
// `grid`, for as long as the segmentation reads it), then the segmenter.  Throws what the two handles throw.
inline void segmentScene(const SegmentOptions& o, const Cloud::Ptr& cloud, pft::VoxelGrid& grid, pft::ModelSegmenter& seg) {
  configureSegmenter(o, seg);
  if (o.leaf > 0.0f) {  // cluster_euclid.cpp:40-44: VoxelGrid, then everything else on its output
    grid.setLeafSize(o.leaf, o.leaf, o.leaf);
    grid.setInputCloud(cloud);
    const pft_point_xyzrgba* d_pts = nullptr;
    size_t n_out = 0;
    grid.filterDevice(&d_pts, &n_out);
    std::fprintf(stderr, "PointCloud after VoxelGrid: %zu data points.\n", n_out);
    seg.setInputCloudDevice(d_pts, n_out);
  } else {
    seg.setInputCloud(cloud);
  }
  seg.apply();
}

}  // namespace app

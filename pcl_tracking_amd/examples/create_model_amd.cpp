// create_model_amd.cpp -- the reference's model-creation nodes without ROS / tf: create_model_planar_segmentation.cpp
// (removeZeroPoints, plane RANSAC, ExtractIndices negative, PassThrough y then x, EuclideanClusterExtraction) and, with
// --no-plane, create_model.cpp (PassThrough z, y, x, then the clustering), as one device pipeline.
//
//   create_model_amd <scene> --out DIR [--no-plane] [--transform m00 m01 ... m33] [--box xmin,xmax,ymin,ymax,zmin,zmax]
//                    [--tolerance T] [--min-size N] [--max-size N] [--ascii]
//                    [--planes MAX[,FRACTION]] [--tree-refit] [--sac ITER,THRESHOLD] [--voxel LEAF]
//
// --planes makes it the loop of the reference's test/cluster_euclid.cpp:59-85 and test/cluster_extraction.cpp: planes
// are removed one after the other while more than FRACTION (default 0.3) of the points is left, at most MAX (1 .. 16)
// of them; --sac sets SACSegmentation's iterations and distance threshold (100,0.02 there); --voxel runs the device
// VoxelGrid first (cluster_euclid.cpp:40-44, leaf 0.01) and hands its output to the segmentation without leaving the
// device; --tree-refit selects the parallel summation order of the refit.  One `plane` line is printed per round.
//
// <scene>: a sensor frame, *.pcd or a raw array of 32-byte pcl::PointXYZRGBA records.  --transform is the camera ->
// base matrix of the tf lookup (row-major); the box and the clustering work in the base frame.  Writes DIR/<j>.pcd in
// cluster order (:241-246), holding the input's own points (the reference writes the points after a base -> camera
// round trip, which moves them by rounding), and prints the cluster sizes.  The files feed auto_tracking_amd as they
// are.  PCD binary by default (every bit kept); --ascii writes what PCDWriter::write(..., false) writes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pft/filters.hpp"
#include "pft/pcd_io.hpp"
#include "pft/segmentation.hpp"
#include "tracking_app.hpp"

int main(int argc, char** argv) {
  const char* scene = nullptr;
  std::string out_dir;
  bool plane = true, ascii = false;
  bool have_transform = false, have_box = false;
  float T[16];
  float box[6];
  double tol = -1.0;
  int min_size = -1, max_size = -1;
  int max_planes = 0, sac_iter = -1;
  double fraction = 0.3, sac_thr = -1.0;
  float leaf = 0.0f;
  bool tree_refit = false;
  for (int i = 1; i < argc; i++) {
    if (!std::strcmp(argv[i], "--out") && i + 1 < argc) out_dir = argv[++i];
    else if (!std::strcmp(argv[i], "--no-plane")) plane = false;
    else if (!std::strcmp(argv[i], "--ascii")) ascii = true;
    else if (!std::strcmp(argv[i], "--transform") && i + 16 < argc) {
      for (int k = 0; k < 16; k++) T[k] = std::strtof(argv[++i], nullptr);
      have_transform = true;
    } else if (!std::strcmp(argv[i], "--box") && i + 1 < argc) {
      if (std::sscanf(argv[++i], "%f,%f,%f,%f,%f,%f", &box[0], &box[1], &box[2], &box[3], &box[4], &box[5]) != 6) {
        std::fprintf(stderr, "--box xmin,xmax,ymin,ymax,zmin,zmax\n");
        return 2;
      }
      have_box = true;
    } else if (!std::strcmp(argv[i], "--tolerance") && i + 1 < argc) tol = std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--min-size") && i + 1 < argc) min_size = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--max-size") && i + 1 < argc) max_size = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--tree-refit")) tree_refit = true;
    else if (!std::strcmp(argv[i], "--voxel") && i + 1 < argc) leaf = std::strtof(argv[++i], nullptr);
    else if (!std::strcmp(argv[i], "--planes") && i + 1 < argc) {
      const int got = std::sscanf(argv[++i], "%d,%lf", &max_planes, &fraction);
      if (got < 1 || max_planes < 1 || max_planes > PFT_SEGMENT_MAX_PLANES || !(fraction >= 0.0 && fraction <= 1.0)) {
        std::fprintf(stderr, "--planes MAX[,FRACTION]: MAX 1 .. %d, FRACTION within [0, 1]\n", (int)PFT_SEGMENT_MAX_PLANES);
        return 2;
      }
    } else if (!std::strcmp(argv[i], "--sac") && i + 1 < argc) {
      if (std::sscanf(argv[++i], "%d,%lf", &sac_iter, &sac_thr) != 2 || sac_iter < 0 || !(sac_thr >= 0.0)) {
        std::fprintf(stderr, "--sac ITER,THRESHOLD\n");
        return 2;
      }
    }
    else if (!scene) scene = argv[i];
    else {
      std::fprintf(stderr, "unexpected argument %s\n", argv[i]);
      return 2;
    }
  }
  if (!scene || out_dir.empty()) {
    std::fprintf(stderr, "usage: %s <scene> --out DIR [--no-plane] [--transform 16 floats] "
                         "[--box xmin,xmax,ymin,ymax,zmin,zmax] [--tolerance T] [--min-size N] [--max-size N] [--ascii] "
                         "[--planes MAX[,FRACTION]] [--tree-refit] [--sac ITER,THRESHOLD] [--voxel LEAF]\n",
                 argv[0]);
    return 2;
  }
  app::Cloud::Ptr cloud = app::loadCloud(scene);
  if (cloud->points.empty()) {
    std::fprintf(stderr, "no points in %s\n", scene);
    return 1;
  }
  pft::ModelSegmenter seg;
  seg.setPlane(plane);
  pft_segment_config& c = seg.config();
  if (!plane) c.box_enable[2] = 1;  // create_model.cpp: PassThrough z as well
  if (have_box)
    for (int a = 0; a < 3; a++) {
      c.box_min[a] = box[2 * a];
      c.box_max[a] = box[2 * a + 1];
    }
  if (have_transform) seg.setTransform(T);
  if (tol > 0.0) seg.config().cluster_tolerance = tol;
  if (min_size >= 0) seg.config().min_cluster_size = min_size;
  if (max_size >= 0) seg.config().max_cluster_size = max_size;
  if (sac_iter >= 0) {
    seg.config().max_iterations = sac_iter;
    seg.config().distance_threshold = sac_thr;
  }
  std::vector<pft::PointIndices> cluster_indices;
  std::vector<pft::PointCloud<pft::PointXYZRGBA>> clouds;
  pft::VoxelGrid grid;  // its output cloud stays on the device for as long as the segmentation reads it
  try {
    if (max_planes > 0) seg.setPlaneRounds(max_planes, fraction);
    if (tree_refit) seg.setRefitOrder(PFT_SUM_TREE);
    if (leaf > 0.0f) {  // cluster_euclid.cpp:40-44: VoxelGrid, then everything else on its output
      grid.setLeafSize(leaf, leaf, leaf);
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
    seg.clusters(cluster_indices, &clouds);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  const pft_segment_plane pl = seg.plane();
  std::fprintf(stderr, "PointCloud before filtering: %u data points.\n", pl.n_valid);  // :151
  if (pl.status == PFT_PLANE_FOUND)
    std::fprintf(stderr, "plane %.6f %.6f %.6f %.6f: %u inliers, %u RANSAC iterations\n", pl.coefficients[0],
                 pl.coefficients[1], pl.coefficients[2], pl.coefficients[3], pl.inliers, pl.iterations);
  if (max_planes > 0) {  // one line per round that removed a plane
    static const char* const why[] = {"fraction", "no-plane", "max-planes"};
    const size_t np = seg.planeCount();
    for (size_t r = 0; r < np; r++) {
      const pft_segment_plane q = seg.plane(r);
      std::printf("plane %zu coefficients %.6f %.6f %.6f %.6f inliers %u iterations %u of %u\n", r, q.coefficients[0],
                  q.coefficients[1], q.coefficients[2], q.coefficients[3], q.inliers, q.iterations, q.n_valid);
    }
    std::printf("planes %zu stopped-by %s\n", np, why[seg.stoppedBy()]);
  }
  std::fprintf(stderr, "PointCloud after planar filtering: %u data points.\n", pl.n_survivors);  // :193
  std::printf("clusters %zu\n", clouds.size());                                                 // :226
  for (size_t j = 0; j < clouds.size(); j++) {
    const std::string path = out_dir + "/" + std::to_string(j) + ".pcd";
    if (pft::io::writePCDFile(path, clouds[j], !ascii) != 0) {
      std::fprintf(stderr, "cannot write %s\n", path.c_str());
      return 1;
    }
    std::printf("cluster %zu size %zu %s\n", j, clouds[j].points.size(), path.c_str());
  }
  std::fprintf(stderr, "model creation: %.3f ms on the device\n", seg.lastMilliseconds());
  return 0;
}

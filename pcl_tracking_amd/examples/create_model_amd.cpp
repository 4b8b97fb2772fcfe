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
#include "segment_options.hpp"
#include "tracking_app.hpp"

int main(int argc, char** argv) {
  const char* scene = nullptr;
  std::string out_dir;
  bool ascii = false;
  app::SegmentOptions so;  // the flags shared with auto_tracking_amd --segment (segment_options.hpp)
  for (int i = 1; i < argc; i++) {
    if (!std::strcmp(argv[i], "--out") && i + 1 < argc) out_dir = argv[++i];
    else if (!std::strcmp(argv[i], "--ascii")) ascii = true;
    else if (const int got = app::parseSegmentFlag(so, argc, argv, i)) {
      if (got < 0) return 2;
    }
    else if (!scene) scene = argv[i];
    else {
      std::fprintf(stderr, "unexpected argument %s\n", argv[i]);
      return 2;
    }
  }
  if (!scene || out_dir.empty()) {
    std::fprintf(stderr, "usage: %s <scene> --out DIR " APP_SEGMENT_USAGE_1 " [--ascii] " APP_SEGMENT_USAGE_2 "\n", argv[0]);
    return 2;
  }
  app::Cloud::Ptr cloud = app::loadCloud(scene);
  if (cloud->points.empty()) {
    std::fprintf(stderr, "no points in %s\n", scene);
    return 1;
  }
  const int max_planes = so.max_planes;
  pft::ModelSegmenter seg;
  std::vector<pft::PointIndices> cluster_indices;
  std::vector<pft::PointCloud<pft::PointXYZRGBA>> clouds;
  pft::VoxelGrid grid;  // its output cloud stays on the device for as long as the segmentation reads it
  try {
    app::segmentScene(so, cloud, grid, seg);
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

// match_throw_tool.cpp -- compute() of the C++ mirror throws (int)PFT_ERR_LOST when the lost rule fires
// (setThrowOnFailure(true) with a match threshold above 0), which is what makes the reference's handler
// `try { tracker_->compute(); } catch (int e) { "Object not recognized" }` (auto_tracking.cpp:692-696) live.
//
//   match_throw_tool <min_ratio> <lost_after> <particles> <model.bin> <frame0.bin> [<frame1.bin> ...]
//
// raw arrays of 32-byte points; prints one line per frame: `frame <k> ok` or `frame <k> threw <status>`
#include <cstdio>
#include <cstdlib>

#include "../../pcl_tracking_amd/examples/tracking_app.hpp"

using namespace app;

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  Options opt;
  opt.particles = std::atoi(argv[3]);
  opt.downsampling_grid_size = 0;
  opt.match = true;
  opt.match_min_ratio = std::atof(argv[1]);
  opt.match_lost_after = std::atoi(argv[2]);
  TrackingApp v(opt);
  v.ref_cloud_dict[0] = loadCloud(argv[4]);
  v.buildTrackers(1, [](ParticleFilter& tr, int) { tr.setThrowOnFailure(true); });
  if (!v.setObjectsToTrack()) return 1;
  for (int f = 5; f < argc; f++) {
    v.tracker_dict[0]->setInputCloud(loadCloud(argv[f]));
    try {
      v.tracker_dict[0]->compute();
      std::printf("frame %d ok\n", f - 4);
    } catch (int e) {
      std::printf("frame %d threw %d\n", f - 4, e);
      if (e != PFT_ERR_LOST) return 1;
    }
  }
  return 0;
}

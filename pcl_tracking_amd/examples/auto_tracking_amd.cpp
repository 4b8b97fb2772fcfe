// auto_tracking_amd.cpp -- the tracking part of /root/reference/src/auto_tracking.cpp without ROS / VTK, for the
// nb_objects objects the reference tracks at once: one tracker per object (:199-257), the "set object to track" step
// (:646-677), then per frame the loop over tracker_dict (:688-697: setInputCloud, compute inside try / catch (int)) and what
// drawResult / viz_cb do with each pose (:300-326, :432-466).  The shared steps live in tracking_app.hpp.
//
//   auto_tracking_amd <model0> [<model1> ...] --frames <frame0> [<frame1> ...] [--particles N] [--seed S] [--raw] [--kld] [--pcl-sums] [--change-detector[=interval,min_points,resolution]]
//                     [--model-leaf L] [--device-report] [--async] [--depth-frames fx,fy,cx,cy[,divisor]] [--device-models] [--match[=min_ratio[,lost_after]]] [--reset-on-loss]
//                     [--reacquire[=n_yaw[,accept_ratio[,inlier_distance]]]] [--refine[=max_iterations[,pair_distance]]]
//                     [--spread[=max_pos_sigma[,min_n_eff[,after]]]] [--discover[=every[,radius]]] [--reacquire-residual]
//                     [--visibility[=min_visible_ratio[,occlusion_margin]]] [--grow-models[=confirm[,reach[,max_radius]]]]
//                     [--view-reference[=angle[,min_points[,max_points]]]] [--view-model FILE]...
//   auto_tracking_amd --segment <scene> [model-creation flags] --frames <frame0> [<frame1> ...] [the flags above]
//   (one model only: `auto_tracking_amd <model> <frame0> [frame1 ...]` also works)
//
// *.pcd = PCD v0.7 ascii / binary / binary_compressed with fields x y z rgba (what create_model.cpp:219-222 writes);
// anything else = raw arrays of 32-byte pcl::PointXYZRGBA records.  A model is a segmented object cluster in the
// camera frame.  Without --raw the frames are already filtered and downsampled; with --raw they are sensor frames and
// go through cloud_cb's front end first (:637 filterPassThrough, :683 gridSampleApprox) on the device, the result
// staying in HBM for all the trackers.  Every object is an independent handle on its own HIP stream: the loop below
// enqueues all of them before it reads any result, so they overlap on the GPU.  --device-report moves drawResult / viz_cb to
// the device as well (pft_report after each compute, still before any result is read): the object line then takes its
// centroid from the report, and a `box` line follows with viz_cb's principal-axis box.  --async (with --raw): the front end
// is enqueued without waiting for it and every tracker takes its output AND its point count on the device
// (setInputCloudFromFilter), so the whole frame -- front end, hand-off, compute, report -- is in flight before the host waits
// for anything; the "before / after downsampled" line then follows the results.  The poses are the same either way.
// --device-models runs the "set object to track" step as one device pipeline per object (pft::ModelPreparation) instead of
// on the host.  --segment <scene> takes no model files: the scene goes through the pipeline of create_model_amd, with
// its flags and their meaning (segment_options.hpp), and every cluster becomes an object, in cluster order, prepared on
// the device from where it lies in HBM -- the reference's service call (:749-772) without files in between.
// --match[=min_ratio[,lost_after]] enqueues the match statistics behind every compute (pft_match, still before any result is
// read) and prints one `match` line per object and frame; an object whose result matched fewer than min_ratio of its model
// points for lost_after frames in a row is lost: `Object not recognized` on stderr, the reference's message (:695), and with
// --reset-on-loss a resetTracking(), so that the next frame starts over from the object's initial position.
// --reacquire[=n_yaw[,accept_ratio[,inlier_distance]]] (with --match) looks for a lost object instead: the frame goes through
// the segmenter with the model-creation flags (segment_options.hpp; one segmentation per frame, shared by all objects lost in
// it), and every lost object, in id order, scores its model at the cluster centroids x n_yaw orientations (pft_reacquire); it
// is restarted at the best candidate if that one has at least accept_ratio of the model's points within inlier_distance,
// and the centre it took is dropped for the others.  One `reacquire obj <j>: centre <c> candidate <k> inliers <n>/<M>
// accepted <0|1>` line per lost object; when nothing is accepted, --reset-on-loss applies if given.
// --refine[=max_iterations[,pair_distance]] (with --reacquire) refines the best candidate against the frame before the restart
// (pft_refine: point-to-point ICP on the device); of an accepted candidate the refined pose is applied if it has more model
// points within the inlier distance, else the candidate's own.  One `refine obj <j>: iterations <n> status <s> inliers
// <before> -> <after>/<M> improved <0|1>` line follows the `reacquire obj` line.
// --spread[=max_pos_sigma[,min_n_eff[,after]]] enqueues the population statistics behind every compute (pft_spread, still
// before any result is read) and prints one `spread obj <j>: n_eff ... zero ... pos_sigma ... rpy_sigma ... flagged <0|1>` line
// per object and frame; the pose is flagged after `after` frames in a row whose largest position sigma exceeded max_pos_sigma
// or whose effective sample size fell below min_n_eff (the defaults inf,0,1 never flag).
// --discover[=every[,radius]] (default: every frame, 0.02) finds objects that were not there when the tracking began: after the
// frame's results, every object that is not lost is bound to a scene subtraction (pft::SceneSubtraction) at its result pose, the
// frame is subtracted on the device, and the residual goes through the segmenter with the model-creation flags
// (segment_options.hpp).  Every cluster becomes a new object with the next free id, prepared on the device as --segment
// prepares its objects, and is tracked from the next frame on: one `discover frame <f>: cluster <c> -> obj <j> (<n> points)`
// line per new object, and with --match one `support obj <j> <n>` line per subtracted object (the frame points it holds).
// A frame in which an object is lost discovers nothing: the lost object's own points are unexplained there.
// --grow-models[=confirm[,reach[,max_radius]]] (with --discover; the defaults 3,2,0.5) folds surface that is seen next to a
// tracked object's model into the model (pft::ModelGrowth): after the frame's subtraction, every subtracted object grows on
// the RESIDUAL at its result pose, with the plane that --segment removed from the scene as the exclusion plane, and prints
// one `grow obj <j>: candidates <n> added <n> model <n>` line.  A model that grew becomes its tracker's report cloud and is
// what the subtraction takes from the next frame on, so a face that turns into view is not discovered as an object of its
// own.  The tracker's REFERENCE cloud stays the one view it was given: a model with faces the camera cannot see has no
// likelihood maximum at the true pose.
// --visibility[=min_visible_ratio[,occlusion_margin]] enqueues the visibility of every model at its result pose behind the
// match (pft_visibility: two depth images from the camera at the origin) and prints one `visibility obj <j> visible <n>/<M>
// occluded <n> self <n> out <n>` line per object and frame.  With --match the occlusion-aware rule decides about a loss: an
// object of which less than min_visible_ratio is visible is `Object occluded`, never `Object not recognized`, and
// --reset-on-loss and --reacquire leave it alone; otherwise it is lost after lost_after frames in a row in which fewer than
// min_ratio of its VISIBLE points were matched.
// --view-reference[=angle[,min_points[,max_points]]] (default angle 0.2 rad) lets the reference cloud follow the side of a
// full-surface model that the camera sees (pft_view_select / pft_set_reference_from_view): after a frame's result, once the
// result has turned more than `angle` away from the pose of the object's last selection -- the first result always selects
// --, the visible points of the model at the result pose, at most max_points of them, become the reference cloud.  The full
// model is the grown one under --grow-models, else --view-model FILE, one per object in object order, in the coordinates of
// that object's model file (it is moved by the same re-centring transform).  One `view obj <j> frame <f>: model <n> visible
// <n> kept <n>` line per selection; a selection that keeps fewer than min_points is refused with its text on stderr and the
// tracking goes on with the old reference.
// --depth-frames fx,fy,cx,cy[,divisor] (implies --raw): every --frames entry is a `depth.pgm:colour.ppm` pair -- a registered
// 16-bit depth image (binary PGM, maxval 65535; divided by divisor, default 1000: millimetres) and an RGB image (binary PPM)
// -- or a bare `depth.pgm` without colour, and the organised cloud is formed on the device (InputFilter::setInputDepth):
// 5 bytes per pixel cross the bus instead of the 32-byte record.  The lines are those of the --raw flow.  With --async the
// images go through the front end's two pinned slots, frame f + 1 read from its files while frame f is in flight; with
// --segment the scene is such a pair too and is segmented where the front end formed it (pft_filter_input_device).
// --reacquire-residual (with --reacquire): the segmentation that serves the lost objects runs on the frame minus the objects
// that are not lost, so a lost object is never scored at the cluster of an object that is still tracked.
#include <cstdlib>

#include "pft/pnm_io.hpp"
#include "segment_options.hpp"
#include "tracking_app.hpp"

using namespace app;

// --depth-frames: one frame = `depth.pgm:colour.ppm` (binary PGM, maxval 65535 / binary PPM, maxval 255; pft/pnm_io.hpp), or
// a bare `depth.pgm` without colour
struct DepthFrameFiles {
  pft::DepthImage depth;
  pft::ColorImage color;
  pft_depth_frame desc;
  const void* colorData() const { return desc.color_format == PFT_COLOR_NONE ? nullptr : color.data.data(); }
};
static bool loadDepthFrame(const char* spec, const pft::DepthCamera& cam, float divisor, DepthFrameFiles& out) {
  const std::string s(spec);
  const size_t colon = s.find(':');
  std::string err;
  if (!pft::loadPgm16(s.substr(0, colon), out.depth, err)) {
    std::fprintf(stderr, "%s\n", err.c_str());
    return false;
  }
  const bool has_color = colon != std::string::npos;
  if (has_color) {
    if (!pft::loadPpm8(s.substr(colon + 1), out.color, err)) {
      std::fprintf(stderr, "%s\n", err.c_str());
      return false;
    }
    if (out.color.width != out.depth.width || out.color.height != out.depth.height) {
      std::fprintf(stderr, "%s: the two images differ in size\n", spec);
      return false;
    }
  }
  out.desc = pft::InputFilter::depthFrame(out.depth.width, out.depth.height, cam, PFT_DEPTH_U16, divisor,
                                          has_color ? PFT_COLOR_RGB8 : PFT_COLOR_NONE);
  return true;
}

int main(int argc, char** argv) {
  std::vector<const char*> models, frames, view_models;
  Options opt;
  bool raw = false, in_frames = false, async = false, device_models = false, depth_frames = false;
  pft::DepthCamera depth_cam;
  float depth_divisor = 1000.0f;
  const char* segment_scene = nullptr;
  SegmentOptions so;
  for (int i = 1; i < argc; i++) {
    if (!std::strcmp(argv[i], "--raw")) raw = true;
    else if (!std::strcmp(argv[i], "--device-models")) device_models = true;
    else if (!std::strcmp(argv[i], "--segment") && i + 1 < argc) segment_scene = argv[++i];
    else if (const int got = parseSegmentFlag(so, argc, argv, i)) {
      if (got < 0) return 2;
    }
    else if (!std::strcmp(argv[i], "--async")) async = true;
    else if (!std::strcmp(argv[i], "--depth-frames") && i + 1 < argc) {
      depth_frames = raw = true;  // --depth-frames fx,fy,cx,cy[,divisor]: the frames are image pairs, and sensor frames
      const int got = std::sscanf(argv[++i], "%f,%f,%f,%f,%f", &depth_cam.fx, &depth_cam.fy, &depth_cam.cx, &depth_cam.cy, &depth_divisor);
      if (got < 4) {
        std::fprintf(stderr, "--depth-frames fx,fy,cx,cy[,divisor]\n");
        return 2;
      }
    }
    else if (!std::strcmp(argv[i], "--kld")) opt.use_fixed = false;
    else if (!std::strcmp(argv[i], "--pcl-sums")) opt.pcl_sums = true;
    else if (!std::strcmp(argv[i], "--device-report")) opt.device_report = true;
    else if (!std::strncmp(argv[i], "--change-detector", 17) && (argv[i][17] == 0 || argv[i][17] == '=')) {
      opt.change_detector = true;  // --change-detector[=interval,min_points,resolution]; PCL's defaults 10,10,0.01
      if (argv[i][17] == '=') {
        unsigned int iv = opt.cd_interval, mp = opt.cd_min_points;
        double res = opt.cd_resolution;
        if (std::sscanf(argv[i] + 18, "%u,%u,%lf", &iv, &mp, &res) != 3) {
          std::fprintf(stderr, "--change-detector=interval,min_points,resolution\n");
          return 2;
        }
        opt.cd_interval = iv;
        opt.cd_min_points = mp;
        opt.cd_resolution = res;
      }
    }
    else if (!std::strncmp(argv[i], "--match", 7) && (argv[i][7] == 0 || argv[i][7] == '=')) {
      opt.match = true;  // --match[=min_ratio[,lost_after]]; the defaults 0,1 never report a loss
      if (argv[i][7] == '=') {
        double ratio = 0.0;
        int after = 1;
        const int got = std::sscanf(argv[i] + 8, "%lf,%d", &ratio, &after);
        if (got < 1 || !(ratio >= 0.0 && ratio <= 1.0) || after < 1) {
          std::fprintf(stderr, "--match=min_ratio[,lost_after] with min_ratio in [0, 1] and lost_after >= 1\n");
          return 2;
        }
        opt.match_min_ratio = ratio;
        opt.match_lost_after = after;
      }
    }
    else if (!std::strcmp(argv[i], "--reset-on-loss")) opt.reset_on_loss = true;
    else if (!std::strncmp(argv[i], "--spread", 8) && (argv[i][8] == 0 || argv[i][8] == '=')) {
      opt.spread = true;  // --spread[=max_pos_sigma[,min_n_eff[,after]]]; the defaults inf,0,1 never flag
      if (argv[i][8] == '=') {
        double sigma = opt.spread_max_pos_sigma, n_eff = opt.spread_min_n_eff;
        int after = opt.spread_after;
        const int got = std::sscanf(argv[i] + 9, "%lf,%lf,%d", &sigma, &n_eff, &after);
        if (got < 1 || !(sigma >= 0.0) || !(n_eff >= 0.0) || after < 1) {
          std::fprintf(stderr, "--spread=max_pos_sigma[,min_n_eff[,after]] with max_pos_sigma >= 0, min_n_eff >= 0 and after >= 1\n");
          return 2;
        }
        opt.spread_max_pos_sigma = sigma;
        opt.spread_min_n_eff = n_eff;
        opt.spread_after = after;
      }
    }
    else if (!std::strncmp(argv[i], "--reacquire", 11) && (argv[i][11] == 0 || argv[i][11] == '=')) {
      opt.reacquire = true;  // --reacquire[=n_yaw[,accept_ratio[,inlier_distance]]]; the defaults 8,0.5,0.02
      if (argv[i][11] == '=') {
        int n_yaw = opt.rq_n_yaw;
        double ratio = opt.rq_accept_ratio, inl = opt.rq_inlier_distance;
        const int got = std::sscanf(argv[i] + 12, "%d,%lf,%lf", &n_yaw, &ratio, &inl);
        if (got < 1 || n_yaw < 1 || !(ratio >= 0.0 && ratio <= 1.0) || !(inl > 0.0)) {
          std::fprintf(stderr, "--reacquire=n_yaw[,accept_ratio[,inlier_distance]] with n_yaw >= 1, accept_ratio in [0, 1] and inlier_distance > 0\n");
          return 2;
        }
        opt.rq_n_yaw = n_yaw;
        opt.rq_accept_ratio = ratio;
        opt.rq_inlier_distance = inl;
      }
    }
    else if (!std::strncmp(argv[i], "--refine", 8) && (argv[i][8] == 0 || argv[i][8] == '=')) {
      opt.refine = true;  // --refine[=max_iterations[,pair_distance]]; the defaults 16 and the tracker's max_distance
      if (argv[i][8] == '=') {
        int it = opt.rf_max_iterations;
        double pd = opt.rf_pair_distance;
        const int got = std::sscanf(argv[i] + 9, "%d,%lf", &it, &pd);
        if (got < 1 || it < 1 || it > PFT_REFINE_MAX_ITERATIONS || !(pd >= 0.0)) {
          std::fprintf(stderr, "--refine=max_iterations[,pair_distance] with 1 <= max_iterations <= %d and pair_distance >= 0\n", PFT_REFINE_MAX_ITERATIONS);
          return 2;
        }
        opt.rf_max_iterations = it;
        opt.rf_pair_distance = pd;
      }
    }
    else if (!std::strncmp(argv[i], "--discover", 10) && (argv[i][10] == 0 || argv[i][10] == '=')) {
      opt.discover = true;  // --discover[=every[,radius]]; the defaults 1,0.02
      if (argv[i][10] == '=') {
        int every = opt.discover_every;
        double radius = opt.discover_radius;
        const int got = std::sscanf(argv[i] + 11, "%d,%lf", &every, &radius);
        if (got < 1 || every < 1 || !(radius > 0.0)) {
          std::fprintf(stderr, "--discover=every[,radius] with every >= 1 and radius > 0\n");
          return 2;
        }
        opt.discover_every = every;
        opt.discover_radius = radius;
      }
    }
    else if (!std::strncmp(argv[i], "--grow-models", 13) && (argv[i][13] == 0 || argv[i][13] == '=')) {
      opt.grow_models = true;  // --grow-models[=confirm[,reach[,max_radius]]]; the defaults 3,2,0.5
      if (argv[i][13] == '=') {
        int confirm = opt.grow_confirm, reach = opt.grow_reach;
        double max_radius = opt.grow_max_radius;
        const int got = std::sscanf(argv[i] + 14, "%d,%d,%lf", &confirm, &reach, &max_radius);
        if (got < 1 || confirm < 1 || confirm > 255 || reach < 1 || reach > 4 || !(max_radius > 0.0) || !std::isfinite(max_radius)) {
          std::fprintf(stderr, "--grow-models=confirm[,reach[,max_radius]] with 1 <= confirm <= 255, 1 <= reach <= 4 and max_radius > 0\n");
          return 2;
        }
        opt.grow_confirm = confirm;
        opt.grow_reach = reach;
        opt.grow_max_radius = max_radius;
      }
    }
    else if (!std::strcmp(argv[i], "--reacquire-residual")) opt.reacquire_residual = true;
    else if (!std::strncmp(argv[i], "--visibility", 12) && (argv[i][12] == 0 || argv[i][12] == '=')) {
      opt.visibility = true;  // --visibility[=min_visible_ratio[,occlusion_margin]]; the defaults 0.25,0.03
      if (argv[i][12] == '=') {
        double ratio = opt.vis_min_visible_ratio, margin = opt.vis_occlusion_margin;
        const int got = std::sscanf(argv[i] + 13, "%lf,%lf", &ratio, &margin);
        if (got < 1 || !(ratio >= 0.0 && ratio <= 1.0) || !(margin >= 0.0) || !std::isfinite(margin)) {
          std::fprintf(stderr, "--visibility=min_visible_ratio[,occlusion_margin] with min_visible_ratio in [0, 1] and occlusion_margin >= 0\n");
          return 2;
        }
        opt.vis_min_visible_ratio = ratio;
        opt.vis_occlusion_margin = margin;
      }
    }
    else if (!std::strncmp(argv[i], "--view-reference", 16) && (argv[i][16] == 0 || argv[i][16] == '=')) {
      opt.view_reference = true;  // --view-reference[=angle[,min_points[,max_points]]]; the defaults 0.2,1,0
      if (argv[i][16] == '=') {
        double angle = opt.view_angle;
        unsigned min_points = opt.view_min_points, max_points = opt.view_max_points;
        const int got = std::sscanf(argv[i] + 17, "%lf,%u,%u", &angle, &min_points, &max_points);
        if (got < 1 || !(angle >= 0.0) || !std::isfinite(angle)) {
          std::fprintf(stderr, "--view-reference=angle[,min_points[,max_points]] with angle >= 0\n");
          return 2;
        }
        opt.view_angle = angle;
        opt.view_min_points = min_points;
        opt.view_max_points = max_points;
      }
    }
    else if (!std::strcmp(argv[i], "--view-model") && i + 1 < argc) view_models.push_back(argv[++i]);
    else if (!std::strcmp(argv[i], "--frames")) in_frames = true;
    else if (!std::strcmp(argv[i], "--model-leaf") && i + 1 < argc) opt.downsampling_grid_size = std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--particles") && i + 1 < argc) opt.particles = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) opt.seed = std::strtoull(argv[++i], nullptr, 10);
    else (in_frames ? frames : models).push_back(argv[i]);
  }
  if (!in_frames && models.size() >= 2) {  // `<model> <frame>...`
    frames.assign(models.begin() + 1, models.end());
    models.resize(1);
  }
  if (segment_scene ? !models.empty() || frames.empty() : models.empty() || frames.empty()) {
    std::fprintf(stderr, "usage: %s <model>... --frames <frame>... [--particles N] [--seed S] [--raw] [--kld] [--pcl-sums] [--change-detector[=interval,min_points,resolution]] [--model-leaf L] [--device-report] [--async] [--depth-frames fx,fy,cx,cy[,divisor]] [--device-models] [--match[=min_ratio[,lost_after]]] [--reset-on-loss] [--reacquire[=n_yaw[,accept_ratio[,inlier_distance]]]] [--refine[=max_iterations[,pair_distance]]] [--spread[=max_pos_sigma[,min_n_eff[,after]]]] [--discover[=every[,radius]]] [--grow-models[=confirm[,reach[,max_radius]]]] [--reacquire-residual] [--visibility[=min_visible_ratio[,occlusion_margin]]] [--view-reference[=angle[,min_points[,max_points]]]] [--view-model FILE]...\n"
                         "       %s --segment <scene> " APP_SEGMENT_USAGE_1 " " APP_SEGMENT_USAGE_2 " --frames <frame>... [the flags above]\n", argv[0], argv[0]);
    return 2;
  }
  if (opt.reset_on_loss && !opt.match) {
    std::fprintf(stderr, "--reset-on-loss needs --match: it is the match that says an object is lost\n");
    return 2;
  }
  if (opt.reacquire && !opt.match) {
    std::fprintf(stderr, "--reacquire needs --match: it is the match that says an object is lost\n");
    return 2;
  }
  if (opt.refine && !opt.reacquire) {
    std::fprintf(stderr, "--refine needs --reacquire: it is the re-acquired pose that is refined\n");
    return 2;
  }
  if (opt.reacquire_residual && !opt.reacquire) {
    std::fprintf(stderr, "--reacquire-residual needs --reacquire: it is the re-acquisition's segmentation that runs on the residual\n");
    return 2;
  }
  if (opt.grow_models && !opt.discover) {
    std::fprintf(stderr, "--grow-models needs --discover: it is the residual of its subtraction that the models grow on\n");
    return 2;
  }
  if (async && !raw) {
    std::fprintf(stderr, "--async needs --raw: it is the front end that is not waited for\n");
    return 2;
  }
  if (opt.view_reference ? !opt.grow_models && view_models.empty() : !view_models.empty()) {
    std::fprintf(stderr, "--view-reference takes the full models from --grow-models or from one --view-model FILE per object, and --view-model needs --view-reference\n");
    return 2;
  }

  TrackingApp v(opt);
  float scene_plane[4] = {};  // --segment: the plane the model creation removed, --grow-models' exclusion plane
  bool have_scene_plane = false;
  if (segment_scene) {  // model creation and model preparation in this process, the clusters never leaving HBM
    Cloud::Ptr scene(new Cloud());
    DepthFrameFiles scene_images;
    if (depth_frames ? !loadDepthFrame(segment_scene, depth_cam, depth_divisor, scene_images)
                     : (scene = loadCloud(segment_scene))->points.empty()) {
      std::fprintf(stderr, "no points in %s\n", segment_scene);
      return 1;
    }
    pft::ModelSegmenter seg;
    pft::VoxelGrid grid;  // its output cloud stays on the device for as long as the segmentation reads it
    InputFilter scene_cloud;  // --depth-frames: forms the scene's organised cloud, which is segmented where it lies
    try {
      if (depth_frames) {
        scene_cloud.setPassThrough("z", 0.0f, 10.0f, false, false);
        scene_cloud.setVoxelMode(PFT_VOXEL_NONE);
        scene_cloud.setInputDepth(scene_images.desc, scene_images.depth.data.data(), scene_images.colorData());
        scene_cloud.filterAsync();
        const pft_point_xyzrgba* d_scene = nullptr;
        size_t n_scene = 0;
        scene_cloud.inputDevice(&d_scene, &n_scene);
        segmentDeviceCloud(so, d_scene, n_scene, grid, seg);
      } else {
        segmentScene(so, scene, grid, seg);
      }
      if (opt.grow_models && so.plane && !so.have_transform) {  // (a transformed scene's plane is not in the camera frame)
        const pft_segment_plane pl = seg.plane();
        have_scene_plane = pl.status == PFT_PLANE_FOUND;
        std::memcpy(scene_plane, pl.coefficients, sizeof(scene_plane));
      }
      const std::vector<uint32_t> sizes = seg.clusterSizes();
      std::fprintf(stderr, "clusters %zu\n", sizes.size());
      if (sizes.empty()) return 1;
      v.buildTrackers((int)sizes.size(), [](ParticleFilter& tr, int) { tr.setThrowOnFailure(false); });
      if (!v.setObjectsToTrackOnDevice(seg)) return 1;
    } catch (const std::exception& e) {
      std::fprintf(stderr, "%s\n", e.what());
      return 1;
    }
  } else {
    const int nb_objects = (int)models.size();
    for (int obj_id = 0; obj_id < nb_objects; obj_id++) v.ref_cloud_dict[obj_id] = loadCloud(models[obj_id]);
    v.buildTrackers(nb_objects, [](ParticleFilter& tr, int) { tr.setThrowOnFailure(false); });
    try {
      if (!(device_models ? v.setObjectsToTrackOnDevice() : v.setObjectsToTrack())) return 1;
    } catch (const std::exception& e) {
      std::fprintf(stderr, "%s\n", e.what());
      return 1;
    }
  }

  for (size_t k = 0; k < view_models.size() && !opt.grow_models; k++) {  // --view-model: object k's full-surface model
    const Cloud::Ptr full = loadCloud(view_models[k]);
    if (!v.setViewModel((int)k, *full)) {
      std::fprintf(stderr, "--view-model %s: no points, or no object %zu\n", view_models[k], k);
      return 1;
    }
  }

  InputFilter front_end;  // filterPassThrough (z in [0, 10]) + gridSampleApprox (0.01), fused on the device
  // --depth-frames --async: frame f is read into pinned slot f % 2 of the front end, frame f + 1 while frame f is in flight
  pft_depth_frame slot_desc[PFT_DEPTH_SLOTS];
  void* slot_depth[PFT_DEPTH_SLOTS] = {nullptr, nullptr};
  void* slot_color[PFT_DEPTH_SLOTS] = {nullptr, nullptr};
  size_t staged = (size_t)-1;
  auto stageDepthFrame = [&](size_t f) {
    if (staged == f) return true;
    const int slot = (int)(f % PFT_DEPTH_SLOTS);
    DepthFrameFiles files;
    if (!loadDepthFrame(frames[f], depth_cam, depth_divisor, files)) return false;
    front_end.depthSlotDone(slot, true);  // the slot's last upload has finished before it is written again
    front_end.depthHostBuffers(slot, files.desc, &slot_depth[slot], &slot_color[slot]);
    std::memcpy(slot_depth[slot], files.depth.data.data(), files.depth.data.size() * sizeof(uint16_t));
    if (slot_color[slot]) std::memcpy(slot_color[slot], files.color.data.data(), files.color.data.size());
    slot_desc[slot] = files.desc;
    staged = f;
    return true;
  };
  for (size_t f = 0; f < frames.size(); f++) {
    Cloud::Ptr cloud = depth_frames ? Cloud::Ptr(new Cloud()) : loadCloud(frames[f]);
    DepthFrameFiles files;  // --depth-frames without --async: the images live here until the frame's filter call returned
    const pft_point_xyzrgba* d_cloud = nullptr;
    size_t n_down = 0;
    if (depth_frames) {  // the images instead of the cloud: staged in a pinned slot (--async), else borrowed for the call
      try {
        if (async) {
          if (!stageDepthFrame(f)) return 1;
          const int slot = (int)(f % PFT_DEPTH_SLOTS);
          front_end.setInputDepth(slot_desc[slot], slot_depth[slot], slot_color[slot]);
        } else {
          if (!loadDepthFrame(frames[f], depth_cam, depth_divisor, files)) return 1;
          front_end.setInputDepth(files.desc, files.depth.data.data(), files.colorData());
        }
      } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
      }
    } else if (raw) {
      front_end.setInputCloud(cloud);
    }
    if (async) {
      front_end.filterAsync();
    } else if (raw) {
      front_end.filterDevice(&d_cloud, &n_down);
      std::fprintf(stderr, "PointCloud before downsampled: %zu data points.\nPointCloud after downsampled: %zu data points.\n",
                   front_end.passedPoints(), n_down);  // auto_tracking.cpp:682, 684
    }
    // the frame where the subtraction reads it: the front end's output in HBM (--raw; with --async asked for once the
    // frame's results are on the host), else the host cloud
    auto frameOnDevice = [&]() {
      if (async && !d_cloud) pft_filter_output_device(front_end.nativeHandle(), &d_cloud, &n_down);
    };
    for (auto& kv : v.tracker_dict) {  // :688-697 -- asynchronous: all objects are in flight before a result is read
      if (async) kv.second->setInputCloudFromFilter(front_end);
      else if (raw) kv.second->setInputCloudDevice(d_cloud, n_down);
      else kv.second->setInputCloud(cloud);
      try {
        kv.second->compute();
      } catch (int e) {
        std::fprintf(stderr, "Object not recognized (%s)\n", pft_status_string(e));
      }
      if (opt.device_report) kv.second->computeReport();
      if (opt.match) kv.second->computeMatch();
      if (opt.visibility) kv.second->computeVisibility();  // behind the match: its pairs count the visible matched points
      if (opt.spread) kv.second->computeSpread();
    }
    if (depth_frames && async && f + 1 < frames.size() && !stageDepthFrame(f + 1)) return 1;  // while this frame is in flight
    std::vector<int> lost;  // --reacquire: the objects the match reported lost in this frame
    bool any_lost = false;
    std::map<int, ParticleT> results;  // --view-reference: the poses the reference clouds follow, once the frame is done
    for (auto& kv : v.tracker_dict) {
      const ParticleT result = kv.second->getResult();
      if (opt.view_reference) results[kv.first] = result;
      if (opt.spread) v.reportSpread(kv.first);
      if (opt.visibility) v.reportVisibility(kv.first);
      if (opt.match && v.reportMatch(f + 1, kv.first, !opt.reacquire)) {
        any_lost = true;
        if (opt.reacquire) lost.push_back(kv.first);
      }
      if (opt.device_report) {
        const pft_object_report rep = kv.second->getReport();
        printObjectLine(f + 1, kv.first, result, rep.centroid);
        printBoxLine(f + 1, kv.first, rep);
        continue;
      }
      float centroid[4];
      v.objectPosition(kv.first, result, centroid);
      printObjectLine(f + 1, kv.first, result, centroid);
    }
    if (!lost.empty()) {  // one segmentation of the frame for all of them
      try {
        pft::ModelSegmenter frame_seg;
        pft::VoxelGrid frame_grid;
        if (opt.reacquire_residual) {  // the frame minus the objects that are still tracked
          frameOnDevice();
          const pft_point_xyzrgba* d_res = nullptr;
          size_t n_res = 0;
          v.subtractTracked(*cloud, d_cloud, n_down, lost).residualDevice(&d_res, &n_res);
          if (n_res) segmentDeviceCloud(so, d_res, n_res, frame_grid, frame_seg);
          else throw std::runtime_error("the tracked objects explain the whole frame");
        } else {
          if (depth_frames) front_end.inputCloud(*cloud);  // the sensor frame the front end formed
          segmentScene(so, cloud, frame_grid, frame_seg);
        }
        v.reacquireLost(lost, frame_seg);
      } catch (const std::exception& e) {
        std::fprintf(stderr, "reacquire: %s\n", e.what());
        if (opt.reset_on_loss)
          for (const int obj_id : lost) v.tracker_dict[obj_id]->resetTracking();
      }
    }
    if (opt.discover && !any_lost && f % (size_t)opt.discover_every == 0) {
      try {
        frameOnDevice();
        const pft_point_xyzrgba* d_res = nullptr;
        size_t n_res = 0;
        pft::SceneSubtraction& sub = v.subtractTracked(*cloud, d_cloud, n_down, lost);
        sub.residualDevice(&d_res, &n_res);
        if (opt.match) {
          const std::vector<uint32_t> support = sub.support();
          for (size_t k = 0; k < v.boundIds().size(); k++) std::printf("support obj %d %u\n", v.boundIds()[k], support[k]);
        }
        if (opt.grow_models) v.growModels(sub, have_scene_plane ? scene_plane : nullptr);
        if (n_res) {
          pft::ModelSegmenter res_seg;
          pft::VoxelGrid res_grid;
          segmentDeviceCloud(so, d_res, n_res, res_grid, res_seg);
          v.discoverObjects(f + 1, res_seg, [](ParticleFilter& tr, int) { tr.setThrowOnFailure(false); });
        }
      } catch (const std::exception& e) {
        std::fprintf(stderr, "discover: %s\n", e.what());
      }
    }
    for (const auto& kv : results) v.updateViewReference(f + 1, kv.first, kv.second);  // (behind the frame's growth)
    if (async)  // the counts, now that the frame's results are on the host
      std::fprintf(stderr, "PointCloud before downsampled: %zu data points.\nPointCloud after downsampled: %zu data points.\n",
                   front_end.passedPoints(), front_end.outputPoints());
  }
  return 0;
}

// pft_api_features.hip -- the optional features of the tracker handle, each with its own buffers and one reserve function:
// the change detector's settings, the object report, the match statistics with the lost rule and resetTracking, the
// population statistics with the spread rule, the visibility, re-acquisition and pose refinement.  The kernels are in
// pft_change.hip, pft_report.hip, pft_match.hip, pft_spread.hip, pft_visibility.hip, pft_reacquire.hip and pft_refine.hip.
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "pft_tracker.h"
#include "../../include/pft_segment.h"

// ---- change detection ----
extern "C" int pft_set_change_detector(pft_tracker* t, int use, int interval, int min_points, double resolution) {
  if (!t || interval < 0 || min_points < 0 || !(resolution > 0)) return PFT_ERR_INVALID_ARG;
  if (use && t->cfg.world_size != 1) {
    t->err = "change detection is not supported on a sharded handle (world_size > 1)";
    return PFT_ERR_INVALID_ARG;
  }
  if (use && t->cfg.exact_nearest) {
    t->err = "change detection is not supported with the exact nearest-neighbour coherence (exact_nearest)";
    return PFT_ERR_INVALID_ARG;
  }
  hipSetDevice(t->cfg.device_id);
  if (use && !t->cd_ever) {
    // the device takes over change_counter_ and changed_ from the host: every iteration so far evaluated
    int r = pftt_cd_reserve(t, t->cd, t->in_cap, false);
    if (r != PFT_OK) return r;
    PftChangeState st;
    memset(&st, 0, sizeof(st));
    st.counter = t->cd_counter;
    st.gate = t->changed ? 1u : 0u;
    PFT_HIPCHK(t, hipMemcpyAsync(t->cd.b.st, &st, sizeof(st), hipMemcpyHostToDevice, t->stream));
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
    t->cd_ever = true;
  }
  t->cd_use = use ? 1 : 0;
  t->cd_interval = (uint32_t)interval;
  t->cd_min_points = (uint32_t)min_points;
  t->cd_res = resolution;
  return PFT_OK;
}

extern "C" int pft_get_change_detector(pft_tracker* t, int* use, int* interval, int* min_points, double* resolution) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (use) *use = t->cd_use;
  if (interval) *interval = (int)t->cd_interval;
  if (min_points) *min_points = (int)t->cd_min_points;
  if (resolution) *resolution = t->cd_res;
  return PFT_OK;
}

// ---- object report (pft_report.hip) ----
// the refusals of a report cloud that do not depend on where the cloud lies; first_bad: the first point with a non-finite
// coordinate, SIZE_MAX = none
static int report_cloud_refusal(pft_tracker* t, bool empty, size_t n, size_t first_bad) {
  if (t->cfg.world_size != 1) {
    t->err = "the object report is not supported on a sharded handle (world_size > 1)";
    return PFT_ERR_INVALID_ARG;
  }
  if (empty) {
    t->err = "pft_set_report_cloud: empty report cloud";
    return PFT_ERR_INVALID_ARG;
  }
  if (n > 0x7fffffffu) return PFT_ERR_CAPACITY;
  if (first_bad != SIZE_MAX) {  // the reference's cloud went through removeZeroPoints
    t->err = "pft_set_report_cloud: point " + std::to_string(first_bad) + " has a non-finite coordinate";
    return PFT_ERR_INVALID_ARG;
  }
  return PFT_OK;
}

static int store_report_cloud(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n, hipMemcpyKind kind);

extern "C" int pft_set_report_cloud(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  size_t first_bad = SIZE_MAX;
  if (t->cfg.world_size == 1 && pts && n <= 0x7fffffffu)
    for (size_t i = 0; i < n && first_bad == SIZE_MAX; i++)
      if (!std::isfinite(pts[i].x) || !std::isfinite(pts[i].y) || !std::isfinite(pts[i].z)) first_bad = i;
  const int r = report_cloud_refusal(t, !pts || n == 0, n, first_bad);
  if (r != PFT_OK) return r;
  return store_report_cloud(t, pts, n, hipMemcpyHostToDevice);
}

// pts: a host cloud, or one in this handle's HBM (kind), already accepted by report_cloud_refusal
static int store_report_cloud(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n, hipMemcpyKind kind) {
  hipSetDevice(t->cfg.device_id);
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));  // a report in flight may still read the previous cloud
  PFTT_GROW(t, t->d_report.reserve(1));
  if (n > t->d_rep_tracked.cap()) {
    t->d_rep_tracked.reset();  // (the pair's capacity: zero until both are there)
    t->rep_n = 0;
    t->rep_tracked_n = 0;
    PFTT_GROW(t, t->d_rep_pts.alloc(n));
    PFTT_GROW(t, t->d_rep_tracked.alloc(n));
  }
  PFT_HIPCHK(t, hipMemcpyAsync(t->d_rep_pts, pts, n * sizeof(pft_point_xyzrgba), kind, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  t->rep_n = (uint32_t)n;
  return PFT_OK;
}

// setReferenceCloud + setTrans (+ setReportCloud) from a model-preparation handle (pft_model.hip).  Every refusal is
// decided before anything is applied.  The downsampled reference goes through the host (pft_set_reference orders it and
// takes its hull subset there); the full-resolution report cloud is copied device to device.
extern "C" int pft_set_object_from_model(pft_tracker* t, pft_model* m, int set_report_cloud) {
  if (!t || !m) return PFT_ERR_INVALID_ARG;
  PftModelView v;
  if (pftm_view(m, &v) != PFT_OK) {
    t->err = "pft_set_object_from_model: the model has not been prepared";
    return PFT_ERR_STATE;
  }
  if (v.device_id != t->cfg.device_id) {
    t->err = "pft_set_object_from_model: the model lives on device " + std::to_string(v.device_id) +
             ", the tracker on device " + std::to_string(t->cfg.device_id);
    return PFT_ERR_INVALID_ARG;
  }
  if (set_report_cloud) {
    const int r = report_cloud_refusal(t, v.n_recentred == 0, v.n_recentred,
                                       v.first_nonfinite == 0xFFFFFFFFu ? SIZE_MAX : (size_t)v.first_nonfinite);
    if (r != PFT_OK) return r;
  }
  hipSetDevice(t->cfg.device_id);
  std::vector<pft_point_xyzrgba> ref(v.n_reference);
  if (v.n_reference)  // (the model's prepare has returned: its stream is idle)
    PFT_HIPCHK(t, hipMemcpy(ref.data(), v.reference, v.n_reference * sizeof(pft_point_xyzrgba), hipMemcpyDeviceToHost));
  int r = pft_set_reference(t, ref.data(), ref.size());
  if (r != PFT_OK) return r;
  r = pft_set_trans(t, v.trans);
  if (r != PFT_OK) return r;
  if (set_report_cloud) r = store_report_cloud(t, v.recentred, v.n_recentred, hipMemcpyDeviceToDevice);
  return r;
}

extern "C" int pft_report(pft_tracker* t) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!t->initialized) {
    t->err = "pft_report before the first pft_compute: there is no result yet";
    return PFT_ERR_STATE;
  }
  if (!t->rep_n) {
    t->err = "pft_report without a report cloud (pft_set_report_cloud)";
    return PFT_ERR_STATE;
  }
  hipSetDevice(t->cfg.device_id);
  pftk_report(t->stream, t->d_rep_pts, t->rep_n, t->d_hdr, t->prm.sum_order, t->d_rep_tracked, t->d_report);
  PFT_HIPCHK(t, hipGetLastError());
  t->rep_issued = true;
  t->rep_tracked_n = t->rep_n;
  return PFT_OK;
}

extern "C" int pft_get_report(pft_tracker* t, pft_object_report* out) {
  if (!t || !out) return PFT_ERR_INVALID_ARG;
  if (!t->rep_issued) {
    t->err = "pft_get_report before the first pft_report";
    return PFT_ERR_STATE;
  }
  PFT_HIPCHK(t, hipMemcpyAsync(out, t->d_report, sizeof(pft_object_report), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

extern "C" int pft_get_tracked_cloud(pft_tracker* t, pft_point_xyzrgba* out, size_t cap, size_t* n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!t->rep_issued || !t->rep_tracked_n) {
    t->err = "pft_get_tracked_cloud: no tracked cloud (no pft_report since the report cloud last grew)";
    return PFT_ERR_STATE;
  }
  if (n) *n = t->rep_tracked_n;
  if (!out) return PFT_OK;
  const size_t c = cap < t->rep_tracked_n ? cap : t->rep_tracked_n;
  PFT_HIPCHK(t, hipMemcpyAsync(out, t->d_rep_tracked, c * sizeof(pft_point_xyzrgba), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

// ---- match statistics of the result pose, the lost rule, resetTracking (pft_match.hip) ----
extern "C" int pft_set_match_threshold(pft_tracker* t, double min_ratio, int lost_after) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!(min_ratio >= 0.0 && min_ratio <= 1.0) || lost_after < 1) {
    t->err = "pft_set_match_threshold: min_ratio must lie in [0, 1] and lost_after must be at least 1";
    return PFT_ERR_INVALID_ARG;
  }
  t->match_min_ratio = min_ratio;
  t->match_lost_after = lost_after;
  return PFT_OK;
}

extern "C" int pft_get_match_threshold(pft_tracker* t, double* min_ratio, int* lost_after) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (min_ratio) *min_ratio = t->match_min_ratio;
  if (lost_after) *lost_after = t->match_lost_after;
  return PFT_OK;
}

// the first match for a reference cloud: the block's result fields and the pairs start as "nothing matched" (a match that
// is not evaluated leaves them so); the lost rule's state and the call count stay
__global__ __launch_bounds__(256) void k_match_clear(pft_match_stats* out, int32_t* input_idx, float* sq_dist, uint32_t M) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
    input_idx[i] = -1;
    sq_dist[i] = INFINITY;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int k = 0; k < 12; k++) out->transform[k] = 0.0f;
    out->coherence = 0.0;
    out->sum_sq_dist = 0.0;
    out->n_reference = M;
    out->n_matched = 0u;
    out->n_crop = 0u;
    out->evaluated = 0u;
  }
}

extern "C" int pft_match(pft_tracker* t) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (t->cfg.world_size != 1) {
    t->err = "the match statistics are not supported on a sharded handle (world_size > 1)";
    return PFT_ERR_INVALID_ARG;
  }
  if (t->cfg.exact_nearest) {
    t->err = "the match statistics are not supported with the exact nearest-neighbour coherence (exact_nearest): that mode builds no octree";
    return PFT_ERR_INVALID_ARG;
  }
  if (!t->initialized || !t->has_ref) {
    t->err = "pft_match before the first pft_compute: there is no result yet";
    return PFT_ERR_STATE;
  }
  if (!t->tree_of_compute) {
    t->err = "pft_match: the tree on the device is not the last pft_compute's any more (pft_eval_weights, a debug hook, a new "
             "reference or a larger input cloud came after it)";
    return PFT_ERR_STATE;
  }
  hipSetDevice(t->cfg.device_id);
  if (!t->d_match) {
    PFTT_GROW(t, t->d_match.alloc(1));
    PFT_HIPCHK(t, hipMemsetAsync(t->d_match, 0, sizeof(pft_match_stats), t->stream));
  }
  const uint32_t M = t->prm.M;
  if (M > t->d_match_d2.cap()) {
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));  // a match in flight may still write the previous arrays
    t->d_match_d2.reset();  // (the pair's capacity: zero until both are there)
    t->match_n = 0;
    PFTT_GROW(t, t->d_match_idx.alloc(M));
    PFTT_GROW(t, t->d_match_d2.alloc(M));
  }
  if (t->match_n != M || !t->match_issued)  // (pft_set_reference zeroes match_n: no pair of another model survives it)
    hipLaunchKernelGGL(k_match_clear, dim3(M / 256u < 1u ? 1u : (M / 256u > 64u ? 64u : M / 256u)), dim3(256), 0, t->stream,
                       t->d_match.get(), t->d_match_idx.get(), t->d_match_d2.get(), M);
  pftt_sync_dev(t);
  PftDev d = t->dev;
  d.gate = t->cd_ever ? &t->cd.b.st->gate : nullptr;  // the last iteration's decision, still in the detector's state
  pftk_match(t->stream, t->prm, d, t->match_min_ratio, (uint32_t)t->match_lost_after, t->d_match, t->d_match_idx,
             t->d_match_d2);
  PFT_HIPCHK(t, hipGetLastError());
  t->match_issued = true;
  t->match_of_compute = true;
  t->match_n = M;
  return PFT_OK;
}

extern "C" int pft_get_match(pft_tracker* t, pft_match_stats* out) {
  if (!t || !out) return PFT_ERR_INVALID_ARG;
  if (!t->match_issued) {
    t->err = "pft_get_match before the first pft_match";
    return PFT_ERR_STATE;
  }
  PFT_HIPCHK(t, hipMemcpyAsync(out, t->d_match, sizeof(pft_match_stats), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

extern "C" int pft_get_match_pairs(pft_tracker* t, int32_t* input_idx, float* sq_dist, size_t cap, size_t* n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!t->match_issued || !t->match_n) {
    t->err = "pft_get_match_pairs: no pairs (no pft_match since the reference cloud was last set)";
    return PFT_ERR_STATE;
  }
  if (n) *n = t->match_n;
  const size_t c = cap < t->match_n ? cap : t->match_n;
  if (input_idx && c) PFT_HIPCHK(t, hipMemcpyAsync(input_idx, t->d_match_idx, c * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
  if (sq_dist && c) PFT_HIPCHK(t, hipMemcpyAsync(sq_dist, t->d_match_d2, c * sizeof(float), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

// ParticleFilterTracker::resetTracking(): the handle forgets its population.  The next pft_compute (or
// pft_dist_begin_frame) is a first frame: initParticles(true) around the trans in force then, motion zero, resample
// epoch 0, the first-frame schedule, builder hints reset -- host state plus the init launch the first frame already has.
// The change detector keeps its state, as PCL keeps its detector.  One deliberate difference: PCL keeps changed_ and the
// stale motion_ and would resample the fresh uniform population once before the first weight(); here the frame after a
// reset runs exactly like the first frame of a fresh handle.
extern "C" int pft_reset_tracking(pft_tracker* t) {
  if (!t) return PFT_ERR_INVALID_ARG;
  hipSetDevice(t->cfg.device_id);
  t->initialized = false;
  t->changed = false;
  t->resample_epoch = 0;
  t->tree_of_compute = false;
  if (t->h_stat) t->h_stat[0] = t->h_stat[1] = 0;
  return pftt_match_clear_streak(t);
}

// ---- population statistics and the spread rule (pft_spread.hip) ----
extern "C" int pft_set_spread_threshold(pft_tracker* t, double max_pos_sigma, double min_n_eff, int after) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!(max_pos_sigma >= 0.0) || !(min_n_eff >= 0.0) || after < 1) {
    t->err = "pft_set_spread_threshold: max_pos_sigma and min_n_eff must be numbers >= 0 and after must be at least 1";
    return PFT_ERR_INVALID_ARG;
  }
  t->spread_max_pos_sigma = max_pos_sigma;
  t->spread_min_n_eff = min_n_eff;
  t->spread_after = after;
  return PFT_OK;
}

extern "C" int pft_get_spread_threshold(pft_tracker* t, double* max_pos_sigma, double* min_n_eff, int* after) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (max_pos_sigma) *max_pos_sigma = t->spread_max_pos_sigma;
  if (min_n_eff) *min_n_eff = t->spread_min_n_eff;
  if (after) *after = t->spread_after;
  return PFT_OK;
}

extern "C" int pft_spread(pft_tracker* t) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (t->cfg.world_size != 1) {
    t->err = "the population statistics are not supported on a sharded handle (world_size > 1)";
    return PFT_ERR_INVALID_ARG;
  }
  if (!t->initialized) {
    t->err = "pft_spread before the first pft_compute: there is no population yet";
    return PFT_ERR_STATE;
  }
  hipSetDevice(t->cfg.device_id);
  const uint32_t n_max = t->prm.kld ? t->Pcap : t->prm.P_total;  // (a KLD handle's count is read on the device)
  if (!t->d_spread) {
    const size_t blocks = pftk_spread_blocks(n_max);
    PFTT_GROW(t, t->d_spread_part.alloc((size_t)29 * blocks));
    PFTT_GROW(t, t->d_spread_zero.alloc(blocks));
    PFTT_GROW(t, t->d_spread_wmax.alloc(blocks));
    PFTT_GROW(t, t->d_spread_imax.alloc(blocks));
    PFTT_GROW(t, t->d_spread.alloc(1));  // (last: the test above sees the five or none)
    PFT_HIPCHK(t, hipMemsetAsync(t->d_spread, 0, sizeof(pft_population_stats), t->stream));
  }
  pftt_sync_dev(t);
  pftk_spread(t->stream, t->dev, n_max, t->d_spread_part, t->d_spread_zero, t->d_spread_wmax, t->d_spread_imax,
              t->spread_max_pos_sigma, t->spread_min_n_eff, (uint32_t)t->spread_after, t->d_spread);
  PFT_HIPCHK(t, hipGetLastError());
  t->spread_issued = true;
  return PFT_OK;
}

extern "C" int pft_get_spread(pft_tracker* t, pft_population_stats* out) {
  if (!t || !out) return PFT_ERR_INVALID_ARG;
  if (!t->spread_issued) {
    t->err = "pft_get_spread before the first pft_spread";
    return PFT_ERR_STATE;
  }
  PFT_HIPCHK(t, hipMemcpyAsync(out, t->d_spread, sizeof(pft_population_stats), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

// ---- visibility of the model at a pose and the occlusion-aware lost rule (pft_visibility.hip) ----
extern "C" int pft_set_visibility_camera(pft_tracker* t, const pft_visibility_config* c) {
  if (!t || !c) return PFT_ERR_INVALID_ARG;
  const char* bad = nullptr;
  if (c->width < 1 || c->width > PFT_VIS_MAX_IMAGE || c->height < 1 || c->height > PFT_VIS_MAX_IMAGE)
    bad = "width and height must lie in 1 .. 1024";
  else if (!std::isfinite(c->fx) || !std::isfinite(c->fy) || !(c->fx > 0.0f) || !(c->fy > 0.0f))
    bad = "fx and fy must be finite and > 0";
  else if (!std::isfinite(c->cx) || !std::isfinite(c->cy))
    bad = "cx and cy must be finite";
  else if (!std::isfinite(c->z_near) || !(c->z_near >= 0.0f))
    bad = "z_near must be finite and >= 0";
  else if (c->splat < 0 || c->splat > PFT_VIS_MAX_SPLAT)
    bad = "splat must lie in 0 .. 4";
  else if (!std::isfinite(c->occlusion_margin) || !(c->occlusion_margin >= 0.0) || !std::isfinite(c->self_margin) ||
           !(c->self_margin >= 0.0))
    bad = "occlusion_margin and self_margin must be finite and >= 0";
  if (bad) {
    t->err = std::string("pft_set_visibility_camera: ") + bad;
    return PFT_ERR_INVALID_ARG;
  }
  t->vis_cam = *c;
  return PFT_OK;
}

extern "C" int pft_get_visibility_camera(pft_tracker* t, pft_visibility_config* c) {
  if (!t || !c) return PFT_ERR_INVALID_ARG;
  *c = t->vis_cam;
  return PFT_OK;
}

extern "C" int pft_set_visibility_threshold(pft_tracker* t, double min_visible_ratio, double min_ratio, int lost_after) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!(min_visible_ratio >= 0.0 && min_visible_ratio <= 1.0) || !(min_ratio >= 0.0 && min_ratio <= 1.0) || lost_after < 1) {
    t->err = "pft_set_visibility_threshold: min_visible_ratio and min_ratio must lie in [0, 1] and lost_after must be at least 1";
    return PFT_ERR_INVALID_ARG;
  }
  t->vis_min_visible_ratio = min_visible_ratio;
  t->vis_min_ratio = min_ratio;
  t->vis_lost_after = lost_after;
  return PFT_OK;
}

extern "C" int pft_get_visibility_threshold(pft_tracker* t, double* min_visible_ratio, double* min_ratio, int* lost_after) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (min_visible_ratio) *min_visible_ratio = t->vis_min_visible_ratio;
  if (min_ratio) *min_ratio = t->vis_min_ratio;
  if (lost_after) *lost_after = t->vis_lost_after;
  return PFT_OK;
}

extern "C" int pft_visibility(pft_tracker* t, const float* m12) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (t->cfg.world_size != 1) {
    t->err = "the visibility is not supported on a sharded handle (world_size > 1)";
    return PFT_ERR_INVALID_ARG;
  }
  if (m12)
    for (int k = 0; k < 12; k++)
      if (!std::isfinite(m12[k])) {
        t->err = "pft_visibility: entry " + std::to_string(k) + " of the matrix is not finite";
        return PFT_ERR_INVALID_ARG;
      }
  const int ready = pftt_check_ready(t);  // no input cloud, no reference cloud: as pft_compute
  if (ready != PFT_OK) return ready;
  if (!m12 && !t->initialized) {
    t->err = "pft_visibility without a matrix before the first pft_compute: there is no result pose yet";
    return PFT_ERR_STATE;
  }
  if (t->n_on_device && t->raw_pending) {
    t->err = "pft_visibility: the input handed over by pft_set_input_from_filter has not been through a pft_compute yet "
             "(its count is still the filter's)";
    return PFT_ERR_STATE;
  }
  const uint32_t M = t->prm.M;
  const PftVisCam cam = pftk_visibility_cam(t->vis_cam);
  const size_t words = 2u * (size_t)cam.W * (size_t)cam.H;
  if (!t->d_vis) {
    PFTT_GROW(t, t->d_vis_ctl.reserve(1));
    PFTT_GROW(t, t->d_vis.alloc(1));
    PFT_HIPCHK(t, hipMemsetAsync(t->d_vis, 0, sizeof(pft_visibility_stats), t->stream));
  }
  if (words > t->d_vis_z.cap()) {
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));  // a call in flight may still write the previous images
    PFTT_GROW(t, t->d_vis_z.alloc(words));
  }
  if (M > t->d_vis_mgap.cap()) {
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
    t->d_vis_mgap.reset();  // (the capacity of the four: zero until all are there)
    t->vis_n = 0;
    PFTT_GROW(t, t->d_vis_q.alloc(M));
    PFTT_GROW(t, t->d_vis_state.alloc(M));
    PFTT_GROW(t, t->d_vis_sgap.alloc(M));
    PFTT_GROW(t, t->d_vis_mgap.alloc(M));
  }
  const PftVisBufs b = {t->d_vis_ctl, t->d_vis_z, t->d_vis_q, t->d_vis_state, t->d_vis_sgap, t->d_vis_mgap, t->d_vis};
  if (t->vis_n != M || !t->vis_issued)  // (pft_set_reference zeroes vis_n: no point of another model survives it)
    pftk_visibility_clear(t->stream, b, M);
  PftVisArgs a;
  memset(&a, 0, sizeof(a));
  if (m12) memcpy(a.m, m12, sizeof(a.m));
  a.use_rep = m12 ? 0u : 1u;
  // (pft_set_reference zeroes match_n: the pairs of another model are not read)
  a.match_enqueued = !m12 && t->match_of_compute && t->match_issued && t->match_n == M ? 1u : 0u;
  a.lost_after = (uint32_t)t->vis_lost_after;
  a.min_visible_ratio = t->vis_min_visible_ratio;
  a.min_ratio = t->vis_min_ratio;
  pftt_sync_dev(t);
  // the frame: the 16-byte records, or PCL's 32-byte layout while the frame's first crop has not formed them yet
  const float4* pts = t->raw_pending ? reinterpret_cast<const float4*>(t->raw_pending) : t->d_in_pts.get();
  pftk_visibility(t->stream, t->dev, M, pts, t->raw_pending ? 2u : 1u, t->N, t->dev.n_dev, cam, a, b, t->d_match,
                  t->d_match_idx, t->num_cus);
  PFT_HIPCHK(t, hipGetLastError());
  t->vis_issued = true;
  t->vis_n = M;
  return PFT_OK;
}

extern "C" int pft_get_visibility(pft_tracker* t, pft_visibility_stats* out) {
  if (!t || !out) return PFT_ERR_INVALID_ARG;
  if (!t->vis_issued) {
    t->err = "pft_get_visibility before the first pft_visibility";
    return PFT_ERR_STATE;
  }
  PFT_HIPCHK(t, hipMemcpyAsync(out, t->d_vis, sizeof(pft_visibility_stats), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

extern "C" int pft_get_visibility_points(pft_tracker* t, uint8_t* state, float* scene_gap, float* self_gap, size_t cap,
                                         size_t* n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!t->vis_issued || !t->vis_n) {
    t->err = "pft_get_visibility_points: no points (no pft_visibility since the reference cloud was last set)";
    return PFT_ERR_STATE;
  }
  if (n) *n = t->vis_n;
  const size_t c = cap < t->vis_n ? cap : t->vis_n;
  if (state && c) PFT_HIPCHK(t, hipMemcpyAsync(state, t->d_vis_state, c, hipMemcpyDeviceToHost, t->stream));
  if (scene_gap && c) PFT_HIPCHK(t, hipMemcpyAsync(scene_gap, t->d_vis_sgap, c * sizeof(float), hipMemcpyDeviceToHost, t->stream));
  if (self_gap && c) PFT_HIPCHK(t, hipMemcpyAsync(self_gap, t->d_vis_mgap, c * sizeof(float), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

// ---- re-acquisition of a lost object (pft_reacquire.hip) ----
extern "C" void pft_reacquire_config_default(pft_reacquire_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->n_roll = c->n_pitch = 1;
  c->n_yaw = 8;
  c->span_rpy[2] = 6.2831853071795864769f;  // yaw over the full circle
  c->inlier_distance = 0.02;
  c->accept_ratio = 0.5;
  c->apply = 1;
}

static int rq_reserve(pft_tracker* t, uint32_t K, uint32_t n_centres) {
  if (K > t->rq_cap) {
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
    t->rq_cap = 0;
    t->rq_valid = false;
    t->rq_sc = {};
    PFTT_GROW(t, t->d_rq_part.alloc((size_t)K));
    PFTT_GROW(t, t->d_rq_mats.alloc((size_t)K * 12u));
    PFTT_GROW(t, t->d_rq_n_inliers.alloc((size_t)K));
    PFTT_GROW(t, t->d_rq_n_matched.alloc((size_t)K));
    PFTT_GROW(t, t->d_rq_coherence.alloc((size_t)K));
    PFTT_GROW(t, t->d_rq_sum_sq_dist.alloc((size_t)K));
    PFTT_GROW(t, t->d_rq_inlier_sq_dist.alloc((size_t)K));
    t->rq_sc = {t->d_rq_n_inliers, t->d_rq_n_matched, t->d_rq_coherence, t->d_rq_sum_sq_dist, t->d_rq_inlier_sq_dist};
    t->rq_cap = K;
  }
  if (n_centres > t->d_rq_count.cap()) {
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
    t->d_rq_count.reset();  // (the capacity of the three: zero until all are there)
    PFTT_GROW(t, t->d_rq_centres.alloc((size_t)n_centres * 3u));
    PFTT_GROW(t, t->d_rq_first.alloc((size_t)n_centres));
    PFTT_GROW(t, t->d_rq_count.alloc((size_t)n_centres));
  }
  PFTT_GROW(t, t->d_rq_bbox_part.reserve((size_t)t->num_cus * 6u));
  PFTT_GROW(t, t->d_rq_result.reserve(1));
  return PFT_OK;
}

// ---- shared by the evaluators that score foreign poses in the handle's octree (pft_reacquire*, pft_refine) ----
static int tree_refusals(pft_tracker* t, const char* who) {
  if (t->cfg.world_size != 1) {
    t->err = std::string(who) + " is not supported on a sharded handle (world_size > 1)";
    return PFT_ERR_INVALID_ARG;
  }
  if (t->cfg.exact_nearest) {
    t->err = std::string(who) + " is not supported with the exact nearest-neighbour coherence (exact_nearest): that mode builds no octree";
    return PFT_ERR_INVALID_ARG;
  }
  return PFT_OK;
}

// the crop and the tree of the n matrices at `mats`, built by the handle's own launches; returns what the scoring
// launches take.  (pft_eval_weights keeps a block of its own: the handle's bbox_part, the gate, other flags)
static PftDev rebuild_tree_for(pft_tracker* t, float* mats, uint32_t n) {
  PftDev d = t->dev;
  d.p_active = nullptr;  // explicit matrix count (a KLD handle's device-side count does not apply here)
  d.mats = mats;
  d.bbox_part = t->d_rq_bbox_part;
  d.bbox_grid = (uint32_t)t->num_cus;
  d.bbox_part_cap = (uint32_t)t->num_cus;
  d.bbox6 = t->d_bbox6;
  d.gate = nullptr;
  // the change detector's state belongs to the frames the tracker computes: this crop is not tested
  const bool gate_on = t->gate_on;
  t->gate_on = false;
  pftt_stage_aabb(t, d, n, false);
  pftt_stage_crop_octree_likelihood(t, d, n, false, true, false, false);
  t->gate_on = gate_on;
  return d;
}

static void m16_from_m12(const float* m12, float m[16]) {
  memcpy(m, m12, sizeof(float) * 12);
  m[12] = m[13] = m[14] = 0.0f;
  m[15] = 1.0f;
}
// a row-major 3x4 transform becomes the handle's pose, and tracking starts over from it
static int apply_pose(pft_tracker* t, const float* m12) {
  float m[16];
  m16_from_m12(m12, m);
  const int r = pft_set_trans(t, m);
  return r == PFT_OK ? pft_reset_tracking(t) : r;
}

// the refusals that do not depend on the centres; *per_centre = n_roll * n_pitch * n_yaw
static int rq_check(pft_tracker* t, const pft_reacquire_config* c, const char* who, uint64_t* per_centre) {
  int r = tree_refusals(t, who);
  if (r == PFT_OK) r = pftt_check_ready(t);
  if (r != PFT_OK) return r;
  bool ok = c->n_roll >= 1 && c->n_pitch >= 1 && c->n_yaw >= 1;
  for (int a = 0; a < 3; a++) ok = ok && std::isfinite(c->base_rpy[a]) && std::isfinite(c->span_rpy[a]) && c->span_rpy[a] >= 0.0f;
  ok = ok && c->inlier_distance > 0.0 && c->inlier_distance <= t->cfg.max_distance;
  ok = ok && c->accept_ratio >= 0.0 && c->accept_ratio <= 1.0;
  if (!ok) {
    t->err = std::string(who) + ": bad configuration value (n_roll, n_pitch, n_yaw >= 1; base_rpy finite; span_rpy finite and >= 0; "
             "0 < inlier_distance <= max_distance; accept_ratio in [0, 1])";
    return PFT_ERR_INVALID_ARG;
  }
  *per_centre = (uint64_t)c->n_roll * (uint64_t)c->n_pitch * (uint64_t)c->n_yaw;
  return PFT_OK;
}

static int rq_capacity(pft_tracker* t, const char* who, uint64_t per_centre, size_t n_centres) {
  if (per_centre > PFT_REACQUIRE_MAX_CANDIDATES || (uint64_t)n_centres > PFT_REACQUIRE_MAX_CANDIDATES ||
      per_centre * (uint64_t)n_centres > PFT_REACQUIRE_MAX_CANDIDATES) {
    t->err = std::string(who) + ": " + std::to_string(n_centres) + " centres x " + std::to_string(per_centre) +
             " orientations exceed PFT_REACQUIRE_MAX_CANDIDATES (" + std::to_string(PFT_REACQUIRE_MAX_CANDIDATES) + ")";
    return PFT_ERR_CAPACITY;
  }
  return PFT_OK;
}

// the centres are in t->rq_centres (host) and, with on_device, already in d_rq_centres as well
static int rq_run(pft_tracker* t, const char* who, const pft_reacquire_config* c, uint64_t per_centre, bool on_device,
                  pft_reacquire_result* out) {
  const uint32_t n_centres = (uint32_t)(t->rq_centres.size() / 3u);
  for (size_t i = 0; i < t->rq_centres.size(); i++)
    if (!std::isfinite(t->rq_centres[i])) {
      t->err = std::string(who) + ": centre " + std::to_string(i / 3u) + " has a non-finite coordinate";
      t->rq_valid = false;
      return PFT_ERR_INVALID_ARG;
    }
  const uint32_t K = (uint32_t)(per_centre * n_centres), M = t->prm.M;
  memset(out, 0, sizeof(*out));
  out->n_centres = n_centres;
  out->n_reference = M;
  out->best = out->best_centre = -1;
  t->rq_n = K;
  if (K == 0) {  // nothing to score: the tracker, its tree included, is left as it is
    t->rq_valid = true;
    return PFT_OK;
  }
  t->rq_valid = false;
  int r = rq_reserve(t, K, n_centres);
  if (r != PFT_OK) return r;
  pftt_sync_dev(t);
  t->tree_of_compute = false;  // the crop and the tree are rebuilt for the candidates
  if (!on_device)
    PFT_HIPCHK(t, hipMemcpyAsync(t->d_rq_centres, t->rq_centres.data(), t->rq_centres.size() * sizeof(float), hipMemcpyHostToDevice,
                             t->stream));
  PftRqLattice lat;
  lat.n[0] = (uint32_t)c->n_roll;
  lat.n[1] = (uint32_t)c->n_pitch;
  lat.n[2] = (uint32_t)c->n_yaw;
  for (int a = 0; a < 3; a++) {
    lat.base[a] = c->base_rpy[a];
    lat.span[a] = c->span_rpy[a];
  }
  pftk_reacquire_candidates(t->stream, t->d_rq_centres, K, lat, t->d_rq_part, t->d_rq_mats);
  PftDev d = rebuild_tree_for(t, t->d_rq_mats, K);
  d.part_cur = t->d_rq_part;  // (k_reacquire_select reads the candidates' poses)
  d.part_all = t->d_rq_part;
  pftk_reacquire_score(t->stream, t->prm, d, K, c->inlier_distance * c->inlier_distance, t->rq_sc);
  pftk_reacquire_select(t->stream, t->prm, d, t->rq_sc, K, n_centres, (uint32_t)per_centre, c->accept_ratio, t->d_rq_result);
  PFT_HIPCHK(t, hipGetLastError());
  PFT_HIPCHK(t, hipMemcpyAsync(out, t->d_rq_result, sizeof(*out), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  t->rq_valid = true;
  r = pftt_check_device_error(t);
  if (r != PFT_OK) {  // the scores had no target: nothing is accepted, nothing applied
    out->accepted = 0u;
    return r;
  }
  if (c->apply && out->accepted) {
    r = apply_pose(t, out->transform);
    if (r != PFT_OK) return r;
    out->applied = 1u;
  }
  return PFT_OK;
}

extern "C" int pft_reacquire(pft_tracker* t, const float* centres_xyz, size_t n_centres, const pft_reacquire_config* cfg,
                             pft_reacquire_result* out) {
  if (!t || !cfg || !out || (!centres_xyz && n_centres)) return PFT_ERR_INVALID_ARG;
  uint64_t per_centre = 0;
  int r = rq_check(t, cfg, "pft_reacquire", &per_centre);
  if (r != PFT_OK) return r;
  r = rq_capacity(t, "pft_reacquire", per_centre, n_centres);
  if (r != PFT_OK) return r;
  t->rq_centres.assign(centres_xyz, centres_xyz + 3u * n_centres);
  return rq_run(t, "pft_reacquire", cfg, per_centre, false, out);
}

extern "C" int pft_reacquire_from_segmenter(pft_tracker* t, pft_segment* s, const pft_reacquire_config* cfg,
                                            pft_reacquire_result* out) {
  if (!t || !s || !cfg || !out) return PFT_ERR_INVALID_ARG;
  const char* who = "pft_reacquire_from_segmenter";
  uint64_t per_centre = 0;
  int r = rq_check(t, cfg, who, &per_centre);
  if (r != PFT_OK) return r;
  const pft_point_xyzrgba* d_pts = nullptr;
  size_t total = 0, nc = 0;
  if (pft_segment_clusters_device(s, &d_pts, &total) != PFT_OK || pft_segment_cluster_count(s, &nc) != PFT_OK) {
    t->err = std::string(who) + ": the segmenter has not been applied yet";
    return PFT_ERR_STATE;
  }
  if (pftsg_device_id(s) != t->cfg.device_id) {
    t->err = std::string(who) + ": the segmenter lives on device " + std::to_string(pftsg_device_id(s)) +
             ", the tracker on device " + std::to_string(t->cfg.device_id);
    return PFT_ERR_INVALID_ARG;
  }
  r = rq_capacity(t, who, per_centre, nc);
  if (r != PFT_OK) return r;
  t->rq_centres.assign(3u * nc, 0.0f);
  if (nc) {
    std::vector<uint32_t> sizes(nc), first(nc);
    r = pft_segment_cluster_sizes(s, sizes.data(), nc);
    if (r != PFT_OK) return r;
    size_t off = 0;
    for (size_t k = 0; k < nc; k++) {
      first[k] = (uint32_t)off;
      off += sizes[k];
    }
    if (off > total || !d_pts) return PFT_ERR_STATE;
    r = rq_reserve(t, 0u, (uint32_t)nc);
    if (r != PFT_OK) return r;
    // the segmenter's apply has finished on its stream (it returns when the clusters are known); the clusters are read by
    // this call's launch only, which has finished when it returns
    PFT_HIPCHK(t, hipMemcpyAsync(t->d_rq_first, first.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
    PFT_HIPCHK(t, hipMemcpyAsync(t->d_rq_count, sizes.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
    pftk_reacquire_centroids(t->stream, d_pts, t->d_rq_first, t->d_rq_count, (uint32_t)nc, t->d_rq_centres);
    PFT_HIPCHK(t, hipGetLastError());
    PFT_HIPCHK(t, hipMemcpyAsync(t->rq_centres.data(), t->d_rq_centres, 3u * nc * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  }
  return rq_run(t, who, cfg, per_centre, true, out);
}

extern "C" int pft_get_reacquire_scores(pft_tracker* t, pft_particle* cand, float* mats12, uint32_t* n_inliers,
                                        uint32_t* n_matched, double* coherence, double* sum_sq_dist, double* inlier_sq_dist,
                                        float* centres_xyz, size_t cap, size_t* n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!t->rq_valid) {
    t->err = "pft_get_reacquire_scores: no completed pft_reacquire call to read";
    return PFT_ERR_STATE;
  }
  if (n) *n = t->rq_n;
  if (centres_xyz && !t->rq_centres.empty()) memcpy(centres_xyz, t->rq_centres.data(), t->rq_centres.size() * sizeof(float));
  const size_t c = cap < t->rq_n ? cap : t->rq_n;
  if (!c) return PFT_OK;
  hipSetDevice(t->cfg.device_id);
  const hipMemcpyKind k = hipMemcpyDeviceToHost;
  if (cand) PFT_HIPCHK(t, hipMemcpyAsync(cand, t->d_rq_part, c * sizeof(pft_particle), k, t->stream));
  if (mats12) PFT_HIPCHK(t, hipMemcpyAsync(mats12, t->d_rq_mats, c * 12u * sizeof(float), k, t->stream));
  if (n_inliers) PFT_HIPCHK(t, hipMemcpyAsync(n_inliers, t->rq_sc.n_inliers, c * sizeof(uint32_t), k, t->stream));
  if (n_matched) PFT_HIPCHK(t, hipMemcpyAsync(n_matched, t->rq_sc.n_matched, c * sizeof(uint32_t), k, t->stream));
  if (coherence) PFT_HIPCHK(t, hipMemcpyAsync(coherence, t->rq_sc.coherence, c * sizeof(double), k, t->stream));
  if (sum_sq_dist) PFT_HIPCHK(t, hipMemcpyAsync(sum_sq_dist, t->rq_sc.sum_sq_dist, c * sizeof(double), k, t->stream));
  if (inlier_sq_dist) PFT_HIPCHK(t, hipMemcpyAsync(inlier_sq_dist, t->rq_sc.inlier_sq_dist, c * sizeof(double), k, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return PFT_OK;
}

// ---- refinement of a pose against the frame (pft_refine.hip) ----
extern "C" void pft_refine_config_default(pft_refine_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->max_iterations = 16;
  c->min_pairs = 3;
  c->inlier_distance = 0.02;
  c->trans_eps = 1e-4;
  c->rot_eps = 1e-3;
}

static int rf_reserve(pft_tracker* t, uint32_t M) {
  const uint32_t G = pftk_refine_blocks(M) ? pftk_refine_blocks(M) : 1u;
  uint32_t g_cap = t->rf.g_cap;
  t->rf = {};  // formed anew at the end: a failure on the way leaves it empty (g_cap 0), with rf_valid false
  t->rf_valid = false;
  if (G > g_cap) {
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
    PFTT_GROW(t, t->d_rf_part.alloc((size_t)PFT_REFINE_N_SUMS * G));
    PFTT_GROW(t, t->d_rf_part_n.alloc((size_t)2 * G));
    g_cap = G;
  }
  PFTT_GROW(t, t->d_rf_ctl.reserve(pftk_refine_ctl_bytes()));
  PFTT_GROW(t, t->d_rf_result.reserve(1));
  PFTT_GROW(t, t->d_rf_trace.reserve((size_t)PFT_REFINE_MAX_ITERATIONS + 1u));
  PFTT_GROW(t, t->d_rf_mats.reserve((size_t)8 * 12));
  PFTT_GROW(t, t->d_rq_bbox_part.reserve((size_t)t->num_cus * 6u));
  t->rf = {reinterpret_cast<PftRefineCtl*>(t->d_rf_ctl.get()), t->d_rf_part, t->d_rf_part_n, g_cap, t->d_rf_result,
           t->d_rf_trace};
  return PFT_OK;
}

extern "C" int pft_refine(pft_tracker* t, const float* start12, const pft_refine_config* c, pft_refine_result* out) {
  if (!t || !c || !out) return PFT_ERR_INVALID_ARG;
  int r = tree_refusals(t, "pft_refine");
  if (r == PFT_OK) r = pftt_check_ready(t);
  if (r != PFT_OK) return r;
  bool ok = c->max_iterations >= 1 && c->max_iterations <= PFT_REFINE_MAX_ITERATIONS && c->min_pairs >= 3;
  ok = ok && std::isfinite(c->pair_distance) && c->pair_distance >= 0.0;
  ok = ok && std::isfinite(c->inlier_distance) && c->inlier_distance > 0.0;
  ok = ok && std::isfinite(c->margin) && c->margin >= 0.0;
  ok = ok && std::isfinite(c->trans_eps) && c->trans_eps >= 0.0 && std::isfinite(c->rot_eps) && c->rot_eps >= 0.0;
  if (!ok) {
    t->err = "pft_refine: bad configuration value (1 <= max_iterations <= PFT_REFINE_MAX_ITERATIONS; min_pairs >= 3; "
             "pair_distance, margin, trans_eps, rot_eps finite and >= 0; inlier_distance finite and > 0)";
    return PFT_ERR_INVALID_ARG;
  }
  if (start12) {
    for (int k = 0; k < 12; k++)
      if (!std::isfinite(start12[k])) {
        t->err = "pft_refine: the start has a non-finite entry";
        return PFT_ERR_INVALID_ARG;
      }
  } else if (!t->initialized) {
    t->err = "pft_refine without a start before the first pft_compute: there is no result pose yet";
    return PFT_ERR_STATE;
  }
  const uint32_t M = t->prm.M;
  t->rf_valid = false;
  r = rf_reserve(t, M);
  if (r != PFT_OK) return r;
  PftRefineArgs a;
  memset(&a, 0, sizeof(a));
  if (start12) memcpy(a.start, start12, sizeof(a.start));
  a.use_rep = start12 ? 0u : 1u;
  a.max_iterations = (uint32_t)c->max_iterations;
  a.min_pairs = (uint32_t)c->min_pairs;
  const double pd = c->pair_distance > 0.0 ? c->pair_distance : t->cfg.max_distance;
  a.pair2 = pd * pd;
  a.inl2 = c->inlier_distance * c->inlier_distance;
  a.margin = c->margin > 0.0 ? c->margin : pd;
  a.trans_eps2 = c->trans_eps * c->trans_eps;
  a.rot_eps2 = c->rot_eps * c->rot_eps;
  pftt_sync_dev(t);
  t->tree_of_compute = false;  // the crop and the tree are rebuilt around the start
  pftk_refine_init(t->stream, a, t->rf, t->d_hdr, t->d_rf_mats);
  const PftDev d = rebuild_tree_for(t, t->d_rf_mats, 8u);
  pftk_refine_passes(t->stream, t->prm, d, t->rf, a);
  PFT_HIPCHK(t, hipGetLastError());
  PFT_HIPCHK(t, hipMemcpyAsync(out, t->rf.result, sizeof(*out), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  t->rf_n = out->iterations + 1u;
  t->rf_valid = true;
  float m[16];
  m16_from_m12(out->transform, m);
  pft_to_state(m, &out->pose);
  r = pftt_check_device_error(t);
  if (r != PFT_OK) {  // the passes had no target: nothing is applied
    out->improved = 0u;
    return r;
  }
  if (c->apply && out->improved) {
    r = apply_pose(t, out->transform);
    if (r != PFT_OK) return r;
    out->applied = 1u;
  }
  return PFT_OK;
}

extern "C" int pft_get_refine_trace(pft_tracker* t, pft_refine_trace_entry* entries, size_t cap, size_t* n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!t->rf_valid) {
    t->err = "pft_get_refine_trace: no completed pft_refine call to read";
    return PFT_ERR_STATE;
  }
  if (n) *n = t->rf_n;
  const size_t c = cap < t->rf_n ? cap : t->rf_n;
  if (!c || !entries) return PFT_OK;
  hipSetDevice(t->cfg.device_id);
  PFT_HIPCHK(t, hipMemcpyAsync(entries, t->rf.trace, c * sizeof(pft_refine_trace_entry), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return PFT_OK;
}

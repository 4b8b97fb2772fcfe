/*
 * pft_view.h -- C ABI of the view-dependent reference: at a pose, pick from a full-surface model the points the camera
 * can see, and make those the tracker's reference cloud.  Functions of the tracker handle of pft.h, exported by the same
 * libpft_hip.so.  DESIGN.md section 3.17 repeats this specification.
 *
 * Camera, projection (in_view, u, v), footprint and xform are exactly those of pft_visibility.h; the camera is the
 * handle's visibility camera (pft_set_visibility_camera): width, height, fx, fy, cx, cy, z_near, splat and self_margin.
 * occlusion_margin is unused.  All arithmetic is IEEE float, unfused; `/` is the correctly rounded division.
 *
 * Input: a model of N 32-byte records in the object frame, a row-major 3x4 T, and max_points.  T is explicit, or with
 * m12 == NULL pose_to_matrix of the last result, formed on the device as pft_visibility forms it.
 *
 * Per record i, the first rule that holds gives state[i]:
 *   1. PFT_VIEW_NONFINITE      a coordinate of the record is not finite.  (A record with z = +inf projects into view, splats
 *                              nothing and has inf - inf -> fmaxf(NaN, 0) = 0 as its gap: without this rule it would be
 *                              selected, and a non-finite reference point is an illegal access in the likelihood.)
 *   2. PFT_VIEW_OUT_OF_VIEW    q_i = xform(T, p_i) has a non-finite coordinate, or is not in_view
 *   3. Zm[pixel] = the smallest q.z over the footprints of the points that passed rules 1 and 2, else +inf;
 *      self_gap[i] = fmaxf(q_i.z - Zm[u_i, v_i], 0);
 *      PFT_VIEW_SELF_OCCLUDED  self_gap[i] > (float)self_margin  (strict)
 *   4. otherwise the point is visible.  n_visible counts these points; r is a visible point's rank among them in index
 *      order.  With K = max_points:
 *        K == 0 or n_visible <= K                                       PFT_VIEW_KEPT
 *        else ((r + 1) K) / n_visible > (r K) / n_visible  (uint64)     PFT_VIEW_KEPT, otherwise PFT_VIEW_DECIMATED
 *      Exactly K points are kept then; the kept point of rank r is the ((r K) / n_visible)-th of the view cloud.
 * self_gap is 0 for the states of rules 1 and 2.
 *
 * Outputs: state[N] and self_gap[N]; kept_index[n_kept], ascending; the view cloud -- the kept records copied whole (all
 * 32 bytes) in that order; the counts.  No output depends on the launch shape or on scheduling.
 *
 * The scene is deliberately not consulted: a point hidden by an occluder stays in the reference, so that an occluded
 * object's model does not shrink.
 *
 * Opt-in: a select is enqueued on the handle's stream and never synchronises; no launch of pft_compute changes.
 */
#ifndef PFT_VIEW_H
#define PFT_VIEW_H

#include "pft_visibility.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PFT_VIEW_KEPT = 0, PFT_VIEW_DECIMATED = 1, PFT_VIEW_SELF_OCCLUDED = 2, PFT_VIEW_OUT_OF_VIEW = 3, PFT_VIEW_NONFINITE = 4 };
enum { PFT_VIEW_MAX_MODEL_POINTS = 1 << 22 };

typedef struct pft_view_stats {
  float transform[12];   /* the T used, row-major 3x4 */
  uint32_t n_model;      /* N */
  uint32_t n_state[5];   /* records per PFT_VIEW_* state */
  uint32_t n_visible;    /* n_state[KEPT] + n_state[DECIMATED] */
  uint32_t n_kept;       /* n_state[KEPT]: the size of the view cloud */
  uint32_t evaluated;    /* 0: the matrix was NULL and the last iteration raised PftHeader::error: every field but `calls`
                            (and the arrays, and the view cloud) keeps the values of the last evaluated select */
  uint32_t calls;        /* selects launched so far */
} pft_view_stats;        /* 88 B */

/* enqueues the selection over n records at host_pts (copied in stream order) / at device_pts (16-byte aligned, in this
 * handle's HBM, written in the order of the handle's stream or before the call; read until the select has run) at m12
 * (row-major 3x4), or with m12 == NULL at the result pose of the last pft_compute.  max_points: 0 = no limit.
 *   PFT_ERR_INVALID_ARG with a text   a sharded handle (world_size > 1), a non-finite entry of m12, a misaligned device_pts
 *   PFT_ERR_STATE                     m12 == NULL before the first pft_compute
 *   PFT_ERR_CAPACITY                  n > PFT_VIEW_MAX_MODEL_POINTS
 * n == 0 is allowed and selects nothing.  An explicit matrix needs neither a reference nor an input cloud.  KLD and
 * exact-NN handles are accepted.  A select that has to grow the handle's buffers drops the results of the selects before
 * it (an unevaluated select then leaves n_model = 0). */
int pft_view_select(pft_tracker* t, const pft_point_xyzrgba* host_pts, size_t n, const float* m12, uint32_t max_points);
int pft_view_select_device(pft_tracker* t, const pft_point_xyzrgba* device_pts, size_t n, const float* m12, uint32_t max_points);

/* the getters synchronise and report device-side failures as pft_get_result does; PFT_ERR_STATE before the first select */
int pft_get_view(pft_tracker* t, pft_view_stats* out);
/* per record: state (PFT_VIEW_*) and self_gap.  Either array may be NULL; *n = n_model, up to cap entries are copied */
int pft_get_view_points(pft_tracker* t, uint8_t* state, float* self_gap, size_t cap, size_t* n);
/* the kept records' indices into the model, ascending; *n = n_kept */
int pft_get_view_indices(pft_tracker* t, uint32_t* idx, size_t cap, size_t* n);
/* the view cloud; *n = n_kept */
int pft_get_view_cloud(pft_tracker* t, pft_point_xyzrgba* pts, size_t cap, size_t* n);
/* the view cloud where it lies in HBM, valid until the next select on this handle */
int pft_view_cloud_device(pft_tracker* t, const pft_point_xyzrgba** ptr, size_t* n);

/* synchronises, takes the view cloud of the last evaluated select and makes it the reference cloud, with exactly the
 * effect of pft_set_reference on those records in that order (the cloud crosses to the host for its Morton order and hull
 * subset) -- except that the object is the same: the streaks and flags of the match lost rule, the visibility rule and
 * the spread rule are kept.  The particles, trans and the epoch are untouched, as in pft_set_reference; the per-point
 * arrays of pft_match and pft_visibility belonged to the old reference and are dropped.
 *   PFT_ERR_STATE with a text, the current reference still usable: no select since the last one was consumed, a last
 *   select that was not evaluated, n_kept < max(min_points, 1) */
int pft_set_reference_from_view(pft_tracker* t, uint32_t min_points);

/* test hook: the grid (workgroups) of every pass of the selects that follow, 0 = the default.  Latched per handle */
int pft_debug_set_view_grid(pft_tracker* t, uint32_t blocks);

#ifdef __cplusplus
}
#endif
#endif

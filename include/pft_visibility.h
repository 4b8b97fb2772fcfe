/*
 * pft_visibility.h -- C ABI of the model's visibility at a pose: how much of the reference cloud the camera can see, and
 * an occlusion-aware lost rule on top of it.  Functions of the tracker handle of pft.h, exported by the same
 * libpft_hip.so.  DESIGN.md section 3.15 is the specification; in short:
 *
 * The camera sits at the origin and looks along +z (the frame of the reference's Kinect clouds).  All arithmetic is IEEE
 * float, unfused; `/` is the correctly rounded division.
 *
 *   projection of (x, y, z):
 *     front   = z > z_near                                   (NaN fails)
 *     xn = x / z, yn = y / z;  uf = fx * xn + cx,  vf = fy * yn + cy
 *     in_view = front && uf >= 0 && uf < (float)width && vf >= 0 && vf < (float)height      (NaN fails)
 *     u = (int)floorf(uf), v = (int)floorf(vf)               (formed only when in_view)
 *   footprint of an in-view point: the pixels [u - splat, u + splat] x [v - splat, v + splat], clipped to the image
 *   Zs[pixel]  the smallest z over the FRAME points whose footprint covers the pixel, else +inf.  The frame is the
 *              tracker's current input cloud
 *   Zm[pixel]  the same over the moved reference points q_j = T ref_j (per row ((T0 x + T1 y) + T2 z) + T3)
 *
 *   per reference point j, in the CALLER's order:
 *     q_j not in_view                                  -> PFT_VIS_OUT_OF_VIEW, both gaps 0
 *     self_gap  = fmaxf(z_j - Zm[u, v], 0),  scene_gap = fmaxf(z_j - Zs[u, v], 0)
 *     self_gap  > (float)self_margin                   -> PFT_VIS_SELF_OCCLUDED
 *     else scene_gap > (float)occlusion_margin         -> PFT_VIS_OCCLUDED
 *     else                                             -> PFT_VIS_VISIBLE
 *
 * T is pose_to_matrix(result pose) formed on the device -- exactly the T pft_match stores -- or an explicit matrix.
 *
 * The occlusion-aware lost rule (one lane, after the counts; M = n_reference):
 *     hidden = (double)n_visible < min_visible_ratio * (double)M
 *     !has_match or hidden:  below = 0, the streak is held
 *     else  below = (double)n_visible_matched < min_ratio * (double)n_visible;  streak = below ? streak + 1 : 0
 *     lost = streak >= lost_after
 * has_match: the matrix was NULL, a pft_match was enqueued after the last pft_compute, and that match was evaluated;
 * n_visible_matched then counts the VISIBLE points that pft_match paired (input_idx >= 0), else it is 0.
 * pft_reset_tracking and pft_set_reference clear {below, streak, lost}.  The rule of pft_match is untouched.
 *
 * Opt-in: pft_visibility is enqueued on the handle's stream and never synchronises; no launch of pft_compute changes.
 */
#ifndef PFT_VISIBILITY_H
#define PFT_VISIBILITY_H

#include "pft.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PFT_VIS_VISIBLE = 0, PFT_VIS_OCCLUDED = 1, PFT_VIS_SELF_OCCLUDED = 2, PFT_VIS_OUT_OF_VIEW = 3 };
enum { PFT_VIS_MAX_IMAGE = 1024, PFT_VIS_MAX_SPLAT = 4 };

/* The default camera is a Kinect2 qhd pinhole (960 x 540, f = 540, c = (479.5, 269.5)) divided by six: one pixel is about
 * 1.1 cm at 1 m, the spacing of a 1 cm voxel cloud.  The defaults are reasoned, not tuned on sensor data */
typedef struct pft_visibility_config {
  int32_t width, height;   /* 1 .. PFT_VIS_MAX_IMAGE each                          160 x 90   */
  float fx, fy;            /* focal lengths in pixels: finite, > 0                 90, 90     */
  float cx, cy;            /* principal point: finite                              79.5, 44.5 */
  float z_near;            /* near plane: finite, >= 0                             0.05       */
  int32_t splat;           /* half-width of a point's footprint, 0 .. PFT_VIS_MAX_SPLAT   1   */
  double occlusion_margin; /* depth margin of the scene test: finite, >= 0         0.03       */
  double self_margin;      /* depth margin of the self test: finite, >= 0          0.03       */
} pft_visibility_config;   /* 48 B */

typedef struct pft_visibility_stats {
  float transform[12];     /* the T used, row-major 3x4 */
  uint32_t n_reference, n_visible, n_occluded, n_self, n_out;
  uint32_t n_frame;        /* frame points the depth image was taken over (the device-side count after a filter hand-off) */
  uint32_t has_match, n_visible_matched;
  uint32_t hidden, below, streak, lost;
  uint32_t evaluated;      /* 0: the matrix was NULL and the last iteration raised PftHeader::error: every field but
                              `calls` (and the per-point arrays) keeps the values of the last evaluated call */
  uint32_t calls;          /* pft_visibility launches so far */
} pft_visibility_stats;    /* 104 B */

void pft_visibility_config_default(pft_visibility_config* cfg);
/* the projection above on the host (the device runs the same function).  Returns in_view (0 / 1; 0 for a null argument);
 * uv[0] = u, uv[1] = v are written only when it is 1.  cfg is not validated */
int pft_visibility_project(const pft_visibility_config* cfg, const float xyz[3], int32_t uv[2]);

/* the camera of the pft_visibility calls that follow.  PFT_ERR_INVALID_ARG with a text for a value outside the ranges above */
int pft_set_visibility_camera(pft_tracker* t, const pft_visibility_config* cfg);
int pft_get_visibility_camera(pft_tracker* t, pft_visibility_config* cfg);
/* min_visible_ratio and min_ratio in [0, 1] (defaults 0.25 and 0: never below), lost_after >= 1 (default 1) */
int pft_set_visibility_threshold(pft_tracker* t, double min_visible_ratio, double min_ratio, int lost_after);
int pft_get_visibility_threshold(pft_tracker* t, double* min_visible_ratio, double* min_ratio, int* lost_after);

/* enqueues the visibility of the reference cloud at m12 (row-major 3x4), or with m12 == NULL at the result pose of the
 * last pft_compute, against the handle's current input cloud.  Never synchronises.
 *   PFT_ERR_INVALID_ARG with a text   a sharded handle (world_size > 1), a non-finite entry of m12
 *   PFT_ERR_NO_REFERENCE / PFT_ERR_NO_INPUT   as pft_compute
 *   PFT_ERR_STATE   m12 == NULL before the first pft_compute; an input handed over by pft_set_input_from_filter that no
 *                   pft_compute has read yet (its count is still the filter's)
 * An explicit m12 works right after pft_set_input / pft_set_input_device.  KLD and exact-NN handles are accepted: only
 * the result pose, the model and the input are read */
int pft_visibility(pft_tracker* t, const float* m12);
/* synchronises and copies the last result out; device-side failures are reported as by pft_get_result */
int pft_get_visibility(pft_tracker* t, pft_visibility_stats* out);
/* per reference point in the CALLER's order: state (PFT_VIS_*), scene_gap, self_gap.  Any array may be NULL; *n = the
 * reference size, up to cap entries are copied.  PFT_ERR_STATE without a pft_visibility since the reference was last set */
int pft_get_visibility_points(pft_tracker* t, uint8_t* state, float* scene_gap, float* self_gap, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif
#endif

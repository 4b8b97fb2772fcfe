/*
 * pft_subtract.h -- C ABI of scene subtraction: given the tracked objects at their current poses, say which points of a
 * frame they explain and return the rest as a cloud, without the frame leaving HBM.  Exported by the same libpft_hip.so
 * as pft.h.  DESIGN.md section 3.14 is the specification; in short:
 *
 *   A handle holds up to PFT_SUBTRACT_MAX_OBJECTS slots.  A filled slot s is the point set
 *       Q_s = { xform(T_s, p) : p in model_s },   xform per row ((T0 x + T1 y) + T2 z) + T3 in float, unfused,
 *   T_s a 3x4 float matrix.  Moved points with a non-finite coordinate explain nothing.
 *   For a frame point x and a moved point q:  d2 = (dx dx + dy dy) + dz dz  in float.
 *   x is EXPLAINED iff some filled slot has a q with (double)d2 < (double)radius * (double)radius (strict).
 *   sq_dist[i]  the smallest such d2 over all slots (+inf: unexplained)
 *   owner[i]    the slot attaining it, ties between slots to the lowest slot number (-1: unexplained)
 *   support[s]  the number of frame points with owner == s
 *   residual    the unexplained input points in input order, whole 32-byte records; residual indices ascending
 *   A frame point with a non-finite coordinate is never explained and stays in the residual byte for byte.
 * No result depends on the stored order of a model cloud, on the launch shape or on scheduling.
 *
 * A slot's points are either explicit (a host cloud and a matrix) or bound to a tracker: then every apply takes the
 * tracker's model and its current result pose on the device, T = pose_to_matrix(result), in stream order behind the
 * pft_compute calls made so far.  The move runs on the tracker's stream into this handle's buffers, so a pft_compute
 * enqueued after the apply does not change what the apply saw, and the host never waits.
 *
 * A bound tracker is BORROWED: remove the slot (pft_subtract_remove_object / _clear) or destroy this handle before
 * destroying the tracker.
 *
 * An apply enqueues and returns.  pft_subtract_counts, the getters and pft_subtract_residual_device wait for the
 * handle's stream and return any deferred error.  There is no CPU path.
 */
#ifndef PFT_SUBTRACT_H
#define PFT_SUBTRACT_H

#include "pft.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pft_subtract pft_subtract;

enum { PFT_SUBTRACT_MAX_OBJECTS = 64 };
/* capacity limits (PFT_ERR_CAPACITY): model points of all filled slots together, points of a frame */
enum { PFT_SUBTRACT_MAX_MODEL_POINTS = 1 << 22, PFT_SUBTRACT_MAX_FRAME_POINTS = 1 << 26 };
/* which cloud of a bound tracker is moved: the reference cloud (the default), or the report cloud of pft_set_report_cloud */
enum { PFT_SUBTRACT_REFERENCE_CLOUD = 0, PFT_SUBTRACT_REPORT_CLOUD = 1 };

typedef struct pft_subtract_config {
  uint32_t abi_version; /* PFT_ABI_VERSION */
  int32_t device_id;
  float radius;         /* 0.02: the cluster tolerance of the model-creation nodes */
  int32_t cloud;        /* PFT_SUBTRACT_REFERENCE_CLOUD / _REPORT_CLOUD, for the slots bound from now on */
} pft_subtract_config;

void pft_subtract_default_config(pft_subtract_config* cfg);
/* PFT_ERR_INVALID_ARG: a radius that is not a positive finite number, an unknown cloud, a bad device */
int pft_subtract_create(const pft_subtract_config* cfg, pft_subtract** out);
void pft_subtract_destroy(pft_subtract* s);
const char* pft_subtract_last_error_string(const pft_subtract* s);

/* explicit slot: n points (only x, y, z are read; n = 0 is a filled slot that explains nothing) and a row-major 3x4
 * matrix.  The model is copied once.  PFT_ERR_INVALID_ARG with a text: a slot outside [0, PFT_SUBTRACT_MAX_OBJECTS), a
 * non-finite matrix entry or model coordinate.  PFT_ERR_CAPACITY: more than PFT_SUBTRACT_MAX_MODEL_POINTS points */
int pft_subtract_set_object(pft_subtract* s, int slot, const pft_point_xyzrgba* host_pts, size_t n, const float m12[12]);
/* a new matrix for an explicit slot, without a new upload.  PFT_ERR_STATE: the slot is empty or bound */
int pft_subtract_set_object_matrix(pft_subtract* s, int slot, const float m12[12]);
/* bound slot (see above).  PFT_ERR_INVALID_ARG with a text: a sharded tracker (world_size > 1), a tracker on another
 * device.  PFT_ERR_STATE: the report cloud was asked for and the tracker has none.  A tracker that has not run a
 * pft_compute since it was created or reset is refused by the APPLY, with PFT_ERR_STATE.  KLD and exact-NN trackers are
 * accepted: only the result pose and the model are read */
int pft_subtract_bind_tracker(pft_subtract* s, int slot, pft_tracker* tracker);
int pft_subtract_remove_object(pft_subtract* s, int slot);
int pft_subtract_clear(pft_subtract* s);

/* subtract the filled slots from n points in host / device memory (the device cloud must stay valid, and must have been
 * written, in the order of the handle's stream or before the call).  Enqueues and returns.  n = 0 or no filled slot:
 * PFT_OK, the residual is the input.  PFT_ERR_CAPACITY with a text naming the limit */
int pft_subtract_apply(pft_subtract* s, const pft_point_xyzrgba* host_pts, size_t n);
int pft_subtract_apply_device(pft_subtract* s, const pft_point_xyzrgba* device_pts, size_t n);

/* results of the last apply (PFT_ERR_STATE before the first); any pointer may be NULL */
int pft_subtract_counts(pft_subtract* s, size_t* n_in, size_t* n_explained, size_t* n_residual);
int pft_subtract_get_owner(pft_subtract* s, int32_t* host_owner, size_t capacity);      /* n_in entries */
int pft_subtract_get_sq_dist(pft_subtract* s, float* host_sq_dist, size_t capacity);    /* n_in entries */
int pft_subtract_get_support(pft_subtract* s, uint32_t* host_support, size_t capacity); /* PFT_SUBTRACT_MAX_OBJECTS */
int pft_subtract_get_residual(pft_subtract* s, pft_point_xyzrgba* host_pts, size_t capacity, size_t* n);
int pft_subtract_get_residual_indices(pft_subtract* s, int32_t* host_idx, size_t capacity, size_t* n);
/* the residual where it is, in HBM: valid until the handle's next apply; what pft_segment_apply_device takes */
int pft_subtract_residual_device(pft_subtract* s, const pft_point_xyzrgba** device_pts, size_t* n);
/* the matrix and the moved points (x, y, z per point, in the model's stored order) that the last apply used for a slot:
 * *n = the slot's points, min(capacity, *n) of them are written.  PFT_ERR_STATE: the slot was not filled at that apply */
int pft_subtract_get_object(pft_subtract* s, int slot, float m12[12], float* moved_xyz, size_t capacity, size_t* n);
/* GPU time of the last apply on the handle's stream, milliseconds (moves on the trackers' streams are waited for) */
int pft_subtract_last_ms(pft_subtract* s, double* ms);

#ifdef __cplusplus
}
#endif
#endif

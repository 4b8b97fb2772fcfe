/*
 * pft_grow.h -- C ABI of model growth: fold surface that is seen next to an object's model, frame after frame, into the
 * model, on the device.  Exported by the same libpft_hip.so as pft.h.  This comment is the specification (DESIGN.md
 * section 3.16 repeats it and adds the kernel design); tests/grow_model.py restates it in NumPy and the device reproduces
 * that restatement byte for byte.  One handle per object, on a stream of its own.  There is no CPU path.
 *
 * STATE
 *   cloud   the model, 32-byte records in the OBJECT frame: the initial points in the caller's order, appended points behind
 *   a       the apply counter (uint32): 0 after set_model, the first apply is 1
 *   table   a set of voxels keyed by three signed 21-bit cell indices; a voxel is MODEL or PENDING, and a PENDING voxel
 *           carries hits, last_seen and the representative of the current apply
 *
 * HOST-SIDE CONSTANTS (the device never divides)
 *   inv_leaf = 1.0f / leaf (the correctly rounded float quotient);  max_r2 = max_radius * max_radius in float.
 *   For an apply with the row-major 3x4 float matrix T = [R | t] (object frame -> camera frame), the inverse Ti is formed
 *   in double from the float entries:  Ri[r][c] = R[c][r],  ti[r] = -((R[0][r] t0 + R[1][r] t1) + R[2][r] t2),  and every
 *   entry is rounded to float.  T must be finite; that it is rigid is the caller's business.
 *
 * KEY of an object-frame point y:  k_c = (int32)floorf(y_c * inv_leaf) per axis (float, unfused).  The point has no key if
 *   some |k_c| >= 2^20.
 *
 * APPLY.  a += 1.  For each input point i the FIRST rule that holds gives state[i]:
 *   1 NONFINITE  a coordinate is not finite
 *   2 PLANE      fabsf(((a x + b y) + c z) + d) <= plane_margin for one of the planes (float, unfused; camera frame)
 *   3 FAR        with y = xform(Ti, x), per row ((T0 x + T1 y) + T2 z) + T3 as in pft_subtract.h:
 *                (y0 y0 + y1 y1) + y2 y2 > max_r2, or y has no key
 *   4 KNOWN      the key is a MODEL voxel
 *   5 UNREACHED  no MODEL voxel m has max_c |k_c - m_c| <= reach
 *   6 CANDIDATE  everything else
 *   MODEL in rules 4 and 5 is the MODEL set as it was when the apply began.
 *   For every voxel v that holds a candidate of this apply, once per apply however many candidates fall into it:
 *     v not in the table: it becomes PENDING with hits = 1;  else if a - last_seen > forget: hits = 1;  else hits += 1.
 *     In all cases last_seen = a, and rep(v) is the LOWEST i among its candidates of this apply.
 *   After all points, every PENDING voxel seen in this apply with hits >= confirm becomes MODEL (it keeps its hits and
 *   last_seen); the record {x, y, z = y of rep(v), w = 1.0f, rgba = the rgba of input record rep(v), pad = 0} is appended
 *   to the cloud, state[rep(v)] becomes ADDED, and the appended points are in ASCENDING rep.
 *   No result depends on the launch shape, on scheduling or on where an entry sits in the table.
 *
 * CAPACITY, stated so that it is deterministic.  The table has exactly max_voxels slots; an insertion finds a free slot
 *   whenever one exists.  Dead PENDING entries (a - last_seen > forget) keep their slots.  BEFORE an apply (a already
 *   counts that apply), if more than max_voxels / 2 slots are occupied, the table is rebuilt from the MODEL voxels and the
 *   live PENDING ones; n_rebuilds counts this.  An apply OVERFLOWS iff (occupied slots after that check) + (distinct new
 *   voxels of this apply) > max_voxels.  Then nothing is confirmed, ALL PENDING voxels are dropped (occupied becomes
 *   n_model_voxels), MODEL and the cloud are untouched, state[] still holds rules 1-6, the statistics read overflow = 1
 *   with n_candidate_voxels = n_added = 0, the next synchronising call returns PFT_ERR_CAPACITY once, and the handle stays
 *   usable.  The cloud buffer is n_initial + max_voxels records and so cannot overflow.
 *
 * The defaults of the configuration are reasoned, not tuned: leaf is the reference's downsampling grid (1 cm), so a voxel
 * holds about one frame point; reach 2 cells is the subtraction's 2 cm radius; confirm 3 asks for a surface that three
 * frames agree on (sensor speckle does not repeat); forget 2 lets a voxel miss two frames between sightings; max_radius
 * 0.5 m is above the half diagonal of anything the reference tracks; plane_margin is the reference's RANSAC threshold.
 *
 * An apply enqueues and returns.  The getters wait for the handle's stream and return any deferred error.
 */
#ifndef PFT_GROW_H
#define PFT_GROW_H

#include "pft.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pft_grow pft_grow;

enum {
  PFT_GROW_NONFINITE = 0,
  PFT_GROW_PLANE = 1,
  PFT_GROW_FAR = 2,
  PFT_GROW_KNOWN = 3,
  PFT_GROW_UNREACHED = 4,
  PFT_GROW_CANDIDATE = 5,
  PFT_GROW_ADDED = 6,
  PFT_GROW_N_STATES = 7
};
enum { PFT_GROW_KIND_MODEL = 1, PFT_GROW_KIND_PENDING = 2 };
enum { PFT_GROW_MAX_PLANES = 4, PFT_GROW_MAX_FRAME_POINTS = 1 << 26, PFT_GROW_MAX_MODEL_POINTS = 1 << 22 };

typedef struct pft_grow_config {
  uint32_t abi_version; /* PFT_ABI_VERSION */
  int32_t device_id;
  float leaf;           /* 0.01   finite, > 0 */
  int32_t reach;        /* 2      1 .. 4 cells, Chebyshev */
  int32_t confirm;      /* 3      1 .. 255 applies a voxel must be seen in */
  int32_t forget;       /* 2      1 .. 2^20: a pending voxel not seen for more than this many applies starts again */
  float max_radius;     /* 0.5    finite, > 0: metres from the object-frame origin */
  uint32_t max_voxels;  /* 2^18   a power of two, 64 .. 2^22: table slots */
  float plane_margin;   /* 0.015  finite, >= 0 */
} pft_grow_config;

/* the counts of the last apply and the handle's state behind it, 80 bytes */
typedef struct pft_grow_stats {
  uint32_t applies;                     /* a */
  uint32_t n_in;
  uint32_t n_state[PFT_GROW_N_STATES];  /* input points per final state; n_state[CANDIDATE] excludes the ADDED ones */
  uint32_t n_candidate_voxels;          /* distinct voxels that held a candidate */
  uint32_t n_added;
  uint32_t n_model_points, n_model_voxels;
  uint32_t n_pending_live;              /* PENDING voxels with a - last_seen <= forget */
  uint32_t occupied, n_rebuilds, overflow;
  uint32_t pad[3];
} pft_grow_stats;

void pft_grow_default_config(pft_grow_config* cfg);
/* PFT_ERR_INVALID_ARG with a text: a value outside its range, a bad device.  There is no handle then: the text is what
 * pft_grow_last_error_string returns for a NULL handle (this thread's last refused create) */
int pft_grow_create(const pft_grow_config* cfg, pft_grow** out);
void pft_grow_destroy(pft_grow* g);
const char* pft_grow_last_error_string(const pft_grow* g);

/* copies the cloud, clears the table, makes the voxel of every point MODEL, a = 0; no planes are forgotten.
 * PFT_ERR_INVALID_ARG with a text: a non-finite coordinate, a point without a key.  PFT_ERR_CAPACITY: more than
 * max_voxels / 2 distinct voxels, more than PFT_GROW_MAX_MODEL_POINTS points.  n = 0 is allowed: such a model never grows */
int pft_grow_set_model(pft_grow* g, const pft_point_xyzrgba* host_pts, size_t n);
int pft_grow_set_model_device(pft_grow* g, const pft_point_xyzrgba* device_pts, size_t n);
/* 0 .. PFT_GROW_MAX_PLANES planes {a, b, c, d} in the CAMERA frame, for the applies from now on: what
 * pft_segment_get_plane returns for the table.  PFT_ERR_INVALID_ARG with a text: more planes, a non-finite coefficient */
int pft_grow_set_planes(pft_grow* g, const float* abcd, size_t n_planes);

/* n points in host / device memory (the device cloud must stay valid, and must have been written, in the order of the
 * handle's stream or before the call) and the object's pose m12.  Enqueues and returns.  PFT_ERR_STATE before
 * pft_grow_set_model; PFT_ERR_INVALID_ARG with a text: a non-finite matrix entry; PFT_ERR_CAPACITY: more than
 * PFT_GROW_MAX_FRAME_POINTS points.  A refused apply does not count */
int pft_grow_apply(pft_grow* g, const pft_point_xyzrgba* host_pts, size_t n, const float m12[12]);
int pft_grow_apply_device(pft_grow* g, const pft_point_xyzrgba* device_pts, size_t n, const float m12[12]);

/* results (PFT_ERR_STATE before pft_grow_set_model; states and transform: before the first apply).  After an apply that
 * overflowed the first of these calls returns PFT_ERR_CAPACITY (pft_grow_get_stats still fills *out) */
int pft_grow_get_stats(pft_grow* g, pft_grow_stats* out);
int pft_grow_get_states(pft_grow* g, uint8_t* host_states, size_t capacity);  /* n_in entries */
int pft_grow_get_model(pft_grow* g, pft_point_xyzrgba* host_pts, size_t capacity, size_t* n);
/* the model where it is, in HBM: valid until the handle's next apply or set_model */
int pft_grow_model_device(pft_grow* g, const pft_point_xyzrgba** device_pts, size_t* n);
int pft_grow_get_transform(pft_grow* g, float ti12[12]);  /* the Ti of the last apply */
int pft_grow_last_ms(pft_grow* g, double* ms);            /* GPU time of the last apply, milliseconds */
/* every MODEL and live PENDING entry, sorted by (kx, ky, kz): kxyz receives three int32 per entry; a MODEL voxel of
 * set_model has hits = last_seen = 0.  *n = the entries; min(capacity, *n) are written; any pointer may be NULL */
int pft_debug_grow_get_table(pft_grow* g, int32_t* kxyz, uint32_t* kind, uint32_t* hits, uint32_t* last_seen,
                             size_t capacity, size_t* n);

#ifdef __cplusplus
}
#endif
#endif

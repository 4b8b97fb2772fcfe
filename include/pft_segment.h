/*
 * pft_segment.h -- C ABI of model creation on the device: the two model-creation nodes of the reference
 * (cmaestre/pcl_tracking, PCL 1.8.0 classes), exported by the same libpft_hip.so as pft.h.
 *
 *   create_model_planar_segmentation.cpp:131-203  removeZeroPoints, SACSegmentation (SACMODEL_PLANE, SAC_RANSAC,
 *                                                 1000 iterations, 0.015 m), ExtractIndices (negative), PassThrough
 *                                                 y then x, EuclideanClusterExtraction (0.02 m, 500 .. 25 000 points)
 *   create_model.cpp:131-179                      the same without the plane: PassThrough z, y, x, then the clustering
 *   params.yaml segm_limits                       the box ("normal table")
 *
 * One handle runs the stages in the reference's order as ONE device pipeline over a cloud of 32-byte PCL points:
 *   1. transform (optional, a 4x4 camera->base matrix standing in for the tf lookup, pft/common.hpp operation order)
 *   2. removeZeroPoints on the transformed coordinates (NaN, or all of |x|, |y|, |z| below 0.01, is dropped)
 *   3. plane (optional): RANSAC as SACSegmentation runs it (random = false: mt19937 seeded 12345), refit, inliers
 *   4. ExtractIndices negative: the plane's final inliers are removed (nothing when no plane is found)
 *   5. PassThrough box: per-axis enable, inclusive limits, in the base frame
 *   6. EuclideanClusterExtraction: clusters of min..max points, by size descending, ties by smallest index
 * The output holds each cluster's indices into the caller's INPUT cloud (ascending) and the input's own points.
 * There is no CPU path.  DESIGN.md section 3.7 states the rules and their confidence.
 *
 * Plane rounds (pft_segment_set_plane_rounds) repeat stages 3 and 4 as the reference's cluster_euclid.cpp:59-85 and
 * cluster_extraction.cpp do: planes are taken out one after the other while more than a fraction of the points is
 * left, and only then the box and the clustering run.  The refit's summation order is a second switch
 * (pft_segment_set_refit_order).  Both default to the single plane and PCL's serial sums.
 */
#ifndef PFT_SEGMENT_H
#define PFT_SEGMENT_H

#include "pft.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pft_segment pft_segment;

enum { PFT_PLANE_FOUND = 0, PFT_PLANE_NONE = 1, PFT_PLANE_DISABLED = 2 };

typedef struct pft_segment_config {
  uint32_t abi_version;        /* PFT_ABI_VERSION */
  int32_t device_id;
  void* stream;                /* hipStream_t to run on when stream_is_external, else the handle creates one */
  int32_t stream_is_external;
  /* 1. camera -> base (tf lookup, create_model_planar_segmentation.cpp:119), row-major */
  int32_t transform_enable;
  float transform[16];
  /* 3. SACSegmentation (:161-167) */
  int32_t plane_enable;
  int32_t max_iterations;      /* setMaxIterations (1000); at most 1919 */
  double distance_threshold;   /* setDistanceThreshold (0.015) */
  double probability;          /* setProbability (PCL default 0.99) */
  uint32_t seed;               /* SampleConsensusModel with random = false: 12345 */
  int32_t optimize_coefficients; /* setOptimizeCoefficients (PCL default true) */
  /* 5. PassThrough box (params.yaml segm_limits), base frame, inclusive; axis 0 = x, 1 = y, 2 = z */
  int32_t box_enable[3];
  float box_min[3], box_max[3];
  /* 6. EuclideanClusterExtraction (:184-189) */
  double cluster_tolerance;    /* 0.02 */
  int32_t min_cluster_size;    /* 500 */
  int32_t max_cluster_size;    /* 25 000; min > max: no cluster can be kept, the clustering is skipped */
  uint32_t max_points;         /* initial capacity; grows on demand */
} pft_segment_config;

typedef struct pft_segment_plane {
  int32_t status;              /* PFT_PLANE_FOUND / _NONE (fewer than 3 points, or no good sample) / _DISABLED */
  uint32_t n_valid;            /* points after removeZeroPoints: the cloud RANSAC runs on */
  float coefficients[4];       /* final model (refined when optimize_coefficients), ax + by + cz + d */
  float ransac_coefficients[4];/* the best RANSAC hypothesis before the refit */
  int32_t sample[3];           /* its sample, indices into the removeZeroPoints output */
  uint32_t ransac_inliers;     /* inliers of the best hypothesis */
  uint32_t inliers;            /* final inliers (removed by ExtractIndices negative) */
  uint32_t iterations;         /* RandomSampleConsensus::iterations_ */
  uint32_t hypotheses_scored;  /* hypotheses the device scored (whole batches) */
  uint32_t n_survivors;        /* points handed to the clustering */
} pft_segment_plane;

/* the reference's planar node: transform off, plane on, box x and y of the "normal table" limits, clusters 0.02 m,
 * 500 .. 25 000 points.  create_model.cpp is the same with plane_enable = 0 and box_enable[2] = 1. */
void pft_segment_default_config(pft_segment_config* cfg);
int pft_segment_create(const pft_segment_config* cfg, pft_segment** out);
void pft_segment_destroy(pft_segment* s);
const char* pft_segment_last_error_string(const pft_segment* s);

/* run the pipeline over n points in host / device memory; returns when the clusters are known */
int pft_segment_apply(pft_segment* s, const pft_point_xyzrgba* host_points, size_t n);
int pft_segment_apply_device(pft_segment* s, const pft_point_xyzrgba* device_points, size_t n);

int pft_segment_get_plane(const pft_segment* s, pft_segment_plane* plane);
/* plane inlier indices into the input cloud, ascending: which = 0 the final inliers, 1 those of the best RANSAC
 * hypothesis (before the refit) */
int pft_segment_get_plane_inliers(pft_segment* s, int which, int32_t* host_idx, size_t capacity, size_t* n);
int pft_segment_cluster_count(const pft_segment* s, size_t* n_clusters);
int pft_segment_cluster_sizes(const pft_segment* s, uint32_t* sizes, size_t capacity);
/* all clusters one after the other, in cluster order: indices into the input cloud / the input's points */
int pft_segment_get_cluster_indices(pft_segment* s, int32_t* host_idx, size_t capacity, size_t* n_total);
int pft_segment_get_cluster_points(pft_segment* s, pft_point_xyzrgba* host_pts, size_t capacity, size_t* n_total);
/* the same points where they are, in HBM: cluster j starts at the sum of the sizes of the clusters before it
 * (pft_segment_cluster_sizes).  Valid until the handle's next apply; NULL when there is no cluster */
int pft_segment_clusters_device(const pft_segment* s, const pft_point_xyzrgba** device_pts, size_t* n_total);
/* GPU time of the last apply, milliseconds, without the host's header reads between stages; stage_ms (may be NULL)
 * receives PFT_SEGMENT_STAGES values */
enum { PFT_SEGMENT_STAGES = 7 }; /* compaction, sample stream, scoring, replay, refit, clustering, output */
int pft_segment_last_ms(const pft_segment* s, double* ms, double* stage_ms);

/* ---- plane rounds: cluster_euclid.cpp:59-85 / cluster_extraction.cpp ----
 * With nr the number of points after removeZeroPoints, a round runs while
 *     (double)remaining > min_remaining_fraction * (double)nr        (the reference's size() > 0.3 * nr_points)
 * and fewer than max_planes rounds have run.  Every round is a fresh SACSegmentation::segment over the remaining
 * cloud in ascending input order: the sampler is reseeded, n is the round's cloud size, the refit sums run over the
 * round's inliers.  A round without a plane, or whose plane has no final inlier, ends the loop and removes nothing
 * (the reference's break).  max_planes is this library's cap, the reference has none: reaching it while the condition
 * still holds is reported as PFT_ROUNDS_STOP_MAX_PLANES.  Defaults: max_planes = 1, min_remaining_fraction = 0.0,
 * which is the single plane of create_model_planar_segmentation.cpp. */
enum { PFT_SEGMENT_MAX_PLANES = 16 };
enum { PFT_ROUNDS_STOP_FRACTION = 0, PFT_ROUNDS_STOP_NO_PLANE = 1, PFT_ROUNDS_STOP_MAX_PLANES = 2 };
int pft_segment_set_plane_rounds(pft_segment* s, int max_planes, double min_remaining_fraction);
int pft_segment_get_plane_rounds(const pft_segment* s, int* max_planes, double* min_remaining_fraction);
/* n_planes: planes removed by the last apply; stopped_by: PFT_ROUNDS_STOP_* (either may be NULL) */
int pft_segment_plane_count(const pft_segment* s, size_t* n_planes, int* stopped_by);
/* the record of one round that ran (a last round that found no plane included: status PFT_PLANE_NONE); round 0 always
 * exists and is what pft_segment_get_plane returns.  n_valid is the round's cloud size, sample[3] indexes the round's
 * cloud, n_survivors is the count after all rounds and the box. */
int pft_segment_get_plane_round(const pft_segment* s, size_t round, pft_segment_plane* plane);
/* a round's inliers as indices into the INPUT cloud, ascending; which as in pft_segment_get_plane_inliers */
int pft_segment_get_plane_round_inliers(pft_segment* s, size_t round, int which, int32_t* host_idx, size_t capacity,
                                        size_t* n);

/* summation order of the refit's nine moment sums: PFT_SUM_PCL (default) is computeMeanAndCovarianceMatrix's serial
 * float chain in inlier order; PFT_SUM_TREE is the adjacent-pair tree in float over the inlier list padded with -0.0
 * to a power of two (products rounded to float first), reduced across many workgroups.  Every level of the tree is an
 * aligned subtree, so the bits do not depend on the launch shape.  The two orders are two specifications: their
 * coefficients differ in the last digits and so may the final inliers. */
int pft_segment_set_refit_order(pft_segment* s, int order);

/* the hypotheses of the last apply in draw order, as far as the RANSAC loop consumed them: 3 sample indices (into
 * the removeZeroPoints output) and the inlier count of each; n = RandomSampleConsensus::iterations_ */
int pft_debug_segment_hypotheses(pft_segment* s, int32_t* samples, uint32_t* counts, size_t capacity, size_t* n);
/* the same for one round (sample indices into that round's cloud); round 0 is pft_debug_segment_hypotheses */
int pft_debug_segment_round_hypotheses(pft_segment* s, size_t round, int32_t* samples, uint32_t* counts,
                                       size_t capacity, size_t* n);

/* ---- what the one-lane tail of a round's refit did (csrc/pft_segment_solve.h fills one per solve) ----
 * Everything between the nine sums and the coefficients is + - * / sqrt in float except three library calls; the
 * record holds their arguments and results, so a restatement given the same three values reproduces every other
 * field bit for bit. */
enum {
  PFT_REFIT_SCALE_TINY = 1u << 0,     /* largest |covariance entry| <= FLT_MIN: scale = 1 */
  PFT_REFIT_C0_SMALL = 1u << 1,       /* |c0| < FLT_EPSILON: computeRoots2 */
  PFT_REFIT_A_CLAMPED = 1u << 2,      /* a_over_3 > 0 set to 0 */
  PFT_REFIT_Q_CLAMPED = 1u << 3,      /* q > 0 set to 0 */
  PFT_REFIT_SWAP_01 = 1u << 4,        /* the three swaps of the root sort, in source order */
  PFT_REFIT_SWAP_12 = 1u << 5,
  PFT_REFIT_SWAP_01_AGAIN = 1u << 6,
  PFT_REFIT_R0_FALLBACK = 1u << 7,    /* smallest root <= 0: computeRoots2 */
  PFT_REFIT_D_NEGATIVE = 1u << 8,     /* computeRoots2's discriminant < 0 set to 0 */
  PFT_REFIT_PICK_0 = 1u << 9,         /* the longest cross product: rows (0,1), (0,2), (1,2) */
  PFT_REFIT_PICK_1 = 1u << 10,
  PFT_REFIT_PICK_2 = 1u << 11,
  PFT_REFIT_ZERO_LENGTH = 1u << 12    /* its squared length is 0: the normal is 0 / 0 */
};
typedef struct pft_segment_refit_debug {
  uint32_t m;                  /* inliers of the best hypothesis: the terms of each sum */
  uint32_t branches;           /* PFT_REFIT_* */
  float accu[9];               /* the sums of xx xy xz yy yz zz x y z, divided by m */
  float cov[6];                /* xx xy xz yy yz zz */
  float scale;
  float trig_arg[3];           /* atan2f's y and x, then theta = atan2f(y, x) / 3, the argument of cosf and sinf */
  float trig[3];               /* atan2f(y, x), cosf(theta), sinf(theta); all six are 0 when computeRoots2 came first */
  float roots[3];              /* of the scaled matrix, ascending, as the eigenvector step uses them */
  float len[3];                /* squared lengths of the three cross products */
  float coef[4];               /* the result: pft_segment_plane::coefficients */
} pft_segment_refit_debug;
/* the record of one round's refit (the single plane is round 0).  PFT_ERR_INVALID_ARG: no such round;
 * PFT_ERR_STATE with a text: no apply yet, the round found no plane, or no refit ran (optimize_coefficients off, or
 * fewer than 4 inliers: the coefficients stay) */
int pft_debug_segment_refit(pft_segment* s, size_t round, pft_segment_refit_debug* out);

#ifdef __cplusplus
}
#endif
#endif

/*
 * pft_model.h -- C ABI of the model preparation on the device: the "set object to track" block of the reference's
 * cloud_cb (cmaestre/pcl_tracking auto_tracking.cpp:643-677), exported by the same libpft_hip.so as pft.h.
 *
 *   :659  removeZeroPoints(*ref_cloud, *nonzero_ref)         NaN, or all of |x|, |y|, |z| below 0.01, is dropped
 *   :663  pcl::compute3DCentroid<RefPointType>(*nonzero_ref, c)   dense path: three float chains in index order
 *   :664-668  trans = Identity, translation = c; transformPointCloud(*nonzero_ref, *transed_ref, trans.inverse())
 *   :672  gridSample(transed_ref, *transed_ref_downsampled, downsampling_grid_size_)   pcl::VoxelGrid
 *   :673-675  setReferenceCloud(transed_ref_downsampled), setTrans(trans), reference_dict[obj] = transed_ref
 *
 * One handle runs the four stages in this order as ONE device pipeline on its own stream over a cluster of 32-byte PCL
 * points that lies in host memory, in HBM, or in a segmenter handle (pft_segment.h).  The host reads counts between the
 * stages; no point array crosses to the host.  pft_set_object_from_model (pft.h) gives the result to a tracker.  There is
 * no CPU path.  DESIGN.md section 3.9.
 */
#ifndef PFT_MODEL_H
#define PFT_MODEL_H

#include "pft.h"
#include "pft_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pft_model pft_model;

int pft_model_create(int device_id, pft_model** out);
void pft_model_destroy(pft_model* m);
const char* pft_model_last_error_string(const pft_model* m);

/* Run the stages over n points; returns when the result is in HBM and its counts are known.  leaf > 0: the side of
 * gridSample's VoxelGrid (all three axes; a leaf too small for the cloud hands the re-centred cloud through, as PCL
 * refuses it); leaf <= 0: the reference cloud is the re-centred cloud.  PFT_ERR_NO_INPUT with a text when no point is
 * left after removeZeroPoints (n == 0 included); the handle stays usable.  The input is only read during the call. */
int pft_model_prepare(pft_model* m, const pft_point_xyzrgba* host_pts, size_t n, float leaf);
int pft_model_prepare_device(pft_model* m, const pft_point_xyzrgba* device_pts, size_t n, float leaf);
/* cluster `cluster_index` of the segmenter's last apply, read where it lies.  PFT_ERR_STATE before an apply,
 * PFT_ERR_INVALID_ARG for an index out of range or a segmenter on another device */
int pft_model_prepare_from_segment(pft_model* m, pft_segment* segment, size_t cluster_index, float leaf);

/* n_in: points given; n_nonzero: after removeZeroPoints (the size of transed_ref); n_reference: the size of
 * transed_ref_downsampled.  Any may be NULL */
int pft_model_counts(const pft_model* m, size_t* n_in, size_t* n_nonzero, size_t* n_reference);
/* trans (:664-666): row-major 4x4, the identity with the centroid in column 3 */
int pft_model_get_trans(const pft_model* m, float trans[16]);
/* transed_ref / transed_ref_downsampled: *n = the size, copied when it fits the capacity (else PFT_ERR_CAPACITY) */
int pft_model_get_recentred(pft_model* m, pft_point_xyzrgba* host_out, size_t capacity, size_t* n);
int pft_model_get_reference(pft_model* m, pft_point_xyzrgba* host_out, size_t capacity, size_t* n);
/* both clouds where they are, valid until the handle's next prepare (any pointer may be NULL) */
int pft_model_output_device(const pft_model* m, const pft_point_xyzrgba** recentred, size_t* n_recentred,
                            const pft_point_xyzrgba** reference, size_t* n_reference);
/* GPU time of the last prepare, milliseconds, without the host's reads between the stages; stage_ms (may be NULL)
 * receives PFT_MODEL_STAGES values */
enum { PFT_MODEL_STAGES = 4 }; /* removeZeroPoints, centroid, re-centre, gridSample */
int pft_model_last_ms(const pft_model* m, double* ms, double* stage_ms);

#ifdef __cplusplus
}
#endif
#endif

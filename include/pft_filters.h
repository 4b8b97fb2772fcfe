/*
 * pft_filters.h -- C ABI of the per-frame input filters that run in front of the tracker
 * (SURVEY.md section 8f row 1), exported by the same libpft_hip.so as pft.h.
 *
 * Reference interfaces replaced (cmaestre/pcl_tracking, PCL 1.8.0 classes):
 *   filterPassThrough  /root/reference/src/auto_tracking.cpp:536-547   pcl::PassThrough<PointXYZRGBA>
 *                      (setFilterFieldName("z"), setFilterLimits(0, 10), setKeepOrganized(false)), called :637
 *   gridSampleApprox   /root/reference/src/auto_tracking.cpp:563-575   pcl::ApproximateVoxelGrid<PointXYZRGBA>
 *                      (setLeafSize(0.01 x3)), called per tracked frame :683
 *   gridSample         /root/reference/src/auto_tracking.cpp:549-561   pcl::VoxelGrid<PointXYZRGBA>
 *                      (setLeafSize(0.01 x3)), model preparation :672 and the waiting frames :641
 *
 * One handle runs PassThrough and / or one of the two voxel grids as ONE device pipeline over a cloud of
 * 32-byte PCL points; the output cloud stays in HBM (pft_filter_output_device) so it can be handed to
 * pft_set_input_device() without touching the host.  Results equal the sequential PCL algorithms (the
 * history-table flush order of ApproximateVoxelGrid included); there is no CPU path.
 */
#ifndef PFT_FILTERS_H
#define PFT_FILTERS_H

#include "pft.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PFT_VOXEL_NONE = 0, PFT_VOXEL_APPROX = 1, PFT_VOXEL_EXACT = 2 };

typedef struct pft_filter_config {
  uint32_t abi_version;       /* PFT_ABI_VERSION */
  int32_t device_id;
  void* stream;               /* hipStream_t to run on when stream_is_external, else the handle creates one */
  int32_t stream_is_external;
  /* PassThrough (auto_tracking.cpp:536-547) */
  int32_t pass_enable;
  int32_t pass_field;         /* setFilterFieldName: 0 = "x", 1 = "y", 2 = "z" */
  float pass_min, pass_max;   /* setFilterLimits, inclusive */
  int32_t pass_negative;      /* setFilterLimitsNegative */
  /* voxel grid (auto_tracking.cpp:549-575) */
  int32_t voxel_mode;         /* PFT_VOXEL_NONE / _APPROX (ApproximateVoxelGrid) / _EXACT (VoxelGrid) */
  float leaf_size[3];         /* setLeafSize */
  uint32_t approx_hist_size;  /* ApproximateVoxelGrid history table entries, power of two <= 2048 (PCL: 512) */
  uint32_t max_points;        /* initial capacity; grows on demand */
} pft_filter_config;

typedef struct pft_filter pft_filter;

/* PassThrough z in [0, 10] + ApproximateVoxelGrid(0.01): what the reference runs per tracked frame */
void pft_filter_default_config(pft_filter_config* cfg);
int pft_filter_create(const pft_filter_config* cfg, pft_filter** out);
void pft_filter_destroy(pft_filter* f);
const char* pft_filter_last_error_string(const pft_filter* f);

/* setInputCloud + filter(): run the pipeline over n points in host / device memory.  Returns when the
 * output count is known (one stream synchronisation); the output cloud is then valid in HBM. */
int pft_filter_apply(pft_filter* f, const pft_point_xyzrgba* host_points, size_t n);
int pft_filter_apply_device(pft_filter* f, const pft_point_xyzrgba* device_points, size_t n);
/* The same pipeline (the same launches: the calls above are these followed by the wait), enqueued on the handle's stream
 * without waiting for it.  The host cloud may be reused as soon as the call returns (its upload is the one thing waited
 * for); the device cloud is borrowed until the apply has finished on the device.  The accessors below wait for a pending
 * apply the first time one of them is called after it; pft_set_input_from_filter (pft.h) hands the output to a tracker
 * without any wait.  A VoxelGrid leaf too small for the cloud hands the grid's input through (the whole cloud, or what
 * an enabled PassThrough kept of it), decided on the device.  n == 0 is the empty result, on the host, at once. */
int pft_filter_apply_async(pft_filter* f, const pft_point_xyzrgba* host_points, size_t n);
int pft_filter_apply_device_async(pft_filter* f, const pft_point_xyzrgba* device_points, size_t n);

/* n_pass: points that entered the grid = points that survived PassThrough.  With PassThrough disabled:
 * ApproximateVoxelGrid takes every point, finite or not (n_pass = n); VoxelGrid skips the non-finite points, so n_pass
 * counts the finite ones and pft_filter_get_pass_indices lists them.
 * n_out: points of the output cloud */
int pft_filter_counts(const pft_filter* f, size_t* n_pass, size_t* n_out);
int pft_filter_output_device(const pft_filter* f, const pft_point_xyzrgba** device_points, size_t* n_out);
int pft_filter_get_output(pft_filter* f, pft_point_xyzrgba* host_out, size_t capacity, size_t* n_out);
/* indices (into the input cloud) of the points PassThrough kept, in order (pcl::PassThrough::filter(indices)) */
int pft_filter_get_pass_indices(pft_filter* f, int32_t* host_idx, size_t capacity, size_t* n_pass);
/* GPU time of the last apply (HIP events on the handle's stream), milliseconds */
int pft_filter_last_ms(const pft_filter* f, double* ms);

/* ---- the depth entrance: a registered depth image + colour image instead of the 32-byte records ----
 * The organised cloud is formed on the device (k_depth_deproject) in the handle's own input buffer and the pipeline above
 * runs over it unchanged.  For W x H pixels, pixel (c, r) (column, row) becomes record i = r W + c; there are always W H
 * records, so pft_filter_get_pass_indices lists pixel indices.  All arithmetic is IEEE float, unfused, every operation
 * rounded once:
 *     ifx = 1.0f / fx,  ify = 1.0f / fy                      (host, once per call)
 *     lx = ((float)c - cx) * ifx,  ly = ((float)r - cy) * ify
 *     PFT_DEPTH_U16: valid iff d != 0;                z = (float)d / depth_divisor   (correctly rounded division)
 *     PFT_DEPTH_F32: valid iff d is finite and d > 0; z = d                           (metres)
 *     valid:    {lx * z, ly * z, z, 1.0f}, rgba = 0xff000000 | r << 16 | g << 8 | b (an alpha byte in the image is ignored;
 *               PFT_COLOR_NONE: 0xff000000), the 12 padding bytes zero
 *     invalid:  x = y = z = the quiet NaN 0x7fc00000, data[3] = 1.0f, rgba = 0, padding zero
 * Samples are in host byte order.  A row stride is in bytes; 0 = tightly packed, else >= width x bytes per pixel, any value
 * (odd ones included); bytes between the end of a row and the next row never influence a result and the last row needs
 * only its pixels.  1 <= width, height <= PFT_DEPTH_MAX_AXIS. */
enum { PFT_DEPTH_U16 = 0, PFT_DEPTH_F32 = 1 };
enum { PFT_COLOR_NONE = 0, PFT_COLOR_BGR8 = 1, PFT_COLOR_RGB8 = 2, PFT_COLOR_BGRA8 = 3, PFT_COLOR_RGBA8 = 4 };
enum { PFT_DEPTH_MAX_AXIS = 16384, PFT_DEPTH_SLOTS = 2 };

typedef struct pft_depth_frame {
  uint32_t abi_version;          /* PFT_ABI_VERSION */
  int32_t width, height;
  float fx, fy, cx, cy;          /* fx, fy finite and > 0; cx, cy finite */
  int32_t depth_format;          /* PFT_DEPTH_U16 | PFT_DEPTH_F32 */
  float depth_divisor;           /* U16 only: finite, > 0 */
  int32_t color_format;          /* PFT_COLOR_NONE | _BGR8 | _RGB8 | _BGRA8 | _RGBA8 */
  uint32_t depth_stride, color_stride;
} pft_depth_frame;

/* Kinect2 qhd: 960 x 540, fx = fy = 540, cx = 479.5, cy = 269.5 (six times the default camera of pft_visibility.h);
 * U16 / 1000 (millimetres); BGR8; packed */
void pft_depth_frame_default(pft_depth_frame* d);

/* Errors of the two applies: PFT_ERR_INVALID_ARG with a text that names the field (fx, fy, cx, cy, depth_divisor,
 * depth_format, color_format, depth_stride, color_stride, width, height, depth, color: a null depth pointer, a colour
 * pointer that is missing while a format is set); PFT_ERR_CAPACITY above PFT_DEPTH_MAX_AXIS.  An image without a valid
 * pixel is no error: W H records, an empty output where PassThrough or VoxelGrid drop the NaN records.
 * pft_filter_apply_depth waits for the counts, like pft_filter_apply.  pft_filter_apply_depth_async only enqueues: caller
 * memory is borrowed until its upload is done, the one thing waited for, exactly like pft_filter_apply_async.  Depth and
 * record applies may alternate on one handle in any order. */
int pft_filter_apply_depth(pft_filter* f, const pft_depth_frame* d, const void* depth, const void* color);
int pft_filter_apply_depth_async(pft_filter* f, const pft_depth_frame* d, const void* depth, const void* color);

/* PFT_DEPTH_SLOTS slots of pinned host memory, each sized for the description (grown when a larger one is asked for, which
 * waits for the slot's upload first; *color = NULL with PFT_COLOR_NONE).  An async apply whose depth pointer (and colour
 * pointer, when a format is set) are a slot's waits for nothing: the slot is then busy until its upload has finished,
 * which pft_filter_depth_slot_done reports (wait != 0: waits for it), and the caller writes to a slot only when it is
 * done.  An apply from a slot that is still busy waits for that earlier upload before it enqueues its own. */
int pft_filter_depth_host_buffers(pft_filter* f, const pft_depth_frame* d, int slot, void** depth, void** color);
int pft_filter_depth_slot_done(pft_filter* f, int slot, int wait, int* done);

/* the input cloud of the last apply where the handle owns it -- the organised cloud of a depth apply, the upload of a
 * host record apply -- in HBM, valid until the next apply: what pft_segment_apply_device / pft_subtract_apply_device
 * take.  Waits for a pending apply.  PFT_ERR_STATE before the first apply and after an apply of a device cloud (the handle
 * does not own that cloud) */
int pft_filter_input_device(const pft_filter* f, const pft_point_xyzrgba** device_points, size_t* n);
int pft_filter_get_input(pft_filter* f, pft_point_xyzrgba* host_out, size_t capacity, size_t* n);

#ifdef __cplusplus
}
#endif
#endif

// pft_model.hip -- model preparation on the device (include/pft_model.h): the "set object to track" block of the
// reference's cloud_cb (auto_tracking.cpp:643-677) as one chain of launches on the handle's stream.
//
//   removeZeroPoints   pftk_remove_zero_points: RULE zero of pft_segment.hip and its select / scan / emit compaction, as
//                      the kept input indices and their coordinates in order
//   centroid           k_md_centroid: compute3DCentroid's dense path -- three dependent float chains in index order.  One
//                      workgroup stages the kept coordinates in LDS in rounds, three lanes run the chains (the pattern of
//                      k_sg_refit).  It also forms trans (identity, centroid in column 3) and the inverse's rows
//   re-centre          k_md_recentre: whole 32-byte records gathered in kept order, x' = ((T00 x + T01 y) + T02 z) + T03
//                      with the inverse translation's rows read from memory (pft/common.hpp transformPointCloud: for an
//                      infinite coordinate 0 * inf = NaN reaches the other rows, which x - c would not give)
//   gridSample         the device VoxelGrid of pft_filters.hip (exact mode) on the handle's stream over the re-centred
//                      cloud in HBM; its "leaf too small" hand-through stays
//
// Every kernel takes its count from a device word (the kept count) or from a size the host holds (the input size).
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "pft_devbuf.h"
#include "pft_device_utils.h"
#include "../../include/pft_filters.h"
#include "../../include/pft_model.h"

#define MD_TILE 1024u
#define MD_THREADS 256
#define MD_CEN_THREADS 1024u
#define MD_CEN_STAGE 4096u   // float4 per round: 64 KiB of LDS

struct MdHdr {
  uint32_t n_nonzero;        // points removeZeroPoints kept (k_sg_scan's total)
  uint32_t first_nonfinite;  // first re-centred point with a non-finite coordinate (0xFFFFFFFF: none)
  float centroid[4];
  float trans[16];           // row-major, the centroid in column 3
  float inv[12];             // rows 0..2 of trans.inverse(): the identity, translation negated
};

// compute3DCentroid (PCL 1.8.0 common/impl/centroid.hpp, dense): lane a of wave 0 runs accumulator a over the kept
// points in index order, centroid[a] = sum / (float)count, centroid[3] = 1.  No point kept: nothing is written.
__global__ __launch_bounds__(MD_CEN_THREADS) void k_md_centroid(MdHdr* __restrict__ h, const float4* __restrict__ pts) {
  __shared__ float4 stage[MD_CEN_STAGE];
  const uint32_t tid = threadIdx.x, m = h->n_nonzero;
  if (m == 0) return;  // (uniform)
  const float* sf = reinterpret_cast<const float*>(stage);
  float acc = 0.0f;
  for (uint32_t s0 = 0; s0 < m; s0 += MD_CEN_STAGE) {
    const uint32_t cnt = min(MD_CEN_STAGE, m - s0);
    for (uint32_t k = tid; k < cnt; k += MD_CEN_THREADS) stage[k] = pts[s0 + k];
    __syncthreads();
    if (tid < 3) {
#pragma unroll 8
      for (uint32_t k = 0; k < cnt; k++) acc += sf[4 * k + tid];
    }
    __syncthreads();
  }
  if (tid < 3) {
    const float c = acc / (float)m;
    h->centroid[tid] = c;
    h->trans[4 * tid + 3] = c;
    h->inv[4 * tid + 3] = -c;  // Eigen: -(I * c), exact
  } else if (tid == 3) {
    h->centroid[3] = 1.0f;
  } else if (tid >= 64 && tid < 64 + 16) {  // the rest of trans: the identity
    const uint32_t e = tid - 64;
    if (e % 4 != 3 || e == 15) h->trans[e] = (e % 5 == 0) ? 1.0f : 0.0f;
  } else if (tid >= 128 && tid < 128 + 12) {
    const uint32_t e = tid - 128;
    if (e % 4 != 3) h->inv[e] = (e % 5 == 0) ? 1.0f : 0.0f;
  }
}

// transformPointCloud(nonzero_ref, transed_ref, trans.inverse()): record keep[i] of the input, every byte copied, the
// coordinates replaced
__global__ __launch_bounds__(MD_THREADS) void k_md_recentre(MdHdr* __restrict__ h, const pft_point_xyzrgba* __restrict__ in,
                                                            const uint32_t* __restrict__ keep,
                                                            pft_point_xyzrgba* __restrict__ out) {
  const uint32_t i = blockIdx.x * MD_THREADS + threadIdx.x;
  if (i >= h->n_nonzero) return;
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = h->inv[k];
  const float4* src = reinterpret_cast<const float4*>(in + keep[i]);
  float4 a = src[0];
  const float4 b = src[1];
  float x, y, z;
  xform(T, a.x, a.y, a.z, x, y, z);
  a.x = x;
  a.y = y;
  a.z = z;
  float4* dst = reinterpret_cast<float4*>(out + i);
  dst[0] = a;
  dst[1] = b;
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicMin(&h->first_nonfinite, i);
}

// ---------------------------------------------------------------------------------------------------------------
// host side
enum { MD_NEV = PFT_MODEL_STAGES };  // events: start, after removeZeroPoints, after the centroid, after the re-centring

struct pft_model {
  int device_id = 0;
  hipStream_t stream = nullptr;
  std::string err;
  size_t cap = 0;
  pft_point_xyzrgba* in_own = nullptr;  // upload of a host cloud
  float4* xyz = nullptr;                // scratch of the compaction
  uint8_t* flag = nullptr;
  uint32_t* tile = nullptr;
  uint32_t* keep = nullptr;             // kept input indices
  float4* keep_xyz = nullptr;           // their coordinates
  pft_point_xyzrgba* recentred = nullptr;
  MdHdr* hdr = nullptr;
  MdHdr* host_hdr = nullptr;            // pinned copy
  hipEvent_t ev[MD_NEV] = {};
  pft_filter* grid = nullptr;           // gridSample's VoxelGrid, on this handle's stream
  float grid_leaf = 0.0f;
  // result of the last prepare
  bool have_result = false;
  size_t n_in = 0, n_nonzero = 0, n_reference = 0;
  const pft_point_xyzrgba* reference = nullptr;
  MdHdr res = {};
  double stage_ms[PFT_MODEL_STAGES] = {};
};

static void free_buffers(pft_model* m) {
  pft_dfree(m->in_own); pft_dfree(m->xyz); pft_dfree(m->flag); pft_dfree(m->tile); pft_dfree(m->keep); pft_dfree(m->keep_xyz);
  pft_dfree(m->recentred);
  m->cap = 0;
}

static int ensure_capacity(pft_model* m, size_t n) {
  if (n <= m->cap) return PFT_OK;
  PFT_HIPCHK(m, hipStreamSynchronize(m->stream));
  free_buffers(m);
  const size_t cap = (n + MD_TILE - 1) / MD_TILE * MD_TILE;
  PFT_HIPCHK(m, pft_dalloc(&m->in_own, cap));
  PFT_HIPCHK(m, pft_dalloc(&m->xyz, cap));
  PFT_HIPCHK(m, pft_dalloc(&m->flag, cap));
  PFT_HIPCHK(m, pft_dalloc(&m->tile, cap / MD_TILE));
  PFT_HIPCHK(m, pft_dalloc(&m->keep, cap));
  PFT_HIPCHK(m, pft_dalloc(&m->keep_xyz, cap));
  PFT_HIPCHK(m, pft_dalloc(&m->recentred, cap));
  m->cap = cap;
  return PFT_OK;
}

extern "C" int pft_model_create(int device_id, pft_model** out) {
  if (!out) return PFT_ERR_INVALID_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PFT_ERR_NO_DEVICE;  // no CPU path
  if (device_id < 0 || device_id >= ndev) return PFT_ERR_INVALID_ARG;
  if (hipSetDevice(device_id) != hipSuccess) return PFT_ERR_NO_DEVICE;
  pft_model* m = new pft_model();
  m->device_id = device_id;
  bool ok = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) == hipSuccess;
  if (!ok) m->stream = nullptr;
  for (int k = 0; ok && k < MD_NEV; k++) ok = hipEventCreate(&m->ev[k]) == hipSuccess;
  if (ok)
    ok = pft_dalloc(&m->hdr, 1) == hipSuccess &&
         hipHostMalloc(reinterpret_cast<void**>(&m->host_hdr), sizeof(MdHdr), hipHostMallocDefault) == hipSuccess;
  if (ok) ok = ensure_capacity(m, 25000) == PFT_OK;  // the largest cluster the reference keeps
  if (!ok) {
    pft_model_destroy(m);
    return PFT_ERR_HIP;
  }
  *out = m;
  return PFT_OK;
}

extern "C" void pft_model_destroy(pft_model* m) {
  if (!m) return;
  hipSetDevice(m->device_id);
  if (m->stream) hipStreamSynchronize(m->stream);
  if (m->grid) pft_filter_destroy(m->grid);  // (before the stream it runs on)
  free_buffers(m);
  pft_dfree(m->hdr);
  if (m->host_hdr) hipHostFree(m->host_hdr);
  for (hipEvent_t e : m->ev)
    if (e) hipEventDestroy(e);
  if (m->stream) hipStreamDestroy(m->stream);
  delete m;
}

extern "C" const char* pft_model_last_error_string(const pft_model* m) { return m ? m->err.c_str() : "null handle"; }

// gridSample (:549-561): pcl::VoxelGrid with the leaf on all three axes, the handle re-created when the leaf changes
static int ensure_grid(pft_model* m, float leaf, size_t n) {
  if (m->grid && m->grid_leaf == leaf) return PFT_OK;
  if (m->grid) pft_filter_destroy(m->grid);
  m->grid = nullptr;
  pft_filter_config c;
  pft_filter_default_config(&c);
  c.device_id = m->device_id;
  c.stream = m->stream;
  c.stream_is_external = 1;
  c.pass_enable = 0;
  c.voxel_mode = PFT_VOXEL_EXACT;
  c.leaf_size[0] = c.leaf_size[1] = c.leaf_size[2] = leaf;
  c.max_points = (uint32_t)(n > 25000 ? n : 25000);
  const int r = pft_filter_create(&c, &m->grid);
  if (r != PFT_OK) {
    m->grid = nullptr;
    m->err = "gridSample (stage 4): pft_filter_create failed";
    return r;
  }
  m->grid_leaf = leaf;
  return PFT_OK;
}

static int prepare_common(pft_model* m, const pft_point_xyzrgba* pts, size_t n, float leaf, bool on_device) {
  if (!m || (!pts && n)) return PFT_ERR_INVALID_ARG;
  if (n > 0x7fffffffu) return PFT_ERR_CAPACITY;
  m->have_result = false;
  if (n == 0) {
    m->err = "model preparation: no point left after removeZeroPoints (stage 1): the input cloud is empty";
    return PFT_ERR_NO_INPUT;
  }
  PFT_HIPCHK(m, hipSetDevice(m->device_id));
  int r = ensure_capacity(m, n);
  if (r != PFT_OK) return r;
  hipStream_t st = m->stream;
  const pft_point_xyzrgba* d_in = pts;
  if (!on_device) {
    PFT_HIPCHK(m, hipMemcpyAsync(m->in_own, pts, n * sizeof(pft_point_xyzrgba), hipMemcpyHostToDevice, st));
    d_in = m->in_own;
  }
  MdHdr h0 = {};
  h0.first_nonfinite = 0xFFFFFFFFu;
  PFT_HIPCHK(m, hipMemcpyAsync(m->hdr, &h0, sizeof(MdHdr), hipMemcpyHostToDevice, st));
  PFT_HIPCHK(m, hipEventRecord(m->ev[0], st));
  // 1. removeZeroPoints
  pftk_remove_zero_points(st, d_in, (uint32_t)n, m->xyz, m->flag, m->tile, m->keep, m->keep_xyz, &m->hdr->n_nonzero);
  PFT_HIPCHK(m, hipEventRecord(m->ev[1], st));
  // 2. compute3DCentroid, trans
  hipLaunchKernelGGL(k_md_centroid, dim3(1), dim3(MD_CEN_THREADS), 0, st, m->hdr, (const float4*)m->keep_xyz);
  PFT_HIPCHK(m, hipEventRecord(m->ev[2], st));
  // 3. transformPointCloud by trans.inverse()
  hipLaunchKernelGGL(k_md_recentre, dim3((uint32_t)((n + MD_THREADS - 1) / MD_THREADS)), dim3(MD_THREADS), 0, st, m->hdr,
                     d_in, (const uint32_t*)m->keep, m->recentred);
  PFT_HIPCHK(m, hipEventRecord(m->ev[3], st));
  PFT_HIPCHK(m, hipGetLastError());
  PFT_HIPCHK(m, hipMemcpyAsync(m->host_hdr, m->hdr, sizeof(MdHdr), hipMemcpyDeviceToHost, st));
  PFT_HIPCHK(m, hipStreamSynchronize(st));  // the kept count sizes stage 4
  PFT_HIPCHK(m, hipGetLastError());
  m->res = *m->host_hdr;
  const size_t nz = m->res.n_nonzero;
  if (nz == 0) {
    m->err = "model preparation: no point left after removeZeroPoints (stage 1) of " + std::to_string(n) + " points";
    return PFT_ERR_NO_INPUT;
  }
  for (int k = 0; k < 3; k++) {
    float ms = 0.0f;
    PFT_HIPCHK(m, hipEventElapsedTime(&ms, m->ev[k], m->ev[k + 1]));
    m->stage_ms[k] = ms;
  }
  m->stage_ms[3] = 0.0;
  // 4. gridSample
  m->reference = m->recentred;
  size_t nref = nz;
  if (leaf > 0.0f) {
    r = ensure_grid(m, leaf, nz);
    if (r != PFT_OK) return r;
    r = pft_filter_apply_device(m->grid, m->recentred, nz);
    if (r == PFT_OK) r = pft_filter_output_device(m->grid, &m->reference, &nref);
    if (r != PFT_OK) {
      m->err = std::string("gridSample (stage 4): ") + pft_filter_last_error_string(m->grid);
      return r;
    }
    pft_filter_last_ms(m->grid, &m->stage_ms[3]);
  }
  m->n_in = n;
  m->n_nonzero = nz;
  m->n_reference = nref;
  m->have_result = true;
  return PFT_OK;
}

extern "C" int pft_model_prepare(pft_model* m, const pft_point_xyzrgba* host_pts, size_t n, float leaf) {
  return prepare_common(m, host_pts, n, leaf, false);
}
extern "C" int pft_model_prepare_device(pft_model* m, const pft_point_xyzrgba* device_pts, size_t n, float leaf) {
  return prepare_common(m, device_pts, n, leaf, true);
}

extern "C" int pft_model_prepare_from_segment(pft_model* m, pft_segment* segment, size_t cluster_index, float leaf) {
  if (!m || !segment) return PFT_ERR_INVALID_ARG;
  m->have_result = false;
  const pft_point_xyzrgba* d_pts = nullptr;
  size_t total = 0, nc = 0;
  if (pft_segment_clusters_device(segment, &d_pts, &total) != PFT_OK || pft_segment_cluster_count(segment, &nc) != PFT_OK) {
    m->err = "pft_model_prepare_from_segment: the segmenter has not been applied yet";
    return PFT_ERR_STATE;
  }
  if (pftsg_device_id(segment) != m->device_id) {
    m->err = "pft_model_prepare_from_segment: the segmenter lives on device " + std::to_string(pftsg_device_id(segment)) +
             ", the model preparation on device " + std::to_string(m->device_id);
    return PFT_ERR_INVALID_ARG;
  }
  if (cluster_index >= nc) {
    m->err = "pft_model_prepare_from_segment: cluster " + std::to_string(cluster_index) + " of " + std::to_string(nc);
    return PFT_ERR_INVALID_ARG;
  }
  std::vector<uint32_t> sizes(nc);
  const int r = pft_segment_cluster_sizes(segment, sizes.data(), nc);
  if (r != PFT_OK) return r;
  size_t off = 0;
  for (size_t k = 0; k < cluster_index; k++) off += sizes[k];
  if (off + sizes[cluster_index] > total) return PFT_ERR_STATE;
  // the segmenter's apply has finished on its stream (it returns when the clusters are known); the cluster is read by
  // this call's launches only, which have finished when it returns
  return prepare_common(m, d_pts + off, sizes[cluster_index], leaf, true);
}

extern "C" int pft_model_counts(const pft_model* m, size_t* n_in, size_t* n_nonzero, size_t* n_reference) {
  if (!m) return PFT_ERR_INVALID_ARG;
  if (!m->have_result) return PFT_ERR_STATE;
  if (n_in) *n_in = m->n_in;
  if (n_nonzero) *n_nonzero = m->n_nonzero;
  if (n_reference) *n_reference = m->n_reference;
  return PFT_OK;
}

extern "C" int pft_model_get_trans(const pft_model* m, float trans[16]) {
  if (!m || !trans) return PFT_ERR_INVALID_ARG;
  if (!m->have_result) return PFT_ERR_STATE;
  memcpy(trans, m->res.trans, sizeof(float) * 16);
  return PFT_OK;
}

static int get_cloud(pft_model* m, const pft_point_xyzrgba* src, size_t cnt, pft_point_xyzrgba* host_out, size_t capacity,
                     size_t* n) {
  if (!m || !n) return PFT_ERR_INVALID_ARG;
  if (!m->have_result) return PFT_ERR_STATE;
  *n = cnt;
  if (cnt > capacity) return PFT_ERR_CAPACITY;
  if (!host_out) return PFT_ERR_INVALID_ARG;
  PFT_HIPCHK(m, hipSetDevice(m->device_id));
  PFT_HIPCHK(m, hipMemcpyAsync(host_out, src, cnt * sizeof(pft_point_xyzrgba), hipMemcpyDeviceToHost, m->stream));
  PFT_HIPCHK(m, hipStreamSynchronize(m->stream));
  return PFT_OK;
}

extern "C" int pft_model_get_recentred(pft_model* m, pft_point_xyzrgba* host_out, size_t capacity, size_t* n) {
  return get_cloud(m, m ? m->recentred : nullptr, m ? m->n_nonzero : 0, host_out, capacity, n);
}
extern "C" int pft_model_get_reference(pft_model* m, pft_point_xyzrgba* host_out, size_t capacity, size_t* n) {
  return get_cloud(m, m ? m->reference : nullptr, m ? m->n_reference : 0, host_out, capacity, n);
}

extern "C" int pft_model_output_device(const pft_model* m, const pft_point_xyzrgba** recentred, size_t* n_recentred,
                                       const pft_point_xyzrgba** reference, size_t* n_reference) {
  if (!m) return PFT_ERR_INVALID_ARG;
  if (!m->have_result) return PFT_ERR_STATE;
  if (recentred) *recentred = m->recentred;
  if (n_recentred) *n_recentred = m->n_nonzero;
  if (reference) *reference = m->reference;
  if (n_reference) *n_reference = m->n_reference;
  return PFT_OK;
}

extern "C" int pft_model_last_ms(const pft_model* m, double* ms, double* stage_ms) {
  if (!m || !ms) return PFT_ERR_INVALID_ARG;
  if (!m->have_result) return PFT_ERR_STATE;
  *ms = 0.0;
  for (int k = 0; k < PFT_MODEL_STAGES; k++) {
    *ms += m->stage_ms[k];
    if (stage_ms) stage_ms[k] = m->stage_ms[k];
  }
  return PFT_OK;
}

int pftm_view(const pft_model* m, PftModelView* v) {
  if (!m->have_result) return PFT_ERR_STATE;
  v->recentred = m->recentred;
  v->n_recentred = m->n_nonzero;
  v->reference = m->reference;
  v->n_reference = m->n_reference;
  memcpy(v->trans, m->res.trans, sizeof(v->trans));
  v->first_nonfinite = m->res.first_nonfinite;
  v->device_id = m->device_id;
  return PFT_OK;
}

// pft_view.hip -- the view-dependent reference (include/pft_view.h): at a pose, the points of a
// full-surface model that the camera can see, compacted in index order into a cloud that pft_set_reference_from_view makes
// the reference.  The model can be a grown one (up to 2^22 records), so every pass but the scan of the tile totals runs
// over many workgroups.  Five launches on the handle's stream; PftHeader::rep is read on the device, nothing synchronises.
//
//   k_view_fill      the depth image to +inf; one lane forms T (explicit, or pose_to_matrix of the result) and `run`
//   k_view_project   grid-stride over the records: xyz as one 16-byte load, rules 1 and 2, q = xform(T, p), the pixel,
//                    Zm splatted with atomicMin on the depth bits; {z bits, pixel} stored per record
//   k_view_classify  per tile of 256 records: the gap and the state by rule 3, the four counts of the tile by wave ballots
//   k_view_scan      one workgroup: exclusive scan of the tiles' visible counts, the totals, the result block
//   k_view_compact   per tile: a visible record's global rank = tile base + waves before + lanes before (ballot, mbcnt);
//                    rule 4's decimation on the rank; the kept record's index stored and its 32 bytes copied as 2 x 16
//
// A tile is 256 consecutive records whatever the grid, a workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...;
// the depth image is a minimum of integers and the ranks are sums of integers, so no output depends on the grid or on the
// order in which workgroups run.  No loop waits on another workgroup.
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "pft_tracker.h"
#include "pft_device_utils.h"
#include "pft_vis_project.h"
#include "../../include/pft_view.h"

#define VW_THREADS 256
#define VW_WAVES (VW_THREADS / 64)
#define VW_SCAN_THREADS 1024
#define VW_NONFINITE 0xfffffffeu  // PftViewBufs::q[i].y of a record that rule 1 takes out (VS_NO_PIXEL: rule 2)

__global__ void __launch_bounds__(VW_THREADS) k_view_fill(const PftHeader* __restrict__ hdr, uint32_t words, PftViewArgs a,
                                                          PftViewBufs b) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) b.zbuf[i] = VS_INF_BITS;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // the result pose of an iteration that ran without a target is not evaluated (k_view_scan says so)
    const int run = !(a.use_rep && hdr->error != 0u);
    if (run) {
      float m[12];
      if (a.use_rep) {
        pose_to_matrix(hdr->rep, m);
      } else {
#pragma unroll
        for (int k = 0; k < 12; k++) m[k] = a.m[k];
      }
#pragma unroll
      for (int k = 0; k < 12; k++) b.ctl->T[k] = m[k];
    }
    b.ctl->run = (uint32_t)run;
  }
}

__device__ __forceinline__ bool vw_finite3(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z);
}

// model: the records as pairs of 16 bytes; x y z are the first 12 bytes of the first
__global__ void __launch_bounds__(VW_THREADS) k_view_project(const float4* __restrict__ model, uint32_t N, PftVisCam cam,
                                                             PftViewBufs b) {
  if (!b.ctl->run) return;  // (uniform)
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = b.ctl->T[k];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const float4 r = model[2u * (size_t)i];
    uint32_t zb = 0u, pix = VW_NONFINITE;
    if (vw_finite3(r.x, r.y, r.z)) {
      float qx, qy, qz;
      xform(T, r.x, r.y, r.z, qx, qy, qz);
      int u, v;
      pix = VS_NO_PIXEL;
      zb = __float_as_uint(qz);
      if (vw_finite3(qx, qy, qz) && vis_project(cam, qx, qy, qz, u, v)) {  // (in view: 0 <= u < W, 0 <= v < H, qz > z_near >= 0)
        pix = (uint32_t)v * (uint32_t)cam.W + (uint32_t)u;
        vis_splat(b.zbuf, cam.W, max(u - cam.splat, 0), min(u + cam.splat, cam.W - 1), max(v - cam.splat, 0),
                  min(v + cam.splat, cam.H - 1), zb);
      }
    }
    b.q[i] = make_uint2(zb, pix);
  }
}

// visible records leave as PFT_VIEW_KEPT; k_view_compact turns the decimated ones into PFT_VIEW_DECIMATED
__global__ void __launch_bounds__(VW_THREADS) k_view_classify(uint32_t N, uint32_t n_tiles, PftVisCam cam, PftViewBufs b) {
  __shared__ uint32_t sh[VW_WAVES][4];
  if (!b.ctl->run) return;  // (uniform)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t j = tile * VW_THREADS + tid;
    uint32_t st = 0xffu;  // (beyond N: counted nowhere)
    if (j < N) {
      const uint2 q = b.q[j];
      float gap = 0.0f;
      if (q.y == VW_NONFINITE) {
        st = PFT_VIEW_NONFINITE;
      } else if (q.y == VS_NO_PIXEL) {
        st = PFT_VIEW_OUT_OF_VIEW;
      } else {
        gap = fmaxf(__uint_as_float(q.x) - __uint_as_float(b.zbuf[q.y]), 0.0f);
        st = gap > cam.self_margin ? PFT_VIEW_SELF_OCCLUDED : PFT_VIEW_KEPT;
      }
      b.state[j] = (uint8_t)st;
      b.gap[j] = gap;
    }
    const uint32_t c0 = (uint32_t)__popcll(__ballot(st == PFT_VIEW_KEPT));
    const uint32_t c1 = (uint32_t)__popcll(__ballot(st == PFT_VIEW_SELF_OCCLUDED));
    const uint32_t c2 = (uint32_t)__popcll(__ballot(st == PFT_VIEW_OUT_OF_VIEW));
    const uint32_t c3 = (uint32_t)__popcll(__ballot(st == PFT_VIEW_NONFINITE));
    if (lane == 0) {
      sh[wave][0] = c0;
      sh[wave][1] = c1;
      sh[wave][2] = c2;
      sh[wave][3] = c3;
    }
    __syncthreads();
    if (tid == 0) {
      uint4 c = make_uint4(0u, 0u, 0u, 0u);
      for (int w = 0; w < VW_WAVES; w++) {
        c.x += sh[w][0];
        c.y += sh[w][1];
        c.z += sh[w][2];
        c.w += sh[w][3];
      }
      b.tile_cnt[tile] = c;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(VW_SCAN_THREADS) k_view_scan(uint32_t N, uint32_t n_tiles, uint32_t K, PftViewBufs b) {
  __shared__ uint32_t scratch[18];
  __shared__ uint32_t tot[3];
  const uint32_t tid = threadIdx.x;
  pft_view_stats* out = b.out;
  if (!b.ctl->run) {  // nothing to evaluate: the block, the arrays and the view cloud keep their values
    if (tid == 0) {
      out->evaluated = 0u;
      out->calls = out->calls + 1u;
    }
    return;
  }
  if (tid < 3) tot[tid] = 0u;
  __syncthreads();
  uint32_t carry = 0u, s1 = 0u, s2 = 0u, s3 = 0u;
  for (uint32_t base = 0; base < n_tiles; base += VW_SCAN_THREADS) {  // (uniform trip count)
    const uint32_t tile = base + tid;
    uint4 c = make_uint4(0u, 0u, 0u, 0u);
    if (tile < n_tiles) c = b.tile_cnt[tile];
    uint32_t total;
    const uint32_t ex = block_excl_scan<uint32_t, true>(c.x, scratch, &total);
    if (tile < n_tiles) b.tile_base[tile] = carry + ex;
    carry += total;
    s1 += c.y;
    s2 += c.z;
    s3 += c.w;
  }
  if (s1) atomicAdd(&tot[0], s1);
  if (s2) atomicAdd(&tot[1], s2);
  if (s3) atomicAdd(&tot[2], s3);
  __syncthreads();
  if (tid == 0) {
    const uint32_t n_vis = carry;
    const uint32_t n_kept = (K == 0u || n_vis <= K) ? n_vis : K;
    for (int k = 0; k < 12; k++) out->transform[k] = b.ctl->T[k];
    out->n_model = N;
    out->n_state[PFT_VIEW_KEPT] = n_kept;
    out->n_state[PFT_VIEW_DECIMATED] = n_vis - n_kept;
    out->n_state[PFT_VIEW_SELF_OCCLUDED] = tot[0];
    out->n_state[PFT_VIEW_OUT_OF_VIEW] = tot[1];
    out->n_state[PFT_VIEW_NONFINITE] = tot[2];
    out->n_visible = n_vis;
    out->n_kept = n_kept;
    out->evaluated = 1u;
    out->calls = out->calls + 1u;
  }
}

__global__ void __launch_bounds__(VW_THREADS) k_view_compact(const float4* __restrict__ model, uint32_t N, uint32_t n_tiles,
                                                             uint32_t K, PftViewBufs b) {
  __shared__ uint32_t sh[VW_WAVES];
  if (!b.ctl->run) return;  // (uniform)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n_vis = b.out->n_visible;  // (k_view_scan's, a launch ago)
  const bool decimate = K != 0u && n_vis > K;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t j = tile * VW_THREADS + tid;
    const bool vis = j < N && b.state[j] == (uint8_t)PFT_VIEW_KEPT;
    const unsigned long long bal = __ballot(vis);
    if (lane == 0) sh[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = b.tile_base[tile];
    for (uint32_t w = 0; w < wave; w++) before += sh[w];
    if (vis) {
      const uint32_t r = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));  // the rank among the visible, index order
      bool keep = true;
      uint32_t pos = r;
      if (decimate) {
        const unsigned long long lo = ((unsigned long long)r * K) / n_vis, hi = ((unsigned long long)(r + 1u) * K) / n_vis;
        keep = hi > lo;
        pos = (uint32_t)lo;  // (K <= n_vis: the quotient rises by at most one per rank, so lo kept records lie before)
      }
      if (keep) {  // pos < n_kept <= N: inside kept_idx and cloud
        b.kept_idx[pos] = j;
        const float4 r0 = model[2u * (size_t)j], r1 = model[2u * (size_t)j + 1u];
        b.cloud[2u * (size_t)pos] = r0;
        b.cloud[2u * (size_t)pos + 1u] = r1;
      } else {
        b.state[j] = (uint8_t)PFT_VIEW_DECIMATED;
      }
    }
    __syncthreads();
  }
}

void pftk_view(hipStream_t s, const PftHeader* hdr, const float4* model, uint32_t N, const PftVisCam& cam,
               const PftViewArgs& a, const PftViewBufs& b, uint32_t grid, int num_cus) {
  const uint32_t words = (uint32_t)cam.W * (uint32_t)cam.H;
  const uint32_t n_tiles = (N + VW_THREADS - 1u) / VW_THREADS;
  const uint32_t cap = 8u * (uint32_t)(num_cus > 0 ? num_cus : 256);
  auto shape = [&](uint32_t want) { return dim3(grid ? grid : (want < 1u ? 1u : (want < cap ? want : cap))); };
  hipLaunchKernelGGL(k_view_fill, shape((words + 1023u) / 1024u), dim3(VW_THREADS), 0, s, hdr, words, a, b);
  hipLaunchKernelGGL(k_view_project, shape(n_tiles), dim3(VW_THREADS), 0, s, model, N, cam, b);
  hipLaunchKernelGGL(k_view_classify, shape(n_tiles), dim3(VW_THREADS), 0, s, N, n_tiles, cam, b);
  hipLaunchKernelGGL(k_view_scan, dim3(1), dim3(VW_SCAN_THREADS), 0, s, N, n_tiles, a.K, b);
  hipLaunchKernelGGL(k_view_compact, shape(n_tiles), dim3(VW_THREADS), 0, s, model, N, n_tiles, a.K, b);
}

// ---- host ----
static_assert(sizeof(pft_view_stats) == 88, "pft_view_stats is part of the ABI");
static_assert(sizeof(pft_point_xyzrgba) == 32, "the records are copied as two 16-byte halves");

static int view_select(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n, const float* m12, uint32_t max_points,
                       bool device) {
  if (!t || (!pts && n)) return PFT_ERR_INVALID_ARG;
  if (t->cfg.world_size != 1) {
    t->err = "the view selection is not supported on a sharded handle (world_size > 1)";
    return PFT_ERR_INVALID_ARG;
  }
  if (m12)
    for (int k = 0; k < 12; k++)
      if (!std::isfinite(m12[k])) {
        t->err = "pft_view_select: entry " + std::to_string(k) + " of the matrix is not finite";
        return PFT_ERR_INVALID_ARG;
      }
  if (device && ((uintptr_t)pts & 15u)) {
    t->err = "pft_view_select_device: the cloud is not aligned to 16 bytes";
    return PFT_ERR_INVALID_ARG;
  }
  if (!m12 && !t->initialized) {
    t->err = "pft_view_select without a matrix before the first pft_compute: there is no result pose yet";
    return PFT_ERR_STATE;
  }
  if (n > (size_t)PFT_VIEW_MAX_MODEL_POINTS) {
    t->err = "pft_view_select: " + std::to_string(n) + " records, the maximum is " + std::to_string((int)PFT_VIEW_MAX_MODEL_POINTS);
    return PFT_ERR_CAPACITY;
  }
  hipSetDevice(t->cfg.device_id);
  const uint32_t N = (uint32_t)n;
  const PftVisCam cam = pftk_visibility_cam(t->vis_cam);
  const size_t words = (size_t)cam.W * (size_t)cam.H;
  if (!t->d_view) {
    PFTT_GROW(t, t->d_view_ctl.reserve(1));
    PFTT_GROW(t, t->d_view.alloc(1));
    PFT_HIPCHK(t, hipMemsetAsync(t->d_view, 0, sizeof(pft_view_stats), t->stream));
  }
  if (words > t->d_view_z.cap()) {
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));  // a select in flight may still write the previous image
    PFTT_GROW(t, t->d_view_z.alloc(words));
  }
  if (N > t->d_view_cloud.cap() || !t->d_view_cloud) {
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
    t->d_view_cloud.reset();  // (the capacity of the group: zero until all are there)
    const size_t tiles = ((size_t)N + VW_THREADS - 1u) / VW_THREADS;
    PFTT_GROW(t, t->d_view_q.alloc(N));
    PFTT_GROW(t, t->d_view_state.alloc(N));
    PFTT_GROW(t, t->d_view_gap.alloc(N));
    PFTT_GROW(t, t->d_view_tile.alloc(tiles));
    PFTT_GROW(t, t->d_view_base.alloc(tiles));
    PFTT_GROW(t, t->d_view_idx.alloc(N));
    PFTT_GROW(t, t->d_view_cloud.alloc(N));
    // the results of the selects so far went with the buffers: an unevaluated select finds nothing to keep
    PFT_HIPCHK(t, hipMemsetAsync(t->d_view, 0, offsetof(pft_view_stats, calls), t->stream));
  }
  const pft_point_xyzrgba* model = pts;
  if (!device) {
    if (N > t->d_view_model.cap()) {
      PFT_HIPCHK(t, hipStreamSynchronize(t->stream));  // a select in flight may still read the previous copy
      PFTT_GROW(t, t->d_view_model.alloc(N));
    }
    if (N) PFT_HIPCHK(t, hipMemcpyAsync(t->d_view_model, pts, (size_t)N * sizeof(pft_point_xyzrgba), hipMemcpyHostToDevice, t->stream));
    model = t->d_view_model;
  }
  PftViewArgs a;
  memset(&a, 0, sizeof(a));
  if (m12) memcpy(a.m, m12, sizeof(a.m));
  a.use_rep = m12 ? 0u : 1u;
  a.K = max_points;
  const PftViewBufs b = {t->d_view_ctl, t->d_view_z, t->d_view_q, t->d_view_state, t->d_view_gap, t->d_view_tile,
                         t->d_view_base, t->d_view_idx, reinterpret_cast<float4*>(t->d_view_cloud.get()), t->d_view};
  pftk_view(t->stream, t->d_hdr, reinterpret_cast<const float4*>(model), N, cam, a, b, t->view_grid, t->num_cus);
  PFT_HIPCHK(t, hipGetLastError());
  t->view_issued = true;
  t->view_fresh = true;
  return PFT_OK;
}

extern "C" int pft_view_select(pft_tracker* t, const pft_point_xyzrgba* host_pts, size_t n, const float* m12, uint32_t max_points) {
  return view_select(t, host_pts, n, m12, max_points, false);
}

extern "C" int pft_view_select_device(pft_tracker* t, const pft_point_xyzrgba* device_pts, size_t n, const float* m12,
                                      uint32_t max_points) {
  return view_select(t, device_pts, n, m12, max_points, true);
}

extern "C" int pft_debug_set_view_grid(pft_tracker* t, uint32_t blocks) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (blocks > 65535u) {
    t->err = "pft_debug_set_view_grid: at most 65535 workgroups";
    return PFT_ERR_INVALID_ARG;
  }
  t->view_grid = blocks;
  return PFT_OK;
}

// waits for the last select and copies its block out
static int view_stats(pft_tracker* t, const char* who, pft_view_stats* st) {
  if (!t->view_issued) {
    t->err = std::string(who) + " before the first pft_view_select";
    return PFT_ERR_STATE;
  }
  PFT_HIPCHK(t, hipMemcpyAsync(st, t->d_view, sizeof(pft_view_stats), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return PFT_OK;
}

extern "C" int pft_get_view(pft_tracker* t, pft_view_stats* out) {
  if (!t || !out) return PFT_ERR_INVALID_ARG;
  const int r = view_stats(t, "pft_get_view", out);
  return r != PFT_OK ? r : pftt_check_device_error(t);
}

extern "C" int pft_get_view_points(pft_tracker* t, uint8_t* state, float* self_gap, size_t cap, size_t* n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  pft_view_stats st;
  const int r = view_stats(t, "pft_get_view_points", &st);
  if (r != PFT_OK) return r;
  if (n) *n = st.n_model;
  const size_t c = cap < st.n_model ? cap : st.n_model;
  if (state && c) PFT_HIPCHK(t, hipMemcpyAsync(state, t->d_view_state, c, hipMemcpyDeviceToHost, t->stream));
  if (self_gap && c) PFT_HIPCHK(t, hipMemcpyAsync(self_gap, t->d_view_gap, c * sizeof(float), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

extern "C" int pft_get_view_indices(pft_tracker* t, uint32_t* idx, size_t cap, size_t* n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  pft_view_stats st;
  const int r = view_stats(t, "pft_get_view_indices", &st);
  if (r != PFT_OK) return r;
  if (n) *n = st.n_kept;
  const size_t c = cap < st.n_kept ? cap : st.n_kept;
  if (idx && c) PFT_HIPCHK(t, hipMemcpyAsync(idx, t->d_view_idx, c * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

extern "C" int pft_get_view_cloud(pft_tracker* t, pft_point_xyzrgba* pts, size_t cap, size_t* n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  pft_view_stats st;
  const int r = view_stats(t, "pft_get_view_cloud", &st);
  if (r != PFT_OK) return r;
  if (n) *n = st.n_kept;
  const size_t c = cap < st.n_kept ? cap : st.n_kept;
  if (pts && c) PFT_HIPCHK(t, hipMemcpyAsync(pts, t->d_view_cloud, c * sizeof(pft_point_xyzrgba), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

extern "C" int pft_view_cloud_device(pft_tracker* t, const pft_point_xyzrgba** ptr, size_t* n) {
  if (!t || !ptr || !n) return PFT_ERR_INVALID_ARG;
  pft_view_stats st;
  const int r = view_stats(t, "pft_view_cloud_device", &st);
  if (r != PFT_OK) return r;
  *ptr = t->d_view_cloud;
  *n = st.n_kept;
  return pftt_check_device_error(t);
}

// Every refusal is decided before the current reference is touched
extern "C" int pft_set_reference_from_view(pft_tracker* t, uint32_t min_points) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!t->view_issued || !t->view_fresh) {
    t->err = "pft_set_reference_from_view: no pft_view_select since the last one was consumed";
    return PFT_ERR_STATE;
  }
  hipSetDevice(t->cfg.device_id);
  pft_view_stats st;
  const int r = view_stats(t, "pft_set_reference_from_view", &st);
  if (r != PFT_OK) return r;
  if (!st.evaluated) {
    t->err = "pft_set_reference_from_view: the last pft_view_select was not evaluated (the iteration before it raised an error)";
    return PFT_ERR_STATE;
  }
  const uint32_t need = min_points > 1u ? min_points : 1u;
  if (st.n_kept < need) {
    t->err = "pft_set_reference_from_view: the view keeps " + std::to_string(st.n_kept) + " points, fewer than the " +
             std::to_string(need) + " asked for; the reference cloud stays";
    return PFT_ERR_STATE;
  }
  std::vector<pft_point_xyzrgba> cloud(st.n_kept);
  PFT_HIPCHK(t, hipMemcpy(cloud.data(), t->d_view_cloud, (size_t)st.n_kept * sizeof(pft_point_xyzrgba), hipMemcpyDeviceToHost));
  t->view_fresh = false;
  return pftt_set_reference(t, cloud.data(), cloud.size(), true);
}

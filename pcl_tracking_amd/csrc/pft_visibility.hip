// pft_visibility.hip -- visibility of the reference cloud at a pose (pft_visibility): two depth
// images from the camera at the origin, one of the frame and one of the moved model, tell a model point the scene covers
// from one the model itself covers and from one the camera sees; the occlusion-aware lost rule sits on top.  Four launches
// on the handle's stream, in the pattern of k_match: PftHeader::rep and the input count are read on the device, so
// nothing synchronises.
//
//   k_vis_fill      both images to +inf (one buffer: Zs then Zm)
//   k_vis_model     one workgroup: T, q_j = xform(T, ref_j), the pixel of q_j, Zm splatted; the pixel rectangle of the
//                   in-view model points and their largest z go to the control block
//   k_vis_frame     the frame: z reject (z > z_near, z <= largest model z), projection, rectangle reject, Zs splatted over
//                   the footprint clipped to the rectangle.  Neither reject changes an output: a gap is fmaxf(z_j - Z, 0),
//                   Zs is read at the model points' own pixels only, and a frame point behind every model point adds 0
//   k_vis_classify  one workgroup: gaps, states, the counts by wave ballots with one total per wave through LDS, the
//                   per-point results in the caller's order (ref_perm), the rule in one lane
//
// Depths are the uint32 bit patterns of positive floats (z > z_near >= 0): order-preserving, +inf = 0x7f800000, updated
// with atomicMin.  Only these integer atomics and the kernel boundaries cross workgroups; no loop waits on anything.
#include "pft_device_utils.h"
#include "pft_vis_project.h"  // the projection and the splat, shared with pft_view.hip
#include "../../include/pft_visibility.h"

#define VS_THREADS 1024
#define VS_WAVES (VS_THREADS / 64)

__global__ void __launch_bounds__(256) k_vis_fill(uint32_t* __restrict__ z, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) z[i] = VS_INF_BITS;
}

struct VsModelSh {
  float T[12];
  int run;
  int u0, v0, u1, v1;
  uint32_t zmax, n_in_view;
};

__global__ void __launch_bounds__(VS_THREADS) k_vis_model(PftDev d, uint32_t M, PftVisCam cam, PftVisArgs a, PftVisBufs b) {
  __shared__ VsModelSh sh;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    // the result pose of an iteration that ran without a target is not evaluated (k_vis_classify says so)
    const int run = !(a.use_rep && d.hdr->error != 0u);
    sh.run = run;
    sh.u0 = sh.v0 = 0x7fffffff;
    sh.u1 = sh.v1 = -1;
    sh.zmax = 0u;
    sh.n_in_view = 0u;
    if (run) {
      float m[12];
      if (a.use_rep) {
        pose_to_matrix(d.hdr->rep, m);
      } else {
#pragma unroll
        for (int k = 0; k < 12; k++) m[k] = a.m[k];
      }
#pragma unroll
      for (int k = 0; k < 12; k++) {
        sh.T[k] = m[k];
        b.ctl->T[k] = m[k];
      }
    }
    b.ctl->run = (uint32_t)run;
  }
  __syncthreads();
  if (!sh.run) return;
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = sh.T[k];
  uint32_t* Zm = b.zbuf + (size_t)cam.W * (size_t)cam.H;
  int u0 = 0x7fffffff, v0 = 0x7fffffff, u1 = -1, v1 = -1;
  uint32_t zmax = 0u, seen = 0u;
  for (uint32_t j = tid; j < M; j += VS_THREADS) {
    const float4 r = d.ref_xyz[j];
    float qx, qy, qz;
    xform(T, r.x, r.y, r.z, qx, qy, qz);
    int u, v;
    const uint32_t zb = __float_as_uint(qz);
    uint32_t pix = VS_NO_PIXEL;
    if (vis_project(cam, qx, qy, qz, u, v)) {
      pix = (uint32_t)v * (uint32_t)cam.W + (uint32_t)u;
      vis_splat(Zm, cam.W, max(u - cam.splat, 0), min(u + cam.splat, cam.W - 1), max(v - cam.splat, 0),
                min(v + cam.splat, cam.H - 1), zb);
      u0 = min(u0, u);
      u1 = max(u1, u);
      v0 = min(v0, v);
      v1 = max(v1, v);
      zmax = max(zmax, zb);
      seen++;
    }
    b.q[j] = make_uint2(zb, pix);
  }
  if (seen) {
    atomicMin(&sh.u0, u0);
    atomicMin(&sh.v0, v0);
    atomicMax(&sh.u1, u1);
    atomicMax(&sh.v1, v1);
    atomicMax(&sh.zmax, zmax);
    atomicAdd(&sh.n_in_view, seen);
  }
  __syncthreads();
  if (tid == 0) {
    b.ctl->u0 = sh.u0;
    b.ctl->v0 = sh.v0;
    b.ctl->u1 = sh.u1;
    b.ctl->v1 = sh.v1;
    b.ctl->zmax = sh.zmax;
    b.ctl->n_in_view = sh.n_in_view;
  }
}

// pts: the frame's records, x y z in the first 12 bytes of every stride4 x 16 bytes (the packed 16-byte records, or PCL's
// 32-byte layout while the frame's first crop has not formed them yet)
__global__ void __launch_bounds__(256) k_vis_frame(const float4* __restrict__ pts, uint32_t stride4, uint32_t N,
                                                   const uint32_t* __restrict__ n_dev, PftVisCam cam, PftVisBufs b) {
  const PftVisCtl* ctl = b.ctl;
  if (!ctl->run || ctl->n_in_view == 0u) return;  // (uniform)
  const int u0 = ctl->u0, v0 = ctl->v0, u1 = ctl->u1, v1 = ctl->v1;
  const float zmax = __uint_as_float(ctl->zmax);
  const uint32_t n = n_dev ? min(*n_dev, N) : N;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pts[(size_t)i * stride4];
    if (!(p.z > cam.z_near) || !(p.z <= zmax)) continue;  // (NaN fails both)
    int u, v;
    if (!vis_project(cam, p.x, p.y, p.z, u, v)) continue;
    const int ua = max(u - cam.splat, u0), ub = min(u + cam.splat, u1);
    const int va = max(v - cam.splat, v0), vb = min(v + cam.splat, v1);
    if (ua > ub || va > vb) continue;
    vis_splat(b.zbuf, cam.W, ua, ub, va, vb, __float_as_uint(p.z));
  }
}

__global__ void __launch_bounds__(VS_THREADS) k_vis_classify(PftDev d, uint32_t M, uint32_t N,
                                                             const uint32_t* __restrict__ n_dev, PftVisCam cam, PftVisArgs a,
                                                             PftVisBufs b, const pft_match_stats* __restrict__ match,
                                                             const int32_t* __restrict__ match_idx) {
  __shared__ uint32_t sh[VS_WAVES][5];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  pft_visibility_stats* out = b.out;
  if (!b.ctl->run) {  // nothing to evaluate: the block and the per-point arrays keep their values
    if (tid == 0) {
      out->evaluated = 0u;
      out->calls = out->calls + 1u;
    }
    return;
  }
  const bool has_match = a.match_enqueued && match->evaluated != 0u;
  const uint32_t* Zs = b.zbuf;
  const uint32_t* Zm = b.zbuf + (size_t)cam.W * (size_t)cam.H;
  uint32_t n_vis = 0u, n_occ = 0u, n_self = 0u, n_out = 0u, n_vm = 0u;  // (wave-uniform: popcounts of ballots)
  const uint32_t n_tiles = (M + VS_THREADS - 1u) / VS_THREADS;
  for (uint32_t tile = 0; tile < n_tiles; tile++) {
    const uint32_t j = tile * VS_THREADS + tid;
    uint32_t st = 0xffu;  // (beyond M: counted nowhere)
    bool vm = false;
    if (j < M) {
      const uint2 q = b.q[j];
      const uint32_t o = d.ref_perm[j];  // the caller's order, as the match pairs
      float sgap = 0.0f, mgap = 0.0f;
      if (q.y == VS_NO_PIXEL) {
        st = PFT_VIS_OUT_OF_VIEW;
      } else {
        const float z = __uint_as_float(q.x);
        mgap = fmaxf(z - __uint_as_float(Zm[q.y]), 0.0f);
        sgap = fmaxf(z - __uint_as_float(Zs[q.y]), 0.0f);
        st = mgap > cam.self_margin ? PFT_VIS_SELF_OCCLUDED : (sgap > cam.occlusion_margin ? PFT_VIS_OCCLUDED : PFT_VIS_VISIBLE);
      }
      b.state[o] = (uint8_t)st;
      b.scene_gap[o] = sgap;
      b.self_gap[o] = mgap;
      vm = has_match && st == PFT_VIS_VISIBLE && match_idx[o] >= 0;
    }
    n_vis += (uint32_t)__popcll(__ballot(st == PFT_VIS_VISIBLE));
    n_occ += (uint32_t)__popcll(__ballot(st == PFT_VIS_OCCLUDED));
    n_self += (uint32_t)__popcll(__ballot(st == PFT_VIS_SELF_OCCLUDED));
    n_out += (uint32_t)__popcll(__ballot(st == PFT_VIS_OUT_OF_VIEW));
    n_vm += (uint32_t)__popcll(__ballot(vm));
  }
  if (lane == 0) {
    sh[wave][0] = n_vis;
    sh[wave][1] = n_occ;
    sh[wave][2] = n_self;
    sh[wave][3] = n_out;
    sh[wave][4] = n_vm;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u, c4 = 0u;
    for (int w = 0; w < VS_WAVES; w++) {
      c0 += sh[w][0];
      c1 += sh[w][1];
      c2 += sh[w][2];
      c3 += sh[w][3];
      c4 += sh[w][4];
    }
    for (int k = 0; k < 12; k++) out->transform[k] = b.ctl->T[k];
    out->n_reference = M;
    out->n_visible = c0;
    out->n_occluded = c1;
    out->n_self = c2;
    out->n_out = c3;
    out->n_frame = n_dev ? min(*n_dev, N) : N;
    out->has_match = has_match ? 1u : 0u;
    out->n_visible_matched = c4;
    // the occlusion-aware lost rule: a hidden object is neither below nor recovered -- the streak is held
    const uint32_t hidden = (double)c0 < a.min_visible_ratio * (double)M ? 1u : 0u;
    const uint32_t prev = out->streak;
    uint32_t below = 0u, streak = prev;
    if (has_match && !hidden) {
      below = (double)c4 < a.min_ratio * (double)c0 ? 1u : 0u;
      streak = below ? (prev == 0xffffffffu ? prev : prev + 1u) : 0u;
    }
    out->hidden = hidden;
    out->below = below;
    out->streak = streak;
    out->lost = streak >= a.lost_after ? 1u : 0u;
    out->evaluated = 1u;
    out->calls = out->calls + 1u;
  }
}

// the first call for a reference cloud: the result fields and the per-point arrays start as "nothing evaluated" (a call
// that is not evaluated leaves them so); the rule's state and the call count stay
__global__ void __launch_bounds__(256) k_vis_clear(PftVisBufs b, uint32_t M) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
    b.state[i] = (uint8_t)PFT_VIS_OUT_OF_VIEW;
    b.scene_gap[i] = 0.0f;
    b.self_gap[i] = 0.0f;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    pft_visibility_stats* out = b.out;
    for (int k = 0; k < 12; k++) out->transform[k] = 0.0f;
    out->n_reference = M;
    out->n_visible = out->n_occluded = out->n_self = out->n_out = 0u;
    out->n_frame = 0u;
    out->has_match = out->n_visible_matched = 0u;
    out->hidden = 0u;
    out->evaluated = 0u;
  }
}

void pftk_visibility_clear(hipStream_t s, const PftVisBufs& b, uint32_t M) {
  const uint32_t g = M / 256u < 1u ? 1u : (M / 256u > 64u ? 64u : M / 256u);
  hipLaunchKernelGGL(k_vis_clear, dim3(g), dim3(256), 0, s, b, M);
}

void pftk_visibility(hipStream_t s, const PftDev& d, uint32_t M, const float4* pts, uint32_t stride4, uint32_t N,
                     const uint32_t* n_dev, const PftVisCam& cam, const PftVisArgs& a, const PftVisBufs& b,
                     const pft_match_stats* match, const int32_t* match_idx, int num_cus) {
  const uint32_t words = 2u * (uint32_t)cam.W * (uint32_t)cam.H;
  const uint32_t gf = (words + 1023u) / 1024u;
  hipLaunchKernelGGL(k_vis_fill, dim3(gf < 2048u ? gf : 2048u), dim3(256), 0, s, b.zbuf, words);
  hipLaunchKernelGGL(k_vis_model, dim3(1), dim3(VS_THREADS), 0, s, d, M, cam, a, b);
  const uint32_t cap = 8u * (uint32_t)(num_cus > 0 ? num_cus : 256);
  const uint32_t gn = (N + 255u) / 256u;
  hipLaunchKernelGGL(k_vis_frame, dim3(gn < 1u ? 1u : (gn < cap ? gn : cap)), dim3(256), 0, s, pts, stride4, N, n_dev, cam, b);
  hipLaunchKernelGGL(k_vis_classify, dim3(1), dim3(VS_THREADS), 0, s, d, M, N, n_dev, cam, a, b, match, match_idx);
}

// ---- host ----
extern "C" void pft_visibility_config_default(pft_visibility_config* c) {
  if (!c) return;
  c->width = 160;
  c->height = 90;
  c->fx = c->fy = 90.0f;
  c->cx = 79.5f;
  c->cy = 44.5f;
  c->z_near = 0.05f;
  c->splat = 1;
  c->occlusion_margin = 0.03;
  c->self_margin = 0.03;
}

PftVisCam pftk_visibility_cam(const pft_visibility_config& c) {
  PftVisCam k;
  k.W = c.width;
  k.H = c.height;
  k.splat = c.splat;
  k.fx = c.fx;
  k.fy = c.fy;
  k.cx = c.cx;
  k.cy = c.cy;
  k.z_near = c.z_near;
  k.occlusion_margin = (float)c.occlusion_margin;
  k.self_margin = (float)c.self_margin;
  return k;
}

extern "C" int pft_visibility_project(const pft_visibility_config* cfg, const float xyz[3], int32_t uv[2]) {
  if (!cfg || !xyz || !uv) return 0;
  const PftVisCam k = pftk_visibility_cam(*cfg);
  int u, v;
  if (!vis_project(k, xyz[0], xyz[1], xyz[2], u, v)) return 0;
  uv[0] = u;
  uv[1] = v;
  return 1;
}

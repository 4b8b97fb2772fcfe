// pft_report.hip -- the object report (pft_report): what auto_tracking.cpp's drawResult (:301-326)
// and viz_cb (:432-470) compute from a tracker's result, on the device, after pft_compute on the handle's stream:
//
//   T        pose_to_matrix(PftHeader::rep) with T[2][3] += -0.005f                      drawResult :309-316
//   tracked  ((T0 x + T1 y) + T2 z) + T3 per row of every report point, other fields kept   transformPointCloud
//   centroid sums of the tracked x, y, z / n, [3] = 1                                     compute3DCentroid
//   cov      pt = p - c; y y, y z, z z; pt *= pt.x; x x, x y, x z; / n                     computeCovarianceMatrixNormalized
//   axes     SelfAdjointEigenSolver<Matrix3f>, then col 2 = col 0 x col 1               (report_solve, one lane)
//   box      p2w = [axes^T | -(axes^T c)], getMinMax3D of p2w * tracked, centre, quaternion, size
//
// ONE 1024-thread workgroup: the passes over the points are separated by the one-lane solver, so every hand-off is a
// workgroup barrier.  The moved coordinates are recomputed from the report cloud in each pass (25 000 x 12 B do not fit
// in LDS; the transform is 9 multiplies and adds).
//
// Summation order (pft_config::sum_order):
//   PFT_SUM_TREE  adjacent-pair trees (pft_pair_tree.h, ungated) over the index range padded with -0.0 (the exact additive
//                 identity): a thread's 8 consecutive points (registers), the wave, the 16 waves, then the 8192-point tiles.
//   PFT_SUM_PCL   index-order float chains from +0.0 (PCL's loops): 1024-point tiles are staged in LDS by all threads,
//                 then one lane per sum runs its chain over the tile.
// Min / max are index-ordered with ties to the later point (SSE minps / maxps as getMinMax3D runs them) in both orders.
#include <float.h>

#include "pft_device_utils.h"
#include "pft_pair_tree.h"
#include "pft_report_solve.h"

#define RP_THREADS 1024
#define RP_WAVES (RP_THREADS / 64)
#define RP_PER_THREAD 8
#define RP_PT_LEVELS 4                        // log2(RP_PER_THREAD) + 1
#define RP_TILE (RP_THREADS * RP_PER_THREAD)  // points per tree tile (an aligned subtree of 8192)
#define RP_SEQ_TILE RP_THREADS                // points per LDS tile of the PCL-order chains
#define RP_SEQ_STRIDE (RP_SEQ_TILE + 1)       // one word of padding: the chain lanes read different banks

struct RpSh {
  float T[12];     // the transform used (row-major 3x4)
  float P[12];     // p2w (row-major 3x4)
  float c[3];      // centroid
  float part[RP_WAVES][6];            // per-wave partial sums / minima / maxima
  float stk[PT_MAX_LEVELS][6];        // tile-level binary counter (tree order)
  float acc[6];                       // running results (tile sums, chains, min / max)
  float seq[6][RP_SEQ_STRIDE];        // PCL order: the staged terms of one tile
};

__device__ __forceinline__ void rp_load(const pft_point_xyzrgba* p, uint32_t i, float& x, float& y, float& z) {
  const float4 v = *reinterpret_cast<const float4*>(p + i);
  x = v.x;
  y = v.y;
  z = v.z;
}
// ((T0 x + T1 y) + T2 z) + T3 -- -ffp-contract=off keeps every product and sum rounded on its own
__device__ __forceinline__ void rp_xform(const float* T, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}
// getMinMax3D's running min / max: the new value unless the running one is strictly smaller (larger)
__device__ __forceinline__ float rp_min(float lo, float hi) { return lo < hi ? lo : hi; }
__device__ __forceinline__ float rp_max(float lo, float hi) { return lo > hi ? lo : hi; }

// ---- tree order: K sums of term(i, v[K]) over [0, n); the result lands in sh.acc[0 .. K) ----
template <int K, class Term>
__device__ void rp_tree_sums(RpSh& sh, uint32_t n, Term term) {
  const uint32_t tid = threadIdx.x;
  const uint32_t n_tiles = (n + RP_TILE - 1) / RP_TILE;
  for (uint32_t tile = 0; tile < n_tiles; tile++) {
    const uint32_t base = tile * RP_TILE + tid * RP_PER_THREAD;
    float stk[RP_PT_LEVELS][K];  // binary counter over the thread's 8 points: stk[l] = pending subtree of 2^l points
#pragma unroll
    for (int k = 0; k < RP_PER_THREAD; k++) {
      float v[K];
      const uint32_t i = base + (uint32_t)k;
      if (i < n) {
        term(i, v);
      } else {
#pragma unroll
        for (int j = 0; j < K; j++) v[j] = -0.0f;
      }
      int l = 0;
#pragma unroll
      for (int b = k; b & 1; b >>= 1, l++)
#pragma unroll
        for (int j = 0; j < K; j++) v[j] = stk[l][j] + v[j];
#pragma unroll
      for (int j = 0; j < K; j++) stk[l][j] = v[j];
    }
    float s[K];
#pragma unroll
    for (int j = 0; j < K; j++) s[j] = stk[RP_PT_LEVELS - 1][j];
    pt_wave<false>(s);
    const float root = pt_waves<false, RP_WAVES>(s, sh.part);
    if (tid < (uint32_t)K) pt_push(sh.stk, tile, root);
    __syncthreads();
  }
  if (tid < (uint32_t)K) sh.acc[tid] = pt_fold(sh.stk, n_tiles);
  __syncthreads();
}

// ---- PCL order: K index-order chains of term(i, v[K]) over [0, n); the result lands in sh.acc[0 .. K) ----
template <int K, class Term>
__device__ void rp_chain_sums(RpSh& sh, uint32_t n, Term term) {
  const uint32_t tid = threadIdx.x;
  float acc = 0.0f;  // lane j < K of wave 0 carries chain j
  for (uint32_t base = 0; base < n; base += RP_SEQ_TILE) {
    const uint32_t i = base + tid;
    if (i < n) {
      float v[K];
      term(i, v);
#pragma unroll
      for (int j = 0; j < K; j++) sh.seq[j][tid] = v[j];
    }
    __syncthreads();
    if (tid < (uint32_t)K) {
      const uint32_t m = min((uint32_t)RP_SEQ_TILE, n - base);
      const float* s = sh.seq[tid];
      for (uint32_t k = 0; k < m; k++) acc = acc + s[k];
    }
    __syncthreads();
  }
  if (tid < (uint32_t)K) sh.acc[tid] = acc;
  __syncthreads();
}

// ---- the principal-frame box: index-ordered min / max of p2w * tracked; sh.acc = {min xyz, max xyz} ----
__device__ void rp_minmax(RpSh& sh, const pft_point_xyzrgba* pts, uint32_t n) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n_tiles = (n + RP_TILE - 1) / RP_TILE;
  float T[12], P[12];
#pragma unroll
  for (int k = 0; k < 12; k++) {
    T[k] = sh.T[k];
    P[k] = sh.P[k];
  }
  if (tid == 0)
    for (int j = 0; j < 3; j++) {
      sh.acc[j] = INFINITY;
      sh.acc[3 + j] = -INFINITY;
    }
  for (uint32_t tile = 0; tile < n_tiles; tile++) {
    const uint32_t base = tile * RP_TILE + tid * RP_PER_THREAD;
    float mm[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < RP_PER_THREAD; k++) {
      const uint32_t i = base + (uint32_t)k;
      if (i >= n) break;
      float x, y, z, tx, ty, tz, u[3];
      rp_load(pts, i, x, y, z);
      rp_xform(T, x, y, z, tx, ty, tz);
      rp_xform(P, tx, ty, tz, u[0], u[1], u[2]);
#pragma unroll
      for (int j = 0; j < 3; j++) {
        mm[j] = rp_min(mm[j], u[j]);
        mm[3 + j] = rp_max(mm[3 + j], u[j]);
      }
    }
    // in index order across the lanes: the lower lane is the left operand
#pragma unroll
    for (int j = 0; j < 6; j++)
      for (int o = 1; o < 64; o <<= 1) {
        const float other = __shfl_xor(mm[j], o);
        const bool upper = (lane & (uint32_t)o) != 0;
        const float lo = upper ? other : mm[j], hi = upper ? mm[j] : other;
        mm[j] = j < 3 ? rp_min(lo, hi) : rp_max(lo, hi);
      }
    if (lane == 0)
#pragma unroll
      for (int j = 0; j < 6; j++) sh.part[wave][j] = mm[j];
    __syncthreads();
    if (tid < 6u) {
      float v = sh.acc[tid];
      for (int q = 0; q < RP_WAVES; q++) v = tid < 3u ? rp_min(v, sh.part[q][tid]) : rp_max(v, sh.part[q][tid]);
      sh.acc[tid] = v;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(RP_THREADS) k_report(const pft_point_xyzrgba* __restrict__ pts, uint32_t n,
                                                       const PftHeader* __restrict__ hdr, int sum_order,
                                                       pft_point_xyzrgba* __restrict__ tracked,
                                                       pft_object_report* __restrict__ out) {
  __shared__ RpSh sh;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    float m[12];
    pose_to_matrix(hdr->rep, m);
    m[11] = m[11] + -0.005f;  // drawResult: "move a little bit for better visualization"
    for (int k = 0; k < 12; k++) sh.T[k] = m[k];
  }
  __syncthreads();
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = sh.T[k];

  // pass 1: the tracked cloud and the centroid's three sums
  for (uint32_t i = tid; i < n; i += RP_THREADS) {
    pft_point_xyzrgba p = pts[i];
    float x, y, z;
    rp_xform(T, p.x, p.y, p.z, x, y, z);
    p.x = x;
    p.y = y;
    p.z = z;
    tracked[i] = p;
  }
  auto centroid_terms = [&](uint32_t i, float* v) {
    float x, y, z;
    rp_load(pts, i, x, y, z);
    rp_xform(T, x, y, z, v[0], v[1], v[2]);
  };
  if (sum_order == PFT_SUM_PCL) rp_chain_sums<3>(sh, n, centroid_terms);
  else rp_tree_sums<3>(sh, n, centroid_terms);
  const float nf = (float)n;
  if (tid == 0)
    for (int j = 0; j < 3; j++) sh.c[j] = sh.acc[j] / nf;
  __syncthreads();
  const float cx = sh.c[0], cy = sh.c[1], cz = sh.c[2];

  // pass 2: the covariance's six sums, in computeCovarianceMatrix's order {C11, C12, C22, C00, C01, C02}
  auto cov_terms = [&](uint32_t i, float* v) {
    float x, y, z, tx, ty, tz;
    rp_load(pts, i, x, y, z);
    rp_xform(T, x, y, z, tx, ty, tz);
    const float px = tx - cx, py = ty - cy, pz = tz - cz;
    v[0] = py * py;
    v[1] = py * pz;
    v[2] = pz * pz;
    v[3] = px * px;  // pt *= pt.x
    v[4] = py * px;
    v[5] = pz * px;
  };
  if (sum_order == PFT_SUM_PCL) rp_chain_sums<6>(sh, n, cov_terms);
  else rp_tree_sums<6>(sh, n, cov_terms);

  float cov[3][3], evals[3], axes[3][3];
  if (tid == 0) {
    cov[1][1] = sh.acc[0] / nf;
    cov[1][2] = sh.acc[1] / nf;
    cov[2][2] = sh.acc[2] / nf;
    cov[0][0] = sh.acc[3] / nf;
    cov[0][1] = sh.acc[4] / nf;
    cov[0][2] = sh.acc[5] / nf;
    cov[1][0] = cov[0][1];
    cov[2][0] = cov[0][2];
    cov[2][1] = cov[1][2];
    const uint32_t info = report_solve(cov, evals, axes);
    const float c[3] = {cx, cy, cz};
    for (int i = 0; i < 3; i++) {  // p2w = [axes^T | -(axes^T c)], Eigen's a0 + (a1 + a2)
      const float r0 = axes[0][i], r1 = axes[1][i], r2 = axes[2][i];
      sh.P[4 * i + 0] = r0;
      sh.P[4 * i + 1] = r1;
      sh.P[4 * i + 2] = r2;
      sh.P[4 * i + 3] = -(r0 * c[0] + (r1 * c[1] + r2 * c[2]));
    }
    for (int k = 0; k < 12; k++) out->transform[k] = sh.T[k];
    out->transform[12] = 0.0f;
    out->transform[13] = 0.0f;
    out->transform[14] = 0.0f;
    out->transform[15] = 1.0f;
    out->centroid[0] = cx;
    out->centroid[1] = cy;
    out->centroid[2] = cz;
    out->centroid[3] = 1.0f;
    for (int r = 0; r < 3; r++)
      for (int q = 0; q < 3; q++) {
        out->covariance[3 * r + q] = cov[r][q];
        out->axes[3 * r + q] = axes[r][q];
      }
    for (int j = 0; j < 3; j++) out->eigenvalues[j] = evals[j];
    out->n_points = n;
    out->info = info;
  }
  __syncthreads();

  // pass 3: the box in the principal frame
  rp_minmax(sh, pts, n);
  if (tid == 0) {
    float mn[3], mx[3], md[3], q[4];
    for (int j = 0; j < 3; j++) {
      mn[j] = sh.acc[j];
      mx[j] = sh.acc[3 + j];
      md[j] = 0.5f * (mx[j] + mn[j]);
    }
    const float c[3] = {cx, cy, cz};
    for (int i = 0; i < 3; i++) {
      out->box_min[i] = mn[i];
      out->box_max[i] = mx[i];
      out->box_centre[i] = (axes[i][0] * md[0] + (axes[i][1] * md[1] + axes[i][2] * md[2])) + c[i];
      out->box_size[i] = mx[i] - mn[i];
    }
    rp_quaternion(axes, q);
    for (int j = 0; j < 4; j++) out->box_quat[j] = q[j];
  }
}

void pftk_report(hipStream_t s, const pft_point_xyzrgba* pts, uint32_t n, const PftHeader* hdr, int sum_order,
                 pft_point_xyzrgba* tracked, pft_object_report* out) {
  hipLaunchKernelGGL(k_report, dim3(1), dim3(RP_THREADS), 0, s, pts, n, hdr, sum_order, tracked, out);
}

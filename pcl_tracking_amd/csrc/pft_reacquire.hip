// pft_reacquire.hip -- re-acquisition of a lost object (pft_reacquire): K candidate poses -- every
// centre with every orientation of a lattice -- scored against the frame in the search pft_match uses, and the best one
// selected, all on the device.  The crop and the tree between k_reacquire_candidates and k_reacquire_score are the handle's
// own launches (pftk_aabb, pftk_crop, pftk_octree / pftk_octree_sorted), driven by pft_api_features.hip as pft_eval_weights drives them.
//
//   k_reacquire_centroids   compute3DCentroid of every cluster of a segmenter (PCL's three serial float chains, the chain of
//                           k_md_centroid), one workgroup per cluster: the centres of pft_reacquire_from_segmenter
//   k_reacquire_candidates  candidate k = ((c n_roll + ir) n_pitch + ip) n_yaw + iy: the pose and its 3x4 matrix
//   k_reacquire_score       one workgroup per candidate over tiles of RQ_THREADS reference points in stored (Morton) order:
//                           q = T_k p_j, mt_search (pft_match_search.h), the two gates, five sums
//   k_reacquire_select      one workgroup: the best candidate and the result block
//
// Sums: n_matched and n_inliers are integers; coherence, sum_sq_dist and inlier_sq_dist are adjacent-pair trees in double
// (pft_pair_tree.h, ungated) over the positions 0 .. M-1 padded with +0.0 (every term is >= +0.0): a lane's one position,
// the wave, the waves of the tile, then the tiles.  The first two are k_match's bits for the same T and the same tree.
#include "pft_device_utils.h"
#include "pft_match_search.h"
#include "pft_pair_tree.h"

#define RQ_THREADS 256
#define RQ_WAVES (RQ_THREADS / 64)
#define RQ_CEN_THREADS 256u
#define RQ_CEN_STAGE 1024u  // points per round: 12 KiB of LDS

// ---- the centres of the segmenter form ----
// compute3DCentroid (PCL 1.8.0 common/impl/centroid.hpp, dense): lane a of wave 0 runs accumulator a over the cluster's
// points in index order, centre[a] = sum / (float)count
__global__ __launch_bounds__(RQ_CEN_THREADS) void k_reacquire_centroids(const pft_point_xyzrgba* __restrict__ pts,
                                                                        const uint32_t* __restrict__ first,
                                                                        const uint32_t* __restrict__ count,
                                                                        float* __restrict__ centres) {
  __shared__ float stage[RQ_CEN_STAGE][3];
  const uint32_t c = blockIdx.x, tid = threadIdx.x, m = count[c];
  const pft_point_xyzrgba* p = pts + first[c];
  float acc = 0.0f;
  for (uint32_t s0 = 0; s0 < m; s0 += RQ_CEN_STAGE) {
    const uint32_t cnt = min(RQ_CEN_STAGE, m - s0);
    for (uint32_t k = tid; k < cnt; k += RQ_CEN_THREADS) {
      const float4 v = *reinterpret_cast<const float4*>(&p[s0 + k]);
      stage[k][0] = v.x;
      stage[k][1] = v.y;
      stage[k][2] = v.z;
    }
    __syncthreads();
    if (tid < 3) {
#pragma unroll 8
      for (uint32_t k = 0; k < cnt; k++) acc += stage[k][tid];
    }
    __syncthreads();
  }
  if (tid < 3) centres[3u * c + tid] = m ? acc / (float)m : 0.0f;
}

// ---- the candidates ----
__device__ __forceinline__ float rq_angle(float base, float span, uint32_t i, uint32_t n) {
  return (float)((double)base + (double)span * (((double)i + 0.5) / (double)n - 0.5));
}

__global__ __launch_bounds__(256) void k_reacquire_candidates(const float* __restrict__ centres, uint32_t K, PftRqLattice lat,
                                                              pft_particle* __restrict__ part, float* __restrict__ mats) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const uint32_t iy = k % lat.n[2], r1 = k / lat.n[2];
  const uint32_t ip = r1 % lat.n[1], r2 = r1 / lat.n[1];
  const uint32_t ir = r2 % lat.n[0], c = r2 / lat.n[0];
  pft_particle q;
  q.x = centres[3u * c];
  q.y = centres[3u * c + 1u];
  q.z = centres[3u * c + 2u];
  q.w = 1.0f;
  q.roll = rq_angle(lat.base[0], lat.span[0], ir, lat.n[0]);
  q.pitch = rq_angle(lat.base[1], lat.span[1], ip, lat.n[1]);
  q.yaw = rq_angle(lat.base[2], lat.span[2], iy, lat.n[2]);
  q.weight = 0.0f;
  part[k] = q;
  float m[12];
  pose_to_matrix(q, m);
  store_matrix(mats, k, m);
}

// ---- the scores ----
struct RqSh {
  double part[RQ_WAVES][3];
  double stk[PT_MAX_LEVELS][3];
  uint32_t n_matched, n_inliers;
};

__global__ void __launch_bounds__(RQ_THREADS) k_reacquire_score(PftParams prm, PftDev d, double inl2, PftRqScores out) {
  __shared__ RqSh sh;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, k = blockIdx.x;
  const PftHeader* hdr = d.hdr;
  if (tid == 0) {
    sh.n_matched = 0u;
    sh.n_inliers = 0u;
  }
  __syncthreads();
  float T[12];
  load_matrix(d.mats, k, T);

  const uint32_t M = prm.M;
  const MtTree tree = mt_load_tree(hdr, d, prm);
  const double maxd2 = prm.maxd2;

  uint32_t my_matched = 0u, my_inliers = 0u;
  const uint32_t n_tiles = (M + RQ_THREADS - 1u) / RQ_THREADS;
  for (uint32_t tile = 0; tile < n_tiles; tile++) {
    const uint32_t j = tile * RQ_THREADS + tid;
    double v[3] = {0.0, 0.0, 0.0};  // coherence, sum_sq_dist, inlier_sq_dist
    if (j < M) {
      const float4 r = d.ref_xyz[j];
      float qx, qy, qz;
      xform(T, r.x, r.y, r.z, qx, qy, qz);
      float bd;
      float4 bt;
      uint32_t pos;
      const bool found = mt_search(tree, d, qx, qy, qz, bd, bt, pos);
      if (found && (double)bd < maxd2) {
        v[0] = mt_pair_value(prm, qx, qy, qz, bt, d.ref_hsv[j]);
        v[1] = (double)bd;
        my_matched++;
      }
      if (found && (double)bd < inl2) {
        v[2] = (double)bd;
        my_inliers++;
      }
    }
    pt_wave<false>(v);
    const double root = pt_waves<false, RQ_WAVES>(v, sh.part);
    if (tid < 3u) pt_push(sh.stk, tile, root);
    __syncthreads();
  }
  my_matched = wave_sum(my_matched);
  my_inliers = wave_sum(my_inliers);
  if (lane == 0 && my_matched) atomicAdd(&sh.n_matched, my_matched);
  if (lane == 0 && my_inliers) atomicAdd(&sh.n_inliers, my_inliers);
  __syncthreads();
  if (tid < 3u) {
    double* dst = tid == 0u ? out.coherence : (tid == 1u ? out.sum_sq_dist : out.inlier_sq_dist);
    dst[k] = pt_fold(sh.stk, n_tiles);
  }
  if (tid == 0) {
    out.n_matched[k] = sh.n_matched;
    out.n_inliers[k] = sh.n_inliers;
  }
}

// ---- the selection ----
struct RqBest {
  uint32_t n, k;
  double d;
};
// a before b: more inliers; then the smaller inlier_sq_dist, in double; then the lower index
__device__ __forceinline__ bool rq_before(const RqBest& a, const RqBest& b) {
  if (a.n != b.n) return a.n > b.n;
  if (a.d != b.d) return a.d < b.d;
  return a.k < b.k;
}

__global__ void __launch_bounds__(RQ_THREADS) k_reacquire_select(PftDev d, PftRqScores sc, uint32_t K, uint32_t n_centres,
                                                                 uint32_t per_centre, uint32_t M, double accept_ratio,
                                                                 const pft_particle* __restrict__ part,
                                                                 pft_reacquire_result* __restrict__ out) {
  __shared__ uint32_t s_n[RQ_THREADS], s_k[RQ_THREADS];
  __shared__ double s_d[RQ_THREADS];
  const uint32_t tid = threadIdx.x;
  RqBest b = {0u, 0xffffffffu, 0.0};
  for (uint32_t k = tid; k < K; k += RQ_THREADS) {
    const RqBest c = {sc.n_inliers[k], k, sc.inlier_sq_dist[k]};
    if (b.k == 0xffffffffu || rq_before(c, b)) b = c;
  }
  s_n[tid] = b.n;
  s_k[tid] = b.k;
  s_d[tid] = b.d;
  __syncthreads();
  for (uint32_t h = RQ_THREADS / 2u; h >= 1u; h >>= 1) {
    if (tid < h) {
      const RqBest x = {s_n[tid], s_k[tid], s_d[tid]}, y = {s_n[tid + h], s_k[tid + h], s_d[tid + h]};
      if (y.k != 0xffffffffu && (x.k == 0xffffffffu || rq_before(y, x))) {
        s_n[tid] = y.n;
        s_k[tid] = y.k;
        s_d[tid] = y.d;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const PftHeader* hdr = d.hdr;
    // a failed crop or build left the scores without a target: the flags go to the pinned status block, and the host's
    // next synchronisation point hands them to the caller (as the likelihood launch does for pft_compute)
    if (hdr->error && d.host_stat) {
      d.host_stat[2] = hdr->error;
      d.host_stat[3] |= hdr->error;
    }
    const uint32_t best = s_k[0];
    out->n_centres = n_centres;
    out->n_candidates = K;
    out->n_reference = M;
    out->n_crop = hdr->n_crop;
    out->applied = 0u;
    if (best == 0xffffffffu) {  // K == 0
      out->best = -1;
      out->best_centre = -1;
      const pft_particle z = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      out->pose = z;
      for (int e = 0; e < 12; e++) out->transform[e] = 0.0f;
      out->n_inliers = out->n_matched = out->accepted = 0u;
      out->coherence = out->sum_sq_dist = out->inlier_sq_dist = 0.0;
    } else {
      const uint32_t ni = sc.n_inliers[best];
      out->best = (int32_t)best;
      out->best_centre = (int32_t)(best / per_centre);
      out->pose = part[best];
      for (int e = 0; e < 12; e++) out->transform[e] = d.mats[12u * (size_t)best + e];
      out->n_inliers = ni;
      out->n_matched = sc.n_matched[best];
      out->coherence = sc.coherence[best];
      out->sum_sq_dist = sc.sum_sq_dist[best];
      out->inlier_sq_dist = sc.inlier_sq_dist[best];
      out->accepted = (ni >= 1u && !((double)ni < accept_ratio * (double)M)) ? 1u : 0u;
    }
  }
}

// ---- launchers ----
void pftk_reacquire_centroids(hipStream_t s, const pft_point_xyzrgba* pts, const uint32_t* first, const uint32_t* count,
                              uint32_t n_clusters, float* centres) {
  if (!n_clusters) return;
  hipLaunchKernelGGL(k_reacquire_centroids, dim3(n_clusters), dim3(RQ_CEN_THREADS), 0, s, pts, first, count, centres);
}
void pftk_reacquire_candidates(hipStream_t s, const float* centres, uint32_t K, const PftRqLattice& lat, pft_particle* part,
                               float* mats) {
  if (!K) return;
  hipLaunchKernelGGL(k_reacquire_candidates, dim3((K + 255u) / 256u), dim3(256), 0, s, centres, K, lat, part, mats);
}
void pftk_reacquire_score(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t K, double inlier_d2,
                          const PftRqScores& out) {
  if (!K) return;
  hipLaunchKernelGGL(k_reacquire_score, dim3(K), dim3(RQ_THREADS), 0, s, p, d, inlier_d2, out);
}
void pftk_reacquire_select(hipStream_t s, const PftParams& p, const PftDev& d, const PftRqScores& sc, uint32_t K,
                           uint32_t n_centres, uint32_t per_centre, double accept_ratio, pft_reacquire_result* out) {
  hipLaunchKernelGGL(k_reacquire_select, dim3(1), dim3(RQ_THREADS), 0, s, d, sc, K, n_centres, per_centre, p.M, accept_ratio,
                     d.part_cur, out);
}

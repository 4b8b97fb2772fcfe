// pft_refine.hip -- refinement of a pose against the frame (pft_refine): point-to-point ICP with the
// search of pft_match as the pairing.  The crop and the tree are built once per call by the handle's own launches
// (pftk_aabb, pftk_crop, pftk_octree / pftk_octree_sorted), driven by pft_api_features.hip as pft_reacquire drives them.
//
//   k_refine_init    one lane: the start matrix (the argument, or pose_to_matrix of PftHeader::rep), the state (Q, t) of
//                    it, the eight shifted copies the box is taken over, the control words
//   k_refine_pairs   workgroups of 256 lanes over aligned blocks of 256 stored (Morton) positions: q = T p_j, mt_search
//                    (pft_match_search.h), the two gates, the 17 terms in registers, then the lane -> wave -> workgroup
//                    levels of the one adjacent-pair tree; the block's 17 roots and two counts go to the partial arrays
//   k_refine_step    one workgroup: the grid level of the same tree over the blocks' roots, then pft_refine_solve.h in one
//                    lane: the next T, the trace entry, the loop's decision
//
// Every pass is one k_refine_pairs and one k_refine_step; all max_iterations + 1 passes are enqueued at once and a launch
// that finds the `done` word set returns at once: no atomics, fences or device-scope barriers, and the host waits once.
//
// The tree (pft_pair_tree.h): positions 0 .. M-1 padded with +0.0.  The terms are signed, so every level is the gated form.
#include "pft_device_utils.h"
#include "pft_match_search.h"
#include "pft_pair_tree.h"
#include "pft_refine_solve.h"

#define RF_THREADS 256
#define RF_WAVES (RF_THREADS / 64)

struct PftRefineCtl {
  PftRefineState s;   // the state behind T (unchanged by a zero step)
  float T[12];        // the transform of the next pass
  uint32_t done;      // the loop has ended: later launches return at once
  uint32_t decided;   // the status is known, the next pass is the one that scores the final T
  uint32_t iterations, passes, status;
};

__global__ void k_refine_init(PftRefineArgs a, PftRefineDev r, const PftHeader* __restrict__ hdr, float* __restrict__ mats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float T[12];
  if (a.use_rep)
    pose_to_matrix(hdr->rep, T);
  else
    for (int k = 0; k < 12; k++) T[k] = a.start[k];
  PftRefineState s;
  refine_state_from_matrix(T, &s);
  PftRefineCtl* c = r.ctl;
  c->s = s;
  for (int k = 0; k < 12; k++) {
    c->T[k] = T[k];
    r.result->start[k] = T[k];
  }
  c->done = 0u;
  c->decided = 0u;
  c->iterations = 0u;
  c->passes = 0u;
  c->status = PFT_REFINE_MAX_ITERATIONS_REACHED;
  const float mg = (float)a.margin;
  for (uint32_t k = 0; k < 8u; k++) {
    float m[12];
    for (int e = 0; e < 12; e++) m[e] = T[e];
    m[3] = (k & 4u) ? T[3] + mg : T[3] - mg;
    m[7] = (k & 2u) ? T[7] + mg : T[7] - mg;
    m[11] = (k & 1u) ? T[11] + mg : T[11] - mg;
    store_matrix(mats, k, m);
  }
}

// the lane -> wave -> workgroup levels: v holds one value per lane; npad = the padded size in positions.  The workgroup's
// roots arrive in lanes 0 .. PFT_REFINE_SUMS-1
__device__ __forceinline__ double rf_block_tree(double (&v)[PFT_REFINE_SUMS], uint32_t npad, double (*sh)[PFT_REFINE_SUMS]) {
  pt_wave<true>(v, 1u, npad);
  return pt_waves<true, RF_WAVES>(v, sh, 1u, npad);
}

__global__ void __launch_bounds__(RF_THREADS) k_refine_pairs(PftParams prm, PftDev d, PftRefineDev r, double pair2, double inl2) {
  __shared__ double sh[RF_WAVES][PFT_REFINE_SUMS];
  __shared__ uint32_t sh_n[RF_WAVES][2];
  const PftRefineCtl* ctl = r.ctl;
  if (ctl->done != 0u) return;  // (uniform: the loop has ended)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, g = blockIdx.x;
  const PftHeader* hdr = d.hdr;
  const uint32_t M = prm.M;
  if (g >= r.g_cap || g * RF_THREADS >= M) return;
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = ctl->T[k];
  const double c0 = (double)T[3], c1 = (double)T[7], c2 = (double)T[11];

  const MtTree tree = mt_load_tree(hdr, d, prm);

  double v[PFT_REFINE_SUMS];
#pragma unroll
  for (int q = 0; q < PFT_REFINE_SUMS; q++) v[q] = 0.0;
  uint32_t is_pair = 0u, is_inlier = 0u;
  const uint32_t j = g * RF_THREADS + tid;
  if (j < M) {
    const float4 p = d.ref_xyz[j];
    float qx, qy, qz;
    xform(T, p.x, p.y, p.z, qx, qy, qz);
    float bd;
    float4 bt;
    uint32_t pos;
    const bool found = mt_search(tree, d, qx, qy, qz, bd, bt, pos);
    if (found && (double)bd < pair2) {
      const double a[3] = {(double)qx - c0, (double)qy - c1, (double)qz - c2};
      const double b[3] = {(double)bt.x - c0, (double)bt.y - c1, (double)bt.z - c2};
#pragma unroll
      for (int e = 0; e < 3; e++) {
        v[e] = a[e];
        v[3 + e] = b[e];
#pragma unroll
        for (int f = 0; f < 3; f++) v[6 + 3 * e + f] = a[e] * b[f];
      }
      v[15] = (double)bd;
      is_pair = 1u;
    }
    if (found && (double)bd < inl2) {
      v[16] = (double)bd;
      is_inlier = 1u;
    }
  }
  const uint32_t np = wave_sum(is_pair), ni = wave_sum(is_inlier);
  if (lane == 0) {
    sh_n[wave][0] = np;
    sh_n[wave][1] = ni;
  }
  const double root = rf_block_tree(v, pt_pow2_ceil(M), sh);  // (its barrier also publishes sh_n)
  if (tid < PFT_REFINE_SUMS) r.part[(size_t)tid * r.g_cap + g] = root;
  if (tid == 64) {
    uint32_t a = 0u, b = 0u;
    for (int q = 0; q < RF_WAVES; q++) {
      a += sh_n[q][0];
      b += sh_n[q][1];
    }
    r.part_n[2u * g] = a;
    r.part_n[2u * g + 1u] = b;
  }
}

__global__ void __launch_bounds__(RF_THREADS) k_refine_step(PftDev d, PftRefineDev r, PftRefineArgs a, uint32_t M) {
  __shared__ double sh[RF_WAVES][PFT_REFINE_SUMS];
  __shared__ double stk[PT_MAX_LEVELS][PFT_REFINE_SUMS];
  __shared__ double sums[PFT_REFINE_SUMS];
  __shared__ uint32_t sh_n[RF_WAVES][2];
  PftRefineCtl* ctl = r.ctl;
  if (ctl->done != 0u) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t G = min((M + RF_THREADS - 1u) / RF_THREADS, r.g_cap);  // blocks k_refine_pairs wrote
  const uint32_t NG = pt_pow2_ceil(G);                                   // blocks of the padded tree
  // the grid level: chunks of 256 block roots (one per lane; beyond G the padding), the chunks by a binary counter
  const uint32_t n_chunks = (NG + RF_THREADS - 1u) / RF_THREADS;
  uint32_t my_pairs = 0u, my_inliers = 0u;
  for (uint32_t ch = 0; ch < n_chunks; ch++) {
    const uint32_t g = ch * RF_THREADS + tid;
    double v[PFT_REFINE_SUMS];
#pragma unroll
    for (int q = 0; q < PFT_REFINE_SUMS; q++) v[q] = g < G ? r.part[(size_t)q * r.g_cap + g] : 0.0;
    if (g < G) {
      my_pairs += r.part_n[2u * g];
      my_inliers += r.part_n[2u * g + 1u];
    }
    double root = rf_block_tree(v, NG, sh);
    if (tid < PFT_REFINE_SUMS) {
      root = pt_push(stk, ch, root);
      if (ch + 1u == n_chunks) sums[tid] = root;  // (n_chunks is a power of two: the last merge is the root)
    }
    __syncthreads();  // (sh is written again by the next chunk)
  }
  my_pairs = wave_sum(my_pairs);
  my_inliers = wave_sum(my_inliers);
  if (lane == 0) {
    sh_n[wave][0] = my_pairs;
    sh_n[wave][1] = my_inliers;
  }
  __syncthreads();
  if (tid != 0) return;

  uint32_t n_pairs = 0u, n_inliers = 0u;
  for (int q = 0; q < RF_WAVES; q++) {
    n_pairs += sh_n[q][0];
    n_inliers += sh_n[q][1];
  }
  const PftHeader* hdr = d.hdr;
  pft_refine_result* out = r.result;
  const uint32_t k = ctl->passes;
  pft_refine_trace_entry* e = r.trace + k;
  for (int q = 0; q < 12; q++) e->transform[q] = ctl->T[q];
  e->n_pairs = n_pairs;
  e->n_inliers = n_inliers;
  for (int q = 0; q < PFT_REFINE_SUMS; q++) e->sums[q] = sums[q];
  e->step_t2 = 0.0;
  e->step_r2 = 0.0;
  ctl->passes = k + 1u;
  const pft_refine_score sc = {n_pairs, n_inliers, sums[15], sums[16]};
  if (k == 0u) {
    // a failed crop or build left the passes without a target: the flags go to the pinned status block, and the host's
    // synchronisation point hands them to the caller (as k_reacquire_select does)
    if (hdr->error && d.host_stat) {
      d.host_stat[2] = hdr->error;
      d.host_stat[3] |= hdr->error;
    }
    out->before = sc;
    out->n_reference = M;
    out->n_crop = hdr->n_crop;
    for (int q = 0; q < 6; q++) out->bbox[q] = (double)hdr->bbox[q];
  }
  bool finish = ctl->decided != 0u;  // this pass was the one after the last solve
  if (!finish) {
    if (n_pairs < a.min_pairs) {
      ctl->status = PFT_REFINE_TOO_FEW_PAIRS;
      finish = true;
    } else {
      const double c[3] = {(double)ctl->T[3], (double)ctl->T[7], (double)ctl->T[11]};
      PftRefineState s = ctl->s;
      double dq[4], step2[2];
      refine_solve(sums, n_pairs, c, &s, dq, step2);
      e->step_t2 = step2[0];
      e->step_r2 = step2[1];
      if (!(step2[0] == 0.0 && step2[1] == 0.0)) {
        float T[12];
        refine_transform(&s, T);
        for (int q = 0; q < 12; q++) ctl->T[q] = T[q];
        ctl->s = s;
      }
      ctl->iterations = k + 1u;
      if (step2[0] < a.trans_eps2 && step2[1] < a.rot_eps2) {
        ctl->status = PFT_REFINE_CONVERGED;
        ctl->decided = 1u;
      } else if (k + 1u >= a.max_iterations) {
        ctl->status = PFT_REFINE_MAX_ITERATIONS_REACHED;
        ctl->decided = 1u;
      }
    }
  }
  if (finish) {
    out->after = sc;
    out->status = ctl->status;
    out->iterations = ctl->iterations;
    for (int q = 0; q < 12; q++) out->transform[q] = ctl->T[q];
    const pft_refine_score b = out->before;
    out->improved = (sc.n_inliers > b.n_inliers || (sc.n_inliers == b.n_inliers && sc.inlier_sq_dist < b.inlier_sq_dist)) ? 1u : 0u;
    out->applied = 0u;
    ctl->done = 1u;
  }
}

size_t pftk_refine_ctl_bytes() { return sizeof(PftRefineCtl); }
// blocks the partial arrays must have room for: M reference points
uint32_t pftk_refine_blocks(uint32_t M) { return (M + RF_THREADS - 1u) / RF_THREADS; }

void pftk_refine_init(hipStream_t s, const PftRefineArgs& a, const PftRefineDev& r, const PftHeader* hdr, float* mats) {
  hipLaunchKernelGGL(k_refine_init, dim3(1), dim3(64), 0, s, a, r, hdr, mats);
}

void pftk_refine_passes(hipStream_t s, const PftParams& p, const PftDev& d, const PftRefineDev& r, const PftRefineArgs& a) {
  const uint32_t G = pftk_refine_blocks(p.M);
  for (uint32_t k = 0; k <= a.max_iterations; k++) {
    hipLaunchKernelGGL(k_refine_pairs, dim3(G ? G : 1u), dim3(RF_THREADS), 0, s, p, d, r, a.pair2, a.inl2);
    hipLaunchKernelGGL(k_refine_step, dim3(1), dim3(RF_THREADS), 0, s, d, r, a, p.M);
  }
}

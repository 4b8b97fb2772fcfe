// pft_match.hip -- match statistics of the result pose (pft_match): how much of the reference
// cloud, moved by the frame's result, finds a partner in the frame -- taken in the search the likelihood itself uses --
// and the lost-object rule on top of it.  One launch on the handle's stream after pft_compute, in the pattern of
// k_report: it reads PftHeader::rep on the device, so nothing synchronises.
//
//   T        pose_to_matrix(PftHeader::rep) (double sin / cos rounded to float; no -5 mm offset: that one is drawResult's)
//   q        ((T0 x + T1 y) + T2 z) + T3 per row of every reference point, the likelihood kernel's xform
//   (pos, d2) mt_search of q (pft_match_search.h) in the tree the frame's last iteration built
//   matched  (double)d2 < max_distance^2, the likelihood's gate
//   pair     DistanceCoherence x HSVColorCoherence of (q, partner), restated from pft_likelihood.hip (A7) with the two
//            divisions PCL makes instead of that kernel's one reciprocal of the product: this is not the hot loop
//
// Sums: n_matched is an integer; coherence and sum_sq_dist are adjacent-pair trees in double (pft_pair_tree.h, ungated) over
// the stored (Morton) positions 0 .. M-1 padded with +0.0 (every term is >= +0.0, so the padding adds nothing): a lane's
// one position, the wave, the 16 waves, then the 1024-position tiles.
#include "pft_device_utils.h"
#include "pft_match_search.h"
#include "pft_pair_tree.h"

#define MT_THREADS 1024
#define MT_WAVES (MT_THREADS / 64)

struct MtSh {
  float T[12];
  double part[MT_WAVES][2];
  double stk[PT_MAX_LEVELS][2];
  uint32_t n_matched;
  int run;
};

__global__ void __launch_bounds__(MT_THREADS) k_match(PftParams prm, PftDev d, double min_ratio, uint32_t lost_after,
                                                      pft_match_stats* __restrict__ out,
                                                      int32_t* __restrict__ input_idx, float* __restrict__ sq_dist) {
  __shared__ MtSh sh;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const PftHeader* hdr = d.hdr;
  if (tid == 0) {
    // nothing to evaluate: the last iteration was skipped by the change detector (the crop was rewritten, the tree was
    // not: it must not be read) or ran without a target (PftHeader::error).  The statistics keep their previous values
    const int run = !(pft_unchanged(d.gate) || hdr->error != 0u);
    sh.run = run;
    sh.n_matched = 0u;
    if (run) {
      float m[12];
      pose_to_matrix(hdr->rep, m);
      for (int k = 0; k < 12; k++) sh.T[k] = m[k];
    } else {
      out->evaluated = 0u;
      out->calls = out->calls + 1u;
    }
  }
  __syncthreads();
  if (!sh.run) return;

  const uint32_t M = prm.M;
  // an empty crop (or a tree that was never built) is evaluated: nothing matches
  const MtTree tree = mt_load_tree(hdr, d, prm);
  const double maxd2 = prm.maxd2;

  uint32_t my_matched = 0u;
  const uint32_t n_tiles = (M + MT_THREADS - 1u) / MT_THREADS;
  for (uint32_t tile = 0; tile < n_tiles; tile++) {
    const uint32_t j = tile * MT_THREADS + tid;
    double v[2] = {0.0, 0.0};  // coherence, sum_sq_dist
    if (j < M) {
      float T[12];  // (read per tile: kept across the tiles it would stay in 12 registers through every search)
#pragma unroll
      for (int k = 0; k < 12; k++) T[k] = sh.T[k];
      const float4 r = d.ref_xyz[j];
      float qx, qy, qz;
      xform(T, r.x, r.y, r.z, qx, qy, qz);
      float bd;
      float4 bt;
      uint32_t pos;
      const bool matched = mt_search(tree, d, qx, qy, qz, bd, bt, pos) && (double)bd < maxd2;
      const uint32_t o = d.ref_perm[j];  // the caller's order, as pft_eval_weights reports its pairs
      // (the partner's position in the cropped cloud, then the caller's index of it)
      input_idx[o] = matched ? d.crop_idx[min(d.leaf_order[pos], tree.n_crop - 1u)] : -1;
      sq_dist[o] = bd;
      if (matched) {
        v[0] = mt_pair_value(prm, qx, qy, qz, bt, d.ref_hsv[j]);
        v[1] = (double)bd;
        my_matched++;
      }
    }
    pt_wave<false>(v);
    const double root = pt_waves<false, MT_WAVES>(v, sh.part);
    if (tid < 2u) pt_push(sh.stk, tile, root);
    __syncthreads();
  }
  my_matched = wave_sum(my_matched);
  if (lane == 0 && my_matched) atomicAdd(&sh.n_matched, my_matched);
  if (tid < 2u) sh.part[0][tid] = pt_fold(sh.stk, n_tiles);
  __syncthreads();
  if (tid == 0) {
    const uint32_t nm = sh.n_matched;
    for (int k = 0; k < 12; k++) out->transform[k] = sh.T[k];
    out->coherence = sh.part[0][0];
    out->sum_sq_dist = sh.part[0][1];
    out->n_reference = M;
    out->n_matched = nm;
    out->n_crop = hdr->n_crop;  // (the raw count, also of a crop whose tree is unusable)
    out->evaluated = 1u;
    // the lost rule: `lost_after` frames in a row with fewer than min_ratio * M matched points
    const uint32_t below = (double)nm < min_ratio * (double)M ? 1u : 0u;
    const uint32_t prev = out->streak;
    const uint32_t streak = below ? (prev == 0xffffffffu ? prev : prev + 1u) : 0u;
    out->below = below;
    out->streak = streak;
    out->lost = streak >= lost_after ? 1u : 0u;
    out->calls = out->calls + 1u;
  }
}

void pftk_match(hipStream_t s, const PftParams& p, const PftDev& d, double min_ratio, uint32_t lost_after,
                pft_match_stats* out, int32_t* input_idx, float* sq_dist) {
  hipLaunchKernelGGL(k_match, dim3(1), dim3(MT_THREADS), 0, s, p, d, min_ratio, lost_after, out, input_idx, sq_dist);
}

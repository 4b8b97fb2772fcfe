// pft_match.hip -- match statistics of the result pose (pft_match): how much of the reference
// cloud, moved by the frame's result, finds a partner in the frame -- taken in the search the likelihood itself uses --
// and the lost-object rule on top of it.  One launch on the handle's stream after pft_compute, in the pattern of
// k_report: it reads PftHeader::rep on the device, so nothing synchronises.
//
//   T        pose_to_matrix(PftHeader::rep) (double sin / cos rounded to float; no -5 mm offset: that one is drawResult's)
//   q        ((T0 x + T1 y) + T2 z) + T3 per row of every reference point, the likelihood kernel's xform
//   (pos, d2) OctreePointCloudSearch::approxNearestSearch of q in the tree the frame's last iteration built: at every
//            level the existing child whose voxel centre (float)((k + 0.5) res 2^(D-l) + min) is closest (float x2 + (y2 +
//            z2), strict < in ascending child order), then the leaf's points in insertion order, first strictly smaller
//            wins -- level by level as the CPU restatement under oracle/ walks it
//   matched  (double)d2 < max_distance^2, the likelihood's gate
//   pair     DistanceCoherence x HSVColorCoherence of (q, partner), restated from pft_likelihood.hip (A7) with the two
//            divisions PCL makes instead of that kernel's one reciprocal of the product: this is not the hot loop
//
// The tree is read where the builder left it (words, leaf records through L2): no LDS staging, no centre tables, no
// jump or ancestor table -- M is a downsampled model of a few thousand points, one descent each.
//
// Sums: n_matched is an integer; coherence and sum_sq_dist are adjacent-pair trees in double over the stored (Morton)
// positions 0 .. M-1 padded with +0.0 to a power of two (every term is >= +0.0, so the padding adds nothing): a lane's
// one position, the wave (xor 1 .. 32), the 16 waves (LDS), then the 1024-position tiles (a binary counter in LDS).
// Every level is a subtree of the one tree, so the bits do not depend on the launch shape.
#include "pft_device_utils.h"
#include "pft_match_search.h"

#define MT_THREADS 1024
#define MT_WAVES (MT_THREADS / 64)
#define MT_MAX_LEVELS 32

struct MtSh {
  float T[12];
  double part[MT_WAVES][2];
  double stk[MT_MAX_LEVELS][2];
  uint32_t n_matched;
  int run;
};

__global__ void __launch_bounds__(MT_THREADS) k_match(PftParams prm, PftDev d, double min_ratio, uint32_t lost_after,
                                                      pft_match_stats* __restrict__ out,
                                                      int32_t* __restrict__ input_idx, float* __restrict__ sq_dist) {
  __shared__ MtSh sh;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
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
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = sh.T[k];

  const uint32_t M = prm.M;
  const int D = hdr->depth;
  const uint32_t n_words = hdr->n_words;
  const uint32_t n_pts = hdr->n_crop;
  // an empty crop (or a tree that was never built) is evaluated: nothing matches
  const uint32_t n_crop = (D <= 0 || D > PFT_MAX_DEPTH || n_words == 0u || n_words > d.max_words) ? 0u : n_pts;
  const bool indirect = hdr->leaf_indirect != 0;
  const double omin[3] = {hdr->omin[0], hdr->omin[1], hdr->omin[2]};
  const double res = prm.res, maxd2 = prm.maxd2;

  uint32_t my_matched = 0u;
  const uint32_t n_tiles = (M + MT_THREADS - 1u) / MT_THREADS;
  for (uint32_t tile = 0; tile < n_tiles; tile++) {
    const uint32_t j = tile * MT_THREADS + tid;
    double v_coh = 0.0, v_d2 = 0.0;
    if (j < M) {
      const float4 r = d.ref_xyz[j];
      float qx, qy, qz;
      xform(T, r.x, r.y, r.z, qx, qy, qz);
      float bd = INFINITY;
      uint32_t bcrop = 0xffffffffu;  // the partner's position in the cropped cloud
      float4 bt = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (n_crop != 0u) {
        uint32_t node = 0u, kx = 0u, ky = 0u, kz = 0u;
        bool ok = true;
        for (int lvl = 0; lvl < D; lvl++) {
          const uint32_t wv = d.words[node];
          const uint32_t mask = wv & 0xffu, base = wv >> 8;
          const double vs = res * (double)(1u << (D - lvl - 1));
          const uint32_t bc = mt_min_child(mask, vs, omin, kx, ky, kz, qx, qy, qz);
          node = base + __popc(mask & ((1u << (bc & 7u)) - 1u));
          // (a node without children, or a child index past the words: not a tree the builders write -- no partner
          // instead of a read out of bounds)
          ok = ok && bc != 0xffu && node + 1u < n_words;
          if (!ok) break;
          // U10 (switch point -- the third place that carries it, after the likelihood kernel and the
          // CPU restatement under oracle/): the key handed down is the chosen (minimum) child's, PCL's `minChildKey`;
          // the upstream variant that handed down `new_key` -- the last existing child iterated -- would take the bits of
          // 31 - clz(mask) here instead of bc
          kx = 2u * kx + ((bc >> 2) & 1u);
          ky = 2u * ky + ((bc >> 1) & 1u);
          kz = 2u * kz + (bc & 1u);
        }
        if (ok) {
          const uint32_t ls = d.words[node], le = min(d.words[node + 1u], n_crop);
          // leaf scan in float: the first strictly smaller candidate wins (insertion order)
          for (uint32_t pos = ls; pos < le; pos++) {
            const uint32_t ci = min(d.leaf_order[pos], n_crop - 1u);
            const float4 c = indirect ? d.crop_pts[ci] : d.leaf_pts[pos];
            const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
            const float dd = dx * dx + (dy * dy + dz * dz);
            if (dd < bd) {
              bd = dd;
              bcrop = ci;
              bt = c;
            }
          }
        }
      }
      const bool matched = bcrop != 0xffffffffu && (double)bd < maxd2;
      if (matched) {
        v_coh = mt_pair_value(prm, qx, qy, qz, bt, d.ref_hsv[j]);
        v_d2 = (double)bd;
        my_matched++;
      }
      const uint32_t o = d.ref_perm[j];  // the caller's order, as pft_eval_weights reports its pairs
      input_idx[o] = matched ? d.crop_idx[bcrop] : -1;
      sq_dist[o] = bd;
    }
    // lanes 2i and 2i+1 hold the two halves; both form left + right (addition commutes bit for bit)
    for (int o = 1; o < 64; o <<= 1) {
      v_coh = v_coh + __shfl_xor(v_coh, o);
      v_d2 = v_d2 + __shfl_xor(v_d2, o);
    }
    if (lane == 0) {
      sh.part[wave][0] = v_coh;
      sh.part[wave][1] = v_d2;
    }
    __syncthreads();
    if (tid < 2u) {
      double w[MT_WAVES];
#pragma unroll
      for (int q = 0; q < MT_WAVES; q++) w[q] = sh.part[q][tid];
#pragma unroll
      for (int h = MT_WAVES / 2; h >= 1; h >>= 1)
#pragma unroll
        for (int q = 0; q < h; q++) w[q] = w[2 * q] + w[2 * q + 1];
      // tiles: binary counter (tile t merges the pending subtrees its trailing one bits name)
      double v = w[0];
      uint32_t l = 0;
      for (uint32_t b = tile; b & 1u; b >>= 1, l++) v = sh.stk[l][tid] + v;
      sh.stk[l][tid] = v;
    }
    __syncthreads();
  }
  my_matched = wave_sum(my_matched);
  if (lane == 0 && my_matched) atomicAdd(&sh.n_matched, my_matched);
  if (tid < 2u) {
    // the pending subtrees, from the smallest (rightmost) up: the padding adds +0.0 to sums that are >= +0.0, so the
    // padded tree's root is the right-to-left fold of what the counter holds
    double v = 0.0;
    bool any = false;
    for (uint32_t l = 0; l < MT_MAX_LEVELS; l++)
      if ((n_tiles >> l) & 1u) {
        v = any ? sh.stk[l][tid] + v : sh.stk[l][tid];
        any = true;
      }
    sh.part[0][tid] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t nm = sh.n_matched;
    for (int k = 0; k < 12; k++) out->transform[k] = T[k];
    out->coherence = sh.part[0][0];
    out->sum_sq_dist = sh.part[0][1];
    out->n_reference = M;
    out->n_matched = nm;
    out->n_crop = n_pts;
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

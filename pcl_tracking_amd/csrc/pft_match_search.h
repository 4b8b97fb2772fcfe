// pft_match_search.h -- the result-pose search of pft_match.hip (k_match), pft_reacquire.hip (k_reacquire_score) and
// pft_refine.hip (k_refine_pairs), DESIGN.md section 3.10: the view of the frame's tree, the choice among the existing
// children of one octree level, the descent with the leaf scan, and the value of a matched pair.  The tree is read where
// the builder left it (words and leaf records through L2): no LDS staging, no centre tables, no jump or ancestor table --
// the queries are a downsampled model of a few thousand points, one descent each.
#pragma once
#include "pft_device_utils.h"

// the eight child-centre distances of one level and the choice among the existing children; centres in double as
// genVoxelCenterFromOctreeKey forms them (key k of the PARENT at level lvl: the children are 2k and 2k + 1 per axis)
__device__ __forceinline__ uint32_t mt_min_child(uint32_t mask, double vs, const double omin[3], uint32_t kx, uint32_t ky,
                                                 uint32_t kz, float qx, float qy, float qz) {
  const float cx0 = (float)(((double)(2u * kx) + 0.5) * vs + omin[0]), cx1 = (float)(((double)(2u * kx + 1u) + 0.5) * vs + omin[0]);
  const float cy0 = (float)(((double)(2u * ky) + 0.5) * vs + omin[1]), cy1 = (float)(((double)(2u * ky + 1u) + 0.5) * vs + omin[1]);
  const float cz0 = (float)(((double)(2u * kz) + 0.5) * vs + omin[2]), cz1 = (float)(((double)(2u * kz + 1u) + 0.5) * vs + omin[2]);
  // pointSquaredDist: Vector3f difference, squaredNorm = x2 + (y2 + z2), unfused
  const float dx0 = cx0 - qx, dx1 = cx1 - qx, dy0 = cy0 - qy, dy1 = cy1 - qy, dz0 = cz0 - qz, dz1 = cz1 - qz;
  const float X0 = dx0 * dx0, X1 = dx1 * dx1, Y0 = dy0 * dy0, Y1 = dy1 * dy1, Z0 = dz0 * dz0, Z1 = dz1 * dz1;
  float best = INFINITY;
  uint32_t bc = 0xffu;
#pragma unroll
  for (uint32_t c = 0; c < 8u; c++) {
    const float dc = ((c & 4u) ? X1 : X0) + (((c & 2u) ? Y1 : Y0) + ((c & 1u) ? Z1 : Z0));
    const bool ex = (mask >> c) & 1u;
    // "if (dist >= min) continue" from DBL_MAX: the first existing child is taken whatever its distance (a NaN query
    // keeps it), later ones only when strictly smaller
    if (ex && (bc == 0xffu || dc < best)) {
      best = dc;
      bc = c;
    }
  }
  return bc;
}

// the tree the handle's last crop and build left, as the search reads it
struct MtTree {
  int D;
  uint32_t n_words, n_crop;  // n_crop == 0: the tree must not be read, nothing finds a partner
  bool indirect;             // the leaf records are followed through leaf_order into the crop
  double omin[3], res;
};

// the one gate on the tree: a failed crop or build (PftHeader::error), an empty crop, or a tree that was never built or
// does not fit the words the search may read
__device__ __forceinline__ MtTree mt_load_tree(const PftHeader* hdr, const PftDev& d, const PftParams& prm) {
  MtTree t;
  t.D = hdr->depth;
  t.n_words = hdr->n_words;
  const bool usable = hdr->error == 0u && t.D > 0 && t.D <= PFT_MAX_DEPTH && t.n_words != 0u && t.n_words <= d.max_words;
  t.n_crop = usable ? hdr->n_crop : 0u;
  t.indirect = hdr->leaf_indirect != 0;
  for (int a = 0; a < 3; a++) t.omin[a] = hdr->omin[a];
  t.res = prm.res;
  return t;
}

// OctreePointCloudSearch::approxNearestSearch of q: at every level the existing child whose voxel centre is closest, then
// the leaf's points in insertion order.  Returns whether q has a partner; bd = its float d2 (INFINITY without one), bt its
// record, pos its position among the leaf records (the crop index is min(d.leaf_order[pos], n_crop - 1))
__device__ __forceinline__ bool mt_search(const MtTree& t, const PftDev& d, float qx, float qy, float qz, float& bd,
                                          float4& bt, uint32_t& pos) {
  bd = INFINITY;
  bt = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  pos = 0xffffffffu;
  if (t.n_crop == 0u) return false;
  const int D = t.D;
  uint32_t node = 0u, kx = 0u, ky = 0u, kz = 0u;
  bool ok = true;
  for (int lvl = 0; lvl < D; lvl++) {
    const uint32_t wv = d.words[node];
    const uint32_t mask = wv & 0xffu, base = wv >> 8;
    const double vs = t.res * (double)(1u << (D - lvl - 1));
    const uint32_t bc = mt_min_child(mask, vs, t.omin, kx, ky, kz, qx, qy, qz);
    node = base + __popc(mask & ((1u << (bc & 7u)) - 1u));
    // (a node without children, or a child index past the words: not a tree the builders write -- no partner instead of
    // a read out of bounds)
    ok = ok && bc != 0xffu && node + 1u < t.n_words;
    if (!ok) break;
    // U10 (switch point -- carried here, in the likelihood kernel and in the CPU restatement under
    // oracle/): the key handed down is the chosen (minimum) child's, PCL's `minChildKey`; the upstream variant that
    // handed down `new_key` -- the last existing child iterated -- would take the bits of 31 - clz(mask) here instead of bc
    kx = 2u * kx + ((bc >> 2) & 1u);
    ky = 2u * ky + ((bc >> 1) & 1u);
    kz = 2u * kz + (bc & 1u);
  }
  if (!ok) return false;
  const uint32_t ls = d.words[node], le = min(d.words[node + 1u], t.n_crop);
  // leaf scan in float: the first strictly smaller candidate wins (insertion order)
  for (uint32_t p = ls; p < le; p++) {
    float4 c;
    if (t.indirect)
      c = d.crop_pts[min(d.leaf_order[p], t.n_crop - 1u)];
    else
      c = d.leaf_pts[p];
    const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
    const float dd = dx * dx + (dy * dy + dz * dz);
    if (dd < bd) {
      bd = dd;
      bt = c;
      pos = p;
    }
  }
  return pos != 0xffffffffu;
}

// DistanceCoherence x HSVColorCoherence of the pair (restated from pft_likelihood.hip, A7; PCL's two double divisions)
__device__ __forceinline__ double mt_pair_value(const PftParams& prm, float qx, float qy, float qz, const float4 bt,
                                                const float4 rh) {
  const float ex = qx - bt.x, ey = qy - bt.y, ez = qz - bt.z;
  const float n2 = (ex * ex + ey * ey) + ez * ez;  // Vector4f norm, (dx2 + dy2) + (dz2 + 0)
  const double dist = (double)(float)sqrt((double)n2);  // == sqrtf, correctly rounded (53 >= 2 * 24 + 2 bits)
  const double dc = 1.0 / (1.0 + dist * dist * prm.dist_w);
  const uint32_t pk = __float_as_uint(bt.w);
  const float th = (float)(pk & 0xffu) / 180.0f, ts = (float)((pk >> 8) & 0xffu) / 255.0f,
              tv = (float)((pk >> 16) & 0xffu) / 255.0f;
  const float hd1 = fabsf(rh.x - th);
  float hd2;
  if (rh.x < th)
    hd2 = fabsf(1.0f + rh.x - th);
  else
    hd2 = fabsf(1.0f + th - rh.x);
  float h_diff;
  if (hd1 < hd2)
    h_diff = prm.h_w * hd1 * hd1;
  else
    h_diff = prm.h_w * hd2 * hd2;
  const float s_diff = prm.s_w * (rh.y - ts) * (rh.y - ts);
  const float v_diff = prm.v_w * (rh.z - tv) * (rh.z - tv);
  const float diff2 = h_diff + s_diff + v_diff;
  const double hc = 1.0 / (1.0 + prm.hsv_w * (double)diff2);
  return dc * hc;
}

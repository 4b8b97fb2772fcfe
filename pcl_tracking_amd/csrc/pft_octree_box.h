// pft_octree_box.h -- OctreePointCloud::adoptBoundingBoxToPoint / getKeyBitSize (PCL 1.8.0): the builder's shared state
// and its box routines, included by the per-iteration builder (pft_octree.hip, where they were defined) and by the change
// detector (pft_change.hip).  Device code only: each translation unit is its own device module.
#pragma once
#include <float.h>

#include "pft_internal.h"

struct BuildSh {
  double mn[3], mx[3];
  int depth, ngrow;
  uint32_t cur, err;
  uint32_t variant;  // k_octree_build: bits 0-5 of PftHeader::build_variant, left by the instance that built the tree
  int jump;
  uint32_t u32s[40];
  uint32_t gidx[PFT_MAX_GROW], gshift[PFT_MAX_GROW], gold[PFT_MAX_GROW];
  double gmin[PFT_MAX_GROW + 1][3];
  uint32_t lvl[PFT_MAX_DEPTH + 3];
  // dense top levels (build_tree): per level <= J the occupancy bits in Morton order, their popcount prefix, node counts
  uint32_t dn_bits[PFT_JUMP_MAX_LEVEL + 1][128], dn_pref[PFT_JUMP_MAX_LEVEL + 1][128], dn_cnt[PFT_JUMP_MAX_LEVEL + 1];
};

// first point: box = p +- res/2, then getKeyBitSize() pads it to depth 1 (side 2*res - eps)
__device__ void box_init(BuildSh& S, float4 p0, double res) {
  const double epsd = (double)FLT_EPSILON;
  double lo[3] = {(double)p0.x - res / 2, (double)p0.y - res / 2, (double)p0.z - res / 2};
  double hi[3] = {(double)p0.x + res / 2, (double)p0.y + res / 2, (double)p0.z + res / 2};
  unsigned mk = 0;
  for (int a = 0; a < 3; a++) {
    unsigned k = (unsigned)((hi[a] - lo[a]) / res);
    mk = k > mk ? k : mk;
  }
  unsigned mv = mk > 2u ? mk : 2u;
  // getKeyBitSize: ceil(log2(max key) - eps), at least... mv is 2 for the one-point box (log(2)/log(2) == 1.0 exactly):
  // the two double logarithms are only evaluated in the general case
  double l2 = mv == 2u ? 1.0 : log((double)mv) / log(2.0);
  unsigned dep = (unsigned)ceil(l2 - (double)FLT_EPSILON);
  if (dep > 32u) dep = 32u;
  double side = (double)(1u << dep) * res - epsd;
  for (int a = 0; a < 3; a++) {
    double over = (side - (hi[a] - lo[a])) / 2.0;
    S.mn[a] = lo[a] - over;
    S.mx[a] = hi[a] + over;
    S.gmin[0][a] = S.mn[a];
  }
  S.depth = (int)dep;
}

// adoptBoundingBoxToPoint for one violating point: new root above the old one until the point fits;
// axes without an upper violation extend downwards
__device__ void box_grow(BuildSh& S, float4 p, uint32_t idx, double res) {
  const double epsd = (double)FLT_EPSILON;
  for (;;) {
    bool lx = p.x < S.mn[0], ly = p.y < S.mn[1], lz = p.z < S.mn[2];
    bool ux = p.x >= S.mx[0], uy = p.y >= S.mx[1], uz = p.z >= S.mx[2];
    if (!(lx || ly || lz || ux || uy || uz)) break;
    int g = S.ngrow;
    if (g >= PFT_MAX_GROW || S.depth >= PFT_MAX_DEPTH) {
      S.err |= 2u;
      break;
    }
    double side = (double)(1u << S.depth) * res;
    S.gidx[g] = idx;
    S.gshift[g] = (ux ? 0u : 1u) | (uy ? 0u : 2u) | (uz ? 0u : 4u);
    S.gold[g] = (uint32_t)S.depth;
    if (!ux) S.mn[0] -= side;
    if (!uy) S.mn[1] -= side;
    if (!uz) S.mn[2] -= side;
    S.depth = S.depth + 1;
    side = (double)(1u << S.depth) * res - epsd;
    S.mx[0] = S.mn[0] + side;
    S.mx[1] = S.mn[1] + side;
    S.mx[2] = S.mn[2] + side;
    S.gmin[g + 1][0] = S.mn[0];
    S.gmin[g + 1][1] = S.mn[1];
    S.gmin[g + 1][2] = S.mn[2];
    S.ngrow = g + 1;
  }
}

__device__ __forceinline__ bool box_violates(float x, float y, float z, const double* mn, const double* mx) {
  return (x < mn[0]) || (y < mn[1]) || (z < mn[2]) || (x >= mx[0]) || (y >= mx[1]) || (z >= mx[2]);
}

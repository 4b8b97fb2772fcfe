// pft_match_search.h -- the pieces of the result-pose search that pft_match.hip (k_match) and pft_reacquire.hip
// (k_reacquire_score) share: the choice among the existing children of one octree level and the value of a matched pair.
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

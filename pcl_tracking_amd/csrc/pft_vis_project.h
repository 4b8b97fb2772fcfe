// pft_vis_project.h -- the camera arithmetic of include/pft_visibility.h, shared by pft_visibility.hip and pft_view.hip:
// the projection (host and device, also behind pft_visibility_project) and the footprint's atomicMin splat.
#pragma once
#include "pft_device_utils.h"

#define VS_INF_BITS 0x7f800000u
#define VS_NO_PIXEL 0xffffffffu

__host__ __device__ __forceinline__ bool vis_project(const PftVisCam& c, float x, float y, float z, int& u, int& v) {
  const bool front = z > c.z_near;
  const float xn = x / z, yn = y / z;
  const float uf = c.fx * xn + c.cx, vf = c.fy * yn + c.cy;
  const bool in_view = front && uf >= 0.0f && uf < (float)c.W && vf >= 0.0f && vf < (float)c.H;
  if (!in_view) return false;
  u = (int)floorf(uf);
  v = (int)floorf(vf);
  return true;
}

// min over the pixels [ua, ub] x [va, vb] (inside the image) of the image with zb
__device__ __forceinline__ void vis_splat(uint32_t* __restrict__ img, int W, int ua, int ub, int va, int vb, uint32_t zb) {
  for (int y = va; y <= vb; y++) {
    uint32_t* row = img + (size_t)y * (size_t)W;
    for (int x = ua; x <= ub; x++)
      if (row[x] > zb) atomicMin(row + x, zb);  // (values only fall during a call: a stale read costs one atomic, no more)
  }
}

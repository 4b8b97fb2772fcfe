// pft_segment_solve.h -- the one-lane tail of the plane refit (pft_segment.hip "RULE eigen" / "RULE refit", DESIGN.md
// section 3.7): from the nine means of optimizeModelCoefficients to the four coefficients.  pcl::computeRoots /
// computeRoots2 / eigen33 (the smallest eigenvalue's vector) in float, unfused, in PCL's source order, mirrored line for
// line by tests/segment_model.py (`_roots2`, `_roots`, `eigen33_trace`, `refit_trace`).  Host and device: k_sg_refit and
// k_sg_refit_top run it in one lane, tests/cpp/segment_solve_tool.cpp runs it on the CPU.  Built with -ffp-contract=off
// like the library.  Besides + - * / and sqrtf it calls atan2f, cosf and sinf once each: those three values are the only
// ones that differ between a device, a host libm and NumPy, so the record keeps them with their arguments.
//
// Every solve fills a pft_segment_refit_debug (include/pft_segment.h): what it read, what it computed, the branches it
// took.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pft_segment.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define PFT_SG_HD __host__ __device__
#else
#define PFT_SG_HD
#endif

PFT_SG_HD inline void sg_roots2(float b, float c, float* r, pft_segment_refit_debug* rec) {
  r[0] = 0.0f;
  float d = (float)((double)(b * b) - 4.0 * (double)c);
  if (d < 0.0f) {
    d = 0.0f;
    rec->branches |= PFT_REFIT_D_NEGATIVE;
  }
  const float sd = sqrtf(d);
  r[2] = 0.5f * (b + sd);
  r[1] = 0.5f * (b - sd);
}

PFT_SG_HD inline void sg_roots(const float* m, float* r, pft_segment_refit_debug* rec) {  // m row-major 3x3
  const float m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[4], m12 = m[5], m22 = m[8];
  const float c0 = m00 * m11 * m22 + 2.0f * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
  const float c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
  const float c2 = m00 + m11 + m22;
  if (fabsf(c0) < FLT_EPSILON) {
    rec->branches |= PFT_REFIT_C0_SMALL;
    sg_roots2(c2, c1, r, rec);
    return;
  }
  const float s_inv3 = (float)(1.0 / 3.0);
  const float s_sqrt3 = sqrtf(3.0f);
  const float c2_over_3 = c2 * s_inv3;
  float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.0f) {
    a_over_3 = 0.0f;
    rec->branches |= PFT_REFIT_A_CLAMPED;
  }
  const float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
  float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.0f) {
    q = 0.0f;
    rec->branches |= PFT_REFIT_Q_CLAMPED;
  }
  const float rho = sqrtf(-a_over_3);
  const float ay = sqrtf(-q);
  const float at = atan2f(ay, half_b);
  const float theta = at * s_inv3;
  const float ct = cosf(theta), st = sinf(theta);
  rec->trig_arg[0] = ay;
  rec->trig_arg[1] = half_b;
  rec->trig_arg[2] = theta;
  rec->trig[0] = at;
  rec->trig[1] = ct;
  rec->trig[2] = st;
  r[0] = c2_over_3 + 2.0f * rho * ct;
  r[1] = c2_over_3 - rho * (ct + s_sqrt3 * st);
  r[2] = c2_over_3 - rho * (ct - s_sqrt3 * st);
  float t;
  if (r[0] >= r[1]) {
    t = r[0]; r[0] = r[1]; r[1] = t;
    rec->branches |= PFT_REFIT_SWAP_01;
  }
  if (r[1] >= r[2]) {
    t = r[1]; r[1] = r[2]; r[2] = t;
    rec->branches |= PFT_REFIT_SWAP_12;
    if (r[0] >= r[1]) {
      t = r[0]; r[0] = r[1]; r[1] = t;
      rec->branches |= PFT_REFIT_SWAP_01_AGAIN;
    }
  }
  if (r[0] <= 0.0f) {
    rec->branches |= PFT_REFIT_R0_FALLBACK;
    sg_roots2(c2, c1, r, rec);
  }
}

PFT_SG_HD inline void sg_eigen33(const float* mat, float* vec, pft_segment_refit_debug* rec) {
  float scale = 0.0f;
  for (int k = 0; k < 9; k++) scale = fmaxf(scale, fabsf(mat[k]));
  if (scale <= FLT_MIN) {
    scale = 1.0f;
    rec->branches |= PFT_REFIT_SCALE_TINY;
  }
  rec->scale = scale;
  float m[9];
  for (int k = 0; k < 9; k++) m[k] = mat[k] / scale;
  float r[3];
  sg_roots(m, r, rec);
  for (int k = 0; k < 3; k++) rec->roots[k] = r[k];
  m[0] -= r[0];
  m[4] -= r[0];
  m[8] -= r[0];
  float v[3][3];
  const int ra[3] = {0, 0, 1}, rb[3] = {1, 2, 2};
  float len[3];
  for (int k = 0; k < 3; k++) {
    const float* a = m + 3 * ra[k];
    const float* b = m + 3 * rb[k];
    v[k][0] = a[1] * b[2] - a[2] * b[1];
    v[k][1] = a[2] * b[0] - a[0] * b[2];
    v[k][2] = a[0] * b[1] - a[1] * b[0];
    len[k] = v[k][0] * v[k][0] + (v[k][1] * v[k][1] + v[k][2] * v[k][2]);  // Vector3f::squaredNorm
    rec->len[k] = len[k];
  }
  int pick = 2;
  if (len[0] >= len[1] && len[0] >= len[2]) pick = 0;
  else if (len[1] >= len[0] && len[1] >= len[2]) pick = 1;
  rec->branches |= pick == 0 ? PFT_REFIT_PICK_0 : (pick == 1 ? PFT_REFIT_PICK_1 : PFT_REFIT_PICK_2);
  if (len[pick] == 0.0f) rec->branches |= PFT_REFIT_ZERO_LENGTH;
  const float s = sqrtf(len[pick]);
  vec[0] = v[pick][0] / s;
  vec[1] = v[pick][1] / s;
  vec[2] = v[pick][2] / s;
}

// the refit after the sums: accu = the nine sums divided by the count m.  Writes the record (coef[4] included).
PFT_SG_HD inline void sg_refit_solve(const float* accu, uint32_t m, pft_segment_refit_debug* rec) {
  rec->m = m;
  rec->branches = 0u;
  for (int k = 0; k < 9; k++) rec->accu[k] = accu[k];
  for (int k = 0; k < 3; k++) rec->trig_arg[k] = rec->trig[k] = 0.0f;
  float cov[9];
  cov[0] = accu[0] - accu[6] * accu[6];
  cov[1] = accu[1] - accu[6] * accu[7];
  cov[2] = accu[2] - accu[6] * accu[8];
  cov[4] = accu[3] - accu[7] * accu[7];
  cov[5] = accu[4] - accu[7] * accu[8];
  cov[8] = accu[5] - accu[8] * accu[8];
  cov[3] = cov[1];
  cov[6] = cov[2];
  cov[7] = cov[5];
  rec->cov[0] = cov[0];
  rec->cov[1] = cov[1];
  rec->cov[2] = cov[2];
  rec->cov[3] = cov[4];
  rec->cov[4] = cov[5];
  rec->cov[5] = cov[8];
  float e[3];
  sg_eigen33(cov, e, rec);
  const float dot = (e[0] * accu[6] + e[1] * accu[7]) + (e[2] * accu[8] + 0.0f * 1.0f);
  rec->coef[0] = e[0];
  rec->coef[1] = e[1];
  rec->coef[2] = e[2];
  rec->coef[3] = -1.0f * dot;
}

// pft_report_solve.h -- the one-lane part of the object report (pft_report.hip): SelfAdjointEigenSolver<Matrix3f>,
// the cross product and Quaternion(Matrix3), as plain scalar float code.  Host and device: k_report runs it in one lane,
// tools/report_host_bench.cpp times it on the CPU.  Built with -ffp-contract=off like the library.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define PFT_HD __host__ __device__
#else
#define PFT_HD
#endif

// ---- the one-lane part: SelfAdjointEigenSolver<Matrix3f>::compute (Eigen 3.3) + the cross product; tests/report_model.py
// `solve` line for line ----
PFT_HD inline float rp_hypot(float x, float y) {  // numext::hypot
  const float ax = fabsf(x), ay = fabsf(y);
  const float p = ax > ay ? ax : ay, o = ax > ay ? ay : ax;
  if (p == 0.0f) return 0.0f;
  const float qp = o / p;
  return p * sqrtf(1.0f + qp * qp);
}
PFT_HD inline void rp_make_givens(float p, float q, float& c, float& s) {  // JacobiRotation::makeGivens, real case
  if (q == 0.0f) {
    c = p < 0.0f ? -1.0f : 1.0f;
    s = 0.0f;
  } else if (p == 0.0f) {
    c = 0.0f;
    s = q < 0.0f ? 1.0f : -1.0f;
  } else if (fabsf(p) > fabsf(q)) {
    const float t = q / p;
    float u = sqrtf(1.0f + t * t);
    if (p < 0.0f) u = -u;
    c = 1.0f / u;
    s = -t * c;
  } else {
    const float t = p / q;
    float u = sqrtf(1.0f + t * t);
    if (q < 0.0f) u = -u;
    s = -1.0f / u;
    c = -t * s;
  }
}
// tridiagonal_qr_step with the Wilkinson shift; Q = Q * G (applyOnTheRight(k, k+1, rot))
PFT_HD inline void rp_qr_step(float* diag, float* sub, int start, int end, float (*Q)[3]) {
  const float td = (diag[end - 1] - diag[end]) * 0.5f;
  const float e = sub[end - 1];
  float mu = diag[end];
  if (td == 0.0f) {
    mu = mu - fabsf(e);
  } else {
    const float e2 = e * e;
    const float h = rp_hypot(td, e);
    if (e2 == 0.0f) mu = mu - (e / (td + (td > 0.0f ? 1.0f : -1.0f))) * (e / h);
    else mu = mu - e2 / (td + (td > 0.0f ? h : -h));
  }
  float x = diag[start] - mu;
  float z = sub[start];
  for (int k = start; k < end; k++) {
    float c, s;
    rp_make_givens(x, z, c, s);
    const float sdk = s * diag[k] + c * sub[k];
    const float dkp1 = s * sub[k] + c * diag[k + 1];
    diag[k] = c * (c * diag[k] - s * sub[k]) - s * (c * sub[k] - s * diag[k + 1]);
    diag[k + 1] = s * sdk + c * dkp1;
    sub[k] = c * sdk - s * dkp1;
    if (k > start) sub[k - 1] = c * sub[k - 1] - s * z;
    x = sub[k];
    if (k < end - 1) {
      z = -s * sub[k + 1];
      sub[k + 1] = c * sub[k + 1];
    }
    const float ms = -s;  // apply_rotation_in_the_plane(col k, col k+1, rot.transpose())
    for (int i = 0; i < 3; i++) {
      const float xi = Q[i][k], yi = Q[i][k + 1];
      Q[i][k] = c * xi + ms * yi;
      Q[i][k + 1] = -ms * xi + c * yi;
    }
  }
}
// cov [row][col] symmetric -> eigenvalues (ascending), axes [row][col] (col 2 = col 0 x col 1); returns info (1: no
// convergence within 30 n iterations, the values and vectors are then unsorted as Eigen leaves them)
PFT_HD inline uint32_t report_solve(const float (*cov)[3], float* evals, float (*Q)[3]) {
  float m[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c <= r; c++) m[r][c] = cov[r][c];
  float scale = 0.0f;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c <= r; c++) {
      const float a = fabsf(m[r][c]);
      if (a > scale) scale = a;
    }
  if (scale == 0.0f) scale = 1.0f;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c <= r; c++) m[r][c] = m[r][c] / scale;
  // tridiagonalization_inplace, 3x3 closed form
  float diag[3], sub[2];
  diag[0] = m[0][0];
  const float v1norm2 = m[2][0] * m[2][0];
  if (v1norm2 <= FLT_MIN) {
    diag[1] = m[1][1];
    diag[2] = m[2][2];
    sub[0] = m[1][0];
    sub[1] = m[2][1];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) Q[r][c] = r == c ? 1.0f : 0.0f;
  } else {
    const float beta = sqrtf(m[1][0] * m[1][0] + v1norm2);
    const float inv_beta = 1.0f / beta;
    const float m01 = m[1][0] * inv_beta;
    const float m02 = m[2][0] * inv_beta;
    const float q = (2.0f * m01) * m[2][1] + m02 * (m[2][2] - m[1][1]);
    diag[1] = m[1][1] + m02 * q;
    diag[2] = m[2][2] - m02 * q;
    sub[0] = beta;
    sub[1] = m[2][1] - m01 * q;
    Q[0][0] = 1.0f; Q[0][1] = 0.0f; Q[0][2] = 0.0f;
    Q[1][0] = 0.0f; Q[1][1] = m01;  Q[1][2] = m02;
    Q[2][0] = 0.0f; Q[2][1] = m02;  Q[2][2] = -m01;
  }
  // computeFromTridiagonal_impl
  const int n = 3;
  int end = n - 1, start = 0, iter = 0;
  const float precision = 2.0f * FLT_EPSILON;
  while (end > 0) {
    for (int i = start; i < end; i++)
      if (fabsf(sub[i]) <= (fabsf(diag[i]) + fabsf(diag[i + 1])) * precision || fabsf(sub[i]) <= FLT_MIN) sub[i] = 0.0f;
    while (end > 0 && sub[end - 1] == 0.0f) end--;
    if (end <= 0) break;
    iter++;
    if (iter > 30 * n) break;
    start = end - 1;
    while (start > 0 && sub[start - 1] != 0.0f) start--;
    rp_qr_step(diag, sub, start, end, Q);
  }
  const uint32_t info = iter <= 30 * n ? 0u : 1u;
  if (!info)
    for (int i = 0; i < n - 1; i++) {  // first minimum of diag[i ..]; the vector columns follow
      int k = i;
      for (int j = i + 1; j < n; j++)
        if (diag[j] < diag[k]) k = j;
      if (k > i) {
        const float t = diag[i];
        diag[i] = diag[k];
        diag[k] = t;
        for (int r = 0; r < 3; r++) {
          const float u = Q[r][i];
          Q[r][i] = Q[r][k];
          Q[r][k] = u;
        }
      }
    }
  for (int i = 0; i < 3; i++) evals[i] = diag[i] * scale;
  const float a0 = Q[0][0], a1 = Q[1][0], a2 = Q[2][0], b0 = Q[0][1], b1 = Q[1][1], b2 = Q[2][1];
  Q[0][2] = a1 * b2 - a2 * b1;
  Q[1][2] = a2 * b0 - a0 * b2;
  Q[2][2] = a0 * b1 - a1 * b0;
  return info;
}

// Quaternion(Matrix3) assignment (Shoemake): q = {x, y, z, w}
PFT_HD inline void rp_quaternion(const float (*m)[3], float* q) {
  float t = m[0][0] + (m[1][1] + m[2][2]);
  if (t > 0.0f) {
    t = sqrtf(t + 1.0f);
    q[3] = 0.5f * t;
    t = 0.5f / t;
    q[0] = (m[2][1] - m[1][2]) * t;
    q[1] = (m[0][2] - m[2][0]) * t;
    q[2] = (m[1][0] - m[0][1]) * t;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrtf(((m[i][i] - m[j][j]) - m[k][k]) + 1.0f);
    q[i] = 0.5f * t;
    t = 0.5f / t;
    q[3] = (m[k][j] - m[j][k]) * t;
    q[j] = (m[j][i] + m[i][j]) * t;
    q[k] = (m[k][i] + m[i][k]) * t;
  }
}


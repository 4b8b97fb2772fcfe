// pft_refine_solve.h -- the one-lane part of the pose refinement (pft_refine.hip): from the pair
// moments of one iteration to the next state.  Horn's closed form: the rotation that best maps the centred a onto the
// centred b is the eigenvector of the largest eigenvalue of a symmetric 4x4 matrix, found here by cyclic Jacobi sweeps.
// Plain double arithmetic (+ - x / and a correctly rounded sqrt only), unfused, left to right.  Host and device:
// k_refine_step runs it in one lane, tests/cpp/refine_solve_tool.cpp runs it on the CPU against tests/refine_model.py
// (`solve`, `rotation`, `quat_from_matrix` line for line).  Built with -ffp-contract=off like the library.
//
// Quaternions are {w, x, y, z} throughout.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define PFT_RF_HD __host__ __device__
#else
#define PFT_RF_HD
#endif

#define PFT_REFINE_SUMS 17          // A[3], B[3], H[9] (row by row: a_r b_c), sum_sq_dist, inlier_sq_dist
#define PFT_REFINE_JACOBI_SWEEPS 16  // sweep cap: the off-diagonals of a 4x4 in double reach exact zeros in about ten

struct PftRefineState {
  double Q[4];  // unit quaternion {w, x, y, z}
  double t[3];
};

PFT_RF_HD inline void refine_normalise(double* q) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; k++) q[k] = q[k] / n;
}

// R(Q), row-major 3x3
PFT_RF_HD inline void refine_rotation(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z);
  R[1] = 2.0 * (x * y - w * z);
  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);
  R[4] = 1.0 - 2.0 * (x * x + z * z);
  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);
  R[7] = 2.0 * (y * z + w * x);
  R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// the float transform of a state: T = ((float)R(Q), (float)t), row-major 3x4
PFT_RF_HD inline void refine_transform(const PftRefineState* s, float* T) {
  double R[9];
  refine_rotation(s->Q, R);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
    T[4 * r + 3] = (float)s->t[r];
  }
}

// the branch of Shoemake's method for the largest diagonal entry I (constant indices: no indexed private array on the device)
template <int I>
PFT_RF_HD inline void refine_shoemake(const double (*m)[3], double* q) {
  const int J = (I + 1) % 3, K = (J + 1) % 3;
  double tr = sqrt(((m[I][I] - m[J][J]) - m[K][K]) + 1.0);
  q[1 + I] = 0.5 * tr;
  tr = 0.5 / tr;
  q[0] = (m[K][J] - m[J][K]) * tr;
  q[1 + J] = (m[J][I] + m[I][J]) * tr;
  q[1 + K] = (m[K][I] + m[I][K]) * tr;
}

// the state of a row-major 3x4 float matrix: the Shoemake branches of rp_quaternion in double, normalised; t = its last column
PFT_RF_HD inline void refine_state_from_matrix(const float* T, PftRefineState* s) {
  double m[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) m[r][c] = (double)T[4 * r + c];
  double* q = s->Q;
  double tr = m[0][0] + (m[1][1] + m[2][2]);
  if (tr > 0.0) {
    tr = sqrt(tr + 1.0);
    q[0] = 0.5 * tr;
    tr = 0.5 / tr;
    q[1] = (m[2][1] - m[1][2]) * tr;
    q[2] = (m[0][2] - m[2][0]) * tr;
    q[3] = (m[1][0] - m[0][1]) * tr;
  } else if (!(m[1][1] > m[0][0]) && !(m[2][2] > m[0][0])) {
    refine_shoemake<0>(m, q);
  } else if (m[1][1] > m[0][0] && !(m[2][2] > m[1][1])) {
    refine_shoemake<1>(m, q);
  } else {
    refine_shoemake<2>(m, q);
  }
  refine_normalise(q);
  for (int r = 0; r < 3; r++) s->t[r] = (double)T[4 * r + 3];
}

// One solve.  sums: the 17 tree sums of the iteration (only A, B, H are read), n = n_pairs (>= 1), pivot c = the three
// doubles the terms were centred on.  Updates *s unless the step is exactly zero (dq the identity and t_new == c): a zero
// step leaves the state, and so the float transform, as it is.  dq receives the rotation step, step2 = {step_t2, step_r2}.
// Returns the Jacobi sweeps taken.
PFT_RF_HD inline uint32_t refine_solve(const double* sums, uint32_t n, const double* c, PftRefineState* s, double* dq,
                                    double* step2) {
  const double dn = (double)n;
  double am[3], bm[3], S[3][3];
  for (int r = 0; r < 3; r++) {
    am[r] = sums[r] / dn;
    bm[r] = sums[3 + r] / dn;
  }
  double scale = 0.0;
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) {
      S[r][k] = sums[6 + 3 * r + k] - sums[r] * sums[3 + k] / dn;
      const double a = fabs(S[r][k]);
      if (a > scale) scale = a;
    }
  if (scale == 0.0) scale = 1.0;
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) S[r][k] = S[r][k] / scale;
  // Horn's matrix
  double N[4][4];
  N[0][0] = S[0][0] + S[1][1] + S[2][2];
  N[1][1] = S[0][0] - S[1][1] - S[2][2];
  N[2][2] = -S[0][0] + S[1][1] - S[2][2];
  N[3][3] = -S[0][0] - S[1][1] + S[2][2];
  N[0][1] = N[1][0] = S[1][2] - S[2][1];
  N[0][2] = N[2][0] = S[2][0] - S[0][2];
  N[0][3] = N[3][0] = S[0][1] - S[1][0];
  N[1][2] = N[2][1] = S[0][1] + S[1][0];
  N[1][3] = N[3][1] = S[2][0] + S[0][2];
  N[2][3] = N[3][2] = S[1][2] + S[2][1];
  double V[4][4];
  for (int r = 0; r < 4; r++)
    for (int k = 0; k < 4; k++) V[r][k] = r == k ? 1.0 : 0.0;
  uint32_t sweeps = 0;
  while (sweeps < PFT_REFINE_JACOBI_SWEEPS) {
    bool any = false;
    for (int p = 0; p < 3; p++)
      for (int q = p + 1; q < 4; q++) any = any || N[p][q] != 0.0;
    if (!any) break;
    sweeps++;
    for (int p = 0; p < 3; p++)
      for (int q = p + 1; q < 4; q++) {
        const double apq = N[p][q];
        if (apq == 0.0) continue;
        const double theta = (N[q][q] - N[p][p]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double cs = 1.0 / sqrt(t * t + 1.0);
        const double sn = t * cs;
        N[p][p] = N[p][p] - t * apq;
        N[q][q] = N[q][q] + t * apq;
        N[p][q] = N[q][p] = 0.0;
        for (int r = 0; r < 4; r++) {
          if (r != p && r != q) {
            const double arp = N[r][p], arq = N[r][q];
            N[r][p] = N[p][r] = cs * arp - sn * arq;
            N[r][q] = N[q][r] = sn * arp + cs * arq;
          }
          const double vrp = V[r][p], vrq = V[r][q];
          V[r][p] = cs * vrp - sn * vrq;
          V[r][q] = sn * vrp + cs * vrq;
        }
      }
  }
  int best = 0;  // the largest diagonal entry, the first on ties
  double top = N[0][0];
  for (int k = 1; k < 4; k++)
    if (N[k][k] > top) {
      top = N[k][k];
      best = k;
    }
  for (int k = 0; k < 4; k++) dq[k] = best == 0 ? V[k][0] : (best == 1 ? V[k][1] : (best == 2 ? V[k][2] : V[k][3]));
  refine_normalise(dq);
  if (dq[0] < 0.0)  // q and -q are the same rotation: the one with w >= 0
    for (int k = 0; k < 4; k++) dq[k] = -dq[k];
  double dR[9];
  refine_rotation(dq, dR);
  double tn[3];
  for (int r = 0; r < 3; r++)
    tn[r] = c[r] + (bm[r] - (dR[3 * r] * am[0] + dR[3 * r + 1] * am[1] + dR[3 * r + 2] * am[2]));
  const double e0 = tn[0] - c[0], e1 = tn[1] - c[1], e2 = tn[2] - c[2];
  step2[0] = e0 * e0 + e1 * e1 + e2 * e2;
  step2[1] = 4.0 * (dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
  if (step2[0] == 0.0 && step2[1] == 0.0) return sweeps;
  const double w = s->Q[0], x = s->Q[1], y = s->Q[2], z = s->Q[3];
  s->Q[0] = dq[0] * w - dq[1] * x - dq[2] * y - dq[3] * z;
  s->Q[1] = dq[0] * x + dq[1] * w + dq[2] * z - dq[3] * y;
  s->Q[2] = dq[0] * y - dq[1] * z + dq[2] * w + dq[3] * x;
  s->Q[3] = dq[0] * z + dq[1] * y - dq[2] * x + dq[3] * w;
  refine_normalise(s->Q);
  for (int r = 0; r < 3; r++) s->t[r] = tn[r];
  return sweeps;
}

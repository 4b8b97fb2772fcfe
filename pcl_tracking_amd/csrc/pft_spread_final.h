// pft_spread_final.h -- the one-lane part of the population statistics (pft_spread.hip): from the
// 29 tree sums, the integers and the pivot to every derived field of pft_population_stats, and the spread rule.  Plain
// double arithmetic (+ - x / only), a correctly rounded sqrt, and report_solve for the position ellipsoid.  Host and
// device: k_spread_final runs it in one lane, tests/cpp/spread_final_tool.cpp runs it on the CPU against
// tests/spread_model.py.  Built with -ffp-contract=off like the library.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/pft.h"
#include "pft_report_solve.h"

#define PFT_SPREAD_SUMS 29  // sum_w, sum_w2, s[6], S[21]

// position of S_kl (k <= l) in pft_population_stats::S: the upper triangle row by row
PFT_HD inline int spread_tri(int k, int l) { return k * 6 - k * (k - 1) / 2 + (l - k); }

// sums: {sum_w, sum_w2, s[0..5], S[0..20]}; pivot: the six pose components of the representative state.  Writes every
// field of *out except `calls` (the caller counts launches); out->streak is read as the previous streak
PFT_HD inline void spread_finalize(const double* sums, uint32_t n, uint32_t n_zero, float w_max, uint32_t i_max,
                                   const float* pivot, double max_pos_sigma, double min_n_eff, uint32_t after,
                                   pft_population_stats* out) {
  const double sum_w = sums[0], sum_w2 = sums[1];
  out->sum_w = sum_w;
  out->sum_w2 = sum_w2;
  for (int k = 0; k < 6; k++) out->s[k] = sums[2 + k];
  for (int k = 0; k < 21; k++) out->S[k] = sums[8 + k];
  out->n = n;
  out->n_zero = n_zero;
  out->w_max = w_max;
  out->i_max = i_max;
  const uint32_t prev = out->streak;
  double n_eff = 0.0;
  float sigma_max = 0.0f;
  if (sum_w == 0.0) {  // no particle carries weight: every derived field is 0
    for (int k = 0; k < 6; k++) out->mean[k] = 0.0;
    for (int k = 0; k < 36; k++) out->cov[k] = 0.0;
    for (int a = 0; a < 3; a++) out->rpy_sigma[a] = 0.0;
    for (int a = 0; a < 3; a++) out->pos_sigma[a] = 0.0f;
    for (int a = 0; a < 9; a++) out->pos_axes[a] = 0.0f;
    out->solve_info = 0u;
  } else {
    n_eff = sum_w2 > 0.0 ? (sum_w * sum_w) / sum_w2 : 0.0;
    double m[6];
    for (int k = 0; k < 6; k++) {
      m[k] = sums[2 + k] / sum_w;
      out->mean[k] = (double)pivot[k] + m[k];
    }
    // the position ellipsoid: the 3x3 block rounded to float through the eigen solver of the object report
    float c3[3][3], ev[3], Q[3][3];
    for (int k = 0; k < 6; k++)
      for (int l = k; l < 6; l++) {
        const double c = sums[8 + spread_tri(k, l)] / sum_w - m[k] * m[l];
        out->cov[k * 6 + l] = c;
        out->cov[l * 6 + k] = c;
        if (l < 3) c3[k][l] = c3[l][k] = (float)c;
        if (k == l && k >= 3) out->rpy_sigma[k - 3] = sqrt(c > 0.0 ? c : 0.0);
      }
    out->solve_info = report_solve(c3, ev, Q);
    for (int a = 0; a < 3; a++) out->pos_sigma[a] = sqrtf(ev[a] > 0.0f ? ev[a] : 0.0f);
    sigma_max = sqrtf(ev[2] > 0.0f ? ev[2] : 0.0f);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) out->pos_axes[r * 3 + c] = Q[r][c];
  }
  out->n_eff = n_eff;
  out->evaluated = 1u;
  // the spread rule: `after` evaluated calls in a row with the largest position sigma above max_pos_sigma or fewer than
  // min_n_eff effective particles
  const uint32_t uncertain = ((double)sigma_max > max_pos_sigma || n_eff < min_n_eff) ? 1u : 0u;
  const uint32_t streak = uncertain ? (prev == 0xffffffffu ? prev : prev + 1u) : 0u;
  out->uncertain = uncertain;
  out->streak = streak;
  out->flagged = streak >= after ? 1u : 0u;
}

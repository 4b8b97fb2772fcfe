// pft_pair_tree.h -- the adjacent-pair summation tree of the pose evaluators (pft_report, pft_match, pft_reacquire,
// pft_spread, pft_refine): positions 0 .. n-1 padded to N = the smallest power of two >= n,
// T(k+1)[i] = Tk[2i] + Tk[2i+1], the root is the sum.  The levels below are aligned subtrees of that one tree, so the bits
// depend on neither the workgroup size nor the grid: a lane's value (`unit` positions), the wave (xor 1 .. 32), the waves
// (LDS), then tiles or blocks by a binary counter in LDS and the fold of what the counter still holds.
//
// GATED is the caller's choice per site.  Ungated, every step is taken: right where adding the padding changes nothing
// (+0.0 under terms >= +0.0, -0.0 under any terms), and what the padding is stays with the caller.  Gated, a step is taken
// only while its span lies inside npad, the padded size in positions: above the root nothing is added, so the sign of a
// -0.0 root of signed terms padded with +0.0 survives as in the definition.
//
// Every routine is called by the whole workgroup; sums are indexed by threadIdx.x where a result lands in lanes < NS.
#pragma once
#include "pft_device_utils.h"

#define PT_MAX_LEVELS 32  // counter levels: more units than a 32-bit count names do not exist

__device__ __forceinline__ uint32_t pt_pow2_ceil(uint32_t n) { return n <= 1u ? 1u : 1u << (32 - __clz((int)(n - 1u))); }

// the wave: lanes 2i and 2i+1 hold the two halves; both form left + right (addition commutes bit for bit)
template <bool GATED, typename T, int NS>
__device__ __forceinline__ void pt_wave(T (&v)[NS], uint32_t unit = 1u, uint32_t npad = 0u) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const bool take = !GATED || unit * (uint32_t)o < npad;
#pragma unroll
    for (int q = 0; q < NS; q++) {
      const T t = v[q] + __shfl_xor(v[q], o);
      v[q] = take ? t : v[q];
    }
  }
}

// the waves, sh[w][q] = sum q of wave w: lane q joins its sum over the WAVES waves.  nw = the waves the launch has, where
// that is fewer than WAVES
template <bool GATED, int WAVES, typename T, int LD>
__device__ __forceinline__ T pt_waves_root(T (*sh)[LD], uint32_t unit = 1u, uint32_t npad = 0u, uint32_t nw = WAVES) {
  T w[WAVES];
#pragma unroll
  for (int q = 0; q < WAVES; q++) w[q] = (uint32_t)q < nw ? sh[q][threadIdx.x] : (T)0;
#pragma unroll
  for (int h = 1; h < WAVES; h <<= 1) {
    const bool take = !GATED || unit * (uint32_t)(64 * h) < npad;
#pragma unroll
    for (int q = 0; q + h < WAVES; q += 2 * h) w[q] = take ? w[q] + w[q + h] : w[q];
  }
  return w[0];
}

// lane 0 of each wave hands its NS values to sh, a barrier, then the root of sum q in lane q < NS (other lanes: 0).  The
// caller puts a barrier before sh is written again
template <bool GATED, int WAVES, typename T, int NS, int LD>
__device__ __forceinline__ T pt_waves(const T (&v)[NS], T (*sh)[LD], uint32_t unit = 1u, uint32_t npad = 0u) {
  const uint32_t tid = threadIdx.x;
  if ((tid & 63u) == 0u) {
#pragma unroll
    for (int q = 0; q < NS; q++) sh[tid >> 6][q] = v[q];
  }
  __syncthreads();
  return tid < (uint32_t)NS ? pt_waves_root<GATED, WAVES>(sh, unit, npad) : (T)0;
}

// the binary counter over tiles or blocks, stk[l] = the pending subtree of 2^l units: unit i merges the pending subtrees
// its trailing one bits name (all of them left neighbours inside the padded size, so no step needs a gate).  Lanes < NS
template <typename T, int LD>
__device__ __forceinline__ T pt_push(T (*stk)[LD], uint32_t i, T v) {
  uint32_t l = 0;
  for (uint32_t b = i; b & 1u; b >>= 1, l++) v = stk[l][threadIdx.x] + v;
  stk[l][threadIdx.x] = v;
  return v;
}

// the root after n_units pushes: the pending subtrees from the smallest (rightmost) up.  Padding that adds nothing makes
// the padded tree's root this right-to-left fold of what the counter holds.  Lanes < NS
template <typename T, int LD>
__device__ __forceinline__ T pt_fold(T (*stk)[LD], uint32_t n_units) {
  T v = (T)0;
  bool any = false;
  for (uint32_t l = 0; l < PT_MAX_LEVELS; l++)
    if ((n_units >> l) & 1u) {
      v = any ? stk[l][threadIdx.x] + v : stk[l][threadIdx.x];
      any = true;
    }
  return v;
}

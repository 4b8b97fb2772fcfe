// pft_spread.hip -- population statistics (pft_spread): effective sample size, the weighted
// covariance of the six pose components around the representative state, the position ellipsoid, and the spread rule.
// Two launches on the handle's stream behind pft_compute, in the pattern of k_match: they read PftHeader::rep, the
// particle count of a KLD handle and the population on the device, so nothing synchronises.
//
//   k_spread_partial   one workgroup per aligned block of SP_BLOCK particles, one particle per lane (2 x dwordx4, coalesced):
//                      w, d_k = (double)p_k - (double)rep_k, the 29 terms, then the lane -> wave -> workgroup levels of the
//                      one adjacent-pair tree; the block's 29 roots, zero count and first maximum go to the partial arrays
//   k_spread_final     one workgroup: the grid level of the same tree over the blocks' roots (4 or 16 blocks per lane, the
//                      wave, the waves), the integers, then pft_spread_final.h in one lane
//
// The tree (pft_pair_tree.h): positions 0 .. n-1 padded with +0.0.  The terms are signed, so every level is the gated form:
// the sign of a -0.0 root (all weights zero, all offsets negative) survives as in the definition.  Blocks wholly beyond n
// are not read and not written; the final launch takes them as +0.0.
#include "pft_device_utils.h"
#include "pft_pair_tree.h"
#include "pft_spread_final.h"

#define SP_BLOCK 256                 // particles per workgroup of k_spread_partial (a power of two, one per lane)
#define SP_WAVES (SP_BLOCK / 64)
#define SP_FINAL_MAX 256             // lanes of k_spread_final: 16 blocks each cover PFT_MAX_PARTICLES / SP_BLOCK = 4096

__device__ __forceinline__ uint32_t sp_count(const PftDev& d, uint32_t n_arg) {
  // (a KLD handle's count lives on the device; never beyond what the launch was sized for)
  return d.p_active ? min(*d.p_active, n_arg) : n_arg;
}

// first maximum of (w, i) pairs: the larger weight, on a tie the lower index
__device__ __forceinline__ void sp_max_merge(float& w, uint32_t& i, float ow, uint32_t oi) {
  if (ow > w || (ow == w && oi < i)) {
    w = ow;
    i = oi;
  }
}

__global__ void __launch_bounds__(SP_BLOCK) k_spread_partial(PftDev d, uint32_t n_arg, uint32_t g_cap,
                                                             double* __restrict__ part, uint32_t* __restrict__ part_zero,
                                                             float* __restrict__ part_wmax,
                                                             uint32_t* __restrict__ part_imax) {
  __shared__ double sh[SP_WAVES][PFT_SPREAD_SUMS];
  __shared__ uint32_t sh_zero[SP_WAVES], sh_imax[SP_WAVES];
  __shared__ float sh_wmax[SP_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, g = blockIdx.x;
  if (d.hdr->error != 0u) return;  // a failed iteration is not evaluated (k_spread_final says so)
  const uint32_t n = sp_count(d, n_arg);
  if (g >= g_cap || g * SP_BLOCK >= n) return;  // (uniform: a block wholly beyond the population)
  const uint32_t N = pt_pow2_ceil(n);
  const uint32_t i = g * SP_BLOCK + tid;

  double v[PFT_SPREAD_SUMS];
#pragma unroll
  for (int q = 0; q < PFT_SPREAD_SUMS; q++) v[q] = 0.0;
  uint32_t zero = 0u, imax = 0xffffffffu;
  float wmax = -INFINITY;
  if (i < n) {
    const float4* pp = reinterpret_cast<const float4*>(d.part_all + i);
    const float4 a = pp[0], b = pp[1];
    const pft_particle& r = d.hdr->rep;
    const double w = (double)b.w;
    double dk[6];
    dk[0] = (double)a.x - (double)r.x;
    dk[1] = (double)a.y - (double)r.y;
    dk[2] = (double)a.z - (double)r.z;
    dk[3] = (double)b.x - (double)r.roll;
    dk[4] = (double)b.y - (double)r.pitch;
    dk[5] = (double)b.z - (double)r.yaw;
    v[0] = w;
    v[1] = w * w;
    int q = 8;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double wd = w * dk[k];
      v[2 + k] = wd;
#pragma unroll
      for (int l = k; l < 6; l++) v[q++] = wd * dk[l];
    }
    zero = b.w == 0.0f ? 1u : 0u;
    wmax = b.w;
    imax = i;
  }
  pt_wave<true>(v, 1u, N);
  for (int o = 1; o < 64; o <<= 1) {  // the first maximum of the wave
    const float ow = __shfl_xor(wmax, o);
    const uint32_t oi = __shfl_xor(imax, o);
    sp_max_merge(wmax, imax, ow, oi);
  }
  zero = wave_sum(zero);
  if (lane == 0) {
    sh_zero[wave] = zero;
    sh_wmax[wave] = wmax;
    sh_imax[wave] = imax;
  }
  const double root = pt_waves<true, SP_WAVES>(v, sh, 1u, N);  // (its barrier also publishes the integers and the maxima)
  if (tid < PFT_SPREAD_SUMS) {
    part[(size_t)tid * g_cap + g] = root;
  } else if (tid == 64) {
    uint32_t z = 0u, bi = 0xffffffffu;
    float bw = -INFINITY;
    for (int q = 0; q < SP_WAVES; q++) {
      z += sh_zero[q];
      sp_max_merge(bw, bi, sh_wmax[q], sh_imax[q]);
    }
    part_zero[g] = z;
    part_wmax[g] = bw;
    part_imax[g] = bi;
  }
}

template <int B>  // blocks per lane (a power of two): 4 up to 1 024 blocks, 16 up to the 4 096 of PFT_MAX_PARTICLES
__global__ void __launch_bounds__(SP_FINAL_MAX) k_spread_final(PftDev d, uint32_t n_arg, uint32_t g_cap,
                                                               const double* __restrict__ part,
                                                               const uint32_t* __restrict__ part_zero,
                                                               const float* __restrict__ part_wmax,
                                                               const uint32_t* __restrict__ part_imax, double max_pos_sigma,
                                                               double min_n_eff, uint32_t after,
                                                               pft_population_stats* __restrict__ out) {
  __shared__ double sh[SP_FINAL_MAX / 64][PFT_SPREAD_SUMS];
  __shared__ double sums[PFT_SPREAD_SUMS];
  __shared__ uint32_t sh_zero[SP_FINAL_MAX / 64], sh_imax[SP_FINAL_MAX / 64];
  __shared__ float sh_wmax[SP_FINAL_MAX / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nw = blockDim.x >> 6;
  if (d.hdr->error != 0u) {  // the last iteration ran without a target: nothing to evaluate, the block keeps its values
    if (tid == 0) {
      out->evaluated = 0u;
      out->calls = out->calls + 1u;
    }
    return;
  }
  const uint32_t n = sp_count(d, n_arg);
  const uint32_t G = min((n + SP_BLOCK - 1u) / SP_BLOCK, g_cap);  // blocks k_spread_partial wrote
  const uint32_t NG = pt_pow2_ceil(G);                           // blocks of the padded tree (1 when n <= SP_BLOCK)
  // the grid level: B blocks per lane, the wave, the waves -- positions beyond G are the padding.  The loop over the sums
  // is unrolled so that the loads of several sums are in flight together: a few memory latencies, not 29
  const uint32_t g0 = (uint32_t)B * tid;
  auto lane_root = [&](int q) {  // the lane's B blocks of sum q
    const double* p = part + (size_t)q * g_cap + g0;
    double a[B];
#pragma unroll
    for (int j = 0; j < B; j++) a[j] = g0 + (uint32_t)j < G ? p[j] : 0.0;
#pragma unroll
    for (int h = 1; h < B; h <<= 1) {
      const bool take = (uint32_t)h < NG;
#pragma unroll
      for (int j = 0; j + h < B; j += 2 * h) a[j] = take ? a[j] + a[j + h] : a[j];
    }
    return a[0];
  };
  if constexpr (B == 4) {  // every sum of the lane in registers
    double v[PFT_SPREAD_SUMS];
#pragma unroll
    for (int q = 0; q < PFT_SPREAD_SUMS; q++) v[q] = 0.0;
    if (g0 < G) {  // (lanes beyond G hold +0.0: the padding inside NG, and beyond it what no taken step reads)
#pragma unroll
      for (int q = 0; q < PFT_SPREAD_SUMS; q++) v[q] = lane_root(q);
    }
    if (NG > (uint32_t)B) pt_wave<true>(v, (uint32_t)B, NG);  // (uniform)
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < PFT_SPREAD_SUMS; q++) sh[wave][q] = v[q];
    }
  } else {  // above 262 144 particles: one sum at a time (29 x 16 roots per lane do not fit the registers)
    for (int q = 0; q < PFT_SPREAD_SUMS; q++) {
      double v[1] = {g0 < G ? lane_root(q) : 0.0};
      pt_wave<true>(v, (uint32_t)B, NG);
      if (lane == 0) sh[wave][q] = v[0];
    }
  }
  uint32_t zero = 0u, imax = 0xffffffffu;
  float wmax = -INFINITY;
  for (uint32_t g = tid; g < G; g += blockDim.x) {
    zero += part_zero[g];
    sp_max_merge(wmax, imax, part_wmax[g], part_imax[g]);
  }
  for (int o = 1; o < 64; o <<= 1) {
    const float ow = __shfl_xor(wmax, o);
    const uint32_t oi = __shfl_xor(imax, o);
    sp_max_merge(wmax, imax, ow, oi);
  }
  zero = wave_sum(zero);
  if (lane == 0) {
    sh_zero[wave] = zero;
    sh_wmax[wave] = wmax;
    sh_imax[wave] = imax;
  }
  __syncthreads();
  if (tid < PFT_SPREAD_SUMS) sums[tid] = pt_waves_root<true, SP_FINAL_MAX / 64>(sh, (uint32_t)B, NG, nw);  // 64 B blocks each
  __syncthreads();
  if (tid == 0) {
    uint32_t z = 0u, bi = 0xffffffffu;
    float bw = -INFINITY;
    for (uint32_t q = 0; q < nw; q++) {
      z += sh_zero[q];
      sp_max_merge(bw, bi, sh_wmax[q], sh_imax[q]);
    }
    if (n == 0u) {
      bw = 0.0f;
      bi = 0u;
    }
    const pft_particle r = d.hdr->rep;
    const float pivot[6] = {r.x, r.y, r.z, r.roll, r.pitch, r.yaw};
    spread_finalize(sums, n, z, bw, bi, pivot, max_pos_sigma, min_n_eff, after, out);
    out->calls = out->calls + 1u;
  }
}

// blocks the partial arrays must have room for: n_max particles
uint32_t pftk_spread_blocks(uint32_t n_max) { return (n_max + SP_BLOCK - 1u) / SP_BLOCK; }

void pftk_spread(hipStream_t s, const PftDev& d, uint32_t n_max, double* part, uint32_t* part_zero, float* part_wmax,
                 uint32_t* part_imax, double max_pos_sigma, double min_n_eff, uint32_t after, pft_population_stats* out) {
  const uint32_t g_cap = pftk_spread_blocks(n_max);
  hipLaunchKernelGGL(k_spread_partial, dim3(g_cap), dim3(SP_BLOCK), 0, s, d, n_max, g_cap, part, part_zero, part_wmax,
                     part_imax);
  // B blocks per lane, whole waves: the lanes cover the launch size
  const uint32_t B = g_cap <= 4u * SP_FINAL_MAX ? 4u : 16u;
  uint32_t threads = 64u;
  while (B * threads < g_cap && threads < SP_FINAL_MAX) threads *= 2u;
  if (B == 4u)
    hipLaunchKernelGGL(k_spread_final<4>, dim3(1), dim3(threads), 0, s, d, n_max, g_cap, part, part_zero, part_wmax,
                       part_imax, max_pos_sigma, min_n_eff, after, out);
  else
    hipLaunchKernelGGL(k_spread_final<16>, dim3(1), dim3(threads), 0, s, d, n_max, g_cap, part, part_zero, part_wmax,
                       part_imax, max_pos_sigma, min_n_eff, after, out);
}

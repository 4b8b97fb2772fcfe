// pft_segment.hip -- model creation on the device (include/pft_segment.h): the stages of the reference's
// create_model_planar_segmentation.cpp:131-203 / create_model.cpp:131-179 as one chain of launches on one stream.
//
//   compaction   k_sg_zero (transform + removeZeroPoints flags), k_sg_scan, k_sg_emit: ordered stream compaction
//                (per-tile counts, one-workgroup scan, scatter), the same three kernels serve every compaction below
//   sample       k_sg_sample: one workgroup replays boost::mt19937 (state in LDS, the 624-word twist split over the
//                lanes) and drawIndexSample's swaps (a sparse map in LDS), emitting good samples in draw order
//   scoring      k_sg_score: a tile of points per workgroup against a batch of SG_BATCH planes in LDS; exact counts
//   replay       k_sg_replay: RandomSampleConsensus::computeModel's loop over the scored batch, in one lane
//   refit        k_sg_select + compaction of the best hypothesis' inliers, k_sg_refit: the nine sequential float sums
//                of computeMeanAndCovarianceMatrix (nine lanes) and pcl::eigen33 (one lane)
//                or, PFT_SUM_TREE: k_sg_refit_tiles + k_sg_refit_top, the sums as adjacent-pair trees over many workgroups
//   rounds       pft_segment_set_plane_rounds: sample .. refit repeated on what the last plane left (cluster_euclid.cpp:
//                59-85), k_sg_round_*: a byte per input point tells the round that removed it
//   clustering   survivors sorted by a grid-cell key (the radix sort of pft_filters.hip), lock-free union-find over
//                neighbour cells, component sizes, the size filter, the ordering rule, a stable sort by cluster rank
//
// Each recalled PCL rule has ONE switch point here, marked "RULE <name>", mirrored in tests/segment_model.py.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "pft_devbuf.h"
#include "pft_device_utils.h"
#include "pft_segment_solve.h"
#include "../../include/pft_segment.h"

#define SG_TILE 1024u
#define SG_THREADS 256
#define SG_BATCH 128u        // hypotheses per scoring batch
#define SG_MAPCAP 8192u      // sparse map of drawIndexSample's swaps (LDS), power of two
#define SG_MAPMAX 6144u      // entries allowed (load factor 0.75)
#define SG_MAX_ITER 1919     // the sampler draws whole batches: 3 + 3 hmax <= SG_MAPMAX with hmax = 1920
#define SG_SAMPLE_CHECKS 1000u  // SampleConsensusModel::max_sample_checks_
#define SG_EMPTY 0xFFFFFFFFu
#define SG_OVERFLOW 0xFFFFFFFEu  // sample slot: the sparse map filled up before this sample could be drawn
#define SG_CELL_SLACK 1.03125    // cell side = tol / 2 * (1 + 2^-5): see cell_coord
#define SG_MAX_AXIS_CELLS (1u << 17)
#define SG_SCORE_PTS 8u      // points per thread in k_sg_score

enum { SG_ERR_MAP = 1u };
static_assert(3u + 3u * (((SG_MAX_ITER + 1u) + SG_BATCH - 1u) / SG_BATCH * SG_BATCH) <= SG_MAPMAX,
              "the sparse map holds every position the sampler's whole batches can touch without redraws");

struct SgHdr {
  // RandomSampleConsensus state, carried from batch to batch
  double k;
  int32_t best_count, best_h;
  uint32_t iterations, decided, skipped;
  uint32_t n_valid, n_ransac_inl, n_fin, n_surv;
  uint32_t err;
  float coef_ransac[4];
  float coef_final[4];
  uint32_t n_cells, n_clusters, n_total;
  float bmin[3], bmax[3];
  // sampler state (mt19937 and the sparse map live in HBM between batches)
  uint32_t mt_pos, map_count, emitted;
  // what the one-lane tail of this round's refit did (m = 0: no refit ran)
  pft_segment_refit_debug refit;
};

struct SgHyp {
  int32_t* sample;   // [hmax][3], SG_EMPTY in [0] = no sample could be drawn, SG_OVERFLOW = the sparse map is full
  float4* coef;      // [hmax]
  uint32_t* count;   // [hmax]
};

struct SgParams {
  uint32_t n;
  int transform_enable;
  float T[12];
  float zero_thr;    // 0.01 as the float compare of fabs(float) < 0.01 (double) needs it
  float dist_thr;    // distance threshold, same
  double log_probability;
  int max_iterations;
  uint32_t seed;
  int box_enable[3];
  float box_min[3], box_max[3];
  float tol2;        // (float)(tol * tol)
  float inv_cell;    // 1 / (tol / 2 * SG_CELL_SLACK)
  uint32_t nx, ny, nz;
  uint32_t min_size, max_size;
};

// smallest float f with (double)x < thr <=> x < f for every float x: how `float < double` compares
static float float_bound_below(double thr) {
  float f = (float)thr;
  if ((double)f < thr) f = nextafterf(f, INFINITY);
  return f;
}

// ---------------------------------------------------------------------------------------------------------------
// ordered stream compaction: per-tile counts of a flag array, one-workgroup scan, scatter of the kept positions
__device__ __forceinline__ void sg_tile_count(const uint8_t* flag, uint32_t n, uint32_t* tile) {
  __shared__ uint32_t su[20];
  const uint32_t t = blockIdx.x, i0 = t * SG_TILE + threadIdx.x * 4u;
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) c += (i0 + k < n) ? flag[i0 + k] : 0u;
  uint32_t tot;
  block_excl_scan<uint32_t>(c, su, &tot);
  if (threadIdx.x == 0) tile[t] = tot;
}

// in-place exclusive scan of tile[0..ntiles) (ntiles from the device when n_dev != null); total to *out
__global__ __launch_bounds__(1024) void k_sg_scan(uint32_t* tile, uint32_t ntiles_max, const uint32_t* n_dev,
                                                  uint32_t* out) {
  __shared__ uint32_t scr[20];
  const uint32_t ntiles = n_dev ? (*n_dev + SG_TILE - 1) / SG_TILE : ntiles_max;
  uint32_t carry = 0;
  for (uint32_t t0 = 0; t0 < ntiles; t0 += blockDim.x) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t v = t < ntiles ? tile[t] : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl_scan<uint32_t>(v, scr, &tot);
    if (t < ntiles) tile[t] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *out = carry;
}

// the same scan for the other ordered compactions of the library (pft_subtract.hip): tile[0 .. ntiles) in place, the total to *out
void pftk_tile_scan(hipStream_t st, uint32_t* tile, uint32_t ntiles, uint32_t* out) {
  hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, tile, ntiles, (const uint32_t*)nullptr, out);
}

// out[pos] = map ? map[i] : i for every flagged i, in order; optional gather of float4 src[i] to dst[pos]
__global__ __launch_bounds__(SG_THREADS) void k_sg_emit(const uint8_t* __restrict__ flag, uint32_t n_max,
                                                        const uint32_t* n_dev, const uint32_t* __restrict__ tile,
                                                        const uint32_t* __restrict__ map, uint32_t* __restrict__ out,
                                                        const float4* __restrict__ src, float4* __restrict__ dst) {
  __shared__ uint32_t su[20];
  const uint32_t n = n_dev ? *n_dev : n_max;
  const uint32_t t = blockIdx.x, i0 = t * SG_TILE + threadIdx.x * 4u;
  if (t * SG_TILE >= n) return;  // (workgroup-uniform)
  uint32_t f[4], c = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    f[k] = (i0 + k < n) ? flag[i0 + k] : 0u;
    c += f[k];
  }
  uint32_t tot;
  uint32_t pos = tile[t] + block_excl_scan<uint32_t>(c, su, &tot);
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (f[k]) {
      const uint32_t i = i0 + k;
      out[pos] = map ? map[i] : i;
      if (dst) dst[pos] = src[i];
      pos++;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 1 + 2: transform (pft/common.hpp transformPointCloud: ((T0 x + T1 y) + T2 z) + T3, unfused) and removeZeroPoints
// (create_model_planar_segmentation.cpp:59-77) on the transformed coordinates
__global__ __launch_bounds__(SG_THREADS) void k_sg_zero(SgParams p, const pft_point_xyzrgba* __restrict__ in,
                                                        float4* __restrict__ tx, uint8_t* __restrict__ flag,
                                                        uint32_t* __restrict__ tile) {
  const uint32_t i0 = blockIdx.x * SG_TILE + threadIdx.x * 4u;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t i = i0 + k;
    if (i >= p.n) break;
    const float4 q = *reinterpret_cast<const float4*>(in + i);
    float x = q.x, y = q.y, z = q.z;
    if (p.transform_enable) xform(p.T, q.x, q.y, q.z, x, y, z);
    // RULE zero: dropped when all of |x|, |y|, |z| < 0.01 (float against double) or any coordinate is NaN
    const bool zero = fabsf(x) < p.zero_thr && fabsf(y) < p.zero_thr && fabsf(z) < p.zero_thr;
    const bool keep = !zero && !__builtin_isnan(x) && !__builtin_isnan(y) && !__builtin_isnan(z);
    tx[i] = make_float4(x, y, z, 1.0f);
    flag[i] = keep ? 1 : 0;
  }
  sg_tile_count(flag, p.n, tile);
}

// removeZeroPoints alone, for the model preparation (pft_model.hip): RULE zero without a transform and the compaction
// above.  keep_idx[0 .. *n_keep) = the kept input indices, ascending; keep_xyz = their {x, y, z, 1}.  xyz [n], flag [n]
// and tile [ceil(n / SG_TILE)] are scratch.
void pftk_remove_zero_points(hipStream_t st, const pft_point_xyzrgba* in, uint32_t n, float4* xyz, uint8_t* flag,
                             uint32_t* tile, uint32_t* keep_idx, float4* keep_xyz, uint32_t* n_keep) {
  SgParams p = {};
  p.n = n;
  p.zero_thr = float_bound_below(0.01);
  const uint32_t ntiles = (n + SG_TILE - 1) / SG_TILE;
  hipLaunchKernelGGL(k_sg_zero, dim3(ntiles), dim3(SG_THREADS), 0, st, p, in, xyz, flag, tile);
  hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, tile, ntiles, (const uint32_t*)nullptr, n_keep);
  hipLaunchKernelGGL(k_sg_emit, dim3(ntiles), dim3(SG_THREADS), 0, st, (const uint8_t*)flag, n, (const uint32_t*)nullptr,
                     (const uint32_t*)tile, (const uint32_t*)nullptr, keep_idx, (const float4*)xyz, keep_xyz);
}

// ---------------------------------------------------------------------------------------------------------------
// 3. RANSAC.  RULE rng: boost::uniform_int<>(0, INT_MAX) over boost::mt19937 reduces to engine() >> 1 (bucket size 2).
#define MT_N 624
#define MT_M 397
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}
__device__ __forceinline__ uint32_t mt_next_word(uint32_t a, uint32_t b, uint32_t c) {  // a = mt[i], b = mt[i+1], c = mt[i+M]
  const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
  return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// the sequential twist in four dependency phases: [0,227) reads old words only, [227,454) reads the first phase's
// output, [454,623) the second's, 623 reads mt[0] and mt[396]
__device__ void mt_twist(uint32_t* mt) {
  const uint32_t tid = threadIdx.x;
  const uint32_t lo[4] = {0, 227, 454, 623}, hi[4] = {227, 454, 623, 624};
  for (int ph = 0; ph < 4; ph++) {
    uint32_t v[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const uint32_t i = lo[ph] + tid + r * SG_THREADS;
      if (i < hi[ph]) v[r] = mt_next_word(mt[i], mt[(i + 1) % MT_N], mt[(i + MT_M) % MT_N]);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const uint32_t i = lo[ph] + tid + r * SG_THREADS;
      if (i < hi[ph]) mt[i] = v[r];
    }
    __syncthreads();
  }
}

__device__ __forceinline__ uint32_t map_slot(uint32_t key) { return (key * 2654435761u) >> (32 - 13); }
__device__ __forceinline__ uint32_t map_get(const uint32_t* mk, const uint32_t* mv, uint32_t key) {
  for (uint32_t s = map_slot(key);; s = (s + 1u) & (SG_MAPCAP - 1u)) {
    if (mk[s] == key) return mv[s];
    if (mk[s] == SG_EMPTY) return key;  // untouched position of shuffled_indices_ = its own index
  }
}
__device__ __forceinline__ bool map_set(uint32_t* mk, uint32_t* mv, uint32_t* count, uint32_t key, uint32_t val) {
  for (uint32_t s = map_slot(key);; s = (s + 1u) & (SG_MAPCAP - 1u)) {
    if (mk[s] == key) {
      mv[s] = val;
      return true;
    }
    if (mk[s] == SG_EMPTY) {
      if (*count >= SG_MAPMAX) return false;
      mk[s] = key;
      mv[s] = val;
      (*count)++;
      return true;
    }
  }
}

// RULE good: isSampleGood -- dy1dy2 = (p1 - p0) / (p2 - p0); good iff dy1dy2[0] != dy1dy2[1] || dy1dy2[2] != dy1dy2[1]
__device__ __forceinline__ bool sample_good(float4 a, float4 b, float4 c) {
  const float r0 = (b.x - a.x) / (c.x - a.x), r1 = (b.y - a.y) / (c.y - a.y), r2 = (b.z - a.z) / (c.z - a.z);
  return r0 != r1 || r2 != r1;
}

// RULE coef: computeModelCoefficients -- cross product as PCL writes it, normalize() = divide by sqrt of the squared
// norm ((a0^2 + a1^2) + (a2^2 + 0^2), the 4-lane reduction), then d = -((c0 x + c1 y) + (c2 z + 0 * 1))
__device__ __forceinline__ float4 plane_of(float4 p0, float4 p1, float4 p2) {
  const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
  const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
  float c0 = ay * bz - az * by;
  float c1 = az * bx - ax * bz;
  float c2 = ax * by - ay * bx;
  const float sq = (c0 * c0 + c1 * c1) + (c2 * c2 + 0.0f * 0.0f);
  const float nrm = sqrtf(sq);
  c0 = c0 / nrm;
  c1 = c1 / nrm;
  c2 = c2 / nrm;
  const float c3 = 0.0f / nrm;
  const float dot = (c0 * p0.x + c1 * p0.y) + (c2 * p0.z + c3 * 1.0f);
  return make_float4(c0, c1, c2, -1.0f * dot);
}

// RULE dist: |c . (x, y, z, 1)| with the 4-lane reduction (a0 + a1) + (a2 + a3), compared strictly (float vs double)
__device__ __forceinline__ bool within(float4 c, float4 q, float thr) {
  const float d = (c.x * q.x + c.y * q.y) + (c.z * q.z + c.w * 1.0f);
  return fabsf(d) < thr;
}

struct SgSampler {
  uint32_t* mt;      // [624]
  uint32_t* mk;      // [SG_MAPCAP]
  uint32_t* mv;      // [SG_MAPCAP]
};

// one workgroup: the samples of batch b (hypotheses b*SG_BATCH ..), in draw order
__global__ __launch_bounds__(SG_THREADS) void k_sg_sample(SgParams p, SgHdr* __restrict__ h, SgSampler st, SgHyp hy,
                                                          const float4* __restrict__ pts, uint32_t b) {
  __shared__ uint32_t smt[MT_N];
  __shared__ uint32_t sout[MT_N];
  __shared__ uint32_t mk[SG_MAPCAP];
  __shared__ uint32_t mv[SG_MAPCAP];
  __shared__ uint32_t s_pos, s_done, s_count;
  const uint32_t tid = threadIdx.x;
  if (h->decided) return;  // (uniform) an earlier batch ended the loop
  const uint32_t n = h->n_valid;
  if (b == 0) {
    for (uint32_t k = tid; k < SG_MAPCAP; k += SG_THREADS) mk[k] = SG_EMPTY;
    if (tid == 0) {  // std::mt19937 / boost::mt19937 seed(s)
      uint32_t x = p.seed;
      smt[0] = x;
      for (uint32_t i = 1; i < MT_N; i++) {
        x = 1812433253u * (x ^ (x >> 30)) + i;
        smt[i] = x;
      }
      s_pos = MT_N;
      s_count = 0;
    }
  } else {
    for (uint32_t k = tid; k < SG_MAPCAP; k += SG_THREADS) {
      mk[k] = st.mk[k];
      mv[k] = st.mv[k];
    }
    for (uint32_t k = tid; k < MT_N; k += SG_THREADS) smt[k] = st.mt[k];
    if (tid == 0) {
      s_pos = h->mt_pos;
      s_count = h->map_count;
    }
  }
  if (tid == 0) s_done = 0;
  __syncthreads();
  for (uint32_t k = tid; k < MT_N; k += SG_THREADS) sout[k] = mt_temper(smt[k]);
  __syncthreads();
  // lane 0 keeps the draw state in registers across refills: position i in drawIndexSample, failed draws so far
  uint32_t hcur = b * SG_BATCH, hend = hcur + SG_BATCH, di = 0, fails = 0;
  uint32_t cnt = s_count;
  for (;;) {
    if (tid == 0) {
      uint32_t pos = s_pos;
      bool stop = false;
      if (n < 3) {  // getSamples: fewer indices than the sample size -> no sample
        hy.sample[3 * hcur] = (int32_t)SG_EMPTY;
        stop = true;
      }
      while (!stop && pos < MT_N) {
        // RULE draw: swap(shuffled[i], shuffled[i + rnd() % (n - i)]), shuffled never reset between samples
        const uint32_t r = sout[pos++] >> 1;
        const uint32_t j = di + r % (n - di);
        const uint32_t a = map_get(mk, mv, di), c = map_get(mk, mv, j);
        if (!map_set(mk, mv, &cnt, di, c) || !map_set(mk, mv, &cnt, j, a)) {
          // only an error if the RANSAC loop gets as far as this sample (k_sg_replay)
          hy.sample[3 * hcur] = (int32_t)SG_OVERFLOW;
          stop = true;
          break;
        }
        if (++di < 3) continue;
        di = 0;
        const uint32_t s0 = map_get(mk, mv, 0), s1 = map_get(mk, mv, 1), s2 = map_get(mk, mv, 2);
        const float4 q0 = pts[s0], q1 = pts[s1], q2 = pts[s2];
        if (sample_good(q0, q1, q2)) {
          hy.sample[3 * hcur] = (int32_t)s0;
          hy.sample[3 * hcur + 1] = (int32_t)s1;
          hy.sample[3 * hcur + 2] = (int32_t)s2;
          hy.coef[hcur] = plane_of(q0, q1, q2);
          hcur++;
          fails = 0;
          if (hcur == hend) {
            stop = true;
            break;
          }
        } else if (++fails == SG_SAMPLE_CHECKS) {  // RULE checks: 1000 failed draws -> empty sample, loop breaks
          hy.sample[3 * hcur] = (int32_t)SG_EMPTY;
          stop = true;
          break;
        }
      }
      s_pos = pos;
      s_done = stop ? 1u : 0u;
      s_count = cnt;
    }
    __syncthreads();
    if (s_done) break;
    mt_twist(smt);  // all 624 tempered words consumed
    for (uint32_t k = tid; k < MT_N; k += SG_THREADS) sout[k] = mt_temper(smt[k]);
    if (tid == 0) s_pos = 0;
    __syncthreads();
  }
  // state for the next batch
  for (uint32_t k = tid; k < SG_MAPCAP; k += SG_THREADS) {
    st.mk[k] = mk[k];
    st.mv[k] = mv[k];
  }
  for (uint32_t k = tid; k < MT_N; k += SG_THREADS) st.mt[k] = smt[k];
  if (tid == 0) {
    h->mt_pos = s_pos;
    h->map_count = s_count;
    h->emitted = (b + 1u) * SG_BATCH;  // hypotheses this and the earlier batches drew and scored
  }
}

// counts of the batch's hypotheses over all points: SG_SCORE_PTS points per thread, planes from LDS, ballot counts
__global__ __launch_bounds__(SG_THREADS) void k_sg_score(SgParams p, const SgHdr* __restrict__ h, SgHyp hy,
                                                         const float4* __restrict__ pts, uint32_t b) {
  __shared__ float4 sc[SG_BATCH];
  __shared__ uint32_t scnt[SG_BATCH];
  if (h->decided) return;
  const uint32_t n = h->n_valid;
  const uint32_t base = blockIdx.x * (SG_THREADS * SG_SCORE_PTS);
  if (base >= n) return;  // (uniform)
  const uint32_t tid = threadIdx.x, h0 = b * SG_BATCH;
  if (tid < SG_BATCH) {
    const bool ok = (uint32_t)hy.sample[3 * (h0 + tid)] < SG_OVERFLOW;
    sc[tid] = ok ? hy.coef[h0 + tid] : make_float4(NAN, NAN, NAN, NAN);
    scnt[tid] = 0;
  }
  float4 q[SG_SCORE_PTS];
#pragma unroll
  for (uint32_t k = 0; k < SG_SCORE_PTS; k++) {
    const uint32_t i = base + k * SG_THREADS + tid;
    q[k] = i < n ? pts[i] : make_float4(NAN, NAN, NAN, NAN);
  }
  __syncthreads();
  for (uint32_t j = 0; j < SG_BATCH; j++) {
    const float4 c = sc[j];
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < SG_SCORE_PTS; k++) cnt += (uint32_t)__popcll(__ballot(within(c, q[k], p.dist_thr)));
    if (lane_id() == 0 && cnt) atomicAdd(&scnt[j], cnt);
  }
  __syncthreads();
  if (tid < SG_BATCH && scnt[tid]) atomicAdd(&hy.count[h0 + tid], scnt[tid]);
}

// RULE loop: RandomSampleConsensus::computeModel over the batch, one lane, double precision as upstream
__global__ __launch_bounds__(64) void k_sg_replay(SgParams p, SgHdr* __restrict__ h, SgHyp hy, uint32_t b) {
  if (threadIdx.x != 0 || h->decided) return;
  const uint32_t n = h->n_valid;
  const double one_over_indices = 1.0 / (double)n;
  double k = h->k;
  int32_t best = h->best_count, best_h = h->best_h;
  uint32_t it = h->iterations;
  bool decided = false;
  for (uint32_t hh = b * SG_BATCH; hh < (b + 1) * SG_BATCH; hh++) {
    if (!((double)it < k)) {  // while (iterations_ < k && skipped_count < max_skip)
      decided = true;
      break;
    }
    if ((uint32_t)hy.sample[3 * hh] == SG_OVERFLOW) {  // the sample the loop needs next was never drawn
      h->err |= SG_ERR_MAP;
      decided = true;
      break;
    }
    if (hy.sample[3 * hh] == (int32_t)SG_EMPTY) {  // "No samples could be selected!"
      decided = true;
      break;
    }
    const int32_t c = (int32_t)hy.count[hh];
    if (c > best) {
      best = c;
      best_h = (int32_t)hh;
      const double w = (double)best * one_over_indices;
      double p_no_outliers = 1.0 - pow(w, 3.0);
      p_no_outliers = fmax(DBL_EPSILON, p_no_outliers);
      p_no_outliers = fmin(1.0 - DBL_EPSILON, p_no_outliers);
      k = p.log_probability / log(p_no_outliers);
    }
    ++it;
    if ((int)it > p.max_iterations) {  // "RANSAC reached the maximum number of trials."
      decided = true;
      break;
    }
  }
  h->k = k;
  h->best_count = best;
  h->best_h = best_h;
  h->iterations = it;
  if (decided) {
    h->decided = 1;
    if (best_h >= 0) {
      const float4 c = hy.coef[best_h];
      h->coef_ransac[0] = c.x;
      h->coef_ransac[1] = c.y;
      h->coef_ransac[2] = c.z;
      h->coef_ransac[3] = c.w;
    }
  }
}

// flags of the points within the distance of a plane (coef from the header: 0 = best hypothesis, 1 = final);
// with box: also the survivor flags (not an inlier, inside the box)
__global__ __launch_bounds__(SG_THREADS) void k_sg_select(SgParams p, const SgHdr* __restrict__ h, int which,
                                                          const float4* __restrict__ pts, uint8_t* __restrict__ flag,
                                                          uint32_t* __restrict__ tile, uint8_t* __restrict__ sflag,
                                                          uint32_t* __restrict__ stile) {
  const uint32_t n = h->n_valid;
  if (blockIdx.x * SG_TILE >= n) return;  // (uniform)
  const bool have = h->best_h >= 0;
  const float* cf = which ? h->coef_final : h->coef_ransac;
  const float4 c = make_float4(cf[0], cf[1], cf[2], cf[3]);
  const uint32_t i0 = blockIdx.x * SG_TILE + threadIdx.x * 4u;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t i = i0 + k;
    if (i >= n) break;
    const float4 q = pts[i];
    const bool in = have && within(c, q, p.dist_thr);
    flag[i] = in ? 1 : 0;
    if (sflag) {
      // RULE box: PassThrough per enabled axis, inclusive float limits; the chain is the AND of the ranges
      bool keep = !in;
      const float v[3] = {q.x, q.y, q.z};
#pragma unroll
      for (int a = 0; a < 3; a++)
        if (p.box_enable[a] && (v[a] < p.box_min[a] || v[a] > p.box_max[a])) keep = false;
      sflag[i] = keep ? 1 : 0;
    }
  }
  sg_tile_count(flag, n, tile);
  if (sflag) sg_tile_count(sflag, n, stile);
}

// RULE eigen: pcl::computeRoots / computeRoots2 / eigen33 (smallest eigenvalue's vector) in float: pft_segment_solve.h,
// host and device.  The refit after the sums, one lane: accu = the nine sums divided by the count; the record of the
// solve stays in the header for pft_debug_segment_refit
__device__ void sg_refit_tail(SgHdr* __restrict__ h, const float* accu) {
  pft_segment_refit_debug rec;
  sg_refit_solve(accu, h->n_ransac_inl, &rec);
  h->coef_final[0] = rec.coef[0];
  h->coef_final[1] = rec.coef[1];
  h->coef_final[2] = rec.coef[2];
  h->coef_final[3] = rec.coef[3];
  h->refit = rec;
}

// RULE refit: optimizeModelCoefficients -- nine float accumulators summed in inlier index order, divided by the
// count, covariance accu[i] - mean * mean, eigen33, d = -((e0 c0 + e1 c1) + (e2 c2 + 0 * 1)).  Fewer than 4 inliers:
// the coefficients stay.  One workgroup: the points are staged in LDS, nine lanes of wave 0 run the dependent adds.
#define SG_REFIT_THREADS 1024u
#define SG_REFIT_STAGE 4096u
__global__ __launch_bounds__(SG_REFIT_THREADS) void k_sg_refit(SgParams p, SgHdr* __restrict__ h, int optimize,
                                                              const float4* __restrict__ pts,
                                                              const uint32_t* __restrict__ inl) {
  __shared__ float4 stage[SG_REFIT_STAGE];
  __shared__ float accu[9];
  const uint32_t tid = threadIdx.x, m = h->n_ransac_inl;
  const bool have = h->best_h >= 0;
  if (!have) return;  // (uniform)
  if (!optimize || m < 4) {
    if (tid < 4) h->coef_final[tid] = h->coef_ransac[tid];
    return;
  }
  // lane t: accu[t] += a * b with (a, b) = (x,x) (x,y) (x,z) (y,y) (y,z) (z,z), then (x,w) (y,w) (z,w): w = 1.0f, so
  // the product is the coordinate itself, exactly
  const int ia[9] = {0, 0, 0, 1, 1, 2, 0, 1, 2}, ib[9] = {0, 1, 2, 1, 2, 2, 3, 3, 3};
  const int my_a = tid < 9 ? ia[tid] : 0, my_b = tid < 9 ? ib[tid] : 3;
  const float* sf = reinterpret_cast<const float*>(stage);
  float acc = 0.0f;
  for (uint32_t s0 = 0; s0 < m; s0 += SG_REFIT_STAGE) {
    const uint32_t cnt = min(SG_REFIT_STAGE, m - s0);
    for (uint32_t k = tid; k < cnt; k += SG_REFIT_THREADS) stage[k] = pts[inl[s0 + k]];
    __syncthreads();
    if (tid < 9) {
#pragma unroll 8
      for (uint32_t k = 0; k < cnt; k++) acc += sf[4 * k + my_a] * sf[4 * k + my_b];
    }
    __syncthreads();
  }
  if (tid < 9) accu[tid] = acc / (float)m;
  __syncthreads();
  if (tid == 0) sg_refit_tail(h, accu);
}

// RULE refit, PFT_SUM_TREE: the nine sums as adjacent-pair trees in float over the inlier list padded with -0.0 (the
// exact additive identity, so the padding length does not change a bit) to a power of two; the products are rounded to
// float first.  T0 = the terms, T(k+1)[i] = Tk[2i] + Tk[2i+1].  Levels 0..3 are a thread's 8 points, 3..9 the wave's xor
// shuffles (a + b == b + a in IEEE, so both lanes of a pair hold the node), 9..11 the four waves in LDS: a tile of
// SG_RT_TILE inliers is one aligned subtree, whichever workgroup reduces it, and k_sg_refit_top takes the tile sums as
// the upper levels of the same tree.  So the bits do not depend on the launch shape.
#define SG_RT_THREADS 256u
#define SG_RT_PTS 8u
#define SG_RT_TILE (SG_RT_THREADS * SG_RT_PTS)
#define SG_RT_TOP 1024u
__device__ __forceinline__ float sg_pair_wave(float v) {
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) v = v + __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(SG_RT_THREADS) void k_sg_refit_tiles(const SgHdr* __restrict__ h, int optimize,
                                                                  const float4* __restrict__ pts,
                                                                  const uint32_t* __restrict__ inl,
                                                                  float* __restrict__ part) {
  __shared__ float sw[SG_RT_THREADS / WAVE][9];
  const uint32_t tid = threadIdx.x, m = h->n_ransac_inl;
  if (h->best_h < 0 || !optimize || m < 4) return;  // (uniform) k_sg_refit_top copies the coefficients
  const uint32_t ntile = (m + SG_RT_TILE - 1u) / SG_RT_TILE;
  for (uint32_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const uint32_t base = t * SG_RT_TILE + tid * SG_RT_PTS;
    float x[SG_RT_PTS], y[SG_RT_PTS], z[SG_RT_PTS];
    bool ok[SG_RT_PTS];
#pragma unroll
    for (uint32_t k = 0; k < SG_RT_PTS; k++) {
      ok[k] = base + k < m;
      const float4 q = ok[k] ? pts[inl[base + k]] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      x[k] = q.x;
      y[k] = q.y;
      z[k] = q.z;
    }
    float acc[9];
#pragma unroll
    for (int j = 0; j < 9; j++) {
      float tm[SG_RT_PTS];
#pragma unroll
      for (uint32_t k = 0; k < SG_RT_PTS; k++) {
        // (x,x) (x,y) (x,z) (y,y) (y,z) (z,z), then x, y, z (times w = 1.0f, exactly the coordinate)
        const float a = j < 3 ? x[k] : (j < 5 ? y[k] : (j == 5 ? z[k] : (j == 6 ? x[k] : (j == 7 ? y[k] : z[k]))));
        const float b = j == 0 ? x[k] : (j == 1 || j == 3 ? y[k] : (j == 2 || j == 4 || j == 5 ? z[k] : 1.0f));
        tm[k] = ok[k] ? a * b : -0.0f;
      }
      acc[j] = sg_pair_wave(((tm[0] + tm[1]) + (tm[2] + tm[3])) + ((tm[4] + tm[5]) + (tm[6] + tm[7])));
    }
    if (lane_id() == 0) {
#pragma unroll
      for (int j = 0; j < 9; j++) sw[wave_id()][j] = acc[j];
    }
    __syncthreads();
    if (tid < 9) part[(size_t)t * 9u + tid] = (sw[0][tid] + sw[1][tid]) + (sw[2][tid] + sw[3][tid]);
    __syncthreads();
  }
}

// pair tree over SG_RT_TOP values per moment, one per thread: the wave's shuffles, then the 16 wave sums; the nine
// results in threads 0..8
__device__ float sg_top_tree9(float (&v)[9], float (*sw)[9]) {
  const uint32_t tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 9; j++) v[j] = sg_pair_wave(v[j]);
  if (lane_id() == 0) {
#pragma unroll
    for (int j = 0; j < 9; j++) sw[wave_id()][j] = v[j];
  }
  __syncthreads();
  float r = -0.0f;
  if (tid < 9) {
    float a[SG_RT_TOP / WAVE];
#pragma unroll
    for (uint32_t w = 0; w < SG_RT_TOP / WAVE; w++) a[w] = sw[w][tid];
#pragma unroll
    for (uint32_t sz = SG_RT_TOP / WAVE; sz > 1u; sz >>= 1)
#pragma unroll
      for (uint32_t i = 0; i < sz / 2u; i++) a[i] = a[2u * i] + a[2u * i + 1u];
    r = a[0];
  }
  __syncthreads();
  return r;
}

// one workgroup: the tile sums as the upper levels of the tree (chunks of SG_RT_TOP tiles, then the chunk sums: up to
// 2^20 tiles = 2^31 inliers), then the one-lane tail of k_sg_refit
__global__ __launch_bounds__(SG_RT_TOP) void k_sg_refit_top(SgHdr* __restrict__ h, int optimize,
                                                            const float* __restrict__ part) {
  __shared__ float sw[SG_RT_TOP / WAVE][9];
  __shared__ float schunk[9][SG_RT_TOP];
  __shared__ float accu[9];
  const uint32_t tid = threadIdx.x, m = h->n_ransac_inl;
  if (h->best_h < 0) return;  // (uniform)
  if (!optimize || m < 4) {
    if (tid < 4) h->coef_final[tid] = h->coef_ransac[tid];
    return;
  }
  const uint32_t ntile = (m + SG_RT_TILE - 1u) / SG_RT_TILE, nchunk = (ntile + SG_RT_TOP - 1u) / SG_RT_TOP;
  float v[9];
  for (uint32_t c = 0; c < nchunk; c++) {
    const uint32_t t = c * SG_RT_TOP + tid;
#pragma unroll
    for (int j = 0; j < 9; j++) v[j] = t < ntile ? part[(size_t)t * 9u + j] : -0.0f;
    const float r = sg_top_tree9(v, sw);
    if (tid < 9) schunk[tid][c] = r;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 9; j++) v[j] = tid < nchunk ? schunk[j][tid] : -0.0f;
  const float acc = sg_top_tree9(v, sw);
  if (tid < 9) accu[tid] = acc / (float)m;
  __syncthreads();
  if (tid == 0) sg_refit_tail(h, accu);
}

// ---------------------------------------------------------------------------------------------------------------
// plane rounds (pft_segment_set_plane_rounds).  rnd[i], per INPUT index: SG_RND_INVALID = dropped by removeZeroPoints,
// SG_RND_KEPT = never removed, r = a final inlier of round r.  The inlier lists of any round are re-derived from it.
#define SG_RND_INVALID 0xFFu
#define SG_RND_KEPT 0xFEu
__global__ __launch_bounds__(SG_THREADS) void k_sg_round_init(uint32_t n, const uint8_t* __restrict__ flag,
                                                              uint8_t* __restrict__ rnd) {
  const uint32_t i = blockIdx.x * SG_THREADS + threadIdx.x;
  if (i < n) rnd[i] = flag[i] ? SG_RND_KEPT : SG_RND_INVALID;
}

// a fresh SACSegmentation::segment over n_r points: the RANSAC and sampler state of the header, not its error bits
__global__ void k_sg_round_begin(SgHdr* __restrict__ h, uint32_t n_r) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t err = h->err;
  SgHdr z = {};
  z.k = 1.0;
  z.best_count = -INT32_MAX;
  z.best_h = -1;
  z.n_valid = n_r;
  z.err = err;
  *h = z;
}

// final inliers of round r (flags over the round's cloud) -> rnd at their input indices
__global__ __launch_bounds__(SG_THREADS) void k_sg_round_mark(const SgHdr* __restrict__ h,
                                                              const uint8_t* __restrict__ flag,
                                                              const uint32_t* __restrict__ map, uint8_t* __restrict__ rnd,
                                                              uint32_t r) {
  const uint32_t i = blockIdx.x * SG_THREADS + threadIdx.x;
  if (i < h->n_valid && flag[i]) rnd[map[i]] = (uint8_t)r;
}

// flags over the input of round r's inliers: which = 0 the final ones, 1 the points of the round's cloud (valid, not
// removed before round r) within the distance of the round's best hypothesis c
__global__ __launch_bounds__(SG_THREADS) void k_sg_round_flags(uint32_t n, const uint8_t* __restrict__ rnd,
                                                               const float4* __restrict__ tx, uint32_t r, int which,
                                                               float4 c, float thr, uint8_t* __restrict__ flag,
                                                               uint32_t* __restrict__ tile) {
  const uint32_t i0 = blockIdx.x * SG_TILE + threadIdx.x * 4u;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t i = i0 + k;
    if (i >= n) break;
    const uint32_t v = rnd[i];
    const bool in = which == 0 ? v == r : (v != SG_RND_INVALID && v >= r && within(c, tx[i], thr));
    flag[i] = in ? 1 : 0;
  }
  sg_tile_count(flag, n, tile);
}

// ---------------------------------------------------------------------------------------------------------------
// 6. clustering over the survivors (m points, spts[j] in survivor order = ascending input index)
__global__ __launch_bounds__(SG_THREADS) void k_sg_bounds(const SgHdr* __restrict__ h, const float4* __restrict__ spts,
                                                          float* __restrict__ part) {
  __shared__ float sf[6][20];
  const uint32_t m = h->n_surv;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = blockIdx.x * SG_THREADS + threadIdx.x; i < m; i += gridDim.x * SG_THREADS) {
    const float4 q = spts[i];
    mn[0] = fminf(mn[0], q.x); mn[1] = fminf(mn[1], q.y); mn[2] = fminf(mn[2], q.z);
    mx[0] = fmaxf(mx[0], q.x); mx[1] = fmaxf(mx[1], q.y); mx[2] = fmaxf(mx[2], q.z);
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float lo = block_reduce<float>(mn[a], sf[a], OpMinF(), INFINITY);
    const float hi = block_reduce<float>(mx[a], sf[3 + a], OpMaxF(), -INFINITY);
    if (threadIdx.x == 0) {
      part[blockIdx.x * 6 + a] = lo;
      part[blockIdx.x * 6 + 3 + a] = hi;
    }
  }
}
__global__ __launch_bounds__(SG_THREADS) void k_sg_bounds2(SgHdr* __restrict__ h, const float* __restrict__ part,
                                                           uint32_t nparts) {
  __shared__ float sf[6][20];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t t = threadIdx.x; t < nparts; t += SG_THREADS)
    for (int a = 0; a < 3; a++) {
      mn[a] = fminf(mn[a], part[t * 6 + a]);
      mx[a] = fmaxf(mx[a], part[t * 6 + 3 + a]);
    }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    mn[a] = block_reduce<float>(mn[a], sf[a], OpMinF(), INFINITY);
    mx[a] = block_reduce<float>(mx[a], sf[3 + a], OpMaxF(), -INFINITY);
  }
  if (threadIdx.x == 0)
    for (int a = 0; a < 3; a++) {
      h->bmin[a] = mn[a];
      h->bmax[a] = mx[a];
    }
}

// Cell side s = tol / 2 * (1 + 2^-5).  Inside a cell the diagonal is sqrt(3) s = 0.893 tol < tol, so every point of a
// cell joins the cell's first point.  Two points within tol of each other differ by less than 2 / (1 + 2^-5) = 1.939 in
// exact scaled coordinates; the two roundings of (v - lo) * inv add at most 2^-22 U (U the largest scaled coordinate,
// at most 2^17 per axis, checked on the host) = 0.031, so the computed difference stays below 2 and the pair is at most
// 2 cells apart on every axis: the 5 x 5 x 5 block holds every neighbour.
__device__ __forceinline__ uint32_t cell_coord(float v, float lo, float inv, uint32_t nmax) {
  const float f = floorf((v - lo) * inv);
  if (!(f > 0.0f)) return 0u;
  const uint32_t c = (uint32_t)fminf(f, (float)(nmax - 1u));
  return c < nmax ? c : nmax - 1u;
}

// cell key of every survivor (cell side tol / 2), value = survivor index
__global__ __launch_bounds__(SG_THREADS) void k_sg_cellkey(SgParams p, const SgHdr* __restrict__ h,
                                                           const float4* __restrict__ spts, uint32_t* __restrict__ key,
                                                           uint32_t* __restrict__ val, uint32_t m) {
  const uint32_t i = blockIdx.x * SG_THREADS + threadIdx.x;
  if (i >= m) return;
  const float4 q = spts[i];
  const uint32_t ix = cell_coord(q.x, h->bmin[0], p.inv_cell, p.nx);
  const uint32_t iy = cell_coord(q.y, h->bmin[1], p.inv_cell, p.ny);
  const uint32_t iz = cell_coord(q.z, h->bmin[2], p.inv_cell, p.nz);
  key[i] = ix + p.nx * (iy + p.ny * iz);
  val[i] = i;
}

// run heads of the sorted keys, per tile; then (k_sg_cells) cell ids, cell starts, the sorted points and the
// within-cell forest: every point hangs under its cell's first (= smallest) survivor index
__global__ __launch_bounds__(SG_THREADS) void k_sg_heads(const uint32_t* __restrict__ skey, uint32_t m,
                                                         uint8_t* __restrict__ head, uint32_t* __restrict__ tile) {
  const uint32_t i0 = blockIdx.x * SG_TILE + threadIdx.x * 4u;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t j = i0 + k;
    if (j < m) head[j] = (j == 0 || skey[j - 1] != skey[j]) ? 1 : 0;
  }
  __syncthreads();
  sg_tile_count(head, m, tile);
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_cells(const uint32_t* __restrict__ skey,
                                                         const uint32_t* __restrict__ sval, uint32_t m,
                                                         const uint8_t* __restrict__ head,
                                                         const uint32_t* __restrict__ tile,
                                                         uint32_t* __restrict__ cell_start, uint32_t* __restrict__ cell_key,
                                                         const float4* __restrict__ spts, float4* __restrict__ sorted,
                                                         uint32_t* __restrict__ cell_of) {
  __shared__ uint32_t su[20];
  const uint32_t t = blockIdx.x, i0 = t * SG_TILE + threadIdx.x * 4u;
  uint32_t f[4], c = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    f[k] = (i0 + k < m) ? head[i0 + k] : 0u;
    c += f[k];
  }
  uint32_t tot;
  uint32_t run = tile[t] + block_excl_scan<uint32_t>(c, su, &tot);  // heads before i0
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t j = i0 + k;
    if (j >= m) break;
    if (f[k]) {
      cell_start[run] = j;
      cell_key[run] = skey[j];
      run++;
    }
    cell_of[j] = run - 1u;
    sorted[j] = spts[sval[j]];
  }
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_forest(const uint32_t* __restrict__ sval, uint32_t m,
                                                          const uint32_t* __restrict__ cell_of,
                                                          const uint32_t* __restrict__ cell_start,
                                                          uint32_t* __restrict__ parent) {
  const uint32_t j = blockIdx.x * SG_THREADS + threadIdx.x;
  if (j >= m) return;
  parent[sval[j]] = sval[cell_start[cell_of[j]]];
}

__device__ __forceinline__ uint32_t uf_load(const uint32_t* a) {
  return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// parent[x] <= x everywhere; a root is its component's smallest survivor index
__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x) {
  uint32_t p = uf_load(parent + x);
  while (p != x) {
    const uint32_t g = uf_load(parent + p);
    if (g != p) atomicMin(parent + x, g);  // path halving: any ancestor is a valid parent
    x = p;
    p = g;
  }
  return x;
}
__device__ __forceinline__ void uf_union(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a > b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicCAS(parent + b, b, a);  // hook the larger root under the smaller
    if (old == b) return;
    b = old;
  }
}

// RULE link: two points are connected iff ((dx^2 + dy^2) + dz^2) < (float)(tol^2).  Work item = (cell, one of the 62
// neighbour offsets of the 5x5x5 block that come after it): the pair is tested until one pair of points connects.
__global__ __launch_bounds__(SG_THREADS) void k_sg_link(SgParams p, const SgHdr* __restrict__ h,
                                                        const uint32_t* __restrict__ cell_start,
                                                        const uint32_t* __restrict__ cell_key,
                                                        const uint32_t* __restrict__ sval,
                                                        const float4* __restrict__ sorted, uint32_t m,
                                                        uint32_t* __restrict__ parent) {
  const uint32_t nc = h->n_cells;
  const uint64_t total = (uint64_t)nc * 62u;
  for (uint64_t w = (uint64_t)blockIdx.x * SG_THREADS + threadIdx.x; w < total; w += (uint64_t)gridDim.x * SG_THREADS) {
    const uint32_t c = (uint32_t)(w / 62u), L = 63u + (uint32_t)(w % 62u);
    const int dz = (int)(L / 25u) - 2, dy = (int)((L / 5u) % 5u) - 2, dx = (int)(L % 5u) - 2;
    const uint32_t key = cell_key[c];
    const int ix = (int)(key % p.nx), iy = (int)((key / p.nx) % p.ny), iz = (int)(key / p.nx / p.ny);
    const int jx = ix + dx, jy = iy + dy, jz = iz + dz;
    if (jx < 0 || jy < 0 || jz < 0 || jx >= (int)p.nx || jy >= (int)p.ny || jz >= (int)p.nz) continue;
    const uint32_t key2 = (uint32_t)jx + p.nx * ((uint32_t)jy + p.ny * (uint32_t)jz);
    uint32_t lo = c + 1u, hi = nc;  // key2 > key: search the cells after c
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (cell_key[mid] < key2) lo = mid + 1u; else hi = mid;
    }
    if (lo >= nc || cell_key[lo] != key2) continue;
    const uint32_t c2 = lo;
    const uint32_t a0 = cell_start[c], a1 = c + 1u < nc ? cell_start[c + 1u] : m;
    const uint32_t b0 = cell_start[c2], b1 = c2 + 1u < nc ? cell_start[c2 + 1u] : m;
    const uint32_t fa = sval[a0], fb = sval[b0];
    if (uf_find(parent, fa) == uf_find(parent, fb)) continue;
    bool linked = false;
    for (uint32_t a = a0; a < a1 && !linked; a++) {
      const float4 qa = sorted[a];
      for (uint32_t b = b0; b < b1; b++) {
        const float4 qb = sorted[b];
        const float ddx = qa.x - qb.x, ddy = qa.y - qb.y, ddz = qa.z - qb.z;
        if ((ddx * ddx + ddy * ddy) + ddz * ddz < p.tol2) {
          linked = true;
          break;
        }
      }
    }
    if (linked) uf_union(parent, fa, fb);
  }
}

// final labels (root = smallest survivor index of the component) and component sizes
__global__ __launch_bounds__(SG_THREADS) void k_sg_label(uint32_t m, uint32_t* __restrict__ parent,
                                                         uint32_t* __restrict__ label, uint32_t* __restrict__ csize) {
  const uint32_t j = blockIdx.x * SG_THREADS + threadIdx.x;
  if (j >= m) return;
  const uint32_t r = uf_find(parent, j);
  label[j] = r;
  atomicAdd(&csize[r], 1u);
}

// RULE size: a component is kept iff min <= size <= max; flags of the kept roots
__global__ __launch_bounds__(SG_THREADS) void k_sg_roots(SgParams p, uint32_t m, const uint32_t* __restrict__ label,
                                                         const uint32_t* __restrict__ csize, uint8_t* __restrict__ flag,
                                                         uint32_t* __restrict__ tile) {
  const uint32_t i0 = blockIdx.x * SG_TILE + threadIdx.x * 4u;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t j = i0 + k;
    if (j < m) flag[j] = (label[j] == j && csize[j] >= p.min_size && csize[j] <= p.max_size) ? 1 : 0;
  }
  __syncthreads();
  sg_tile_count(flag, m, tile);
}

// RULE order: clusters by size descending, ties by smallest index ascending -- key max_size - size, stable sort of
// the roots (which are in ascending order)
__global__ __launch_bounds__(SG_THREADS) void k_sg_order_keys(SgParams p, uint32_t nc, const uint32_t* __restrict__ roots,
                                                              const uint32_t* __restrict__ csize,
                                                              uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t r = blockIdx.x * SG_THREADS + threadIdx.x;
  if (r >= nc) return;
  key[r] = p.max_size - csize[roots[r]];
  val[r] = roots[r];
}

// cluster rank of every root, the sizes in cluster order
__global__ __launch_bounds__(SG_THREADS) void k_sg_rank(uint32_t nc, const uint32_t* __restrict__ oroot,
                                                        const uint32_t* __restrict__ csize, uint32_t* __restrict__ crank,
                                                        uint32_t* __restrict__ sizes) {
  const uint32_t r = blockIdx.x * SG_THREADS + threadIdx.x;
  if (r >= nc) return;
  crank[oroot[r]] = r;
  sizes[r] = csize[oroot[r]];
}

// sort key of every survivor: its cluster's rank, nc for the dropped ones
__global__ __launch_bounds__(SG_THREADS) void k_sg_member_keys(uint32_t m, uint32_t nc, const uint32_t* __restrict__ label,
                                                               const uint32_t* __restrict__ crank,
                                                               uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t j = blockIdx.x * SG_THREADS + threadIdx.x;
  if (j >= m) return;
  const uint32_t r = crank[label[j]];
  key[j] = r < nc ? r : nc;
  val[j] = j;
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_output(uint32_t total, const uint32_t* __restrict__ sval,
                                                          const uint32_t* __restrict__ surv_in,
                                                          const pft_point_xyzrgba* __restrict__ in,
                                                          int32_t* __restrict__ out_idx,
                                                          pft_point_xyzrgba* __restrict__ out_pts) {
  const uint32_t q = blockIdx.x * SG_THREADS + threadIdx.x;
  if (q >= total) return;
  const uint32_t i = surv_in[sval[q]];
  out_idx[q] = (int32_t)i;
  const float4* s = reinterpret_cast<const float4*>(in + i);
  float4* o = reinterpret_cast<float4*>(out_pts + q);
  o[0] = s[0];
  o[1] = s[1];
}

// ---------------------------------------------------------------------------------------------------------------
// host side
#define SG_NEV 96

struct SgBufs {
  pft_point_xyzrgba* in_own;
  float4* tx;        // transformed, input order
  uint8_t* flag;     // removeZero / inlier flags
  uint8_t* flag2;    // survivor flags
  uint32_t* tile;
  uint32_t* tile2;
  uint32_t* comp_idx;   // compacted -> input index
  float4* comp_pts;     // compacted transformed points
  uint32_t* inl_idx;    // best-hypothesis inliers (compacted indices)
  uint32_t* fin_idx;    // final inliers (input indices)
  uint32_t* surv_in;    // survivor -> input index
  float4* spts;         // survivor points (transformed)
  uint32_t* key[2];
  uint32_t* val[2];
  uint32_t* hist;
  float4* sorted;
  uint32_t* cell_start;
  uint32_t* cell_key;
  uint32_t* cell_of;
  uint32_t* parent;
  uint32_t* label;
  uint32_t* csize;
  uint32_t* roots;
  uint32_t* crank;
  uint32_t* sizes;
  float* bpart;
  int32_t* out_idx;
  pft_point_xyzrgba* out_pts;
  uint8_t* rnd;         // plane rounds: per input index, the round that removed the point
  float* refit_part;    // tree-order refit: nine sums per tile of SG_RT_TILE inliers
};

struct pft_segment {
  pft_segment_config cfg;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  size_t cap = 0;
  SgBufs b = {};
  SgHdr* hdr = nullptr;
  SgHdr* host_hdr = nullptr;  // pinned copy
  SgSampler smp = {};
  SgHyp hyp = {};
  uint32_t hmax = 0;
  std::vector<hipEvent_t> ev;  // SG_NEV at creation; plane rounds add more on demand
  std::vector<int> ev_stage;
  int nev = 0;
  // plane rounds and the refit's summation order (setters; the defaults are the single plane, PCL's chains)
  int max_planes = 1;
  double min_fraction = 0.0;
  int refit_order = PFT_SUM_PCL;
  uint32_t refit_grid = 0;     // PFT_SEGMENT_REFIT_GRID, latched at creation: workgroups of the tile launch (0 = by size)
  uint32_t hyp_rounds = 1;     // rounds the hypothesis buffers hold
  std::vector<SgHdr> rounds;   // header of every round the last apply ran (one synthetic entry when none ran)
  bool by_rounds = false;      // the last apply ran the round loop: inlier lists come from b.rnd
  size_t n_rounds = 0, n_planes = 0;
  int stopped_by = PFT_ROUNDS_STOP_FRACTION;
  // results of the last apply
  bool have_result = false;
  SgHdr res = {};
  size_t n_in = 0;
  std::vector<uint32_t> sizes;
  double last_ms = 0.0, stage_ms[PFT_SEGMENT_STAGES] = {};
};

static void free_buffers(pft_segment* s) {
  SgBufs& b = s->b;
  pft_dfree(b.in_own); pft_dfree(b.tx); pft_dfree(b.flag); pft_dfree(b.flag2); pft_dfree(b.tile); pft_dfree(b.tile2); pft_dfree(b.comp_idx);
  pft_dfree(b.comp_pts); pft_dfree(b.inl_idx); pft_dfree(b.fin_idx); pft_dfree(b.surv_in); pft_dfree(b.spts);
  for (int k = 0; k < 2; k++) {
    pft_dfree(b.key[k]);
    pft_dfree(b.val[k]);
  }
  pft_dfree(b.hist); pft_dfree(b.sorted); pft_dfree(b.cell_start); pft_dfree(b.cell_key); pft_dfree(b.cell_of); pft_dfree(b.parent);
  pft_dfree(b.label); pft_dfree(b.csize); pft_dfree(b.roots); pft_dfree(b.crank); pft_dfree(b.sizes); pft_dfree(b.bpart); pft_dfree(b.out_idx);
  pft_dfree(b.out_pts); pft_dfree(b.rnd); pft_dfree(b.refit_part);
  s->cap = 0;
}

static int ensure_capacity(pft_segment* s, size_t n) {
  if (n <= s->cap) return PFT_OK;
  if (s->stream) PFT_HIPCHK(s, hipStreamSynchronize(s->stream));
  free_buffers(s);
  size_t cap = n < SG_TILE ? SG_TILE : n;
  cap = (cap + SG_TILE - 1) / SG_TILE * SG_TILE;
  const size_t nt = cap / SG_TILE;
  SgBufs& b = s->b;
  PFT_HIPCHK(s, pft_dalloc(&b.in_own, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.tx, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.flag, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.flag2, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.tile, nt));
  PFT_HIPCHK(s, pft_dalloc(&b.tile2, nt));
  PFT_HIPCHK(s, pft_dalloc(&b.comp_idx, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.comp_pts, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.inl_idx, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.fin_idx, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.surv_in, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.spts, cap));
  for (int k = 0; k < 2; k++) {
    PFT_HIPCHK(s, pft_dalloc(&b.key[k], cap));
    PFT_HIPCHK(s, pft_dalloc(&b.val[k], cap));
  }
  PFT_HIPCHK(s, pft_dalloc(&b.hist, 256 * nt + 256));
  PFT_HIPCHK(s, pft_dalloc(&b.sorted, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.cell_start, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.cell_key, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.cell_of, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.parent, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.label, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.csize, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.roots, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.crank, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.sizes, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.bpart, 6 * 1024));
  PFT_HIPCHK(s, pft_dalloc(&b.out_idx, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.out_pts, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.rnd, cap));
  PFT_HIPCHK(s, pft_dalloc(&b.refit_part, 9 * (cap / SG_RT_TILE + 1)));
  s->cap = cap;
  return PFT_OK;
}

extern "C" void pft_segment_default_config(pft_segment_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->abi_version = PFT_ABI_VERSION;
  for (int k = 0; k < 16; k++) c->transform[k] = (k % 5 == 0) ? 1.0f : 0.0f;
  c->plane_enable = 1;                // create_model_planar_segmentation.cpp:161-167
  c->max_iterations = 1000;
  c->distance_threshold = 0.015;
  c->probability = 0.99;              // SampleConsensus::probability_ default
  c->seed = 12345u;                   // SampleConsensusModel(random = false)
  c->optimize_coefficients = 1;       // SACSegmentation default
  c->box_enable[0] = c->box_enable[1] = 1;  // PassThrough y then x (:178-188); create_model.cpp adds z
  c->box_min[0] = 0.45f;  c->box_max[0] = 1.1f;   // params.yaml segm_limits, "normal table"
  c->box_min[1] = -0.6f;  c->box_max[1] = 0.6f;
  c->box_min[2] = -0.17f; c->box_max[2] = 0.2f;
  c->cluster_tolerance = 0.02;        // :186-188
  c->min_cluster_size = 500;
  c->max_cluster_size = 25000;
  c->max_points = 960 * 540;          // Kinect2 qhd
}

extern "C" int pft_segment_create(const pft_segment_config* cfg, pft_segment** out) {
  if (!cfg || !out) return PFT_ERR_INVALID_ARG;
  *out = nullptr;
  if (cfg->abi_version != PFT_ABI_VERSION) return PFT_ERR_INVALID_ARG;
  if (cfg->max_iterations < 0 || cfg->max_iterations > SG_MAX_ITER) return PFT_ERR_INVALID_ARG;
  if (!(cfg->distance_threshold >= 0.0) || !(cfg->probability > 0.0 && cfg->probability < 1.0)) return PFT_ERR_INVALID_ARG;
  if (!(cfg->cluster_tolerance > 0.0) || cfg->min_cluster_size < 0 || cfg->max_cluster_size < 1) return PFT_ERR_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PFT_ERR_NO_DEVICE;  // no CPU path
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return PFT_ERR_INVALID_ARG;
  if (hipSetDevice(cfg->device_id) != hipSuccess) return PFT_ERR_NO_DEVICE;
  pft_segment* s = new pft_segment();
  s->cfg = *cfg;
  bool ok = true;
  if (cfg->stream_is_external) {
    s->stream = reinterpret_cast<hipStream_t>(cfg->stream);
  } else {
    ok = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) == hipSuccess;
    s->own_stream = ok;
  }
  s->ev.assign(SG_NEV, nullptr);
  s->ev_stage.assign(SG_NEV, 0);
  for (int k = 0; ok && k < SG_NEV; k++) ok = hipEventCreate(&s->ev[k]) == hipSuccess;
  if (const char* g = getenv("PFT_SEGMENT_REFIT_GRID")) s->refit_grid = (uint32_t)std::max(0, atoi(g));
  s->hmax = ((uint32_t)cfg->max_iterations + 1u + SG_BATCH - 1u) / SG_BATCH * SG_BATCH;
  if (ok)
    ok = pft_dalloc(&s->hdr, 1) == hipSuccess &&
         hipHostMalloc(reinterpret_cast<void**>(&s->host_hdr), sizeof(SgHdr), hipHostMallocDefault) == hipSuccess &&
         pft_dalloc(&s->smp.mt, MT_N) == hipSuccess && pft_dalloc(&s->smp.mk, SG_MAPCAP) == hipSuccess &&
         pft_dalloc(&s->smp.mv, SG_MAPCAP) == hipSuccess && pft_dalloc(&s->hyp.sample, 3 * (size_t)s->hmax) == hipSuccess &&
         pft_dalloc(&s->hyp.coef, s->hmax) == hipSuccess && pft_dalloc(&s->hyp.count, s->hmax) == hipSuccess;
  if (ok) ok = ensure_capacity(s, cfg->max_points ? cfg->max_points : SG_TILE) == PFT_OK;
  if (!ok) {
    pft_segment_destroy(s);
    return PFT_ERR_HIP;
  }
  *out = s;
  return PFT_OK;
}

extern "C" void pft_segment_destroy(pft_segment* s) {
  if (!s) return;
  if (s->stream) hipStreamSynchronize(s->stream);
  free_buffers(s);
  pft_dfree(s->hdr);
  if (s->host_hdr) hipHostFree(s->host_hdr);
  pft_dfree(s->smp.mt); pft_dfree(s->smp.mk); pft_dfree(s->smp.mv);
  pft_dfree(s->hyp.sample); pft_dfree(s->hyp.coef); pft_dfree(s->hyp.count);
  for (hipEvent_t e : s->ev)
    if (e) hipEventDestroy(e);
  if (s->own_stream && s->stream) hipStreamDestroy(s->stream);
  delete s;
}

extern "C" const char* pft_segment_last_error_string(const pft_segment* s) { return s ? s->err.c_str() : "null handle"; }

// an event after the launches of one stage: the time since the previous event is booked to that stage (stage -1: an
// event right after a host synchronisation, whose gap is host idle time and booked nowhere)
static int mark(pft_segment* s, int stage) {
  if (s->nev >= (int)s->ev.size()) {  // (plane rounds only: one apply of the single plane needs at most 3 per batch + 16)
    hipEvent_t e = nullptr;
    PFT_HIPCHK(s, hipEventCreate(&e));
    s->ev.push_back(e);
    s->ev_stage.push_back(0);
  }
  PFT_HIPCHK(s, hipEventRecord(s->ev[s->nev], s->stream));
  s->ev_stage[s->nev] = stage;
  s->nev++;
  return PFT_OK;
}
#define MARK(st)                         \
  do {                                   \
    int r_ = mark(s, (st));              \
    if (r_ != PFT_OK) return r_;         \
  } while (0)

enum { ST_COMPACT = 0, ST_SAMPLE, ST_SCORE, ST_REPLAY, ST_REFIT, ST_CLUSTER, ST_OUTPUT };

static int read_hdr(pft_segment* s) {
  PFT_HIPCHK(s, hipMemcpyAsync(s->host_hdr, s->hdr, sizeof(SgHdr), hipMemcpyDeviceToHost, s->stream));
  PFT_HIPCHK(s, hipStreamSynchronize(s->stream));
  PFT_HIPCHK(s, hipGetLastError());
  return PFT_OK;
}

// 3. one SACSegmentation::segment over the cloud `pts` (its size in the header's n_valid, at most n_max): RANSAC in
// batches, the inliers of the best hypothesis, the refit.  Leaves coef_ransac / coef_final / n_ransac_inl in the header.
static int plane_stage(pft_segment* s, const SgParams& p, const SgHyp& hyp, const float4* pts, uint32_t n_max,
                       uint32_t ntiles) {
  const pft_segment_config& c = s->cfg;
  hipStream_t st = s->stream;
  SgBufs& b = s->b;
  const uint32_t* n_valid = &s->hdr->n_valid;
  // every launch after the deciding batch returns at once
  PFT_HIPCHK(s, hipMemsetAsync(hyp.count, 0, s->hmax * sizeof(uint32_t), st));
  const uint32_t nscore = (n_max + SG_THREADS * SG_SCORE_PTS - 1) / (SG_THREADS * SG_SCORE_PTS);
  for (uint32_t bt = 0; bt * SG_BATCH < s->hmax; bt++) {
    hipLaunchKernelGGL(k_sg_sample, dim3(1), dim3(SG_THREADS), 0, st, p, s->hdr, s->smp, hyp, pts, bt);
    MARK(ST_SAMPLE);
    hipLaunchKernelGGL(k_sg_score, dim3(nscore), dim3(SG_THREADS), 0, st, p, (const SgHdr*)s->hdr, hyp, pts, bt);
    MARK(ST_SCORE);
    hipLaunchKernelGGL(k_sg_replay, dim3(1), dim3(64), 0, st, p, s->hdr, hyp, bt);
    MARK(ST_REPLAY);
  }
  // inliers of the best hypothesis, refit
  hipLaunchKernelGGL(k_sg_select, dim3(ntiles), dim3(SG_THREADS), 0, st, p, (const SgHdr*)s->hdr, 0, pts, b.flag,
                     b.tile, (uint8_t*)nullptr, (uint32_t*)nullptr);
  hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, b.tile, ntiles, n_valid, &s->hdr->n_ransac_inl);
  hipLaunchKernelGGL(k_sg_emit, dim3(ntiles), dim3(SG_THREADS), 0, st, b.flag, n_max, n_valid, b.tile,
                     (const uint32_t*)nullptr, b.inl_idx, (const float4*)nullptr, (float4*)nullptr);
  if (s->refit_order == PFT_SUM_TREE) {
    // at most one workgroup per tile of the largest inlier list; the tiles are walked grid-stride, so any grid is valid
    uint32_t grid = std::min<uint32_t>((n_max + SG_RT_TILE - 1) / SG_RT_TILE, 1024u);
    if (s->refit_grid) grid = s->refit_grid;
    hipLaunchKernelGGL(k_sg_refit_tiles, dim3(std::max(grid, 1u)), dim3(SG_RT_THREADS), 0, st, (const SgHdr*)s->hdr,
                       c.optimize_coefficients, pts, (const uint32_t*)b.inl_idx, b.refit_part);
    hipLaunchKernelGGL(k_sg_refit_top, dim3(1), dim3(SG_RT_TOP), 0, st, s->hdr, c.optimize_coefficients,
                       (const float*)b.refit_part);
  } else {
    hipLaunchKernelGGL(k_sg_refit, dim3(1), dim3(SG_REFIT_THREADS), 0, st, p, s->hdr, c.optimize_coefficients, pts,
                       (const uint32_t*)b.inl_idx);
  }
  MARK(ST_REFIT);
  return PFT_OK;
}

// the plane rounds of cluster_euclid.cpp:59-85: RULE rounds.  The remaining cloud ping-pongs between (comp_pts,
// comp_idx) and two clustering buffers that are idle until stage 6; the host reads the header once per round for the
// remaining count, which sizes the next round's grids and decides the stop.
static int plane_rounds(pft_segment* s, const SgParams& p, uint32_t n, const float4** cpts, const uint32_t** cidx,
                        uint32_t* n_left) {
  hipStream_t st = s->stream;
  SgBufs& b = s->b;
  SgHdr* H = s->host_hdr;
  SgParams pr = p;  // the rounds remove planes only: the box is stage 5, after the loop
  for (int a = 0; a < 3; a++) pr.box_enable[a] = 0;
  hipLaunchKernelGGL(k_sg_round_init, dim3((n + SG_THREADS - 1) / SG_THREADS), dim3(SG_THREADS), 0, st, n,
                     (const uint8_t*)b.flag, b.rnd);
  MARK(ST_COMPACT);
  int r = read_hdr(s);
  if (r != PFT_OK) return r;
  MARK(-1);
  const uint32_t nr = H->n_valid;
  uint32_t remaining = nr;
  float4* pts[2] = {b.comp_pts, b.sorted};
  uint32_t* idx[2] = {b.comp_idx, b.cell_of};
  int cur = 0;
  for (;;) {
    // RULE rounds: the reference's cloud_filtered->points.size() > 0.3 * nr_points, a double product and compare
    if (!((double)remaining > s->min_fraction * (double)nr)) {
      s->stopped_by = PFT_ROUNDS_STOP_FRACTION;
      break;
    }
    if ((int)s->n_rounds >= s->max_planes) {  // this library's cap; the reference has none
      s->stopped_by = PFT_ROUNDS_STOP_MAX_PLANES;
      break;
    }
    const uint32_t rd = (uint32_t)s->n_rounds;
    const uint32_t nt = (remaining + SG_TILE - 1) / SG_TILE;
    SgHyp hyp = s->hyp;
    hyp.sample += 3 * (size_t)rd * s->hmax;
    hyp.coef += (size_t)rd * s->hmax;
    hyp.count += (size_t)rd * s->hmax;
    hipLaunchKernelGGL(k_sg_round_begin, dim3(1), dim3(64), 0, st, s->hdr, remaining);
    MARK(ST_COMPACT);
    r = plane_stage(s, pr, hyp, pts[cur], remaining, nt);
    if (r != PFT_OK) return r;
    // the round's final inliers leave the cloud (ExtractIndices negative): marked in rnd, the rest compacted
    hipLaunchKernelGGL(k_sg_select, dim3(nt), dim3(SG_THREADS), 0, st, pr, (const SgHdr*)s->hdr, 1,
                       (const float4*)pts[cur], b.flag, b.tile, b.flag2, b.tile2);
    hipLaunchKernelGGL(k_sg_round_mark, dim3((remaining + SG_THREADS - 1) / SG_THREADS), dim3(SG_THREADS), 0, st,
                       (const SgHdr*)s->hdr, (const uint8_t*)b.flag, (const uint32_t*)idx[cur], b.rnd, rd);
    hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, b.tile, nt, &s->hdr->n_valid, &s->hdr->n_fin);
    hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, b.tile2, nt, &s->hdr->n_valid, &s->hdr->n_surv);
    hipLaunchKernelGGL(k_sg_emit, dim3(nt), dim3(SG_THREADS), 0, st, b.flag2, remaining, &s->hdr->n_valid, b.tile2,
                       (const uint32_t*)idx[cur], idx[cur ^ 1], (const float4*)pts[cur], pts[cur ^ 1]);
    MARK(ST_COMPACT);
    r = read_hdr(s);
    if (r != PFT_OK) return r;
    MARK(-1);
    if (H->err & SG_ERR_MAP) {
      s->err = "RANSAC: the sparse map of drawIndexSample's swaps is full (too many degenerate samples)";
      return PFT_ERR_CAPACITY;
    }
    s->rounds.push_back(*H);
    s->n_rounds++;
    if (H->best_h < 0 || H->n_fin == 0) {  // the reference's break: nothing is removed
      s->stopped_by = PFT_ROUNDS_STOP_NO_PLANE;
      break;
    }
    s->n_planes++;
    remaining = H->n_surv;
    cur ^= 1;
  }
  // stages 4 + 5 see the remaining cloud with no plane left to remove
  hipLaunchKernelGGL(k_sg_round_begin, dim3(1), dim3(64), 0, st, s->hdr, remaining);
  MARK(ST_COMPACT);
  *cpts = pts[cur];
  *cidx = idx[cur];
  *n_left = remaining;
  return PFT_OK;
}

static int run_pipeline(pft_segment* s, const pft_point_xyzrgba* d_in, uint32_t n) {
  const pft_segment_config& c = s->cfg;
  hipStream_t st = s->stream;
  SgBufs& b = s->b;
  SgParams p = {};
  p.n = n;
  p.transform_enable = c.transform_enable;
  for (int k = 0; k < 12; k++) p.T[k] = c.transform[k];
  p.zero_thr = float_bound_below(0.01);
  p.dist_thr = float_bound_below(c.distance_threshold);
  p.log_probability = log(1.0 - c.probability);
  p.max_iterations = c.max_iterations;
  p.seed = c.seed;
  for (int a = 0; a < 3; a++) {
    p.box_enable[a] = c.box_enable[a];
    p.box_min[a] = c.box_min[a];
    p.box_max[a] = c.box_max[a];
  }
  p.tol2 = (float)(c.cluster_tolerance * c.cluster_tolerance);
  p.inv_cell = (float)(2.0 / (c.cluster_tolerance * SG_CELL_SLACK));
  p.min_size = (uint32_t)c.min_cluster_size;
  p.max_size = (uint32_t)c.max_cluster_size;
  const uint32_t ntiles = (n + SG_TILE - 1) / SG_TILE;
  SgHdr h0 = {};
  h0.k = 1.0;
  h0.best_count = -INT32_MAX;
  h0.best_h = -1;
  s->nev = 0;
  PFT_HIPCHK(s, hipMemcpyAsync(s->hdr, &h0, sizeof(SgHdr), hipMemcpyHostToDevice, st));
  MARK(ST_COMPACT);
  // 1 + 2: transform, removeZeroPoints, compaction (indices into the input, transformed points)
  hipLaunchKernelGGL(k_sg_zero, dim3(ntiles), dim3(SG_THREADS), 0, st, p, d_in, b.tx, b.flag, b.tile);
  hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, b.tile, ntiles, (const uint32_t*)nullptr, &s->hdr->n_valid);
  hipLaunchKernelGGL(k_sg_emit, dim3(ntiles), dim3(SG_THREADS), 0, st, b.flag, n, (const uint32_t*)nullptr, b.tile,
                     (const uint32_t*)nullptr, b.comp_idx, b.tx, b.comp_pts);
  MARK(ST_COMPACT);
  const uint32_t* n_valid = &s->hdr->n_valid;
  // the cloud stages 4 + 5 read: the removeZeroPoints output, or what the plane rounds left of it
  const float4* cpts = b.comp_pts;
  const uint32_t* cidx = b.comp_idx;
  uint32_t n45 = n, ntiles45 = ntiles;
  s->rounds.clear();
  s->n_rounds = s->n_planes = 0;
  s->stopped_by = PFT_ROUNDS_STOP_FRACTION;
  s->by_rounds = c.plane_enable && !(s->max_planes == 1 && s->min_fraction == 0.0);
  if (c.plane_enable && !s->by_rounds) {
    int r = plane_stage(s, p, s->hyp, b.comp_pts, n, ntiles);
    if (r != PFT_OK) return r;
  } else if (c.plane_enable) {
    int r = plane_rounds(s, p, n, &cpts, &cidx, &n45);
    if (r != PFT_OK) return r;
    ntiles45 = std::max((n45 + SG_TILE - 1) / SG_TILE, 1u);  // (nothing left: the kernels see n_valid = 0)
  }
  // 4 + 5: ExtractIndices negative, PassThrough box (no plane: every point is a non-inlier)
  hipLaunchKernelGGL(k_sg_select, dim3(ntiles45), dim3(SG_THREADS), 0, st, p, (const SgHdr*)s->hdr, 1, cpts, b.flag,
                     b.tile, b.flag2, b.tile2);
  hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, b.tile, ntiles45, n_valid, &s->hdr->n_fin);
  hipLaunchKernelGGL(k_sg_emit, dim3(ntiles45), dim3(SG_THREADS), 0, st, b.flag, n45, n_valid, b.tile, cidx, b.fin_idx,
                     (const float4*)nullptr, (float4*)nullptr);
  hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, b.tile2, ntiles45, n_valid, &s->hdr->n_surv);
  hipLaunchKernelGGL(k_sg_emit, dim3(ntiles45), dim3(SG_THREADS), 0, st, b.flag2, n45, n_valid, b.tile2, cidx, b.surv_in,
                     cpts, b.spts);
  const uint32_t nbparts = 1024;
  hipLaunchKernelGGL(k_sg_bounds, dim3(nbparts), dim3(SG_THREADS), 0, st, (const SgHdr*)s->hdr, (const float4*)b.spts,
                     b.bpart);
  hipLaunchKernelGGL(k_sg_bounds2, dim3(1), dim3(SG_THREADS), 0, st, s->hdr, (const float*)b.bpart, nbparts);
  MARK(ST_COMPACT);
  int r = read_hdr(s);  // the survivor count and their bounds size the clustering
  if (r != PFT_OK) return r;
  SgHdr* H = s->host_hdr;
  if (H->err & SG_ERR_MAP) {
    s->err = "RANSAC: the sparse map of drawIndexSample's swaps is full (too many degenerate samples)";
    return PFT_ERR_CAPACITY;
  }
  const uint32_t m = H->n_surv;
  uint32_t nc = 0, total = 0;
  s->sizes.clear();
  MARK(-1);  // host round trip: booked to no stage
  // RULE size: no cluster can be kept when min > max or when there are fewer survivors than min
  const bool cluster = m > 0 && p.min_size <= p.max_size && m >= p.min_size;
  if (cluster) {
    uint64_t dims[3];
    for (int a = 0; a < 3; a++) {
      const float ext = (H->bmax[a] - H->bmin[a]) * p.inv_cell;
      if (!(ext < 4.0e9f)) {
        s->err = "clustering: survivor bounding box too large for the cell grid (non-finite or far points)";
        return PFT_ERR_CAPACITY;
      }
      dims[a] = (uint64_t)floorf(ext) + 1u;
      if (dims[a] > SG_MAX_AXIS_CELLS) {
        s->err = "clustering: the survivors' bounding box spans more than 2^17 cells of side tolerance / 2 on one axis";
        return PFT_ERR_CAPACITY;
      }
    }
    if (dims[0] * dims[1] * dims[2] >= 0xFFFFFFFFull) {
      s->err = "clustering: more than 2^32 cells of side tolerance / 2 over the survivors' bounding box";
      return PFT_ERR_CAPACITY;
    }
    p.nx = (uint32_t)dims[0];
    p.ny = (uint32_t)dims[1];
    p.nz = (uint32_t)dims[2];
    const uint64_t ncell_grid = dims[0] * dims[1] * dims[2];
    int bits = 0;
    while (bits < 32 && (1ull << bits) < ncell_grid) bits++;
    const uint32_t mt = (m + SG_TILE - 1) / SG_TILE, mb = (m + SG_THREADS - 1) / SG_THREADS;
    hipLaunchKernelGGL(k_sg_cellkey, dim3(mb), dim3(SG_THREADS), 0, st, p, (const SgHdr*)s->hdr, (const float4*)b.spts,
                       b.key[0], b.val[0], m);
    int cur = pftk_radix_sort_pairs(st, b.key, b.val, m, bits, b.hist);
    const uint32_t* skey = b.key[cur];
    const uint32_t* sval = b.val[cur];
    hipLaunchKernelGGL(k_sg_heads, dim3(mt), dim3(SG_THREADS), 0, st, skey, m, b.flag, b.tile);
    hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, b.tile, mt, (const uint32_t*)nullptr, &s->hdr->n_cells);
    hipLaunchKernelGGL(k_sg_cells, dim3(mt), dim3(SG_THREADS), 0, st, skey, sval, m, (const uint8_t*)b.flag,
                       (const uint32_t*)b.tile, b.cell_start, b.cell_key, (const float4*)b.spts, b.sorted, b.cell_of);
    hipLaunchKernelGGL(k_sg_forest, dim3(mb), dim3(SG_THREADS), 0, st, sval, m, (const uint32_t*)b.cell_of,
                       (const uint32_t*)b.cell_start, b.parent);
    const uint32_t nlink = (uint32_t)std::min<uint64_t>(((uint64_t)m * 62u + SG_THREADS - 1) / SG_THREADS, 8192u);
    hipLaunchKernelGGL(k_sg_link, dim3(nlink), dim3(SG_THREADS), 0, st, p, (const SgHdr*)s->hdr,
                       (const uint32_t*)b.cell_start, (const uint32_t*)b.cell_key, sval, (const float4*)b.sorted, m,
                       b.parent);
    PFT_HIPCHK(s, hipMemsetAsync(b.csize, 0, m * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_sg_label, dim3(mb), dim3(SG_THREADS), 0, st, m, b.parent, b.label, b.csize);
    hipLaunchKernelGGL(k_sg_roots, dim3(mt), dim3(SG_THREADS), 0, st, p, m, (const uint32_t*)b.label,
                       (const uint32_t*)b.csize, b.flag, b.tile);
    hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, b.tile, mt, (const uint32_t*)nullptr, &s->hdr->n_clusters);
    hipLaunchKernelGGL(k_sg_emit, dim3(mt), dim3(SG_THREADS), 0, st, b.flag, m, (const uint32_t*)nullptr, b.tile,
                       (const uint32_t*)nullptr, b.roots, (const float4*)nullptr, (float4*)nullptr);
    MARK(ST_CLUSTER);
    r = read_hdr(s);
    if (r != PFT_OK) return r;
    MARK(-1);
    nc = H->n_clusters;
    if (nc > 0) {
      const uint32_t nb = (nc + SG_THREADS - 1) / SG_THREADS;
      hipLaunchKernelGGL(k_sg_order_keys, dim3(nb), dim3(SG_THREADS), 0, st, p, nc, (const uint32_t*)b.roots,
                         (const uint32_t*)b.csize, b.key[0], b.val[0]);
      int kbits = 0;
      while (kbits < 32 && (1ull << kbits) <= (uint64_t)(p.max_size - std::min(p.min_size, p.max_size))) kbits++;
      cur = pftk_radix_sort_pairs(st, b.key, b.val, nc, kbits, b.hist);
      PFT_HIPCHK(s, hipMemsetAsync(b.crank, 0xFF, m * sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_sg_rank, dim3(nb), dim3(SG_THREADS), 0, st, nc, (const uint32_t*)b.val[cur],
                         (const uint32_t*)b.csize, b.crank, b.sizes);
      hipLaunchKernelGGL(k_sg_member_keys, dim3(mb), dim3(SG_THREADS), 0, st, m, nc, (const uint32_t*)b.label,
                         (const uint32_t*)b.crank, b.key[0], b.val[0]);
      int rbits = 0;
      while ((1ull << rbits) <= (uint64_t)nc) rbits++;
      cur = pftk_radix_sort_pairs(st, b.key, b.val, m, rbits, b.hist);
      MARK(ST_CLUSTER);
      s->sizes.resize(nc);
      PFT_HIPCHK(s, hipMemcpyAsync(s->sizes.data(), b.sizes, nc * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      PFT_HIPCHK(s, hipStreamSynchronize(st));
      MARK(-1);
      for (uint32_t k = 0; k < nc; k++) total += s->sizes[k];
      hipLaunchKernelGGL(k_sg_output, dim3((total + SG_THREADS - 1) / SG_THREADS), dim3(SG_THREADS), 0, st, total,
                         (const uint32_t*)b.val[cur], (const uint32_t*)b.surv_in, d_in, b.out_idx, b.out_pts);
      MARK(ST_OUTPUT);
    }
  }
  PFT_HIPCHK(s, hipGetLastError());
  r = read_hdr(s);
  if (r != PFT_OK) return r;
  s->res = *H;
  s->res.n_clusters = nc;
  s->res.n_total = total;
  if (!s->by_rounds) {  // the single plane: one round, told by the same rule
    s->rounds.assign(1, s->res);
    const bool ran = c.plane_enable && H->n_valid > 0;
    const bool removed = ran && H->best_h >= 0 && H->n_fin > 0;
    s->n_rounds = ran ? 1 : 0;
    s->n_planes = removed ? 1 : 0;
    s->stopped_by = !ran ? PFT_ROUNDS_STOP_FRACTION
                         : (!removed ? PFT_ROUNDS_STOP_NO_PLANE
                                     : (H->n_valid > H->n_fin ? PFT_ROUNDS_STOP_MAX_PLANES : PFT_ROUNDS_STOP_FRACTION));
  } else if (s->rounds.empty()) {  // no round ran: round 0 reports the cloud and no plane
    SgHdr z = {};
    z.best_h = -1;
    z.n_valid = H->n_valid;
    s->rounds.assign(1, z);
  }
  s->last_ms = 0.0;
  for (int k = 0; k < PFT_SEGMENT_STAGES; k++) s->stage_ms[k] = 0.0;
  for (int e = 1; e < s->nev; e++) {
    float ms = 0.0f;
    PFT_HIPCHK(s, hipEventElapsedTime(&ms, s->ev[e - 1], s->ev[e]));
    if (s->ev_stage[e] < 0) continue;  // the gap spans a host synchronisation
    s->stage_ms[s->ev_stage[e]] += ms;
    s->last_ms += ms;
  }
  return PFT_OK;
}

static int apply_common(pft_segment* s, const pft_point_xyzrgba* pts, size_t n, bool on_device) {
  if (!s || (!pts && n)) return PFT_ERR_INVALID_ARG;
  if (n > 0x7fffffffu) return PFT_ERR_CAPACITY;
  s->have_result = false;
  PFT_HIPCHK(s, hipSetDevice(s->cfg.device_id));
  if (n == 0) {  // empty input cloud: no plane, no clusters
    s->res = SgHdr();
    s->res.best_h = -1;
    s->sizes.clear();
    s->rounds.assign(1, s->res);
    s->by_rounds = false;
    s->n_rounds = s->n_planes = 0;
    s->stopped_by = PFT_ROUNDS_STOP_FRACTION;
    s->n_in = 0;
    s->last_ms = 0.0;
    for (int k = 0; k < PFT_SEGMENT_STAGES; k++) s->stage_ms[k] = 0.0;
    s->have_result = true;
    return PFT_OK;
  }
  int r = ensure_capacity(s, n);
  if (r != PFT_OK) return r;
  const pft_point_xyzrgba* d_in = pts;
  if (!on_device) {
    if (n) PFT_HIPCHK(s, hipMemcpyAsync(s->b.in_own, pts, n * sizeof(pft_point_xyzrgba), hipMemcpyHostToDevice, s->stream));
    d_in = s->b.in_own;
  }
  r = run_pipeline(s, d_in, (uint32_t)n);
  if (r != PFT_OK) return r;
  s->n_in = n;
  s->have_result = true;
  return PFT_OK;
}

extern "C" int pft_segment_apply(pft_segment* s, const pft_point_xyzrgba* host_points, size_t n) {
  return apply_common(s, host_points, n, false);
}
extern "C" int pft_segment_apply_device(pft_segment* s, const pft_point_xyzrgba* device_points, size_t n) {
  return apply_common(s, device_points, n, true);
}

static int bad_round(const pft_segment* s, const char* fn) {
  const_cast<pft_segment*>(s)->err = std::string(fn) + ": round is not below the number of rounds the last apply ran";
  return PFT_ERR_INVALID_ARG;
}

extern "C" int pft_segment_get_plane_round(const pft_segment* s, size_t round, pft_segment_plane* pl) {
  if (!s || !pl) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) return PFT_ERR_STATE;
  if (round >= s->rounds.size()) return bad_round(s, "pft_segment_get_plane_round");
  const SgHdr& h = s->rounds[round];
  memset(pl, 0, sizeof(*pl));
  pl->n_valid = h.n_valid;
  pl->n_survivors = s->res.n_surv;
  if (!s->cfg.plane_enable) {
    pl->status = PFT_PLANE_DISABLED;
    return PFT_OK;
  }
  pl->iterations = h.iterations;
  pl->hypotheses_scored = h.emitted;
  if (h.best_h < 0) {
    pl->status = PFT_PLANE_NONE;
    pl->sample[0] = pl->sample[1] = pl->sample[2] = -1;
    return PFT_OK;
  }
  pl->status = PFT_PLANE_FOUND;
  for (int k = 0; k < 4; k++) {
    pl->coefficients[k] = h.coef_final[k];
    pl->ransac_coefficients[k] = h.coef_ransac[k];
  }
  pl->ransac_inliers = h.n_ransac_inl;
  pl->inliers = h.n_fin;
  int32_t smp[3];
  pft_segment* sm = const_cast<pft_segment*>(s);
  if (hipMemcpy(smp, s->hyp.sample + 3 * ((size_t)round * s->hmax + (size_t)h.best_h), sizeof(smp),
                hipMemcpyDeviceToHost) != hipSuccess) {
    sm->err = "hipMemcpy of the best sample failed";
    return PFT_ERR_HIP;
  }
  for (int k = 0; k < 3; k++) pl->sample[k] = smp[k];
  return PFT_OK;
}

extern "C" int pft_segment_get_plane(const pft_segment* s, pft_segment_plane* pl) {
  return pft_segment_get_plane_round(s, 0, pl);
}

// the best hypothesis' inliers are kept as compacted indices; mapped to the input on the way out
__global__ void k_sg_map_idx(uint32_t n, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ map,
                             int32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (int32_t)map[idx[i]];
}

extern "C" int pft_segment_get_plane_round_inliers(pft_segment* s, size_t round, int which, int32_t* host_idx,
                                                   size_t capacity, size_t* n) {
  if (!s || !n || (which != 0 && which != 1)) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) return PFT_ERR_STATE;
  if (round >= s->rounds.size()) return bad_round(s, "pft_segment_get_plane_round_inliers");
  const SgHdr& h = s->rounds[round];
  const bool have = s->cfg.plane_enable && h.best_h >= 0;
  const uint32_t cnt = !have ? 0u : (which == 0 ? h.n_fin : h.n_ransac_inl);
  *n = cnt;
  if (cnt > capacity) return PFT_ERR_CAPACITY;
  if (!cnt) return PFT_OK;
  if (!host_idx) return PFT_ERR_INVALID_ARG;
  const int32_t* src = reinterpret_cast<const int32_t*>(s->b.fin_idx);
  if (s->by_rounds) {  // re-derived from the per-point round byte; flag, tile and crank are scratch after an apply
    const uint32_t nin = (uint32_t)s->n_in, nt = (nin + SG_TILE - 1) / SG_TILE;
    int32_t* tmp = reinterpret_cast<int32_t*>(s->b.crank);
    const float4 cf = make_float4(h.coef_ransac[0], h.coef_ransac[1], h.coef_ransac[2], h.coef_ransac[3]);
    hipLaunchKernelGGL(k_sg_round_flags, dim3(nt), dim3(SG_THREADS), 0, s->stream, nin, (const uint8_t*)s->b.rnd,
                       (const float4*)s->b.tx, (uint32_t)round, which, cf, float_bound_below(s->cfg.distance_threshold),
                       s->b.flag, s->b.tile);
    hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, s->stream, s->b.tile, nt, (const uint32_t*)nullptr,
                       &s->hdr->n_total);
    hipLaunchKernelGGL(k_sg_emit, dim3(nt), dim3(SG_THREADS), 0, s->stream, (const uint8_t*)s->b.flag, nin,
                       (const uint32_t*)nullptr, (const uint32_t*)s->b.tile, (const uint32_t*)nullptr,
                       reinterpret_cast<uint32_t*>(tmp), (const float4*)nullptr, (float4*)nullptr);
    PFT_HIPCHK(s, hipGetLastError());
    src = tmp;
  } else if (which == 1) {  // crank is scratch once an apply has finished
    int32_t* tmp = reinterpret_cast<int32_t*>(s->b.crank);
    hipLaunchKernelGGL(k_sg_map_idx, dim3((cnt + 255) / 256), dim3(256), 0, s->stream, cnt,
                       (const uint32_t*)s->b.inl_idx, (const uint32_t*)s->b.comp_idx, tmp);
    PFT_HIPCHK(s, hipGetLastError());
    src = tmp;
  }
  PFT_HIPCHK(s, hipMemcpyAsync(host_idx, src, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  PFT_HIPCHK(s, hipStreamSynchronize(s->stream));
  return PFT_OK;
}

extern "C" int pft_segment_get_plane_inliers(pft_segment* s, int which, int32_t* host_idx, size_t capacity, size_t* n) {
  return pft_segment_get_plane_round_inliers(s, 0, which, host_idx, capacity, n);
}

extern "C" int pft_segment_set_plane_rounds(pft_segment* s, int max_planes, double min_remaining_fraction) {
  if (!s) return PFT_ERR_INVALID_ARG;
  if (max_planes < 1 || max_planes > PFT_SEGMENT_MAX_PLANES) {
    s->err = "pft_segment_set_plane_rounds: max_planes must be 1 .. PFT_SEGMENT_MAX_PLANES (16)";
    return PFT_ERR_INVALID_ARG;
  }
  if (!(min_remaining_fraction >= 0.0 && min_remaining_fraction <= 1.0)) {
    s->err = "pft_segment_set_plane_rounds: min_remaining_fraction must be within [0, 1]";
    return PFT_ERR_INVALID_ARG;
  }
  if ((uint32_t)max_planes > s->hyp_rounds) {  // one set of hypothesis buffers per round
    PFT_HIPCHK(s, hipSetDevice(s->cfg.device_id));
    PFT_HIPCHK(s, hipStreamSynchronize(s->stream));
    SgHyp nh = {};
    const size_t cnt = (size_t)s->hmax * (size_t)max_planes;
    if (pft_dalloc(&nh.sample, 3 * cnt) != hipSuccess || pft_dalloc(&nh.coef, cnt) != hipSuccess ||
        pft_dalloc(&nh.count, cnt) != hipSuccess) {
      pft_dfree(nh.sample); pft_dfree(nh.coef); pft_dfree(nh.count);
      s->err = "pft_segment_set_plane_rounds: hipMalloc of the rounds' hypothesis buffers failed";
      return PFT_ERR_HIP;
    }
    pft_dfree(s->hyp.sample); pft_dfree(s->hyp.coef); pft_dfree(s->hyp.count);
    s->hyp = nh;
    s->hyp_rounds = (uint32_t)max_planes;
    s->have_result = false;  // the last apply's hypotheses went with the old buffers
  }
  s->max_planes = max_planes;
  s->min_fraction = min_remaining_fraction;
  return PFT_OK;
}

extern "C" int pft_segment_get_plane_rounds(const pft_segment* s, int* max_planes, double* min_remaining_fraction) {
  if (!s) return PFT_ERR_INVALID_ARG;
  if (max_planes) *max_planes = s->max_planes;
  if (min_remaining_fraction) *min_remaining_fraction = s->min_fraction;
  return PFT_OK;
}

extern "C" int pft_segment_set_refit_order(pft_segment* s, int order) {
  if (!s) return PFT_ERR_INVALID_ARG;
  if (order != PFT_SUM_PCL && order != PFT_SUM_TREE) {
    s->err = "pft_segment_set_refit_order: order must be PFT_SUM_PCL or PFT_SUM_TREE";
    return PFT_ERR_INVALID_ARG;
  }
  s->refit_order = order;
  return PFT_OK;
}

extern "C" int pft_segment_plane_count(const pft_segment* s, size_t* n_planes, int* stopped_by) {
  if (!s) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) return PFT_ERR_STATE;
  if (n_planes) *n_planes = s->n_planes;
  if (stopped_by) *stopped_by = s->stopped_by;
  return PFT_OK;
}

extern "C" int pft_segment_cluster_count(const pft_segment* s, size_t* n_clusters) {
  if (!s || !n_clusters) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) return PFT_ERR_STATE;
  *n_clusters = s->res.n_clusters;
  return PFT_OK;
}

extern "C" int pft_segment_cluster_sizes(const pft_segment* s, uint32_t* sizes, size_t capacity) {
  if (!s) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) return PFT_ERR_STATE;
  if (s->sizes.size() > capacity) return PFT_ERR_CAPACITY;
  if (!s->sizes.empty()) {
    if (!sizes) return PFT_ERR_INVALID_ARG;
    memcpy(sizes, s->sizes.data(), s->sizes.size() * sizeof(uint32_t));
  }
  return PFT_OK;
}

extern "C" int pft_segment_get_cluster_indices(pft_segment* s, int32_t* host_idx, size_t capacity, size_t* n_total) {
  if (!s || !n_total) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) return PFT_ERR_STATE;
  *n_total = s->res.n_total;
  if (s->res.n_total > capacity) return PFT_ERR_CAPACITY;
  if (!s->res.n_total) return PFT_OK;
  if (!host_idx) return PFT_ERR_INVALID_ARG;
  PFT_HIPCHK(s, hipMemcpyAsync(host_idx, s->b.out_idx, s->res.n_total * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  PFT_HIPCHK(s, hipStreamSynchronize(s->stream));
  return PFT_OK;
}

extern "C" int pft_segment_get_cluster_points(pft_segment* s, pft_point_xyzrgba* host_pts, size_t capacity,
                                              size_t* n_total) {
  if (!s || !n_total) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) return PFT_ERR_STATE;
  *n_total = s->res.n_total;
  if (s->res.n_total > capacity) return PFT_ERR_CAPACITY;
  if (!s->res.n_total) return PFT_OK;
  if (!host_pts) return PFT_ERR_INVALID_ARG;
  PFT_HIPCHK(s, hipMemcpyAsync(host_pts, s->b.out_pts, s->res.n_total * sizeof(pft_point_xyzrgba), hipMemcpyDeviceToHost,
                         s->stream));
  PFT_HIPCHK(s, hipStreamSynchronize(s->stream));
  return PFT_OK;
}

extern "C" int pft_segment_clusters_device(const pft_segment* s, const pft_point_xyzrgba** device_pts, size_t* n_total) {
  if (!s || !device_pts || !n_total) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) return PFT_ERR_STATE;
  *device_pts = s->res.n_total ? s->b.out_pts : nullptr;
  *n_total = s->res.n_total;
  return PFT_OK;
}

int pftsg_device_id(const pft_segment* s) { return s->cfg.device_id; }

extern "C" int pft_segment_last_ms(const pft_segment* s, double* ms, double* stage_ms) {
  if (!s || !ms) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) return PFT_ERR_STATE;
  *ms = s->last_ms;
  if (stage_ms)
    for (int k = 0; k < PFT_SEGMENT_STAGES; k++) stage_ms[k] = s->stage_ms[k];
  return PFT_OK;
}

extern "C" int pft_debug_segment_hypotheses(pft_segment* s, int32_t* samples, uint32_t* counts, size_t capacity,
                                            size_t* n) {
  return pft_debug_segment_round_hypotheses(s, 0, samples, counts, capacity, n);
}

extern "C" int pft_debug_segment_round_hypotheses(pft_segment* s, size_t round, int32_t* samples, uint32_t* counts,
                                                  size_t capacity, size_t* n) {
  if (!s || !n) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) return PFT_ERR_STATE;
  if (round >= s->rounds.size()) return bad_round(s, "pft_debug_segment_round_hypotheses");
  const size_t cnt = s->cfg.plane_enable ? s->rounds[round].iterations : 0, off = round * (size_t)s->hmax;
  *n = cnt;
  if (cnt > capacity) return PFT_ERR_CAPACITY;
  if (!cnt) return PFT_OK;
  if (!samples || !counts) return PFT_ERR_INVALID_ARG;
  PFT_HIPCHK(s, hipMemcpy(samples, s->hyp.sample + 3 * off, 3 * cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
  PFT_HIPCHK(s, hipMemcpy(counts, s->hyp.count + off, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PFT_OK;
}

extern "C" int pft_debug_segment_refit(pft_segment* s, size_t round, pft_segment_refit_debug* out) {
  if (!s || !out) return PFT_ERR_INVALID_ARG;
  if (!s->have_result) {
    s->err = "pft_debug_segment_refit: no apply yet";
    return PFT_ERR_STATE;
  }
  if (round >= s->rounds.size()) return bad_round(s, "pft_debug_segment_refit");
  const SgHdr& h = s->rounds[round];
  if (!s->cfg.plane_enable || h.best_h < 0) {
    s->err = "pft_debug_segment_refit: the round found no plane";
    return PFT_ERR_STATE;
  }
  if (!s->cfg.optimize_coefficients || h.n_ransac_inl < 4 || h.refit.m == 0) {
    s->err = "pft_debug_segment_refit: no refit ran (optimize_coefficients off, or fewer than 4 inliers)";
    return PFT_ERR_STATE;
  }
  *out = h.refit;
  return PFT_OK;
}

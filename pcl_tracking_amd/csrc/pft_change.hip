// pft_change.hip -- ParticleFilterTracker's change detector (PCL 1.8.0 particle_filter.hpp testChangeDetection over
// octree::OctreePointCloudChangeDetector = Octree2BufBase + OctreePointCloud) and the counter schedule of weight():
//
//   if (change_counter_ == 0) {
//     if (!use_change_detector_ || testChangeDetection(crop)) { changed_ = true; change_counter_ = interval; evaluate }
//     else changed_ = false;
//   } else { --change_counter_; evaluate }
//
// testChangeDetection: setInputCloud(crop); addPointsFromInputCloud(); getPointIndicesFromNewVoxels(idx, min_points);
// switchBuffers(); return idx.size() > 0.  The detector octree's bounding box is never reset: it grows over every crop
// tested, in insertion order, by the root-doubling rule of the per-iteration builder (pft_octree_box.h).  A leaf is new when
// its voxel held no point of the previous tested crop; root growth moves old leaves under the new root without making
// them new (Octree2BufBase keeps the old buffer's child bits below the moved root), so the previous set's keys are rebased
// by the growth of this call (+2^old_depth on each axis whose minimum was lowered).
//
// ONE 1024-thread workgroup: the box replay is a chain of dependent events (one parallel pass when nothing grows, which is
// every test once the box has covered the scene), the voxel counting is an open-addressing hash table in HBM keyed by the
// packed 3 x 21-bit voxel key: the previous set goes in first, flagged, then the points of the crop are counted.
#include "pft_device_utils.h"
#include "pft_octree_box.h"

#define CD_THREADS 1024
#define CD_KEY_BITS 21
#define CD_EMPTY 0xffffffffffffffffull

struct CdSh {  // beside the builder's BuildSh (the box routines work on that)
  uint32_t test, n_out, new_vox, new_pts;
};

__device__ __forceinline__ uint32_t cd_hash(unsigned long long k, uint32_t mask) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  return (uint32_t)k & mask;
}
// slot of key k (inserted if absent); the table has room for every key of a test (2x head-room)
__device__ __forceinline__ uint32_t cd_insert(unsigned long long* tab, uint32_t mask, unsigned long long k) {
  uint32_t h = cd_hash(k, mask);
  for (;;) {
    const unsigned long long o = atomicCAS(&tab[h], CD_EMPTY, k);
    if (o == CD_EMPTY || o == k) return h;
    h = (h + 1u) & mask;
  }
}
__device__ __forceinline__ uint32_t cd_find(const unsigned long long* tab, uint32_t mask, unsigned long long k) {
  uint32_t h = cd_hash(k, mask);
  while (tab[h] != k) h = (h + 1u) & mask;
  return h;
}
__device__ __forceinline__ unsigned long long cd_pack(uint32_t kx, uint32_t ky, uint32_t kz) {
  return ((unsigned long long)kx << (2 * CD_KEY_BITS)) | ((unsigned long long)ky << CD_KEY_BITS) | (unsigned long long)kz;
}

__global__ __launch_bounds__(CD_THREADS) void k_change_detect(PftChangeBufs b, const float4* __restrict__ pts,
                                                              const uint32_t* n_ptr, uint32_t n_arg, PftChangeArgs a,
                                                              uint32_t* host_stat) {
  __shared__ BuildSh S;
  __shared__ CdSh X;
  PftChangeState* st = b.st;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const uint32_t n = n_ptr ? *n_ptr : n_arg;
  const double res = a.res;
  uint32_t counter = 0;
  if (tid == 0) {
    counter = st->counter;
    uint32_t test = 0;
    if (a.force) {
      test = 1;
    } else if (counter == 0) {
      if (a.use) {
        test = 1;
      } else {  // (!use_change_detector_ || ...): evaluate
        st->gate = 1u;
        counter = a.interval;
      }
    } else {
      counter--;  // evaluate; changed_ keeps its value (true: the counter is only ever set together with it)
    }
    X.test = test;
    if (!test) {
      st->counter = counter;
      uint32_t* r = st->ring[st->n_calls % PFT_CD_RING];
      r[0] = 0u; r[1] = st->gate; r[2] = 0u; r[3] = 0u; r[4] = counter;
      st->n_calls++;
    } else {
      for (int k = 0; k < 3; k++) {
        S.mn[k] = st->mn[k];
        S.mx[k] = st->mx[k];
        S.gmin[0][k] = st->mn[k];
      }
      S.depth = st->depth;
      S.ngrow = 0;
      S.err = 0u;
      S.cur = 0u;
      X.n_out = X.new_vox = X.new_pts = 0u;
      if (!st->defined && n > 0u) {  // the very first point of the detector's life defines the box
        box_init(S, pts[0], res);
        S.cur = 1u;
      }
    }
  }
  __syncthreads();
  if (!X.test) return;

  // ---- adoptBoundingBoxToPoint over the crop in index order: find the first point outside the box, grow, repeat ----
  for (;;) {
    const uint32_t cur = S.cur;
    const double mn[3] = {S.mn[0], S.mn[1], S.mn[2]}, mx[3] = {S.mx[0], S.mx[1], S.mx[2]};
    uint32_t first = 0xffffffffu;
    for (uint32_t i = cur + tid; i < n; i += nt) {
      const float4 p = pts[i];
      if (box_violates(p.x, p.y, p.z, mn, mx)) {
        first = i;
        break;
      }
    }
    first = block_reduce<uint32_t>(first, S.u32s, OpMinU(), 0xffffffffu);
    if (first == 0xffffffffu) break;
    if (tid == 0) {
      box_grow(S, pts[first], first, res);
      S.cur = first + 1u;
    }
    __syncthreads();
    if (S.err) break;
  }
  __syncthreads();
  const int ngrow = S.ngrow;
  if (S.err || S.depth > CD_KEY_BITS) {
    // error bit 5: the keys do not fit.  The box keeps what it grew; the previous set is forgotten (the next test then
    // finds every voxel new), and this iteration evaluates
    if (tid == 0) {
      for (int k = 0; k < 3; k++) {
        st->mn[k] = S.mn[k];
        st->mx[k] = S.mx[k];
      }
      st->depth = S.depth;
      st->defined = 1u;
      st->n_set[0] = st->n_set[1] = 0u;
      st->gate = 1u;
      st->counter = a.force ? st->counter : a.interval;
      uint32_t* r = st->ring[st->n_calls % PFT_CD_RING];
      r[0] = 1u; r[1] = 1u; r[2] = 0u; r[3] = 0u; r[4] = st->counter;
      st->n_calls++;
      if (host_stat) {
        host_stat[2] = 32u;
        host_stat[3] |= 32u;
      }
    }
    return;
  }

  // ---- count points per voxel; the previous set's voxels go in first, flagged ----
  const uint32_t prev = st->prev, n_prev = st->n_set[prev];
  uint32_t size = 64u;
  while (size < 2u * (n + n_prev) && size < b.tab_cap) size <<= 1;
  const uint32_t mask = size - 1u;
  for (uint32_t s = tid; s < size; s += nt) {
    b.tab_key[s] = CD_EMPTY;
    b.tab_cnt[s] = 0u;
  }
  __threadfence_block();
  __syncthreads();
  // growth of this call, as a per-axis offset of the previous set's keys
  uint32_t off[3] = {0u, 0u, 0u};
  for (int g = 0; g < ngrow; g++)
    for (int k = 0; k < 3; k++)
      if (S.gshift[g] & (1u << k)) off[k] += 1u << S.gold[g];
  const unsigned long long m21 = (1ull << CD_KEY_BITS) - 1ull;
  for (uint32_t j = tid; j < n_prev; j += nt) {
    const unsigned long long k0 = b.set_key[prev][j];
    const unsigned long long k = cd_pack((uint32_t)(k0 >> (2 * CD_KEY_BITS)) + off[0],
                                         (uint32_t)((k0 >> CD_KEY_BITS) & m21) + off[1], (uint32_t)(k0 & m21) + off[2]);
    atomicOr(&b.tab_cnt[cd_insert(b.tab_key, mask, k)], 0x80000000u);
  }
  const uint32_t last_grow = ngrow > 0 ? S.gidx[ngrow - 1] : 0u;
  for (uint32_t i = tid; i < n; i += nt) {
    const float4 p = pts[i];
    int e = ngrow;  // growth epoch of the point (the events a point triggers come before its key)
    if (ngrow > 0 && i < last_grow) {
      e = 0;
      while (e < ngrow && S.gidx[e] <= i) e++;
    }
    // genOctreeKeyforPoint: (unsigned)((p - min) / res) in double
    uint32_t kk[3] = {(uint32_t)(((double)p.x - S.gmin[e][0]) / res), (uint32_t)(((double)p.y - S.gmin[e][1]) / res),
                      (uint32_t)(((double)p.z - S.gmin[e][2]) / res)};
    for (int g = e; g < ngrow; g++)
      for (int k = 0; k < 3; k++)
        if (S.gshift[g] & (1u << k)) kk[k] += 1u << S.gold[g];
    const unsigned long long key = cd_pack(kk[0], kk[1], kk[2]);
    b.pt_key[i] = key;
    atomicAdd(&b.tab_cnt[cd_insert(b.tab_key, mask, key)], 1u);
  }
  __threadfence_block();
  __syncthreads();

  // ---- new voxels (absent from the previous set, at least min_points points), and the current set ----
  const uint32_t minp = a.min_points > 1u ? a.min_points : 1u;  // (a leaf holds at least one point)
  const uint32_t nxt = 1u - prev;
  uint32_t nv = 0u, np = 0u;
  for (uint32_t s = tid; s < size; s += nt) {
    const uint32_t c = b.tab_cnt[s], cnt = c & 0x7fffffffu;
    if (cnt == 0u) continue;
    const uint32_t o = atomicAdd(&X.n_out, 1u);
    b.set_key[nxt][o] = b.tab_key[s];
    b.set_cnt[nxt][o] = cnt;
    if (!(c >> 31) && cnt >= minp) {
      nv++;
      np += cnt;
    }
  }
  nv = wave_sum(nv);
  np = wave_sum(np);
  if (lane_id() == 0) {
    atomicAdd(&X.new_vox, nv);
    atomicAdd(&X.new_pts, np);
  }
  if (b.mark) {
    for (uint32_t i = tid; i < n; i += nt) {
      const uint32_t c = b.tab_cnt[cd_find(b.tab_key, mask, b.pt_key[i])];
      b.mark[i] = (!(c >> 31) && (c & 0x7fffffffu) >= minp) ? 1u : 0u;
    }
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 0; k < 3; k++) {
      st->mn[k] = S.mn[k];
      st->mx[k] = S.mx[k];
    }
    st->depth = S.depth;
    if (n > 0u) st->defined = 1u;
    st->n_set[nxt] = X.n_out;  // switchBuffers()
    st->prev = nxt;
    const bool changed = X.new_vox > 0u;
    if (!a.force) {
      st->gate = changed ? 1u : 0u;
      st->counter = changed ? a.interval : 0u;
    }
    uint32_t* r = st->ring[st->n_calls % PFT_CD_RING];
    r[0] = 1u; r[1] = changed ? 1u : 0u; r[2] = X.new_vox; r[3] = X.new_pts; r[4] = st->counter;
    st->n_calls++;
  }
}

void pftk_change_detect(hipStream_t s, const PftChangeBufs& b, const float4* pts, const uint32_t* n_ptr, uint32_t n,
                        const PftChangeArgs& a, uint32_t* host_stat) {
  hipLaunchKernelGGL(k_change_detect, dim3(1), dim3(CD_THREADS), 0, s, b, pts, n_ptr, n, a, host_stat);
}

// pft_grow.hip -- model growth (include/pft_grow.h is the specification): fold surface that is
// seen next to an object's model into the model.
//
// The voxel table is open addressing in HBM over three arrays of max_voxels words: the packed key (0: a free slot), the
// state word meta = last_seen << 32 | hits << 8 | kind, and the representative word rep = a << 32 | ~i.  A cleared slot is a
// valid empty state and a claimed slot whose meta is still 0 reads as "not in the table", so no lane ever waits for another;
// every probe loop is bounded by max_voxels.
//
//   k_grow_gather   } the rebuild, three launches that return at once unless more than half the slots are occupied (or the
//   k_grow_clear    } last apply overflowed): the kept entries to a list, the table cleared, the list inserted again
//   k_grow_insert   }
//   k_grow_classify the hot kernel, one point per lane: rules 1-3, the MODEL key box grown by reach, the probe of the own
//                   voxel, the probes of the (2 reach + 1)^3 - 1 neighbours; a candidate claims or finds its voxel (64-bit
//                   CAS on the key), counts the voxel's hit once per apply (CAS loop on meta, a no-op when last_seen == a)
//                   and bids for the representative (atomicMax on rep).  Inserting PENDING entries while other lanes still
//                   classify is harmless: rules 4 and 5 only ask for MODEL entries, and none is made before k_grow_confirm
//   k_grow_confirm  per tile of 1024 points: the representative of a voxel with hits >= confirm makes it MODEL, becomes
//                   ADDED and widens the key box; the counts per state; the tile's number of ADDED points
//   pftk_tile_scan + k_grow_emit  the stable compaction: the appended records in ascending input index
//   k_grow_finish   one lane: the bookkeeping (occupied, rebuilds, overflow) and the statistics block
//
// The words the waves of the hot kernel update (GrowCnt) live on another 256-byte line than the words they read (GrowCtl):
// the lesson of ec_pool_used, DESIGN.md section 7.  No float atomics anywhere.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pft_devbuf.h"
#include "pft_device_utils.h"
#include "../../include/pft_grow.h"

#define GR_THREADS 256
#define GR_TILE 1024u
#define GR_TABLE_BLOCKS 1024u
#define GR_KEY_BIAS 1048576  // 2^20: a component k is stored as k + 2^20 in [1, 2^21 - 1], so no key is 0
#define GR_NO_SLOT 0xffffffffu

struct alignas(256) GrowCtl {  // read by the waves of the hot kernel, written between the launches
  uint32_t occupied, n_model_voxels, n_model_points, n_rebuilds, drop_pending, pad[3];
  int32_t box_lo[3], box_hi[3];  // MODEL keys per axis; lo > hi: no MODEL voxel
};
struct alignas(256) GrowCnt {  // updated by the waves
  uint32_t claims, cand_voxels, overflow, list_n;
  uint32_t n_state[PFT_GROW_N_STATES];
};
struct GrowDev {
  GrowCtl ctl;
  GrowCnt cnt;
  pft_grow_stats stats;
  uint32_t n_added;  // the tile scan's total
};

struct GrowTable {
  unsigned long long* key;
  unsigned long long* meta;
  unsigned long long* rep;
  uint32_t mask;  // max_voxels - 1
};

__host__ __device__ __forceinline__ unsigned long long gr_pack_key(int kx, int ky, int kz) {
  return ((unsigned long long)(uint32_t)(kx + GR_KEY_BIAS) << 42) | ((unsigned long long)(uint32_t)(ky + GR_KEY_BIAS) << 21) |
         (unsigned long long)(uint32_t)(kz + GR_KEY_BIAS);
}
__host__ __device__ __forceinline__ void gr_unpack_key(unsigned long long k, int* c) {
  c[0] = (int)((k >> 42) & 0x1fffffu) - GR_KEY_BIAS;
  c[1] = (int)((k >> 21) & 0x1fffffu) - GR_KEY_BIAS;
  c[2] = (int)(k & 0x1fffffu) - GR_KEY_BIAS;
}
__host__ __device__ __forceinline__ uint32_t gr_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}
__host__ __device__ __forceinline__ unsigned long long gr_meta(uint32_t last_seen, uint32_t hits, uint32_t kind) {
  return ((unsigned long long)last_seen << 32) | ((unsigned long long)hits << 8) | kind;
}
__host__ __device__ __forceinline__ uint32_t gr_kind(unsigned long long m) { return (uint32_t)(m & 0xffu); }
__host__ __device__ __forceinline__ uint32_t gr_hits(unsigned long long m) { return (uint32_t)((m >> 8) & 0xffffffu); }
__host__ __device__ __forceinline__ uint32_t gr_seen(unsigned long long m) { return (uint32_t)(m >> 32); }

// the key component of one object-frame coordinate; false: the point has no key
__host__ __device__ __forceinline__ bool gr_cell(float y, float inv_leaf, int* k) {
  const float f = floorf(y * inv_leaf);
  if (!(fabsf(f) < (float)GR_KEY_BIAS)) return false;
  *k = (int)f;
  return true;
}

__device__ __forceinline__ unsigned long long gr_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the slot of a key, or GR_NO_SLOT: stops at the first free slot
__device__ __forceinline__ uint32_t gr_find(const GrowTable& t, unsigned long long key) {
  uint32_t s = gr_hash(key) & t.mask;
  for (uint32_t probe = 0; probe <= t.mask; probe++) {
    const unsigned long long k = gr_load(t.key + s);
    if (k == key) return s;
    if (k == 0ull) return GR_NO_SLOT;
    s = (s + 1u) & t.mask;
  }
  return GR_NO_SLOT;
}
__device__ __forceinline__ bool gr_is_model(const GrowTable& t, unsigned long long key) {
  const uint32_t s = gr_find(t, key);
  return s != GR_NO_SLOT && gr_kind(gr_load(t.meta + s)) == PFT_GROW_KIND_MODEL;
}
// the slot of a key, claimed if the key was not there (*claimed); GR_NO_SLOT: every slot holds another key
__device__ __forceinline__ uint32_t gr_find_or_claim(const GrowTable& t, unsigned long long key, bool* claimed) {
  *claimed = false;
  uint32_t s = gr_hash(key) & t.mask;
  for (uint32_t probe = 0; probe <= t.mask; probe++) {
    unsigned long long k = gr_load(t.key + s);
    if (k == 0ull) {
      k = atomicCAS(t.key + s, 0ull, key);
      if (k == 0ull) {
        *claimed = true;
        return s;
      }
    }
    if (k == key) return s;
    s = (s + 1u) & t.mask;
  }
  return GR_NO_SLOT;
}

// ---- the rebuild ----
// 0: no rebuild before this apply, 1: MODEL and live PENDING entries stay, 2: MODEL entries only (the last apply overflowed)
__device__ __forceinline__ int gr_rebuild_mode(const GrowCtl& c, uint32_t max_voxels) {
  if (c.drop_pending) return 2;
  return c.occupied > max_voxels / 2u ? 1 : 0;
}

__global__ __launch_bounds__(GR_THREADS) void k_grow_gather(GrowDev* d, GrowTable t, GrowTable list, uint32_t a, uint32_t forget) {
  const int mode = gr_rebuild_mode(d->ctl, t.mask + 1u);
  if (!mode) return;  // (uniform)
  for (uint32_t s = blockIdx.x * GR_THREADS + threadIdx.x; s <= t.mask; s += gridDim.x * GR_THREADS) {
    const unsigned long long k = t.key[s];
    if (k == 0ull) continue;
    const unsigned long long m = t.meta[s];
    const bool keep = gr_kind(m) == PFT_GROW_KIND_MODEL ||
                      (mode == 1 && gr_kind(m) == PFT_GROW_KIND_PENDING && a - gr_seen(m) <= forget);
    if (!keep) continue;
    const uint32_t pos = atomicAdd(&d->cnt.list_n, 1u);  // (the order of the list decides nothing)
    if (pos > t.mask) continue;
    list.key[pos] = k;
    list.meta[pos] = m;
    list.rep[pos] = t.rep[s];
  }
}

__global__ __launch_bounds__(GR_THREADS) void k_grow_clear(const GrowDev* d, GrowTable t) {
  if (!gr_rebuild_mode(d->ctl, t.mask + 1u)) return;
  for (uint32_t s = blockIdx.x * GR_THREADS + threadIdx.x; s <= t.mask; s += gridDim.x * GR_THREADS) {
    t.key[s] = 0ull;
    t.meta[s] = 0ull;
    t.rep[s] = 0ull;
  }
}

// force: the list is the model of pft_grow_set_model
__global__ __launch_bounds__(GR_THREADS) void k_grow_insert(const GrowDev* d, GrowTable t, GrowTable list, int force) {
  if (!force && !gr_rebuild_mode(d->ctl, t.mask + 1u)) return;
  const uint32_t n = min(d->cnt.list_n, t.mask + 1u);
  for (uint32_t j = blockIdx.x * GR_THREADS + threadIdx.x; j < n; j += gridDim.x * GR_THREADS) {
    bool claimed;
    const uint32_t s = gr_find_or_claim(t, list.key[j], &claimed);  // (n <= max_voxels distinct keys: there is a slot)
    if (s == GR_NO_SLOT) continue;
    t.meta[s] = list.meta[j];
    t.rep[s] = list.rep[j];
  }
}

// ---- the hot kernel ----
struct GrowApplyArgs {
  const pft_point_xyzrgba* in;
  uint32_t n, a;
  float Ti[12];
  float planes[PFT_GROW_MAX_PLANES][4];
  int n_planes;
  float plane_margin, inv_leaf, max_r2;
  int reach;
  uint32_t forget, confirm;
  GrowTable t;
  GrowDev* d;
  uint8_t* state;
  uint32_t* slot;  // the voxel's slot of every candidate
  uint32_t* tile;
  pft_point_xyzrgba* cloud;
  uint32_t cloud_cap;
};

__global__ __launch_bounds__(GR_THREADS) void k_grow_classify(GrowApplyArgs g) {
  const uint32_t i = blockIdx.x * GR_THREADS + threadIdx.x;
  if (i >= g.n) return;
  const float4 p = *reinterpret_cast<const float4*>(g.in + i);
  uint32_t st;
  unsigned long long key = 0ull;
  int k[3] = {0, 0, 0};
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) {
    st = PFT_GROW_NONFINITE;
  } else {
    bool on_plane = false;
    for (int q = 0; q < g.n_planes; q++)  // (uniform)
      on_plane = on_plane || fabsf(g.planes[q][0] * p.x + g.planes[q][1] * p.y + g.planes[q][2] * p.z + g.planes[q][3]) <= g.plane_margin;
    if (on_plane) {
      st = PFT_GROW_PLANE;
    } else {
      float y0, y1, y2;
      xform(g.Ti, p.x, p.y, p.z, y0, y1, y2);
      const float r2 = y0 * y0 + y1 * y1 + y2 * y2;
      const bool keyed = gr_cell(y0, g.inv_leaf, &k[0]) && gr_cell(y1, g.inv_leaf, &k[1]) && gr_cell(y2, g.inv_leaf, &k[2]);
      if (r2 > g.max_r2 || !keyed) {
        st = PFT_GROW_FAR;
      } else {
        // the MODEL key box grown by reach: outside it no MODEL voxel is the point's own or within reach
        int lo[3], hi[3];
        bool in_box = true;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
          lo[ax] = g.d->ctl.box_lo[ax];
          hi[ax] = g.d->ctl.box_hi[ax];
          in_box = in_box && lo[ax] <= hi[ax] && k[ax] >= lo[ax] - g.reach && k[ax] <= hi[ax] + g.reach;
        }
        st = PFT_GROW_UNREACHED;
        if (in_box) {
          key = gr_pack_key(k[0], k[1], k[2]);
          if (gr_is_model(g.t, key)) {
            st = PFT_GROW_KNOWN;
          } else {
            // the neighbours inside the box only (it holds every MODEL key, and its keys are below 2^20)
            const int R = g.reach;
            const int z0 = max(k[2] - R, lo[2]), z1 = min(k[2] + R, hi[2]);
            const int y0c = max(k[1] - R, lo[1]), y1c = min(k[1] + R, hi[1]);
            const int x0 = max(k[0] - R, lo[0]), x1 = min(k[0] + R, hi[0]);
            for (int mz = z0; mz <= z1 && st == PFT_GROW_UNREACHED; mz++)
              for (int my = y0c; my <= y1c && st == PFT_GROW_UNREACHED; my++)
                for (int mx = x0; mx <= x1 && st == PFT_GROW_UNREACHED; mx++) {
                  if (mx == k[0] && my == k[1] && mz == k[2]) continue;
                  if (gr_is_model(g.t, gr_pack_key(mx, my, mz))) st = PFT_GROW_CANDIDATE;
                }
          }
        }
      }
    }
  }
  g.state[i] = (uint8_t)st;
  if (st != PFT_GROW_CANDIDATE) return;
  bool claimed;
  const uint32_t s = gr_find_or_claim(g.t, key, &claimed);
  g.slot[i] = s;
  if (s == GR_NO_SLOT) {
    atomicOr(&g.d->cnt.overflow, 1u);
    return;
  }
  if (claimed) atomicAdd(&g.d->cnt.claims, 1u);
  unsigned long long old = gr_load(g.t.meta + s);
  while (!(old != 0ull && gr_seen(old) == g.a)) {  // ends: some lane's CAS sets last_seen = a
    const uint32_t hits = (old == 0ull || g.a - gr_seen(old) > g.forget) ? 1u : gr_hits(old) + 1u;
    const unsigned long long want = gr_meta(g.a, hits, PFT_GROW_KIND_PENDING);
    const unsigned long long prev = atomicCAS(g.t.meta + s, old, want);
    if (prev == old) {
      atomicAdd(&g.d->cnt.cand_voxels, 1u);
      break;
    }
    old = prev;
  }
  atomicMax(g.t.rep + s, ((unsigned long long)g.a << 32) | (unsigned long long)(0xffffffffu - i));
}

__global__ __launch_bounds__(GR_THREADS) void k_grow_confirm(GrowApplyArgs g) {
  __shared__ uint32_t su[20];
  __shared__ uint32_t cnt[PFT_GROW_N_STATES];
  __shared__ int box[6];
  const uint32_t tid = threadIdx.x, i0 = blockIdx.x * GR_TILE + tid * 4u;
  if (tid < PFT_GROW_N_STATES) cnt[tid] = 0u;
  if (tid < 3) box[tid] = INT_MAX;
  if (tid >= 3 && tid < 6) box[tid] = INT_MIN;
  __syncthreads();
  const bool overflow = g.d->cnt.overflow != 0u;  // (uniform; written by the launch before)
  uint32_t mine[4], added = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t i = i0 + q;
    mine[q] = PFT_GROW_N_STATES;
    if (i >= g.n) continue;
    uint32_t st = g.state[i];
    if (st == PFT_GROW_CANDIDATE && !overflow) {
      const uint32_t s = g.slot[i];
      if (s != GR_NO_SLOT && g.t.rep[s] == (((unsigned long long)g.a << 32) | (unsigned long long)(0xffffffffu - i))) {
        const unsigned long long m = g.t.meta[s];  // (only the representative reads or writes the word in this launch)
        if (gr_hits(m) >= g.confirm) {
          g.t.meta[s] = gr_meta(gr_seen(m), gr_hits(m), PFT_GROW_KIND_MODEL);
          st = PFT_GROW_ADDED;
          g.state[i] = (uint8_t)st;
          added++;
          int c[3];
          gr_unpack_key(g.t.key[s], c);
          for (int ax = 0; ax < 3; ax++) {
            atomicMin(&box[ax], c[ax]);
            atomicMax(&box[3 + ax], c[ax]);
          }
        }
      }
    }
    mine[q] = st;
  }
#pragma unroll
  for (uint32_t v = 0; v < PFT_GROW_N_STATES; v++) {
    const uint32_t c = wave_sum_dpp((mine[0] == v) + (mine[1] == v) + (mine[2] == v) + (mine[3] == v));
    if (lane_id() == 0 && c) atomicAdd(&cnt[v], c);
  }
  uint32_t tot;
  block_excl_scan<uint32_t, true>(added, su, &tot);
  if (tid == 0) g.tile[blockIdx.x] = tot;
  __syncthreads();
  if (tid < PFT_GROW_N_STATES && cnt[tid]) atomicAdd(&g.d->cnt.n_state[tid], cnt[tid]);
  if (tot) {
    if (tid < 3) atomicMin(&g.d->ctl.box_lo[tid], box[tid]);
    if (tid >= 3 && tid < 6) atomicMax(&g.d->ctl.box_hi[tid - 3], box[tid]);
  }
}

// cloud[n_model_points + pos] = the record of every ADDED i, in input order (tile: the scanned tile counts)
__global__ __launch_bounds__(GR_THREADS) void k_grow_emit(GrowApplyArgs g) {
  __shared__ uint32_t su[20];
  const uint32_t t = blockIdx.x, i0 = t * GR_TILE + threadIdx.x * 4u;
  uint32_t f[4], c = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    f[q] = (i0 + q < g.n && g.state[i0 + q] == PFT_GROW_ADDED) ? 1u : 0u;
    c += f[q];
  }
  uint32_t tot;
  uint32_t pos = g.d->ctl.n_model_points + g.tile[t] + block_excl_scan<uint32_t, true>(c, su, &tot);
#pragma unroll
  for (int q = 0; q < 4; q++)
    if (f[q]) {
      const float4* src = reinterpret_cast<const float4*>(g.in + i0 + q);
      const float4 p = src[0], r = src[1];
      float y0, y1, y2;
      xform(g.Ti, p.x, p.y, p.z, y0, y1, y2);
      if (pos < g.cloud_cap) {
        float4* dst = reinterpret_cast<float4*>(g.cloud + pos);
        dst[0] = make_float4(y0, y1, y2, 1.0f);
        dst[1] = make_float4(r.x, 0.0f, 0.0f, 0.0f);  // (rgba's bits, pad = 0)
      }
      pos++;
    }
}

__global__ __launch_bounds__(WAVE) void k_grow_finish(GrowDev* d, uint32_t max_voxels, uint32_t a, uint32_t n, int ran) {
  if (threadIdx.x != 0) return;
  GrowCtl& c = d->ctl;
  GrowCnt& k = d->cnt;
  const int mode = gr_rebuild_mode(c, max_voxels);
  if (mode) {
    if (c.occupied > max_voxels / 2u) c.n_rebuilds++;
    c.occupied = min(k.list_n, max_voxels);
    c.drop_pending = 0u;
  }
  c.occupied += k.claims;
  const uint32_t overflow = k.overflow ? 1u : 0u;
  const uint32_t added = (ran && !overflow) ? d->n_added : 0u;
  c.n_model_points += added;
  c.n_model_voxels += added;
  if (overflow) {
    c.drop_pending = 1u;
    c.occupied = c.n_model_voxels;
  }
  pft_grow_stats& s = d->stats;
  s.applies = a;
  s.n_in = n;
  for (int v = 0; v < PFT_GROW_N_STATES; v++) s.n_state[v] = k.n_state[v];
  s.n_candidate_voxels = overflow ? 0u : k.cand_voxels;
  s.n_added = added;
  s.n_model_points = c.n_model_points;
  s.n_model_voxels = c.n_model_voxels;
  s.n_pending_live = 0u;  // (counted by k_grow_census when the statistics are asked for)
  s.occupied = c.occupied;
  s.n_rebuilds = c.n_rebuilds;
  s.overflow = overflow;
  k.claims = k.cand_voxels = k.overflow = k.list_n = 0u;
  for (int v = 0; v < PFT_GROW_N_STATES; v++) k.n_state[v] = 0u;
}

__global__ __launch_bounds__(GR_THREADS) void k_grow_census(GrowTable t, uint32_t a, uint32_t forget, uint32_t* out) {
  uint32_t c = 0;
  for (uint32_t s = blockIdx.x * GR_THREADS + threadIdx.x; s <= t.mask; s += gridDim.x * GR_THREADS) {
    const unsigned long long m = t.meta[s];
    c += (t.key[s] != 0ull && gr_kind(m) == PFT_GROW_KIND_PENDING && a - gr_seen(m) <= forget) ? 1u : 0u;
  }
  c = wave_sum_dpp(c);
  if (lane_id() == 0 && c) atomicAdd(out, c);
}

// ---------------------------------------------------------------------------------------------------------------
// host side
struct pft_grow {
  pft_grow_config cfg = {};
  hipStream_t stream = nullptr;
  std::string err;
  float inv_leaf = 0.0f, max_r2 = 0.0f;
  float planes[PFT_GROW_MAX_PLANES][4] = {};
  int n_planes = 0;
  DevBuf<GrowDev> d_dev;
  DevBuf<unsigned long long> d_key, d_meta, d_rep, d_lkey, d_lmeta, d_lrep;
  DevBuf<pft_point_xyzrgba> d_cloud, d_in;
  DevBuf<uint8_t> d_state;
  DevBuf<uint32_t> d_slot, d_tile, d_census;
  pft_grow_stats* h_stats = nullptr;  // pinned
  uint32_t* h_census = nullptr;       // pinned
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool has_model = false, applied = false, pending = false;
  bool census_valid = false, overflow_told = true;
  uint32_t a = 0, n_initial = 0;
  size_t n_in = 0;
  float Ti[12] = {};
  pft_grow_stats stats = {};
  double last_ms = 0.0;
};

static thread_local std::string g_grow_create_err;

#define GR_GROW(g, call)                                                \
  do {                                                                  \
    if (!(call)) {                                                      \
      (g)->err = std::string(#call) + ": " + pft_dev_alloc_error();     \
      return PFT_ERR_HIP;                                               \
    }                                                                   \
  } while (0)

static GrowTable gr_table(pft_grow* g) { return GrowTable{g->d_key.get(), g->d_meta.get(), g->d_rep.get(), g->cfg.max_voxels - 1u}; }
static GrowTable gr_list(pft_grow* g) { return GrowTable{g->d_lkey.get(), g->d_lmeta.get(), g->d_lrep.get(), g->cfg.max_voxels - 1u}; }
static uint32_t gr_table_blocks(const pft_grow* g) {
  const uint32_t b = g->cfg.max_voxels / GR_THREADS;
  return b < 1u ? 1u : (b > GR_TABLE_BLOCKS ? GR_TABLE_BLOCKS : b);
}

extern "C" void pft_grow_default_config(pft_grow_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->abi_version = PFT_ABI_VERSION;
  cfg->device_id = 0;
  cfg->leaf = 0.01f;
  cfg->reach = 2;
  cfg->confirm = 3;
  cfg->forget = 2;
  cfg->max_radius = 0.5f;
  cfg->max_voxels = 1u << 18;
  cfg->plane_margin = 0.015f;
}

static int gr_refuse_create(const std::string& what) {
  g_grow_create_err = "pft_grow_create: " + what;
  return PFT_ERR_INVALID_ARG;
}

extern "C" int pft_grow_create(const pft_grow_config* cfg, pft_grow** out) {
  if (!out) return PFT_ERR_INVALID_ARG;
  *out = nullptr;
  if (!cfg || cfg->abi_version != PFT_ABI_VERSION) return gr_refuse_create("no configuration, or another abi_version");
  if (!(cfg->leaf > 0.0f) || !std::isfinite(cfg->leaf)) return gr_refuse_create("leaf must be a positive finite number");
  if (cfg->reach < 1 || cfg->reach > 4) return gr_refuse_create("reach " + std::to_string(cfg->reach) + " outside 1 .. 4");
  if (cfg->confirm < 1 || cfg->confirm > 255) return gr_refuse_create("confirm " + std::to_string(cfg->confirm) + " outside 1 .. 255");
  if (cfg->forget < 1 || cfg->forget > (1 << 20)) return gr_refuse_create("forget " + std::to_string(cfg->forget) + " outside 1 .. 2^20");
  if (!(cfg->max_radius > 0.0f) || !std::isfinite(cfg->max_radius)) return gr_refuse_create("max_radius must be a positive finite number");
  if (cfg->max_voxels < 64u || cfg->max_voxels > (1u << 22) || (cfg->max_voxels & (cfg->max_voxels - 1u)))
    return gr_refuse_create("max_voxels " + std::to_string(cfg->max_voxels) + " is not a power of two in 64 .. 2^22");
  if (!(cfg->plane_margin >= 0.0f) || !std::isfinite(cfg->plane_margin)) return gr_refuse_create("plane_margin must be finite and >= 0");
  const float inv_leaf = 1.0f / cfg->leaf, max_r2 = cfg->max_radius * cfg->max_radius;
  if (!std::isfinite(inv_leaf) || !std::isfinite(max_r2)) return gr_refuse_create("1 / leaf or max_radius^2 is not a finite float");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PFT_ERR_NO_DEVICE;  // no CPU path
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return gr_refuse_create("device " + std::to_string(cfg->device_id) + " does not exist");
  if (hipSetDevice(cfg->device_id) != hipSuccess) return PFT_ERR_NO_DEVICE;
  pft_grow* g = new pft_grow();
  g->cfg = *cfg;
  g->inv_leaf = inv_leaf;
  g->max_r2 = max_r2;
  bool ok = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) == hipSuccess;
  if (!ok) g->stream = nullptr;
  ok = ok && hipEventCreate(&g->ev0) == hipSuccess && hipEventCreate(&g->ev1) == hipSuccess;
  ok = ok && hipHostMalloc(reinterpret_cast<void**>(&g->h_stats), sizeof(pft_grow_stats), hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc(reinterpret_cast<void**>(&g->h_census), sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
  const size_t mv = cfg->max_voxels;
  ok = ok && g->d_dev.alloc(1) && g->d_census.alloc(1) && g->d_key.alloc(mv) && g->d_meta.alloc(mv) && g->d_rep.alloc(mv) &&
       g->d_lkey.alloc(mv) && g->d_lmeta.alloc(mv) && g->d_lrep.alloc(mv);
  if (!ok) {
    pft_grow_destroy(g);
    return PFT_ERR_HIP;
  }
  *out = g;
  return PFT_OK;
}

extern "C" void pft_grow_destroy(pft_grow* g) {
  if (!g) return;
  hipSetDevice(g->cfg.device_id);
  if (g->stream) hipStreamSynchronize(g->stream);
  if (g->ev0) hipEventDestroy(g->ev0);
  if (g->ev1) hipEventDestroy(g->ev1);
  if (g->h_stats) hipHostFree(g->h_stats);
  if (g->h_census) hipHostFree(g->h_census);
  if (g->stream) hipStreamDestroy(g->stream);
  delete g;  // (the DevBufs)
}

extern "C" const char* pft_grow_last_error_string(const pft_grow* g) { return g ? g->err.c_str() : g_grow_create_err.c_str(); }

extern "C" int pft_grow_set_model(pft_grow* g, const pft_point_xyzrgba* pts, size_t n) {
  if (!g || (!pts && n)) return PFT_ERR_INVALID_ARG;
  if (n > (size_t)PFT_GROW_MAX_MODEL_POINTS) {
    g->err = "pft_grow_set_model: " + std::to_string(n) + " points, the limit is PFT_GROW_MAX_MODEL_POINTS (" +
             std::to_string((size_t)PFT_GROW_MAX_MODEL_POINTS) + ")";
    return PFT_ERR_CAPACITY;
  }
  std::vector<unsigned long long> keys(n);
  GrowCtl ctl = {};
  for (int ax = 0; ax < 3; ax++) {
    ctl.box_lo[ax] = INT_MAX;
    ctl.box_hi[ax] = INT_MIN;
  }
  for (size_t i = 0; i < n; i++) {
    const float c[3] = {pts[i].x, pts[i].y, pts[i].z};
    int k[3];
    for (int ax = 0; ax < 3; ax++) {
      if (!std::isfinite(c[ax])) {
        g->err = "pft_grow_set_model: model point " + std::to_string(i) + " has a non-finite coordinate";
        return PFT_ERR_INVALID_ARG;
      }
      if (!gr_cell(c[ax], g->inv_leaf, &k[ax])) {
        g->err = "pft_grow_set_model: model point " + std::to_string(i) + " has no key (a cell index of 2^20 or more)";
        return PFT_ERR_INVALID_ARG;
      }
      ctl.box_lo[ax] = std::min(ctl.box_lo[ax], k[ax]);
      ctl.box_hi[ax] = std::max(ctl.box_hi[ax], k[ax]);
    }
    keys[i] = gr_pack_key(k[0], k[1], k[2]);
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  const size_t nv = keys.size();
  if (nv > g->cfg.max_voxels / 2u) {
    g->err = "pft_grow_set_model: " + std::to_string(nv) + " distinct voxels, the limit is max_voxels / 2 (" +
             std::to_string(g->cfg.max_voxels / 2u) + ")";
    return PFT_ERR_CAPACITY;
  }
  PFT_HIPCHK(g, hipSetDevice(g->cfg.device_id));
  hipStream_t st = g->stream;
  PFT_HIPCHK(g, hipStreamSynchronize(st));  // an apply in flight may still touch the cloud and the table
  g->has_model = false;
  g->applied = false;
  g->pending = false;
  GR_GROW(g, g->d_cloud.reserve(n + (size_t)g->cfg.max_voxels));
  const size_t mv = g->cfg.max_voxels;
  if (n) PFT_HIPCHK(g, hipMemcpyAsync(g->d_cloud, pts, n * sizeof(pft_point_xyzrgba), hipMemcpyHostToDevice, st));
  PFT_HIPCHK(g, hipMemsetAsync(g->d_key, 0, mv * sizeof(unsigned long long), st));
  PFT_HIPCHK(g, hipMemsetAsync(g->d_meta, 0, mv * sizeof(unsigned long long), st));
  PFT_HIPCHK(g, hipMemsetAsync(g->d_rep, 0, mv * sizeof(unsigned long long), st));
  GrowDev dev = {};
  ctl.occupied = ctl.n_model_voxels = (uint32_t)nv;
  ctl.n_model_points = (uint32_t)n;
  dev.ctl = ctl;
  dev.cnt.list_n = (uint32_t)nv;
  dev.stats.n_model_points = (uint32_t)n;
  dev.stats.n_model_voxels = dev.stats.occupied = (uint32_t)nv;
  PFT_HIPCHK(g, hipMemcpyAsync(g->d_dev, &dev, sizeof(dev), hipMemcpyHostToDevice, st));
  if (nv) {
    std::vector<unsigned long long> meta(nv, gr_meta(0u, 0u, PFT_GROW_KIND_MODEL));
    PFT_HIPCHK(g, hipMemcpyAsync(g->d_lkey, keys.data(), nv * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    PFT_HIPCHK(g, hipMemcpyAsync(g->d_lmeta, meta.data(), nv * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    PFT_HIPCHK(g, hipMemsetAsync(g->d_lrep, 0, nv * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_grow_insert, dim3(gr_table_blocks(g)), dim3(GR_THREADS), 0, st, (const GrowDev*)g->d_dev.get(),
                       gr_table(g), gr_list(g), 1);
  }
  // the list count goes back to zero behind the insert (the host vectors above must outlive their copies: waited for here)
  PFT_HIPCHK(g, hipMemsetAsync(&g->d_dev->cnt, 0, sizeof(GrowCnt), st));
  PFT_HIPCHK(g, hipStreamSynchronize(st));
  PFT_HIPCHK(g, hipGetLastError());
  g->stats = dev.stats;
  g->a = 0;
  g->n_initial = (uint32_t)n;
  g->n_in = 0;
  g->has_model = true;
  g->census_valid = true;  // (no PENDING voxel)
  g->overflow_told = true;
  return PFT_OK;
}

extern "C" int pft_grow_set_model_device(pft_grow* g, const pft_point_xyzrgba* device_pts, size_t n) {
  if (!g || (!device_pts && n)) return PFT_ERR_INVALID_ARG;
  if (n > (size_t)PFT_GROW_MAX_MODEL_POINTS) return pft_grow_set_model(g, nullptr, n);  // (its text)
  PFT_HIPCHK(g, hipSetDevice(g->cfg.device_id));
  std::vector<pft_point_xyzrgba> host(n);  // the keys are validated and counted on the host: set_model is rare
  if (n) PFT_HIPCHK(g, hipMemcpy(host.data(), device_pts, n * sizeof(pft_point_xyzrgba), hipMemcpyDeviceToHost));
  return pft_grow_set_model(g, host.data(), n);
}

extern "C" int pft_grow_set_planes(pft_grow* g, const float* abcd, size_t n_planes) {
  if (!g || (!abcd && n_planes)) return PFT_ERR_INVALID_ARG;
  if (n_planes > (size_t)PFT_GROW_MAX_PLANES) {
    g->err = "pft_grow_set_planes: " + std::to_string(n_planes) + " planes, the limit is PFT_GROW_MAX_PLANES (" +
             std::to_string((int)PFT_GROW_MAX_PLANES) + ")";
    return PFT_ERR_INVALID_ARG;
  }
  for (size_t k = 0; k < 4 * n_planes; k++)
    if (!std::isfinite(abcd[k])) {
      g->err = "pft_grow_set_planes: plane " + std::to_string(k / 4) + " has a non-finite coefficient";
      return PFT_ERR_INVALID_ARG;
    }
  memcpy(g->planes, abcd, 4 * n_planes * sizeof(float));
  g->n_planes = (int)n_planes;
  return PFT_OK;
}

static int gr_apply(pft_grow* g, const pft_point_xyzrgba* pts, size_t n, const float* m12, bool on_device) {
  if (!g || (!pts && n) || !m12) return PFT_ERR_INVALID_ARG;
  if (!g->has_model) {
    g->err = "pft_grow_apply before pft_grow_set_model";
    return PFT_ERR_STATE;
  }
  for (int k = 0; k < 12; k++)
    if (!std::isfinite(m12[k])) {
      g->err = "pft_grow_apply: the matrix has a non-finite entry";
      return PFT_ERR_INVALID_ARG;
    }
  if (n > (size_t)PFT_GROW_MAX_FRAME_POINTS) {
    g->err = "pft_grow_apply: " + std::to_string(n) + " frame points, the limit is PFT_GROW_MAX_FRAME_POINTS (" +
             std::to_string((size_t)PFT_GROW_MAX_FRAME_POINTS) + ")";
    return PFT_ERR_CAPACITY;
  }
  PFT_HIPCHK(g, hipSetDevice(g->cfg.device_id));
  hipStream_t st = g->stream;
  const size_t ntiles = (n + GR_TILE - 1) / GR_TILE;
  if (n > g->d_state.cap() || (!on_device && n > g->d_in.cap())) {
    PFT_HIPCHK(g, hipStreamSynchronize(st));  // a growth frees
    const size_t cap = (n + GR_TILE - 1) / GR_TILE * GR_TILE;
    if (!on_device) GR_GROW(g, g->d_in.reserve(cap));
    GR_GROW(g, g->d_slot.reserve(cap));
    GR_GROW(g, g->d_tile.reserve(cap / GR_TILE));
    GR_GROW(g, g->d_state.reserve(cap));
  }
  // Ti in double from the float entries, rounded to float
  float Ti[12];
  {
    const double t0 = m12[3], t1 = m12[7], t2 = m12[11];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) Ti[4 * r + c] = m12[4 * c + r];
      Ti[4 * r + 3] = (float)(-(((double)m12[r] * t0 + (double)m12[4 + r] * t1) + (double)m12[8 + r] * t2));
    }
  }
  const uint32_t a = g->a + 1u;
  const uint32_t tb = gr_table_blocks(g);
  GrowDev* d = g->d_dev.get();
  PFT_HIPCHK(g, hipEventRecord(g->ev0, st));
  hipLaunchKernelGGL(k_grow_gather, dim3(tb), dim3(GR_THREADS), 0, st, d, gr_table(g), gr_list(g), a, (uint32_t)g->cfg.forget);
  hipLaunchKernelGGL(k_grow_clear, dim3(tb), dim3(GR_THREADS), 0, st, (const GrowDev*)d, gr_table(g));
  hipLaunchKernelGGL(k_grow_insert, dim3(tb), dim3(GR_THREADS), 0, st, (const GrowDev*)d, gr_table(g), gr_list(g), 0);
  if (n) {
    const pft_point_xyzrgba* d_in = pts;
    if (!on_device) {
      PFT_HIPCHK(g, hipMemcpyAsync(g->d_in, pts, n * sizeof(pft_point_xyzrgba), hipMemcpyHostToDevice, st));
      d_in = g->d_in;
    }
    GrowApplyArgs q = {};
    q.in = d_in;
    q.n = (uint32_t)n;
    q.a = a;
    memcpy(q.Ti, Ti, sizeof(Ti));
    memcpy(q.planes, g->planes, sizeof(q.planes));
    q.n_planes = g->n_planes;
    q.plane_margin = g->cfg.plane_margin;
    q.inv_leaf = g->inv_leaf;
    q.max_r2 = g->max_r2;
    q.reach = g->cfg.reach;
    q.forget = (uint32_t)g->cfg.forget;
    q.confirm = (uint32_t)g->cfg.confirm;
    q.t = gr_table(g);
    q.d = d;
    q.state = g->d_state;
    q.slot = g->d_slot;
    q.tile = g->d_tile;
    q.cloud = g->d_cloud;
    q.cloud_cap = (uint32_t)g->d_cloud.cap();
    hipLaunchKernelGGL(k_grow_classify, dim3((uint32_t)((n + GR_THREADS - 1) / GR_THREADS)), dim3(GR_THREADS), 0, st, q);
    hipLaunchKernelGGL(k_grow_confirm, dim3((uint32_t)ntiles), dim3(GR_THREADS), 0, st, q);
    pftk_tile_scan(st, g->d_tile, (uint32_t)ntiles, &d->n_added);
    hipLaunchKernelGGL(k_grow_emit, dim3((uint32_t)ntiles), dim3(GR_THREADS), 0, st, q);
  }
  hipLaunchKernelGGL(k_grow_finish, dim3(1), dim3(WAVE), 0, st, d, g->cfg.max_voxels, a, (uint32_t)n, n ? 1 : 0);
  PFT_HIPCHK(g, hipMemcpyAsync(g->h_stats, &d->stats, sizeof(pft_grow_stats), hipMemcpyDeviceToHost, st));
  PFT_HIPCHK(g, hipEventRecord(g->ev1, st));
  PFT_HIPCHK(g, hipGetLastError());
  g->a = a;
  g->n_in = n;
  memcpy(g->Ti, Ti, sizeof(Ti));
  g->applied = true;
  g->pending = true;
  g->census_valid = false;
  return PFT_OK;
}

extern "C" int pft_grow_apply(pft_grow* g, const pft_point_xyzrgba* host_pts, size_t n, const float* m12) {
  return gr_apply(g, host_pts, n, m12, false);
}
extern "C" int pft_grow_apply_device(pft_grow* g, const pft_point_xyzrgba* device_pts, size_t n, const float* m12) {
  return gr_apply(g, device_pts, n, m12, true);
}

// the one host wait of an apply; need_apply: the call reads what only an apply leaves behind
static int gr_wait(pft_grow* g, const char* who, bool need_apply) {
  if (!g) return PFT_ERR_INVALID_ARG;
  if (!g->has_model || (need_apply && !g->applied)) {
    g->err = std::string(who) + (g->has_model ? " before the first pft_grow_apply" : " before pft_grow_set_model");
    return PFT_ERR_STATE;
  }
  PFT_HIPCHK(g, hipSetDevice(g->cfg.device_id));
  if (g->pending) {
    PFT_HIPCHK(g, hipStreamSynchronize(g->stream));
    PFT_HIPCHK(g, hipGetLastError());
    g->pending = false;
    g->stats = *g->h_stats;
    float ms = 0.0f;
    PFT_HIPCHK(g, hipEventElapsedTime(&ms, g->ev0, g->ev1));
    g->last_ms = ms;
    if (g->stats.overflow) {
      g->overflow_told = false;
      g->census_valid = true;  // (every PENDING voxel was dropped)
    }
  }
  return PFT_OK;
}

// the deferred error of an apply that overflowed, once
static int gr_deferred(pft_grow* g) {
  if (g->overflow_told) return PFT_OK;
  g->overflow_told = true;
  g->err = "pft_grow_apply " + std::to_string(g->stats.applies) + ": the voxel table (max_voxels = " +
           std::to_string(g->cfg.max_voxels) + ") overflowed; every pending voxel was dropped, the model is unchanged";
  return PFT_ERR_CAPACITY;
}

extern "C" int pft_grow_get_stats(pft_grow* g, pft_grow_stats* out) {
  if (!out) return PFT_ERR_INVALID_ARG;
  const int r = gr_wait(g, "pft_grow_get_stats", false);
  if (r != PFT_OK) return r;
  if (!g->census_valid) {
    hipStream_t st = g->stream;
    PFT_HIPCHK(g, hipMemsetAsync(g->d_census, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_grow_census, dim3(gr_table_blocks(g)), dim3(GR_THREADS), 0, st, gr_table(g), g->a,
                       (uint32_t)g->cfg.forget, g->d_census.get());
    PFT_HIPCHK(g, hipMemcpyAsync(g->h_census, g->d_census, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PFT_HIPCHK(g, hipStreamSynchronize(st));
    PFT_HIPCHK(g, hipGetLastError());
    g->stats.n_pending_live = *g->h_census;
    g->census_valid = true;
  }
  *out = g->stats;
  return gr_deferred(g);
}

extern "C" int pft_grow_get_states(pft_grow* g, uint8_t* host_states, size_t capacity) {
  int r = gr_wait(g, "pft_grow_get_states", true);
  if (r != PFT_OK) return r;
  if (g->n_in > capacity) {
    g->err = "pft_grow_get_states: " + std::to_string(g->n_in) + " entries, room for " + std::to_string(capacity);
    return PFT_ERR_CAPACITY;
  }
  if (g->n_in) {
    if (!host_states) return PFT_ERR_INVALID_ARG;
    PFT_HIPCHK(g, hipMemcpyAsync(host_states, g->d_state, g->n_in, hipMemcpyDeviceToHost, g->stream));
    PFT_HIPCHK(g, hipStreamSynchronize(g->stream));
  }
  return gr_deferred(g);
}

extern "C" int pft_grow_get_model(pft_grow* g, pft_point_xyzrgba* host_pts, size_t capacity, size_t* n) {
  int r = gr_wait(g, "pft_grow_get_model", false);
  if (r != PFT_OK) return r;
  const size_t cnt = g->stats.n_model_points;
  if (n) *n = cnt;
  if (cnt > capacity) {
    g->err = "pft_grow_get_model: " + std::to_string(cnt) + " points, room for " + std::to_string(capacity);
    return PFT_ERR_CAPACITY;
  }
  if (cnt) {
    if (!host_pts) return PFT_ERR_INVALID_ARG;
    PFT_HIPCHK(g, hipMemcpyAsync(host_pts, g->d_cloud, cnt * sizeof(pft_point_xyzrgba), hipMemcpyDeviceToHost, g->stream));
    PFT_HIPCHK(g, hipStreamSynchronize(g->stream));
  }
  return gr_deferred(g);
}

extern "C" int pft_grow_model_device(pft_grow* g, const pft_point_xyzrgba** device_pts, size_t* n) {
  int r = gr_wait(g, "pft_grow_model_device", false);
  if (r != PFT_OK) return r;
  if (device_pts) *device_pts = g->stats.n_model_points ? g->d_cloud.get() : nullptr;
  if (n) *n = g->stats.n_model_points;
  return gr_deferred(g);
}

extern "C" int pft_grow_get_transform(pft_grow* g, float* ti12) {
  if (!ti12) return PFT_ERR_INVALID_ARG;
  int r = gr_wait(g, "pft_grow_get_transform", true);
  if (r != PFT_OK) return r;
  memcpy(ti12, g->Ti, sizeof(g->Ti));
  return gr_deferred(g);
}

extern "C" int pft_grow_last_ms(pft_grow* g, double* ms) {
  if (!ms) return PFT_ERR_INVALID_ARG;
  int r = gr_wait(g, "pft_grow_last_ms", true);
  if (r != PFT_OK) return r;
  *ms = g->last_ms;
  return gr_deferred(g);
}

extern "C" int pft_debug_grow_get_table(pft_grow* g, int32_t* kxyz, uint32_t* kind, uint32_t* hits, uint32_t* last_seen,
                                        size_t capacity, size_t* n) {
  int r = gr_wait(g, "pft_debug_grow_get_table", false);
  if (r != PFT_OK) return r;
  const size_t mv = g->cfg.max_voxels;
  std::vector<unsigned long long> key(mv), meta(mv);
  PFT_HIPCHK(g, hipMemcpy(key.data(), g->d_key, mv * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  PFT_HIPCHK(g, hipMemcpy(meta.data(), g->d_meta, mv * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<std::pair<unsigned long long, unsigned long long>> e;
  for (size_t s = 0; s < mv; s++) {
    if (!key[s]) continue;
    const unsigned long long m = meta[s];
    const bool live = gr_kind(m) == PFT_GROW_KIND_PENDING && !g->stats.overflow && g->a - gr_seen(m) <= (uint32_t)g->cfg.forget;
    if (gr_kind(m) == PFT_GROW_KIND_MODEL || live) e.emplace_back(key[s], m);
  }
  std::sort(e.begin(), e.end());  // (the biased components order as the signed ones)
  if (n) *n = e.size();
  const size_t c = std::min(capacity, e.size());
  for (size_t j = 0; j < c; j++) {
    int k[3];
    gr_unpack_key(e[j].first, k);
    if (kxyz) memcpy(kxyz + 3 * j, k, sizeof(k));
    if (kind) kind[j] = gr_kind(e[j].second);
    if (hits) hits[j] = gr_hits(e[j].second);
    if (last_seen) last_seen[j] = gr_seen(e[j].second);
  }
  return gr_deferred(g);
}

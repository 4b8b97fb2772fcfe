// pft_subtract.hip -- scene subtraction (include/pft_subtract.h): which points of a frame do the
// tracked objects at their current poses explain, and the rest as a cloud.
//
//   k_sub_move     per slot that changed (explicit: new model, matrix or place in the pool) or per bound slot, on the
//                  bound tracker's stream: T (explicit, or pose_to_matrix(PftHeader::rep)), the moved points into the
//                  slot's segment of the pool, per-workgroup partial boxes over the finite moved points
//   k_sub_grid     one wave per moved slot: the box inflated by the radius, the grid origin and the cell side
//   k_sub_key      cell key (slot << 18 | z << 12 | y << 6 | x) of every pool point; the stable radix sort of
//                  pft_filters.hip by 24 bits keeps every slot's segment in place and orders it by cell
//   k_sub_gather   the pool in sorted order, and every non-empty cell's [start, end) in its slot's table of 64^3 cells
//   k_sub_query    the hot kernel: one frame point per lane and the box tests against the slots (LDS, wave-uniform); the
//                  few points inside a box are then served by the whole wave, one (point, slot) pair after the other:
//                  27 lanes read the 3 x 3 x 3 cell ranges, a wave scan lays the candidates out, 64 lanes test 64
//                  candidates at a time, a wave minimum returns d2; owner, d2, keep flag, tile counts, support
//   k_sub_emit     ordered compaction of the residual records and their input indices behind the segmenter's tile scan
//
// The cell is only a prune: every decision is the d2 test of the specification, so neither the cell side, the clamping of
// cell coordinates nor the order inside a cell can change a result.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "pft_devbuf.h"
#include "pft_device_utils.h"
#include "pft_tracker.h"
#include "../../include/pft_subtract.h"

#define SB_TILE 1024u
#define SB_THREADS 256
#define SB_MOVE_BLOCKS 64u        // partial boxes per slot
#define SB_AXIS_CELLS 64u         // cells per axis at most: 6 bits each, 18 bits per slot
#define SB_CELL_SLACK 1.03125f    // cell side >= radius * (1 + 2^-5): see sb_cell
#define SB_SLOTS PFT_SUBTRACT_MAX_OBJECTS
#define SB_SLOT_CELLS ((size_t)SB_AXIS_CELLS * SB_AXIS_CELLS * SB_AXIS_CELLS)  // 2^18: the low key bits

struct SubSlot {  // device: what the kernels know of a slot, indexed by slot number
  float T[12];
  float lo[3], hi[3];  // box of the finite moved points inflated by the radius; lo > hi: the slot explains nothing
  float cell, inv_cell;
  uint32_t off, n;     // the slot's segment of the pool
  uint32_t cell_off;   // the slot's 64^3 cell ranges in the cell table
};

struct SubMoveArgs {
  const float4* src;   // model: {x, y, z, .} every `stride` float4
  uint32_t stride, n;
  float T[12];
  const PftHeader* hdr;  // bound slot: T = pose_to_matrix(hdr->rep); else null
  float4* dst;           // pool + off
  SubSlot* slot;
  float* part;           // [SB_MOVE_BLOCKS][6] {min xyz, max xyz}
  uint32_t slot_no, off, cell_off;
};

// Cell coordinate on one axis: floor((v - lo) * inv) clamped to [0, 63]; monotone in v.  Two points whose computed d2 is
// below r^2 are less than r (1 + 2^-22) apart on every axis; the cell side is at least r (1 + 2^-5), so their scaled
// coordinates differ by less than 0.9697 + the two roundings of (v - lo) * inv (2^-23 of at most 65 cells each): less than
// one cell.  Their floors differ by at most 1, and clamping (monotone, 1-Lipschitz) keeps that: the 3 x 3 x 3 block around
// the query's cell holds every model point that can explain it.
__device__ __forceinline__ uint32_t sb_cell(float v, float lo, float inv) {
  const float f = floorf((v - lo) * inv);
  if (!(f > 0.0f)) return 0u;
  return (uint32_t)fminf(f, (float)(SB_AXIS_CELLS - 1u));
}

__global__ __launch_bounds__(SB_THREADS) void k_sub_move(SubMoveArgs a) {
  __shared__ float sT[12];
  __shared__ float red[SB_THREADS / WAVE][6];
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    if (a.hdr) {
      pose_to_matrix(a.hdr->rep, sT);
    } else {
      for (int k = 0; k < 12; k++) sT[k] = a.T[k];
    }
  }
  __syncthreads();
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = sT[k];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  const float w = __uint_as_float(a.slot_no);
  for (uint32_t i = blockIdx.x * SB_THREADS + tid; i < a.n; i += gridDim.x * SB_THREADS) {
    const float4 p = a.src[(size_t)i * a.stride];
    float x, y, z;
    xform(T, p.x, p.y, p.z, x, y, z);
    a.dst[i] = make_float4(x, y, z, w);
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
      mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
      mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    mn[k] = wave_min(mn[k]);
    mx[k] = wave_max(mx[k]);
  }
  if (lane_id() == 0) {
    for (int k = 0; k < 3; k++) {
      red[wave_id()][k] = mn[k];
      red[wave_id()][3 + k] = mx[k];
    }
  }
  __syncthreads();
  if (tid < 6) {
    float v = red[0][tid];
    for (int wv = 1; wv < SB_THREADS / WAVE; wv++) v = tid < 3 ? fminf(v, red[wv][tid]) : fmaxf(v, red[wv][tid]);
    a.part[blockIdx.x * 6u + tid] = v;
  }
  if (blockIdx.x == 0) {
    if (tid < 12) a.slot->T[tid] = sT[tid];
    if (tid == 12) a.slot->off = a.off;
    if (tid == 13) a.slot->n = a.n;
    if (tid == 14) a.slot->cell_off = a.cell_off;
  }
}

struct SubGridArgs {
  uint8_t nblk[SB_SLOTS];  // partial boxes of the slot's move; 0: the slot was not moved by this apply
};

// one wave per slot number: the partial boxes -> the inflated box, the cell side and its inverse
__global__ __launch_bounds__(WAVE) void k_sub_grid(SubGridArgs g, SubSlot* __restrict__ slots, const float* __restrict__ parts,
                                                   float radius) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x, nb = g.nblk[s];
  if (nb == 0) return;  // (uniform)
  const float* p = parts + (size_t)s * SB_MOVE_BLOCKS * 6u;
  float mn[3], mx[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    mn[k] = wave_min(lane < nb ? p[lane * 6u + k] : INFINITY);
    mx[k] = wave_max(lane < nb ? p[lane * 6u + 3 + k] : -INFINITY);
  }
  if (lane != 0) return;
  SubSlot* sl = slots + s;
  // the pad is above the radius by 3 %, and each bound is moved one float outwards after its rounding: no point within
  // the radius of a moved point fails the box test, at any coordinate magnitude
  const float pad = radius * SB_CELL_SLACK;
  float ext = 0.0f;
  for (int k = 0; k < 3; k++) {
    const bool any = mn[k] <= mx[k];
    const float lo = any ? nextafterf(mn[k] - pad, -INFINITY) : INFINITY;
    const float hi = any ? nextafterf(mx[k] + pad, INFINITY) : -INFINITY;
    sl->lo[k] = lo;
    sl->hi[k] = hi;
    if (any) ext = fmaxf(ext, hi - lo);
  }
  const float cell = fmaxf(pad, ext / (float)SB_AXIS_CELLS);
  sl->cell = cell;
  sl->inv_cell = 1.0f / cell;
}

__global__ __launch_bounds__(SB_THREADS) void k_sub_key(const float4* __restrict__ pool, uint32_t total,
                                                        const SubSlot* __restrict__ slots, uint32_t* __restrict__ key,
                                                        uint32_t* __restrict__ val) {
  const uint32_t i = blockIdx.x * SB_THREADS + threadIdx.x;
  if (i >= total) return;
  const float4 q = pool[i];
  const uint32_t s = __float_as_uint(q.w);
  uint32_t k = s << 18;  // a non-finite moved point: this constant, no index is formed from its coordinates (its d2 is
                         // +inf or NaN for every query, which the strict test refuses)
  if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z)) {
    const SubSlot* sl = slots + s;
    const float inv = sl->inv_cell;
    k |= sb_cell(q.x, sl->lo[0], inv) | (sb_cell(q.y, sl->lo[1], inv) << 6) | (sb_cell(q.z, sl->lo[2], inv) << 12);
  }
  key[i] = k;
  val[i] = i;
}

// cells (cleared by the host's memset: an empty cell is [0, 0)): positions relative to the slot's segment
__global__ __launch_bounds__(SB_THREADS) void k_sub_gather(const float4* __restrict__ pool, const uint32_t* __restrict__ key,
                                                           const uint32_t* __restrict__ val, uint32_t total,
                                                           const SubSlot* __restrict__ slots, float4* __restrict__ sorted,
                                                           uint32_t* __restrict__ cells) {
  const uint32_t i = blockIdx.x * SB_THREADS + threadIdx.x;
  if (i >= total) return;
  sorted[i] = pool[val[i]];
  const uint32_t k = key[i];
  const SubSlot* sl = slots + (k >> 18);
  uint32_t* range = cells + 2u * ((size_t)sl->cell_off + (k & 0x3ffffu));
  if (i == 0 || key[i - 1] != k) range[0] = i - sl->off;
  if (i + 1u == total || key[i + 1] != k) range[1] = i - sl->off + 1u;
}

struct SubQueryArgs {
  const pft_point_xyzrgba* in;
  uint32_t n;
  const SubSlot* slots;
  unsigned long long filled;  // bit s: slot s is filled
  const uint2* cells;         // [start, end) of every cell, per slot (SubSlot::cell_off)
  const float4* sorted;       // the pool in cell order
  double r2;                  // (double)radius * (double)radius
  int32_t* owner;
  float* d2;
  uint8_t* keep;
  uint32_t* tile;
  uint32_t* support;
};

__global__ __launch_bounds__(SB_THREADS) void k_sub_query(SubQueryArgs a) {
  __shared__ SubSlot ss[SB_SLOTS];
  __shared__ uint32_t wsum[SB_THREADS / WAVE];
  const uint32_t tid = threadIdx.x, lane = lane_id();
  {
    constexpr uint32_t words = sizeof(SubSlot) / 4u;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.slots);
    uint32_t* dst = reinterpret_cast<uint32_t*>(ss);
    for (uint32_t k = tid; k < SB_SLOTS * words; k += SB_THREADS)
      if ((a.filled >> (k / words)) & 1ull) dst[k] = src[k];
  }
  __syncthreads();
  uint32_t kept = 0;
  for (uint32_t k = 0; k < SB_TILE / SB_THREADS; k++) {
    const uint32_t i = blockIdx.x * SB_TILE + k * SB_THREADS + tid;
    int32_t own = -1;
    float best = INFINITY;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    unsigned long long inside = 0;  // the slots whose padded box holds the point
    if (i < a.n) {
      p = *reinterpret_cast<const float4*>(a.in + i);
      if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
        for (unsigned long long m = a.filled; m; m &= m - 1ull) {  // (uniform)
          const uint32_t s = (uint32_t)__builtin_ctzll(m);
          const SubSlot& sl = ss[s];
          if (p.x >= sl.lo[0] && p.x <= sl.hi[0] && p.y >= sl.lo[1] && p.y <= sl.hi[1] && p.z >= sl.lo[2] && p.z <= sl.hi[2])
            inside |= 1ull << s;
        }
      }
    }
    // The points inside a box are few and scattered over the waves: the wave serves them one (point, slot) pair at a time.
    // Everything that steers the two loops is scalar (a ballot, read-lanes of the leader), so all 64 lanes stay active.
    for (unsigned long long work = __ballot(inside != 0ull); work; work &= work - 1ull) {
      const int l = __builtin_ctzll(work);
      const float lx = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(p.x), l));
      const float ly = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(p.y), l));
      const float lz = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(p.z), l));
      unsigned long long lm = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(inside >> 32), l) << 32) |
                              (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)inside, l);
      for (; lm; lm &= lm - 1ull) {  // slots ascending with a strict <: a tie stays with the lowest slot
        const uint32_t s = (uint32_t)__builtin_ctzll(lm);
        const SubSlot& sl = ss[s];
        const float inv = sl.inv_cell;
        const uint32_t cx = sb_cell(lx, sl.lo[0], inv), cy = sb_cell(ly, sl.lo[1], inv), cz = sb_cell(lz, sl.lo[2], inv);
        const uint32_t ns = sl.n;
        // lanes 0 .. 26: the range of one cell of the 3 x 3 x 3 block, read once
        uint32_t start = 0, cnt = 0;
        if (lane < 27u) {
          const uint32_t xx = cx + lane % 3u - 1u, yy = cy + (lane / 3u) % 3u - 1u, zz = cz + lane / 9u - 1u;
          if (xx < SB_AXIS_CELLS && yy < SB_AXIS_CELLS && zz < SB_AXIS_CELLS) {
            const uint2 r = a.cells[(size_t)sl.cell_off + ((zz << 12) | (yy << 6) | xx)];
            if (r.x < r.y && r.y <= ns) {
              start = r.x;
              cnt = r.y - r.x;
            }
          }
        }
        const uint32_t incl = wave_incl_scan_dpp(cnt), excl = incl - cnt;
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const float4* pts = a.sorted + sl.off;
        float dmin = INFINITY;
        for (uint32_t c0 = 0; c0 < total; c0 += WAVE) {  // (uniform) 64 candidates at a time
          const uint32_t c = c0 + lane;
          uint32_t lo = 0, hi = 32;  // the first lane whose inclusive count is above c: the candidate's cell
#pragma unroll
          for (int step = 0; step < 6; step++) {  // 33 possible answers in [0, 32]: six halvings; lo == hi is a fixed point
            const uint32_t mid = (lo + hi) >> 1;
            const uint32_t v = (uint32_t)__shfl((int)incl, (int)mid);
            if (v > c) hi = mid; else lo = mid + 1u;
          }
          const uint32_t t = lo < 27u ? lo : 26u;
          const uint32_t j = (uint32_t)__shfl((int)start, (int)t) + (c - (uint32_t)__shfl((int)excl, (int)t));
          if (c < total && j < ns) {
            const float4 q = pts[j];
            const float dx = lx - q.x, dy = ly - q.y, dz = lz - q.z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            if ((double)d < a.r2) dmin = fminf(dmin, d);
          }
        }
        dmin = wave_min_dpp(dmin);
        if ((int)lane == l && dmin < best) {
          best = dmin;
          own = (int32_t)s;
        }
      }
    }
    if (i < a.n) {
      a.owner[i] = own;
      a.d2[i] = best;
      a.keep[i] = own < 0 ? 1 : 0;
      kept += own < 0 ? 1u : 0u;
    }
    // support: one atomic per wave and owning slot
    unsigned long long pend = __ballot(own >= 0);
    while (pend) {  // (uniform)
      const int l = __builtin_ctzll(pend);
      const int so = __shfl(own, l);
      const unsigned long long same = __ballot(own == so);
      if ((int)lane == l) atomicAdd(&a.support[so], (uint32_t)__popcll(same));
      pend &= ~same;
    }
  }
  const uint32_t wtot = wave_sum_dpp(kept);
  if (lane == 0) wsum[wave_id()] = wtot;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
    for (int wv = 0; wv < SB_THREADS / WAVE; wv++) t += wsum[wv];
    a.tile[blockIdx.x] = t;
  }
}

// residual[pos] = in[i], idx[pos] = i for every kept i, in input order (tile: the scanned tile counts)
__global__ __launch_bounds__(SB_THREADS) void k_sub_emit(const pft_point_xyzrgba* __restrict__ in, uint32_t n,
                                                         const uint8_t* __restrict__ keep, const uint32_t* __restrict__ tile,
                                                         pft_point_xyzrgba* __restrict__ residual, int32_t* __restrict__ idx) {
  __shared__ uint32_t su[20];
  const uint32_t t = blockIdx.x, i0 = t * SB_TILE + threadIdx.x * 4u;
  uint32_t f[4], c = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    f[k] = (i0 + k < n) ? keep[i0 + k] : 0u;
    c += f[k];
  }
  uint32_t tot;
  uint32_t pos = tile[t] + block_excl_scan<uint32_t, true>(c, su, &tot);
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (f[k]) {
      const uint32_t i = i0 + k;
      const float4* src = reinterpret_cast<const float4*>(in + i);
      float4* dst = reinterpret_cast<float4*>(residual + pos);
      dst[0] = src[0];
      dst[1] = src[1];
      idx[pos] = (int32_t)i;
      pos++;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
enum { SB_EMPTY = 0, SB_EXPLICIT = 1, SB_BOUND = 2 };

struct SubSlotHost {
  int kind = SB_EMPTY;
  DevBuf<float4> model;      // explicit: the uploaded model
  uint32_t n = 0;            // explicit: its points
  float T[12] = {};
  bool dirty = false;        // explicit: model, matrix or place in the pool changed since the last move
  pft_tracker* trk = nullptr;
  int cloud = PFT_SUBTRACT_REFERENCE_CLOUD;
  hipEvent_t moved = nullptr;  // bound: recorded on the tracker's stream behind the move
  // what the last apply used
  bool used = false;
  uint32_t used_off = 0, used_n = 0, used_cell_off = 0;
};

struct pft_subtract {
  pft_subtract_config cfg = {};
  hipStream_t stream = nullptr;
  std::string err;
  SubSlotHost slot[SB_SLOTS];
  DevBuf<SubSlot> d_slots;
  DevBuf<float> d_parts;
  DevBuf<float4> d_pool, d_sorted;
  DevBuf<uint32_t> d_key[2], d_val[2], d_hist;
  DevBuf<uint32_t> d_cells;  // [filled slots][64^3][2]: every cell's [start, end) in its slot's sorted segment
  int sort_cur = 0;
  uint32_t pool_total = 0;   // pool points of the structure on the device
  bool structure_valid = false;
  DevBuf<pft_point_xyzrgba> d_in, d_residual;
  DevBuf<int32_t> d_owner, d_res_idx;
  DevBuf<float> d_d2;
  DevBuf<uint8_t> d_keep;
  DevBuf<uint32_t> d_tile, d_support, d_nres;
  uint32_t* h_nres = nullptr;  // pinned
  hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;
  bool done_recorded = false;
  bool applied = false, pending = false;
  size_t n_in = 0, n_res = 0;
  const pft_point_xyzrgba* residual = nullptr;  // d_residual, or nothing for an empty frame
  double last_ms = 0.0;
};

static int sb_slot_arg(pft_subtract* s, int slot, const char* who) {
  if (!s) return PFT_ERR_INVALID_ARG;
  if (slot < 0 || slot >= SB_SLOTS) {
    s->err = std::string(who) + ": slot " + std::to_string(slot) + " outside [0, " + std::to_string(SB_SLOTS) + ")";
    return PFT_ERR_INVALID_ARG;
  }
  return PFT_OK;
}

static bool sb_finite12(const float* m) {
  for (int k = 0; k < 12; k++)
    if (!std::isfinite(m[k])) return false;
  return true;
}

// a growth of one of the handle's buffers: the failing call's text, PFT_ERR_HIP
#define SB_GROW(s, call)                                                \
  do {                                                                  \
    if (!(call)) {                                                      \
      (s)->err = std::string(#call) + ": " + pft_dev_alloc_error();     \
      return PFT_ERR_HIP;                                               \
    }                                                                   \
  } while (0)

extern "C" void pft_subtract_default_config(pft_subtract_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->abi_version = PFT_ABI_VERSION;
  cfg->device_id = 0;
  cfg->radius = 0.02f;
  cfg->cloud = PFT_SUBTRACT_REFERENCE_CLOUD;
}

extern "C" int pft_subtract_create(const pft_subtract_config* cfg, pft_subtract** out) {
  if (!out) return PFT_ERR_INVALID_ARG;
  *out = nullptr;
  if (!cfg || cfg->abi_version != PFT_ABI_VERSION) return PFT_ERR_INVALID_ARG;
  if (!(cfg->radius > 0.0f) || !std::isfinite(cfg->radius)) return PFT_ERR_INVALID_ARG;
  if (cfg->cloud != PFT_SUBTRACT_REFERENCE_CLOUD && cfg->cloud != PFT_SUBTRACT_REPORT_CLOUD) return PFT_ERR_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PFT_ERR_NO_DEVICE;  // no CPU path
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return PFT_ERR_INVALID_ARG;
  if (hipSetDevice(cfg->device_id) != hipSuccess) return PFT_ERR_NO_DEVICE;
  pft_subtract* s = new pft_subtract();
  s->cfg = *cfg;
  bool ok = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) == hipSuccess;
  if (!ok) s->stream = nullptr;
  ok = ok && hipEventCreate(&s->ev0) == hipSuccess && hipEventCreate(&s->ev1) == hipSuccess &&
       hipEventCreateWithFlags(&s->done, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipHostMalloc(reinterpret_cast<void**>(&s->h_nres), sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
  ok = ok && s->d_slots.alloc(SB_SLOTS) && s->d_parts.alloc((size_t)SB_SLOTS * SB_MOVE_BLOCKS * 6u) &&
       s->d_support.alloc(SB_SLOTS) && s->d_nres.alloc(1);
  if (!ok) {
    pft_subtract_destroy(s);
    return PFT_ERR_HIP;
  }
  *out = s;
  return PFT_OK;
}

extern "C" void pft_subtract_destroy(pft_subtract* s) {
  if (!s) return;
  hipSetDevice(s->cfg.device_id);
  if (s->stream) hipStreamSynchronize(s->stream);  // (every move on a tracker's stream is waited for by this stream)
  for (SubSlotHost& h : s->slot)
    if (h.moved) hipEventDestroy(h.moved);
  if (s->ev0) hipEventDestroy(s->ev0);
  if (s->ev1) hipEventDestroy(s->ev1);
  if (s->done) hipEventDestroy(s->done);
  if (s->h_nres) hipHostFree(s->h_nres);
  if (s->stream) hipStreamDestroy(s->stream);
  delete s;  // (the DevBufs)
}

extern "C" const char* pft_subtract_last_error_string(const pft_subtract* s) { return s ? s->err.c_str() : "null handle"; }

static void sb_empty_slot(SubSlotHost& h) {
  h.kind = SB_EMPTY;
  h.n = 0;
  h.dirty = false;
  h.trk = nullptr;
}

extern "C" int pft_subtract_set_object(pft_subtract* s, int slot, const pft_point_xyzrgba* pts, size_t n, const float* m12) {
  int r = sb_slot_arg(s, slot, "pft_subtract_set_object");
  if (r != PFT_OK) return r;
  if (!m12 || (!pts && n)) return PFT_ERR_INVALID_ARG;
  if (!sb_finite12(m12)) {
    s->err = "pft_subtract_set_object: the matrix has a non-finite entry";
    return PFT_ERR_INVALID_ARG;
  }
  if (n > (size_t)PFT_SUBTRACT_MAX_MODEL_POINTS) {
    s->err = "pft_subtract_set_object: " + std::to_string(n) + " model points, the limit is PFT_SUBTRACT_MAX_MODEL_POINTS (" +
             std::to_string((size_t)PFT_SUBTRACT_MAX_MODEL_POINTS) + ") for all slots together";
    return PFT_ERR_CAPACITY;
  }
  std::vector<float4> xyz(n);
  for (size_t i = 0; i < n; i++) {
    if (!std::isfinite(pts[i].x) || !std::isfinite(pts[i].y) || !std::isfinite(pts[i].z)) {
      s->err = "pft_subtract_set_object: model point " + std::to_string(i) + " has a non-finite coordinate";
      return PFT_ERR_INVALID_ARG;
    }
    xyz[i] = make_float4(pts[i].x, pts[i].y, pts[i].z, 1.0f);
  }
  PFT_HIPCHK(s, hipSetDevice(s->cfg.device_id));
  PFT_HIPCHK(s, hipStreamSynchronize(s->stream));  // a move in flight may still read the previous model
  SubSlotHost& h = s->slot[slot];
  sb_empty_slot(h);
  SB_GROW(s, h.model.reserve(n));
  if (n) PFT_HIPCHK(s, hipMemcpy(h.model, xyz.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  h.kind = SB_EXPLICIT;
  h.n = (uint32_t)n;
  memcpy(h.T, m12, sizeof(h.T));
  h.dirty = true;
  return PFT_OK;
}

extern "C" int pft_subtract_set_object_matrix(pft_subtract* s, int slot, const float* m12) {
  int r = sb_slot_arg(s, slot, "pft_subtract_set_object_matrix");
  if (r != PFT_OK) return r;
  if (!m12) return PFT_ERR_INVALID_ARG;
  if (!sb_finite12(m12)) {
    s->err = "pft_subtract_set_object_matrix: the matrix has a non-finite entry";
    return PFT_ERR_INVALID_ARG;
  }
  SubSlotHost& h = s->slot[slot];
  if (h.kind != SB_EXPLICIT) {
    s->err = "pft_subtract_set_object_matrix: slot " + std::to_string(slot) + " holds no explicit object";
    return PFT_ERR_STATE;
  }
  memcpy(h.T, m12, sizeof(h.T));
  h.dirty = true;
  return PFT_OK;
}

// the cloud of a bound tracker as it is now: PFT_ERR_STATE with a text when there is none
static int sb_bound_cloud(pft_subtract* s, const SubSlotHost& h, int slot, const float4** src, uint32_t* stride, uint32_t* n) {
  const pft_tracker* t = h.trk;
  if (h.cloud == PFT_SUBTRACT_REPORT_CLOUD) {
    if (!t->rep_n) {
      s->err = "pft_subtract: the tracker bound to slot " + std::to_string(slot) + " has no report cloud (pft_set_report_cloud)";
      return PFT_ERR_STATE;
    }
    *src = reinterpret_cast<const float4*>(t->d_rep_pts.get());
    *stride = 2u;
    *n = t->rep_n;
  } else {
    if (!t->has_ref) {
      s->err = "pft_subtract: the tracker bound to slot " + std::to_string(slot) + " has no reference cloud";
      return PFT_ERR_STATE;
    }
    *src = t->d_ref_xyz.get();
    *stride = 1u;
    *n = t->prm.M;
  }
  return PFT_OK;
}

extern "C" int pft_subtract_bind_tracker(pft_subtract* s, int slot, pft_tracker* t) {
  int r = sb_slot_arg(s, slot, "pft_subtract_bind_tracker");
  if (r != PFT_OK) return r;
  if (!t) return PFT_ERR_INVALID_ARG;
  if (t->cfg.world_size != 1) {
    s->err = "pft_subtract_bind_tracker: a sharded handle (world_size > 1) cannot be bound";
    return PFT_ERR_INVALID_ARG;
  }
  if (t->cfg.device_id != s->cfg.device_id) {
    s->err = "pft_subtract_bind_tracker: the tracker lives on device " + std::to_string(t->cfg.device_id) +
             ", the subtraction on device " + std::to_string(s->cfg.device_id);
    return PFT_ERR_INVALID_ARG;
  }
  SubSlotHost probe;
  probe.trk = t;
  probe.cloud = s->cfg.cloud;
  if (probe.cloud == PFT_SUBTRACT_REPORT_CLOUD) {
    const float4* src;
    uint32_t stride, n;
    r = sb_bound_cloud(s, probe, slot, &src, &stride, &n);
    if (r != PFT_OK) return r;
  }
  PFT_HIPCHK(s, hipSetDevice(s->cfg.device_id));
  SubSlotHost& h = s->slot[slot];
  if (!h.moved) PFT_HIPCHK(s, hipEventCreateWithFlags(&h.moved, hipEventDisableTiming));
  sb_empty_slot(h);
  h.kind = SB_BOUND;
  h.trk = t;
  h.cloud = s->cfg.cloud;
  return PFT_OK;
}

extern "C" int pft_subtract_remove_object(pft_subtract* s, int slot) {
  int r = sb_slot_arg(s, slot, "pft_subtract_remove_object");
  if (r != PFT_OK) return r;
  sb_empty_slot(s->slot[slot]);
  return PFT_OK;
}

extern "C" int pft_subtract_clear(pft_subtract* s) {
  if (!s) return PFT_ERR_INVALID_ARG;
  for (SubSlotHost& h : s->slot) sb_empty_slot(h);
  return PFT_OK;
}

static int sb_apply(pft_subtract* s, const pft_point_xyzrgba* pts, size_t n, bool on_device) {
  if (!s || (!pts && n)) return PFT_ERR_INVALID_ARG;
  s->applied = false;  // (an apply that is refused leaves no result behind)
  s->pending = false;
  if (n > (size_t)PFT_SUBTRACT_MAX_FRAME_POINTS) {
    s->err = "pft_subtract_apply: " + std::to_string(n) + " frame points, the limit is PFT_SUBTRACT_MAX_FRAME_POINTS (" +
             std::to_string((size_t)PFT_SUBTRACT_MAX_FRAME_POINTS) + ")";
    return PFT_ERR_CAPACITY;
  }
  // 1. every refusal before anything is enqueued: the slots' clouds as they are now, the pool's layout (slots ascending)
  struct Plan {
    const float4* src;
    uint32_t stride, n, off, cell_off;
    bool move;
  } plan[SB_SLOTS] = {};
  unsigned long long filled = 0;
  size_t total = 0, n_filled = 0;
  for (int k = 0; k < SB_SLOTS; k++) {
    SubSlotHost& h = s->slot[k];
    if (h.kind == SB_EMPTY) continue;
    Plan& p = plan[k];
    if (h.kind == SB_BOUND) {
      if (!h.trk->initialized) {
        s->err = "pft_subtract_apply: the tracker bound to slot " + std::to_string(k) +
                 " has not run a pft_compute since it was created or reset: there is no result pose";
        return PFT_ERR_STATE;
      }
      const int r = sb_bound_cloud(s, h, k, &p.src, &p.stride, &p.n);
      if (r != PFT_OK) return r;
    } else {
      p.src = h.model.get();
      p.stride = 1u;
      p.n = h.n;
    }
    p.off = (uint32_t)total;
    p.cell_off = (uint32_t)(n_filled++ * SB_SLOT_CELLS);
    total += p.n;
    filled |= 1ull << k;
  }
  if (total > (size_t)PFT_SUBTRACT_MAX_MODEL_POINTS) {
    s->err = "pft_subtract_apply: " + std::to_string(total) + " model points in the filled slots together, the limit is " +
             "PFT_SUBTRACT_MAX_MODEL_POINTS (" + std::to_string((size_t)PFT_SUBTRACT_MAX_MODEL_POINTS) + ")";
    return PFT_ERR_CAPACITY;
  }
  PFT_HIPCHK(s, hipSetDevice(s->cfg.device_id));
  hipStream_t st = s->stream;
  // 2. buffers.  A growth frees: the stream is drained first (it has waited for every move on a tracker's stream)
  const size_t ntiles = (n + SB_TILE - 1) / SB_TILE;
  const size_t hist_words = 256u * ((total + 1023u) / 1024u) + 256u;
  const size_t cell_words = 2u * n_filled * SB_SLOT_CELLS;
  const bool grow_pool = total > s->d_val[1].cap() || hist_words > s->d_hist.cap() || cell_words > s->d_cells.cap();
  const bool grow_frame = n > s->d_keep.cap() || ntiles > s->d_tile.cap() || (!on_device && n > s->d_in.cap());
  if (grow_pool || grow_frame) PFT_HIPCHK(s, hipStreamSynchronize(st));
  if (grow_pool) {
    s->structure_valid = false;
    for (SubSlotHost& h : s->slot) h.used = false;  // (the pool's contents go with it: every slot is moved again)
    s->d_val[1].reset();                            // (the group's capacity: zero until all are there)
    const size_t cap = total + total / 2u + 1024u;
    SB_GROW(s, s->d_cells.reserve(cell_words));
    SB_GROW(s, s->d_pool.alloc(cap));
    SB_GROW(s, s->d_sorted.alloc(cap));
    SB_GROW(s, s->d_key[0].alloc(cap));
    SB_GROW(s, s->d_key[1].alloc(cap));
    SB_GROW(s, s->d_val[0].alloc(cap));
    SB_GROW(s, s->d_hist.alloc(256u * ((cap + 1023u) / 1024u) + 256u));
    SB_GROW(s, s->d_val[1].alloc(cap));
  }
  if (grow_frame) {
    s->applied = false;
    s->d_keep.reset();  // (the group's capacity)
    const size_t cap = (n + SB_TILE - 1) / SB_TILE * SB_TILE;
    if (!on_device || s->d_in.cap()) SB_GROW(s, s->d_in.alloc(cap));
    SB_GROW(s, s->d_residual.alloc(cap));
    SB_GROW(s, s->d_owner.alloc(cap));
    SB_GROW(s, s->d_res_idx.alloc(cap));
    SB_GROW(s, s->d_d2.alloc(cap));
    SB_GROW(s, s->d_tile.alloc(cap / SB_TILE));
    SB_GROW(s, s->d_keep.alloc(cap));
  }
  if (!on_device && n > s->d_in.cap()) {  // (a handle that only saw device clouds so far)
    PFT_HIPCHK(s, hipStreamSynchronize(st));
    SB_GROW(s, s->d_in.alloc(s->d_keep.cap()));
  }
  s->applied = false;
  s->pending = false;
  PFT_HIPCHK(s, hipEventRecord(s->ev0, st));
  // 3. the moves: a bound slot on its tracker's stream (behind the pft_compute calls made so far, and behind this
  // handle's last apply, which may still read the pool), an explicit slot that changed on this stream
  SubGridArgs g = {};
  bool rebuilt = !s->structure_valid || (uint32_t)total != s->pool_total;
  for (int k = 0; k < SB_SLOTS; k++) {
    SubSlotHost& h = s->slot[k];
    if (h.kind == SB_EMPTY) {
      h.used = false;
      continue;
    }
    Plan& p = plan[k];
    p.move = h.kind == SB_BOUND || h.dirty || !h.used || h.used_off != p.off || h.used_n != p.n || h.used_cell_off != p.cell_off;
    if (!p.move) continue;
    rebuilt = true;
    SubMoveArgs a = {};
    a.src = p.src;
    a.stride = p.stride;
    a.n = p.n;
    memcpy(a.T, h.T, sizeof(a.T));
    a.hdr = h.kind == SB_BOUND ? h.trk->d_hdr.get() : nullptr;
    a.dst = s->d_pool.get() + p.off;
    a.slot = s->d_slots.get() + k;
    a.part = s->d_parts.get() + (size_t)k * SB_MOVE_BLOCKS * 6u;
    a.slot_no = (uint32_t)k;
    a.off = p.off;
    a.cell_off = p.cell_off;
    uint32_t nblk = (p.n + SB_THREADS - 1) / SB_THREADS;
    nblk = nblk < 1u ? 1u : (nblk > SB_MOVE_BLOCKS ? SB_MOVE_BLOCKS : nblk);
    g.nblk[k] = (uint8_t)nblk;
    hipStream_t ms = st;
    if (h.kind == SB_BOUND) {
      ms = h.trk->stream;
      if (s->done_recorded) PFT_HIPCHK(s, hipStreamWaitEvent(ms, s->done, 0));
    }
    hipLaunchKernelGGL(k_sub_move, dim3(nblk), dim3(SB_THREADS), 0, ms, a);
    if (h.kind == SB_BOUND) {
      PFT_HIPCHK(s, hipEventRecord(h.moved, ms));
      PFT_HIPCHK(s, hipStreamWaitEvent(st, h.moved, 0));
    }
    h.dirty = false;
    h.used = true;
    h.used_off = p.off;
    h.used_n = p.n;
    h.used_cell_off = p.cell_off;
  }
  // 4. the search structure, when anything moved
  if (rebuilt) {
    s->structure_valid = false;
    if (filled) hipLaunchKernelGGL(k_sub_grid, dim3(SB_SLOTS), dim3(WAVE), 0, st, g, s->d_slots.get(),
                                   (const float*)s->d_parts.get(), s->cfg.radius);
    if (total) {
      const uint32_t nb = (uint32_t)((total + SB_THREADS - 1) / SB_THREADS);
      hipLaunchKernelGGL(k_sub_key, dim3(nb), dim3(SB_THREADS), 0, st, (const float4*)s->d_pool.get(), (uint32_t)total,
                         (const SubSlot*)s->d_slots.get(), s->d_key[0].get(), s->d_val[0].get());
      uint32_t* key[2] = {s->d_key[0].get(), s->d_key[1].get()};
      uint32_t* val[2] = {s->d_val[0].get(), s->d_val[1].get()};
      s->sort_cur = pftk_radix_sort_pairs(st, key, val, (uint32_t)total, 24, s->d_hist.get());
      PFT_HIPCHK(s, hipMemsetAsync(s->d_cells, 0, cell_words * sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_sub_gather, dim3(nb), dim3(SB_THREADS), 0, st, (const float4*)s->d_pool.get(),
                         (const uint32_t*)s->d_key[s->sort_cur].get(), (const uint32_t*)s->d_val[s->sort_cur].get(),
                         (uint32_t)total, (const SubSlot*)s->d_slots.get(), s->d_sorted.get(), s->d_cells.get());
    }
    s->pool_total = (uint32_t)total;
    s->structure_valid = true;
  }
  // 5. the query and the compaction
  PFT_HIPCHK(s, hipMemsetAsync(s->d_support, 0, SB_SLOTS * sizeof(uint32_t), st));
  const pft_point_xyzrgba* d_in = pts;
  if (n == 0) {
    PFT_HIPCHK(s, hipMemsetAsync(s->d_nres, 0, sizeof(uint32_t), st));
  } else {
    if (!on_device) {
      PFT_HIPCHK(s, hipMemcpyAsync(s->d_in, pts, n * sizeof(pft_point_xyzrgba), hipMemcpyHostToDevice, st));
      d_in = s->d_in;
    }
    SubQueryArgs q = {};
    q.in = d_in;
    q.n = (uint32_t)n;
    q.slots = s->d_slots;
    q.filled = filled;
    q.cells = reinterpret_cast<const uint2*>(s->d_cells.get());
    q.sorted = s->d_sorted;
    q.r2 = (double)s->cfg.radius * (double)s->cfg.radius;
    q.owner = s->d_owner;
    q.d2 = s->d_d2;
    q.keep = s->d_keep;
    q.tile = s->d_tile;
    q.support = s->d_support;
    hipLaunchKernelGGL(k_sub_query, dim3((uint32_t)ntiles), dim3(SB_THREADS), 0, st, q);
    pftk_tile_scan(st, s->d_tile, (uint32_t)ntiles, s->d_nres);
    hipLaunchKernelGGL(k_sub_emit, dim3((uint32_t)ntiles), dim3(SB_THREADS), 0, st, d_in, (uint32_t)n,
                       (const uint8_t*)s->d_keep.get(), (const uint32_t*)s->d_tile.get(), s->d_residual.get(),
                       s->d_res_idx.get());
  }
  PFT_HIPCHK(s, hipMemcpyAsync(s->h_nres, s->d_nres, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  PFT_HIPCHK(s, hipEventRecord(s->ev1, st));
  PFT_HIPCHK(s, hipEventRecord(s->done, st));
  s->done_recorded = true;
  PFT_HIPCHK(s, hipGetLastError());
  s->n_in = n;
  s->residual = n ? s->d_residual.get() : nullptr;
  s->applied = true;
  s->pending = true;
  return PFT_OK;
}

extern "C" int pft_subtract_apply(pft_subtract* s, const pft_point_xyzrgba* host_pts, size_t n) {
  return sb_apply(s, host_pts, n, false);
}
extern "C" int pft_subtract_apply_device(pft_subtract* s, const pft_point_xyzrgba* device_pts, size_t n) {
  return sb_apply(s, device_pts, n, true);
}

// the one host wait of an apply
static int sb_wait(pft_subtract* s, const char* who) {
  if (!s) return PFT_ERR_INVALID_ARG;
  if (!s->applied) {
    s->err = std::string(who) + " before the first pft_subtract_apply (or after one that failed)";
    return PFT_ERR_STATE;
  }
  PFT_HIPCHK(s, hipSetDevice(s->cfg.device_id));
  if (s->pending) {
    PFT_HIPCHK(s, hipStreamSynchronize(s->stream));
    PFT_HIPCHK(s, hipGetLastError());
    s->pending = false;
    s->n_res = *s->h_nres;
    float ms = 0.0f;
    PFT_HIPCHK(s, hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->last_ms = ms;
  }
  return PFT_OK;
}

extern "C" int pft_subtract_counts(pft_subtract* s, size_t* n_in, size_t* n_explained, size_t* n_residual) {
  const int r = sb_wait(s, "pft_subtract_counts");
  if (r != PFT_OK) return r;
  if (n_in) *n_in = s->n_in;
  if (n_explained) *n_explained = s->n_in - s->n_res;
  if (n_residual) *n_residual = s->n_res;
  return PFT_OK;
}

template <typename T>
static int sb_get(pft_subtract* s, const char* who, const T* src, size_t cnt, T* host_out, size_t capacity, size_t* n) {
  const int r = sb_wait(s, who);
  if (r != PFT_OK) return r;
  if (n) *n = cnt;
  if (cnt > capacity) {
    s->err = std::string(who) + ": " + std::to_string(cnt) + " entries, room for " + std::to_string(capacity);
    return PFT_ERR_CAPACITY;
  }
  if (!cnt) return PFT_OK;
  if (!host_out) return PFT_ERR_INVALID_ARG;
  PFT_HIPCHK(s, hipMemcpyAsync(host_out, src, cnt * sizeof(T), hipMemcpyDeviceToHost, s->stream));
  PFT_HIPCHK(s, hipStreamSynchronize(s->stream));
  return PFT_OK;
}

extern "C" int pft_subtract_get_owner(pft_subtract* s, int32_t* out, size_t capacity) {
  return sb_get<int32_t>(s, "pft_subtract_get_owner", s ? s->d_owner.get() : nullptr, s ? s->n_in : 0, out, capacity, nullptr);
}
extern "C" int pft_subtract_get_sq_dist(pft_subtract* s, float* out, size_t capacity) {
  return sb_get<float>(s, "pft_subtract_get_sq_dist", s ? s->d_d2.get() : nullptr, s ? s->n_in : 0, out, capacity, nullptr);
}
extern "C" int pft_subtract_get_support(pft_subtract* s, uint32_t* out, size_t capacity) {
  return sb_get<uint32_t>(s, "pft_subtract_get_support", s ? s->d_support.get() : nullptr, SB_SLOTS, out, capacity, nullptr);
}
extern "C" int pft_subtract_get_residual(pft_subtract* s, pft_point_xyzrgba* out, size_t capacity, size_t* n) {
  const int r = sb_wait(s, "pft_subtract_get_residual");
  if (r != PFT_OK) return r;
  return sb_get<pft_point_xyzrgba>(s, "pft_subtract_get_residual", s->residual, s->n_res, out, capacity, n);
}
extern "C" int pft_subtract_get_residual_indices(pft_subtract* s, int32_t* out, size_t capacity, size_t* n) {
  const int r = sb_wait(s, "pft_subtract_get_residual_indices");
  if (r != PFT_OK) return r;
  return sb_get<int32_t>(s, "pft_subtract_get_residual_indices", s->d_res_idx.get(), s->n_res, out, capacity, n);
}

extern "C" int pft_subtract_residual_device(pft_subtract* s, const pft_point_xyzrgba** device_pts, size_t* n) {
  const int r = sb_wait(s, "pft_subtract_residual_device");
  if (r != PFT_OK) return r;
  if (device_pts) *device_pts = s->n_res ? s->residual : nullptr;
  if (n) *n = s->n_res;
  return PFT_OK;
}

extern "C" int pft_subtract_get_object(pft_subtract* s, int slot, float* m12, float* moved_xyz, size_t capacity, size_t* n) {
  int r = sb_slot_arg(s, slot, "pft_subtract_get_object");
  if (r != PFT_OK) return r;
  r = sb_wait(s, "pft_subtract_get_object");
  if (r != PFT_OK) return r;
  const SubSlotHost& h = s->slot[slot];
  if (h.kind == SB_EMPTY || !h.used) {
    s->err = "pft_subtract_get_object: slot " + std::to_string(slot) + " was not filled at the last apply";
    return PFT_ERR_STATE;
  }
  if (n) *n = h.used_n;
  if (m12) PFT_HIPCHK(s, hipMemcpy(m12, s->d_slots.get() + slot, 12 * sizeof(float), hipMemcpyDeviceToHost));
  const size_t c = capacity < h.used_n ? capacity : h.used_n;
  if (moved_xyz && c) {
    std::vector<float4> tmp(c);
    PFT_HIPCHK(s, hipMemcpy(tmp.data(), s->d_pool.get() + h.used_off, c * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < c; i++) {
      moved_xyz[3 * i] = tmp[i].x;
      moved_xyz[3 * i + 1] = tmp[i].y;
      moved_xyz[3 * i + 2] = tmp[i].z;
    }
  }
  return PFT_OK;
}

extern "C" int pft_subtract_last_ms(pft_subtract* s, double* ms) {
  if (!ms) return PFT_ERR_INVALID_ARG;
  const int r = sb_wait(s, "pft_subtract_last_ms");
  if (r != PFT_OK) return r;
  *ms = s->last_ms;
  return PFT_OK;
}

// pft_api.hip -- the core of the extern "C" boundary declared in include/pft.h: names and strings, config defaults, the KLD
// helpers, profiling, the device allocator behind pft_devbuf.h, handle lifetime, the path switches, reference and input
// clouds, the hand-offs from a filter and a model, particles and result.  The frame itself is pft_frame.hip, the test
// hooks pft_api_debug.hip, the optional features pft_api_features.hip; the handle is defined in pft_tracker.h.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "pft_tracker.h"

static const char* k_names[PFT_K_COUNT] = {"resample", "aabb", "crop", "octree", "likelihood", "population", "pack"};

extern "C" const char* pft_kernel_name(int id) { return (id >= 0 && id < PFT_K_COUNT) ? k_names[id] : "?"; }

extern "C" const char* pft_status_string(int s) {
  switch (s) {
    case PFT_OK: return "ok";
    case PFT_ERR_INVALID_ARG: return "invalid argument";
    case PFT_ERR_NO_INPUT: return "no input cloud";
    case PFT_ERR_NO_REFERENCE: return "no reference cloud";
    case PFT_ERR_NO_DEVICE: return "no usable HIP device (there is no CPU fallback)";
    case PFT_ERR_HIP: return "HIP error";
    case PFT_ERR_CAPACITY: return "capacity exceeded";
    case PFT_ERR_STATE: return "invalid state";
    case PFT_ERR_LOST: return "object not recognized";
  }
  return "unknown";
}

extern "C" void pft_config_default(pft_config* c) {
  memset(c, 0, sizeof(*c));
  c->abi_version = PFT_ABI_VERSION;
  c->device_id = 0;
  c->stream = nullptr;
  c->stream_is_external = 0;
  c->particle_num = 400;
  c->iteration_num = 2;
  for (int k = 0; k < 6; k++) {
    c->step_noise_cov[k] = 0.015 * 0.015;
    c->initial_noise_cov[k] = 0.00001;
    c->initial_noise_mean[k] = 0.0;
  }
  c->step_noise_cov[3] *= 40.0;
  c->step_noise_cov[4] *= 40.0;
  c->step_noise_cov[5] *= 40.0;
  c->alpha = 15.0;
  c->resample_likelihood_thr = 0.0;
  c->max_distance = 0.1;
  c->octree_resolution = 0.01;
  c->distance_weight = 1.0;
  c->hsv_weight = 0.1;
  c->h_weight = 1.0;
  c->s_weight = 1.0;
  c->v_weight = 0.0;
  c->hsv_pcl180_argorder = 1;
  c->use_normal = 0;
  c->seed = 1;
  c->rank = 0;
  c->world_size = 1;
  c->kld_adaptive = 0;            // the north_star path is the fixed tracker; auto_tracking.cpp:207-222 for the KLD one
  c->maximum_particle_num = 500;  // :209
  c->kld_delta = 0.99;            // :210
  c->kld_epsilon = 0.2;           // :211
  for (int k = 0; k < 6; k++) c->kld_bin_size[k] = 0.1;  // :212-219
  c->motion_ratio = 0.25;
  c->exact_nearest = 0;  // ApproxNearestPairPointCloudCoherence, as the reference runs (:235-236)
  c->sum_order = PFT_SUM_TREE;
}

// KLDAdaptiveParticleFilterTracker::normalQuantile (kld_adaptive_particle_filter.h): despite its name the polynomial
// normal CDF of CACM Algorithm 209; host-side double arithmetic, handed to the resample kernel as a constant
extern "C" double pft_kld_normal_quantile(double u) {
  static const double a[9] = {1.24818987e-4, -1.075204047e-3, 5.198775019e-3, -0.019198292004, 0.059054035642,
                              -0.151968751364, 0.319152932694, -0.5319230073, 0.797884560593};
  static const double b[15] = {-4.5255659e-5, 1.5252929e-4, -1.9538132e-5, -6.76904986e-4, 1.390604284e-3,
                               -7.9462082e-4, -2.034254874e-3, 6.549791214e-3, -0.010557625006, 0.011630447319,
                               -9.279453341e-3, 5.353579108e-3, -2.141268741e-3, 5.35310849e-4, 9.99936657524e-1};
  double w, y, z;
  if (u == 0.) return 0.5;
  y = u / 2.0;
  if (y < -6.) return 0.0;
  if (y > 6.) return 1.0;
  if (y < 0.) y = -y;
  if (y < 1.) {
    w = y * y;
    z = a[0];
    for (int i = 1; i < 9; i++) z = z * w + a[i];
    z *= (y * 2.0);
  } else {
    y -= 2.0;
    z = b[0];
    for (int i = 1; i < 15; i++) z = z * y + b[i];
  }
  if (u < 0.0) return (1. - z) / 2.0;
  return (1. + z) / 2.0;
}

extern "C" double pft_kld_bound(int k, double delta, double epsilon) {
  const double z = pft_kld_normal_quantile(delta);
  const double chi = 1.0 - 2.0 / (9.0 * (k - 1)) + sqrt(2.0 / (9.0 * (k - 1))) * z;
  return ((k - 1.0) / 2.0 / epsilon) * chi * chi * chi;
}

// ---- host-side A1 / A0 helpers (toEigenMatrix / toState), float like PCL ----
extern "C" void pft_to_matrix(const pft_particle* p, float m[16]) {
  float A = cosf(p->yaw), B = sinf(p->yaw), C = cosf(p->pitch), D = sinf(p->pitch);
  float E = cosf(p->roll), F = sinf(p->roll), DE = D * E, DF = D * F;
  m[0] = A * C;  m[1] = A * DF - B * E;  m[2] = B * F + A * DE;  m[3] = p->x;
  m[4] = B * C;  m[5] = A * E + B * DF;  m[6] = B * DE - A * F;  m[7] = p->y;
  m[8] = -D;     m[9] = C * F;           m[10] = C * E;          m[11] = p->z;
  m[12] = 0;     m[13] = 0;              m[14] = 0;              m[15] = 1;
}

extern "C" void pft_to_state(const float m[16], pft_particle* out) {
  memset(out, 0, sizeof(*out));
  out->x = m[3];
  out->y = m[7];
  out->z = m[11];
  out->w = 1.0f;
  out->roll = atan2f(m[9], m[10]);
  out->pitch = asinf(-m[8]);
  out->yaw = atan2f(m[4], m[0]);
}

// ---- profiling (ProfScope: pft_tracker.h) ----
static void prof_collect(pft_tracker* t) {
  hipStreamSynchronize(t->stream);
  for (int k = 0; k < PFT_K_COUNT; k++) {
    for (auto& p : t->ev[k]) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
        t->prof_ms[k] += ms;
        t->prof_n[k] += 1;
      }
      t->ev_free.push_back(p);
    }
    t->ev[k].clear();
  }
}

extern "C" int pft_profile_enable(pft_tracker* t, int on) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!on && t->prof) prof_collect(t);
  t->prof = on != 0;
  return PFT_OK;
}
extern "C" int pft_profile_get(pft_tracker* t, int id, double* total_ms, uint64_t* launches) {
  if (!t || id < 0 || id >= PFT_K_COUNT) return PFT_ERR_INVALID_ARG;
  prof_collect(t);
  if (total_ms) *total_ms = t->prof_ms[id];
  if (launches) *launches = t->prof_n[id];
  return PFT_OK;
}
extern "C" int pft_profile_reset(pft_tracker* t) {
  if (!t) return PFT_ERR_INVALID_ARG;
  prof_collect(t);
  for (int k = 0; k < PFT_K_COUNT; k++) {
    t->prof_ms[k] = 0;
    t->prof_n[k] = 0;
  }
  return PFT_OK;
}

// ---- allocation: the library's side of pft_devbuf.h, shared by the four handles ----
static thread_local hipError_t g_alloc_error = hipSuccess;
int pft_dev_alloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    *p = nullptr;
    g_alloc_error = e;
    (void)hipGetLastError();  // the failure is reported by the caller: it must not surface again in a later launch check
  }
  return (int)e;
}
void pft_dev_free(void* p) { hipFree(p); }
const char* pft_dev_alloc_error() { return hipGetErrorString(g_alloc_error); }

void pftt_sync_dev(pft_tracker* t) {
  PftDev& d = t->dev;
  d.ref_xyz = t->d_ref_xyz;
  d.ref_box = t->d_ref_box;
  d.ref_hsv = t->d_ref_hsv;
  d.in_pts = t->d_in_pts;
  d.N = t->N;
  d.n_dev = t->n_on_device ? t->d_n_in : nullptr;
  d.part_cur = t->d_part[t->cur];
  d.part_all = t->bound_gathered ? static_cast<pft_particle*>(t->bound_gathered) : t->d_part[t->cur];
  d.mats = t->d_mats;
  d.bbox_part = t->d_bbox_part;
  d.bbox_grid = (uint32_t)t->num_cus;
  d.bbox_part_cap = (uint32_t)(t->d_bbox_part.cap() / 6u);
  d.bbox6 = t->bound_bbox6 ? static_cast<float*>(t->bound_bbox6) : t->d_bbox6;
  d.crop_counts = t->d_crop_counts;
  d.crop_slots = t->d_crop_slots;
  d.crop_pts = t->d_crop_pts;
  d.crop_idx = t->d_crop_idx;
  d.words = t->d_words;
  d.max_words = t->max_words;
  d.jump = t->d_jump;
  d.anc = t->d_anc;
  d.ref_perm = t->d_ref_perm;
  d.leaf_pts = t->d_leaf_pts;
  d.leaf_order = t->d_leaf_order;
  d.pt_node = t->d_pt_node;
  d.pt_key = t->d_pt_key;
  d.pt_tmp = t->d_pt_tmp;
  d.pt_key64 = t->d_pt_key64;
  d.host_stat = t->h_stat;
  d.partial = t->d_partial;
  d.alias_list = t->d_alias_list;
  d.alias_pref = t->d_alias_pref;
  d.pop_part = t->d_pop_part;
  d.p_active = t->prm.kld ? &t->d_hdr->p_active : nullptr;
  d.eg_start = t->d_eg_start;
  d.eg_cnt = t->d_eg_cnt;
  d.eg_tile = t->d_eg_tile;
  d.eg_cap = t->d_eg_start ? PFT_EG_CAP : 0u;
  d.ec_slot = t->d_ec_slot;
  d.ec_cells = t->d_ec_cells;
  d.ec_count = t->d_ec_count;
  d.ec_base = t->d_ec_base;
  d.ec_list = t->d_ec_list;
  d.ec_pool_cap = (uint32_t)t->d_ec_list.cap();
  d.ec_slots_cap = t->ec_slots_cap;
  d.eq_cellq = t->d_eq_cellq;
  d.eq_nq = t->d_eq_nq;
  d.eq_qbase = t->d_eq_qbase;
  d.eq_bbase = t->d_eq_bbase;
  d.eq_fill = t->d_eq_fill;
  d.eq_blk = t->d_eq_blk;
  d.eq_sorted = t->d_eq_sorted;
  d.eq_out = t->d_eq_out;
  d.eq_cap = t->eq_cap;
  d.eq_blk_cap = t->eq_blk_cap;
  d.eq_tiles = t->d_eq_tiles;
  d.eq_tiles_cap = t->eq_tiles_cap;
  d.kld_table = t->d_kld_table;
  d.kld_bins = t->d_kld_bins;
  d.alias_pos = t->d_alias_pos;
  d.raw_w = t->d_raw_w;
  d.hdr = t->d_hdr;
  d.nn_idx = t->d_nn_idx;
  d.nn_d2 = t->d_nn_d2;
  d.gate = t->gate_on ? &t->cd.b.st->gate : nullptr;
}

// Device-side failures (PftHeader::error: octree capacity, depth / growth overflow, the one-pass crop's bounded wait)
// make the likelihood launch of that iteration run without a target -- all weights zero, the update degenerates to
// the unweighted mean.  The likelihood kernel mirrors the flags into pinned host memory; every host synchronisation
// point calls this AFTER the stream has drained and hands the failure to the caller (the reference's caller looks for
// one: auto_tracking.cpp:692-696).  The flags are per iteration, so the next compute() starts clean.
int pftt_check_device_error(pft_tracker* t) {
  volatile uint32_t* hs = t->h_stat;
  const uint32_t e = hs ? hs[3] : 0u;
  if (!e) return PFT_OK;
  hs[3] = 0u;
  std::string m = "device error flag(s) raised since the last check:";
  if (e & 1u) m += " [bit0] octree node capacity exceeded (more than 8 x input points + 64 words, or 2^24 nodes);";
  if (e & 2u) m += " [bit1] octree depth / bounding-box growth steps exceeded (PFT_MAX_DEPTH 30, PFT_MAX_GROW 40);";
  if (e & 4u) m += " [bit2] the one-pass crop gave up waiting for a predecessor workgroup;";
  if (e & 16u)
    m += " [bit4] a device-scope barrier of the population kernel timed out (its workgroups did not become co-resident "
         "within the spin limit): that iteration's normalisation, weighted mean and alias table were NOT written -- the "
         "weights, the result pose and the resampling table are those of the last completed iteration;";
  if (e & 32u)
    m += " [bit5] the change detector's octree outgrew 21-bit keys or its growth steps per test (PFT_MAX_GROW 40): that "
         "iteration evaluated as if the scene had changed, and the detector forgot its previous crop (its box is never reset: "
         "once deeper than 21 levels, every later test does the same);";
  if (e & 64u)
    m += " [bit6] pft_set_input_from_filter: the filter's output count on the device exceeded max_points; the crop read "
         "max_points points only;";
  if (e & 128u)
    m += " [bit7] pft_set_input_from_filter: the filter's output count on the device was zero (no input cloud): the "
         "iterations ran with an empty crop;";
  if (e & ~247u) m += " [other] " + std::to_string(e & ~247u) + ";";
  if (e & 7u) m += " the iteration(s) with bit0-2 ran without a target cloud (all likelihoods zero)";
  if (e & 16u) {  // the barrier counters of an interrupted launch are cleared before the next one (the launch resets them itself
                  // when all its workgroups get through; this covers a launch that did not)
    hipStreamSynchronize(t->stream);
    hipMemsetAsync(reinterpret_cast<char*>(t->d_hdr.get()) + offsetof(PftHeader, pop_bar), 0, sizeof(((PftHeader*)nullptr)->pop_bar), t->stream);
  }
  t->err = m;
  if (e & (4u | 16u)) return PFT_ERR_HIP;
  return (e & 128u) && !(e & ~128u) ? PFT_ERR_NO_INPUT : PFT_ERR_CAPACITY;
}

static int ensure_input_capacity(pft_tracker* t, uint32_t n) {
  if (n <= t->in_cap) return PFT_OK;
  if ((uint64_t)n * 8ull + 64ull >= (1ull << 24)) {
    t->err = "input cloud too large for 24-bit octree child offsets";
    return PFT_ERR_CAPACITY;
  }
  hipStreamSynchronize(t->stream);
  t->in_cap = 0;  // a failing allocation below leaves null buffers: they must not look usable
  t->tree_of_compute = false;  // (the tree goes with them,
  t->has_input = false;        // and so does the cloud: the callers set it again with the new one)
  t->raw_pending = nullptr;
  t->sort = {};
  uint32_t cap = n;
  t->max_words = cap * 8u + 64u;
  PFTT_GROW(t, t->d_in_raw.alloc(cap));
  PFTT_GROW(t, t->d_in_pts.alloc(cap));
  PFTT_GROW(t, t->d_crop_counts.alloc((size_t)(cap / 1024 + 2)));
  PFTT_GROW(t, t->d_crop_slots.alloc((size_t)(cap / 1024 + 2)));
  PFTT_GROW(t, t->d_crop_pts.alloc(cap));
  PFTT_GROW(t, t->d_crop_idx.alloc(cap));
  PFTT_GROW(t, t->d_words.alloc(t->max_words));
  PFTT_GROW(t, t->d_leaf_pts.alloc(cap));
  PFTT_GROW(t, t->d_leaf_order.alloc(cap));
  PFTT_GROW(t, t->d_pt_node.alloc(cap));
  PFTT_GROW(t, t->d_pt_key.alloc((size_t)cap * 3));
  PFTT_GROW(t, t->d_pt_tmp.alloc(cap));
  PFTT_GROW(t, t->d_pt_key64.alloc(cap));
  const uint32_t ntiles = (cap + 1023u) / 1024u;
  PFTT_GROW(t, t->d_sort_keys[0].alloc(cap));
  PFTT_GROW(t, t->d_sort_keys[1].alloc(cap));
  PFTT_GROW(t, t->d_sort_vals[0].alloc(cap));
  PFTT_GROW(t, t->d_sort_vals[1].alloc(cap));
  PFTT_GROW(t, t->d_sort_hist.alloc((size_t)256 * ntiles + 256));
  PFTT_GROW(t, t->d_sort_tile_cnt.alloc((size_t)ntiles * (PFT_MAX_DEPTH + 2)));
  PFTT_GROW(t, t->d_sort_tile_box.alloc((size_t)ntiles * 6));
  t->sort = {{t->d_sort_keys[0], t->d_sort_keys[1]}, {t->d_sort_vals[0], t->d_sort_vals[1]}, t->d_sort_hist,
             t->d_sort_tile_cnt, t->d_sort_tile_box, ntiles};
  pftt_sync_dev(t);  // (before the last call that can fail: t->dev holds the new addresses whatever it returns)
  PFT_HIPCHK(t, hipMemsetAsync(t->d_crop_slots, 0, (size_t)(cap / 1024 + 2) * sizeof(unsigned long long), t->stream));
  t->in_cap = cap;
  return PFT_OK;
}

void pftt_cd_free(CdInst& c) { c = CdInst(); }
// room for crops of `cap` points; the state and both voxel sets survive a growth (the stream is synchronised by the caller).
// The new instance is built beside the old one and swapped in when it is complete: a failure on the way frees what was
// built and leaves `c` as it was
int pftt_cd_reserve(pft_tracker* t, CdInst& c, uint32_t cap, bool debug) {
  if (cap < 1024u) cap = 1024u;
  if (c.b.st && cap <= c.b.cap) return PFT_OK;
  CdInst n;
  uint32_t tab = 64u;
  while (tab < 4u * cap) tab <<= 1;
  PFTT_GROW(t, n.st.alloc(1));
  for (int k = 0; k < 2; k++) {
    PFTT_GROW(t, n.set_key[k].alloc(cap));
    PFTT_GROW(t, n.set_cnt[k].alloc(cap));
  }
  PFTT_GROW(t, n.tab_key.alloc(tab));
  PFTT_GROW(t, n.tab_cnt.alloc(tab));
  PFTT_GROW(t, n.pt_key.alloc(cap));
  if (debug) {
    PFTT_GROW(t, n.mark.alloc(cap));
    PFTT_GROW(t, n.pts.alloc(cap));
  }
  n.b = {n.st, {n.set_key[0], n.set_key[1]}, {n.set_cnt[0], n.set_cnt[1]}, n.tab_key, n.tab_cnt, n.pt_key, n.mark, cap, tab};
  if (c.b.st) {
    PFT_HIPCHK(t, hipMemcpyAsync(n.b.st, c.b.st, sizeof(PftChangeState), hipMemcpyDeviceToDevice, t->stream));
    for (int k = 0; k < 2; k++) {
      PFT_HIPCHK(t, hipMemcpyAsync(n.b.set_key[k], c.b.set_key[k], (size_t)c.b.cap * 8u, hipMemcpyDeviceToDevice, t->stream));
      PFT_HIPCHK(t, hipMemcpyAsync(n.b.set_cnt[k], c.b.set_cnt[k], (size_t)c.b.cap * 4u, hipMemcpyDeviceToDevice, t->stream));
    }
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  } else {
    PFT_HIPCHK(t, hipMemsetAsync(n.b.st, 0, sizeof(PftChangeState), t->stream));
  }
  std::swap(c, n);  // (the old instance, now `n`, is freed on return)
  return PFT_OK;
}

// the only reader of the environment: a switch changed later affects the handles created after the change
PftSwitches pft_read_switches() {
  auto on = [](const char* name) { return getenv(name) != nullptr; };
  auto is1 = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };
  PftSwitches w = {};
  w.graph = is1("PFT_GRAPH");
  if (const char* b = getenv("PFT_FORCE_BUILDER")) w.builder = !strcmp(b, "single") ? 1 : (!strcmp(b, "sorted") ? 2 : 0);
  w.leaf_indirect = on("PFT_LEAF_INDIRECT") ? (int)is1("PFT_LEAF_INDIRECT") : -1;
  w.aabb_full = on("PFT_AABB_FULL");
  w.resample_one_lane = on("PFT_RESAMPLE_ONE_LANE");
  w.split_resample = on("PFT_SPLIT_RESAMPLE") || w.resample_one_lane;  // (the one-lane kernel is a resample of its own)
  w.crop_two_pass = on("PFT_CROP_TWO_PASS");
  w.generic_descent = is1("PFT_GENERIC_DESCENT");
  w.ancestor_table = !on("PFT_ANCESTOR_TABLE") || is1("PFT_ANCESTOR_TABLE");
  w.anc_up_force = -1;
  if (const char* u = getenv("PFT_ANC_UP_FORCE")) w.anc_up_force = (u[0] >= '0' && u[0] <= '2' && !u[1]) ? u[0] - '0' : -1;
  w.exact_path = on("PFT_EXACT_SHELLS_ONLY") ? PftExactPath::shells : on("PFT_EXACT_PER_QUERY") ? PftExactPath::per_query : PftExactPath::sorted;
#ifdef PFT_DIAG
  if (const char* a = getenv("PFT_ABLATE")) w.ablate = atoi(a);  // bit0 generic levels, bit1 leaf scan, bit2 coherence
  w.skip_octree = on("PFT_DEBUG_SKIP_OCTREE");
#endif
  return w;
}

#ifdef PFT_DIAG
// timing experiments only (tools/lik_microbench.py): the handle's stage ablation mask.  Not in the product library.
extern "C" void pft_debug_set_ablate(pft_tracker* t, int mask) { if (t) t->sw.ablate = mask; }
#endif

extern "C" int pft_create(const pft_config* cfg, pft_tracker** out) {
  if (!cfg || !out) return PFT_ERR_INVALID_ARG;
  *out = nullptr;
  if (cfg->abi_version != PFT_ABI_VERSION || cfg->particle_num <= 0 || cfg->iteration_num <= 0 ||
      cfg->world_size <= 0 || cfg->rank < 0 || cfg->rank >= cfg->world_size || cfg->use_normal != 0 ||
      cfg->particle_num % cfg->world_size != 0 || !(cfg->octree_resolution > 0) ||
      (cfg->sum_order != PFT_SUM_TREE && cfg->sum_order != PFT_SUM_PCL))
    return PFT_ERR_INVALID_ARG;
  if (cfg->particle_num > PFT_MAX_PARTICLES) return PFT_ERR_CAPACITY;
  if (cfg->kld_adaptive) {
    if (cfg->world_size != 1 || cfg->maximum_particle_num <= 0 || !(cfg->kld_epsilon > 0)) return PFT_ERR_INVALID_ARG;
    for (int k = 0; k < 6; k++)
      if (!(cfg->kld_bin_size[k] > 0)) return PFT_ERR_INVALID_ARG;
    // the population stage of a KLD tracker runs in the single-workgroup kernel
    if (cfg->maximum_particle_num >= PFT_POPM_MIN || cfg->particle_num >= PFT_POPM_MIN) return PFT_ERR_CAPACITY;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device_id >= ndev) return PFT_ERR_NO_DEVICE;
  if (hipSetDevice(cfg->device_id) != hipSuccess) return PFT_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device_id) != hipSuccess) return PFT_ERR_NO_DEVICE;

  pft_tracker* t = new pft_tracker();
  t->cfg = *cfg;
  t->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (cfg->stream_is_external) {
    t->stream = static_cast<hipStream_t>(cfg->stream);
  } else {
    if (hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking) != hipSuccess) {
      delete t;
      return PFT_ERR_HIP;
    }
    t->own_stream = true;
  }
  for (int i = 0; i < 16; i++) t->trans[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  t->sw = pft_read_switches();
  pft_visibility_config_default(&t->vis_cam);
  t->use_graph = t->sw.graph && t->own_stream;

  PftParams& p = t->prm;
  memset(&p, 0, sizeof(p));
  p.alpha = cfg->alpha;
  p.maxd2 = cfg->max_distance * cfg->max_distance;
  p.res = cfg->octree_resolution;
  p.dist_w = cfg->distance_weight;
  p.hsv_w = cfg->hsv_weight;
  p.h_w = (float)cfg->h_weight;
  p.s_w = (float)cfg->s_weight;
  p.v_w = (float)cfg->v_weight;
  p.hsv_argorder = cfg->hsv_pcl180_argorder;
  for (int k = 0; k < 6; k++) {
    p.step_sigma[k] = sqrt(cfg->step_noise_cov[k]);
    p.init_sigma[k] = sqrt(cfg->initial_noise_cov[k]);
    p.init_mean[k] = cfg->initial_noise_mean[k];
  }
  p.seed_lo = (uint32_t)cfg->seed;
  p.seed_hi = (uint32_t)(cfg->seed >> 32);
  p.P_total = (uint32_t)cfg->particle_num;
  p.P_local = p.P_total / (uint32_t)cfg->world_size;
  p.id_offset = p.P_local * (uint32_t)cfg->rank;
  p.M = 0;
  p.nchunk = 1;
  p.ref_chunk = PFT_REF_CHUNK;
  p.split_last = 0;
  p.kld = cfg->kld_adaptive ? 1u : 0u;
  p.kld_max = (uint32_t)cfg->maximum_particle_num;
  p.kld_z = pft_kld_normal_quantile(cfg->kld_delta);
  p.kld_eps = cfg->kld_epsilon;
  for (int k = 0; k < 6; k++) p.kld_bin[k] = (float)cfg->kld_bin_size[k];
  p.motion_ratio = cfg->motion_ratio;
  p.sum_order = cfg->sum_order;
  // capacity in particles: the KLD variant grows / shrinks between particle_num and maximum_particle_num
  t->Pcap = p.kld && p.kld_max > p.P_total ? p.kld_max : p.P_total;

  const size_t Pl = p.kld ? t->Pcap : p.P_local, Pt = t->Pcap;
  bool ok = true;
  auto A = [&](bool r) { ok = ok && r; };
  A(t->d_part[0].alloc(Pt));  // sized P_total so part_all can alias a shard buffer when world_size == 1
  A(t->d_part[1].alloc(Pt));
  A(t->d_mats.alloc(Pl * 12));
  // (one partial box per workgroup of k_aabb / of the fused resample)
  A(t->d_bbox_part.alloc(std::max<size_t>((size_t)t->num_cus, (Pl * 4u + 255u) / 256u) * 6));
  A(t->d_bbox6.alloc(8));
  A(t->d_jump.alloc((size_t)1 << (3 * PFT_JUMP_MAX_LEVEL)));
  if (t->sw.ancestor_table) A(t->d_anc.alloc(PFT_ANC_CAP));  // (node indices < 2^24: the 27 bits of an entry suffice)
  A(t->d_alias_list.alloc(2 * Pt));
  A(t->d_alias_pref.alloc(2 * Pt));
  A(t->d_pop_part.alloc((size_t)PFT_POPM_MAX_WGS * 16));
  A(t->d_alias_pos.alloc(Pt));
  A(t->d_raw_w.alloc(Pt));
  if (cfg->exact_nearest) {
    A(t->d_eg_start.alloc((size_t)PFT_EG_CAP + 1));
    A(t->d_eg_cnt.alloc((size_t)PFT_EG_CAP));
    A(t->d_eg_tile.alloc((size_t)PFT_EG_CAP / 2048 + 2));
    A(t->d_ec_slot.alloc((size_t)PFT_EG_CAP));
    A(t->d_ec_cells.alloc((size_t)PFT_EC_SLOTS));
    A(t->d_ec_count.alloc((size_t)PFT_EC_SLOTS));
    A(t->d_ec_base.alloc((size_t)PFT_EC_SLOTS));
    A(t->d_ec_list.alloc((size_t)PFT_EC_POOL_MIN));
    A(t->d_eq_cellq.alloc((size_t)PFT_EG_CAP));
    A(t->d_eq_nq.alloc((size_t)PFT_EC_SLOTS));
    A(t->d_eq_qbase.alloc((size_t)PFT_EC_SLOTS));
    A(t->d_eq_bbase.alloc((size_t)PFT_EC_SLOTS));
    A(t->d_eq_fill.alloc((size_t)PFT_EC_SLOTS));
  }
  if (p.kld) {
    A(t->d_kld_table.alloc((size_t)6 * p.kld_max + 128));
    A(t->d_kld_bins.alloc((size_t)6 * p.kld_max));
  }
  A(hipHostMalloc(reinterpret_cast<void**>(&t->h_stat), 8 * sizeof(uint32_t), hipHostMallocMapped) == hipSuccess);
  // [0..3]: pft_debug_get_host_stat; [4]: exact-NN pool demand; [5]: ancestor table window sizes (pft_anc_window)
  if (t->h_stat) for (int i = 0; i < 8; i++) t->h_stat[i] = 0;
  A(t->d_hdr.alloc(1));
  A(t->d_dbg_hdr.alloc(1));
  ok = ok && hipMemsetAsync(t->d_hdr, 0, sizeof(PftHeader), t->stream) == hipSuccess;
  ok = ok && hipMemsetAsync(t->d_dbg_hdr, 0, sizeof(PftHeader), t->stream) == hipSuccess;
  if (!ok) {
    pft_destroy(t);
    return PFT_ERR_HIP;
  }
  if (cfg->max_input_points) {
    int r = ensure_input_capacity(t, cfg->max_input_points);
    if (r != PFT_OK) {
      pft_destroy(t);
      return r;
    }
  }
  pftt_sync_dev(t);
  *out = t;
  return PFT_OK;
}

// gives up the link to a filter (the stream has drained, or the link's event has been waited for, when this is called
// for good); the filter frees a link it finds abandoned, an abandoned filter's link is freed here
static void release_borrow(pft_tracker* t) {
  PftBorrow* b = t->borrow;
  t->borrow = nullptr;
  if (!b) return;
  b->tracker_alive = false;
  b->armed = false;
  if (!b->filter_alive) {
    hipEventDestroy(b->ev);
    delete b;
  }
}

pft_tracker::~pft_tracker() {
  release_borrow(this);
  if (graph_exec) hipGraphExecDestroy(graph_exec);
  for (int k = 0; k < PFT_K_COUNT; k++)
    for (auto& p : ev[k]) {
      hipEventDestroy(p.a);
      hipEventDestroy(p.b);
    }
  for (auto& p : ev_free) {
    hipEventDestroy(p.a);
    hipEventDestroy(p.b);
  }
  if (h_stat) hipHostFree(h_stat);
  if (own_stream && stream) hipStreamDestroy(stream);
}

extern "C" void pft_destroy(pft_tracker* t) {
  if (!t) return;
  if (t->stream) hipStreamSynchronize(t->stream);
  delete t;  // (every device buffer is a DevBuf member)
}

extern "C" const char* pft_last_error_string(const pft_tracker* t) { return t ? t->err.c_str() : "null handle"; }

extern "C" int pft_synchronize(pft_tracker* t) {
  if (!t) return PFT_ERR_INVALID_ARG;
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

// the lost rule's state {below, streak, lost} and the spread rule's {uncertain, streak, flagged} back to zero, in stream order
int pftt_match_clear_streak(pft_tracker* t) {
  if (t->d_match) PFT_HIPCHK(t, hipMemsetAsync(&t->d_match->below, 0, 3 * sizeof(uint32_t), t->stream));
  if (t->d_spread) PFT_HIPCHK(t, hipMemsetAsync(&t->d_spread->uncertain, 0, 3 * sizeof(uint32_t), t->stream));
  if (t->d_vis) PFT_HIPCHK(t, hipMemsetAsync(&t->d_vis->below, 0, 3 * sizeof(uint32_t), t->stream));  // the visibility rule's
  return PFT_OK;
}

extern "C" int pft_set_reference(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n) {
  return pftt_set_reference(t, pts, n, false);
}

int pftt_set_reference(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n, bool same_object) {
  if (!t || (!pts && n)) return PFT_ERR_INVALID_ARG;
  if (n > 0x7fffffffu) return PFT_ERR_CAPACITY;
  hipSetDevice(t->cfg.device_id);
  // the handle has no reference until this call has succeeded: a failure below must not leave the previous one, whose
  // buffers are replaced on the way, looking usable
  t->has_ref = false;
  t->tree_of_compute = false;
  t->match_n = 0;
  t->vis_n = 0;
  if (n > t->ref_cap) {
    hipStreamSynchronize(t->stream);
    t->ref_cap = 0;
    PFTT_GROW(t, t->d_ref_raw.alloc(n));
    PFTT_GROW(t, t->d_ref_perm.alloc(n));
    PFTT_GROW(t, t->d_ref_xyz.alloc(n));
    PFTT_GROW(t, t->d_ref_hsv.alloc(n));
    PFTT_GROW(t, t->d_ref_box.alloc(n));
    t->ref_cap = (uint32_t)n;
  }
  t->prm.M = (uint32_t)n;
  {
    // Work item of the likelihood kernels = (particle, ref_chunk reference points).  256 points amortise the per-item
    // cost best when there are plenty of items; with few particles (the reference's own 400-500) smaller items keep
    // all CUs busy: aim at two items per resident wave.
    const uint64_t pl = t->prm.kld ? t->Pcap : t->prm.P_local;
    const uint64_t want_items = 2ull * (uint64_t)PFT_LIK_WGS_PER_CU * (uint64_t)t->num_cus * (PFT_LIK_THREADS / 64u);
    uint64_t c = pl * (uint64_t)n / (want_items ? want_items : 1);
    c = (c / 64u) * 64u;
    if (c < 64u) c = 64u;
    if (c > PFT_REF_CHUNK) c = PFT_REF_CHUNK;
    t->prm.ref_chunk = (uint32_t)c;
  }
  t->prm.nchunk = (uint32_t)((n + t->prm.ref_chunk - 1) / t->prm.ref_chunk);
  if (t->prm.nchunk == 0) t->prm.nchunk = 1;
  // the items a launch ends with decide how long its last waves run alone: the last chunk is cut in two halves, and
  // the halves of all particles are handed out after the full-size items (approximate search only)
  t->prm.split_last = 0;
  if (!t->cfg.exact_nearest && t->prm.ref_chunk >= 128u && n % t->prm.ref_chunk == 0 && t->prm.nchunk >= 2u) {
    t->prm.split_last = t->prm.ref_chunk >= 256u ? 4u : 2u;  // sub-items of at least 64 points (one round of a wave)
    t->prm.nchunk += t->prm.split_last - 1u;
  }
  PFTT_GROW(t, t->d_partial.alloc((size_t)(t->prm.kld ? t->Pcap : t->prm.P_local) * t->prm.nchunk));
  pftt_sync_dev(t);  // (the allocations are done: whatever fails below, t->dev holds live addresses)
  if (n) {
    // The reference cloud is stored in Morton (Z-curve) order: the 64 lanes of a wave then query
    // neighbouring space, so their octree paths and leaf records share LDS words and cache lines.  Every
    // per-particle result is a sum over all reference points, so the order is free; ref_perm maps back.
    std::vector<uint32_t> perm(n);
    std::vector<pft_point_xyzrgba> sorted(n);
    {
      float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (size_t i = 0; i < n; i++) {
        const float c[3] = {pts[i].x, pts[i].y, pts[i].z};
        for (int a = 0; a < 3; a++)
          if (std::isfinite(c[a])) {
            lo[a] = std::min(lo[a], c[a]);
            hi[a] = std::max(hi[a], c[a]);
          }
      }
      float ext = 0.0f;
      for (int a = 0; a < 3; a++)
        if (hi[a] >= lo[a]) ext = std::max(ext, hi[a] - lo[a]);
      const float scale = ext > 0.0f ? 1023.0f / ext : 0.0f;
      std::vector<uint64_t> code(n);
      for (size_t i = 0; i < n; i++) {
        const float c[3] = {pts[i].x, pts[i].y, pts[i].z};
        uint64_t m = 0;
        uint32_t q[3];
        for (int a = 0; a < 3; a++) {
          float v = std::isfinite(c[a]) ? (c[a] - lo[a]) * scale : 0.0f;
          q[a] = (uint32_t)std::min(1023.0f, std::max(0.0f, v));
        }
        for (int b = 9; b >= 0; b--)
          m = (m << 3) | (uint64_t)((((q[0] >> b) & 1u) << 2) | (((q[1] >> b) & 1u) << 1) | ((q[2] >> b) & 1u));
        code[i] = (m << 32) | (uint64_t)i;  // index in the low bits: stable
      }
      std::sort(code.begin(), code.end());
      for (size_t i = 0; i < n; i++) {
        perm[i] = (uint32_t)(code[i] & 0xffffffffu);
        sorted[i] = pts[perm[i]];
      }
    }
    pts = sorted.data();
    PFT_HIPCHK(t, hipMemcpyAsync(t->d_ref_perm, perm.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
    PFT_HIPCHK(t, hipMemcpyAsync(t->d_ref_raw, pts, n * sizeof(pft_point_xyzrgba), hipMemcpyHostToDevice, t->stream));
    pftk_pack_reference(t->stream, t->d_ref_raw, (uint32_t)n, t->prm.hsv_argorder, t->d_ref_xyz, t->d_ref_hsv);
    // A3's input: the points that can be extreme in some rigidly transformed coordinate (the hull's vertices and what lies
    // within the float evaluation's reach of its facets); PFT_AABB_FULL=1 keeps every point (cross-check, A/B timing)
    std::vector<uint32_t> keep;
    if (t->sw.aabb_full) {
      keep.resize(n);
      for (size_t i = 0; i < n; i++) keep[i] = (uint32_t)i;
    } else {
      pft_aabb_support_subset(pts, n, keep);
    }
    std::vector<float4> box(keep.size());
    for (size_t i = 0; i < keep.size(); i++) box[i] = make_float4(pts[keep[i]].x, pts[keep[i]].y, pts[keep[i]].z, 0.0f);
    t->prm.M_box = (uint32_t)keep.size();
    PFT_HIPCHK(t, hipMemcpyAsync(t->d_ref_box, box.data(), box.size() * sizeof(float4), hipMemcpyHostToDevice, t->stream));
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  } else {
    t->prm.M_box = 0;
  }
  t->has_ref = true;
  if (t->h_stat) t->h_stat[0] = t->h_stat[1] = 0;  // new scene: forget the builder hints (unknown depth = all radix passes)
  t->tree_of_compute = false;  // the tree on the device was searched for another model
  t->match_n = 0;
  t->vis_n = 0;
  if (!same_object) {
    const int r = pftt_match_clear_streak(t);  // a new object: the lost rule starts over
    if (r != PFT_OK) return r;
  }
  pftt_sync_dev(t);
  return PFT_OK;
}

extern "C" int pft_set_trans(pft_tracker* t, const float m[16]) {
  if (!t || !m) return PFT_ERR_INVALID_ARG;
  memcpy(t->trans, m, sizeof(float) * 16);
  return PFT_OK;
}

static int set_input_common(pft_tracker* t, const void* src, size_t n, bool device) {
  if (!t || (!src && n)) return PFT_ERR_INVALID_ARG;
  if (n > 0x7fffffffu) return PFT_ERR_CAPACITY;
  hipSetDevice(t->cfg.device_id);
  int r = ensure_input_capacity(t, (uint32_t)n);
  if (r != PFT_OK) return r;
  if (t->cd_ever && t->cd.b.cap < t->in_cap) {  // the detector's sets follow the input capacity (crops are at most N points)
    r = pftt_cd_reserve(t, t->cd, t->in_cap, false);
    if (r != PFT_OK) return r;
  }
  t->N = (uint32_t)n;
  t->n_on_device = false;
  t->n_src = nullptr;
  if (t->borrow) t->borrow->armed = false;
  if (n) {
    const pft_point_xyzrgba* dsrc = static_cast<const pft_point_xyzrgba*>(src);
    if (!device) {
      PFT_HIPCHK(t, hipMemcpyAsync(t->d_in_raw, src, n * sizeof(pft_point_xyzrgba), hipMemcpyHostToDevice, t->stream));
      dsrc = t->d_in_raw;
    }
    // the 16-byte records (d_in_pts) are formed by the first crop of the frame, which reads the 32-byte layout
    t->raw_pending = dsrc;
    if (!device) PFT_HIPCHK(t, hipStreamSynchronize(t->stream));  // the host buffer is only borrowed for this call
  }
  if (!n) t->raw_pending = nullptr;
  t->has_input = n > 0;
  pftt_sync_dev(t);
  return PFT_OK;
}

extern "C" int pft_set_input(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n) {
  return set_input_common(t, pts, n, false);
}
extern "C" int pft_set_input_device(pft_tracker* t, const void* device_pts, size_t n) {
  return set_input_common(t, device_pts, n, true);
}

extern "C" int pft_set_input_from_filter(pft_tracker* t, pft_filter* f, size_t max_points) {
  if (!t || !f) return PFT_ERR_INVALID_ARG;
  if (t->cfg.world_size > 1) {
    t->err = "pft_set_input_from_filter on a sharded handle (world_size > 1): every rank needs the same host-side count";
    return PFT_ERR_INVALID_ARG;
  }
  PftFilterView v;
  if (pftf_view(f, &v) != PFT_OK) {
    t->err = "pft_set_input_from_filter: the filter has not been applied yet";
    return PFT_ERR_STATE;
  }
  if (v.device_id != t->cfg.device_id) {
    t->err = "pft_set_input_from_filter: the filter lives on device " + std::to_string(v.device_id) + ", the tracker on device " +
             std::to_string(t->cfg.device_id) + " (a filter on another device)";
    return PFT_ERR_INVALID_ARG;
  }
  const size_t bound = max_points ? max_points : v.n_in;
  if (bound == 0) return set_input_common(t, nullptr, 0, true);  // an apply over no points: no input cloud
  if (bound > 0x7fffffffu) return PFT_ERR_CAPACITY;
  hipSetDevice(t->cfg.device_id);
  int r = ensure_input_capacity(t, (uint32_t)bound);
  if (r != PFT_OK) return r;
  if (t->cd_ever && t->cd.b.cap < t->in_cap) {
    r = pftt_cd_reserve(t, t->cd, t->in_cap, false);
    if (r != PFT_OK) return r;
  }
  if (!t->d_n_in) {
    PFTT_GROW(t, t->d_n_in.alloc(1));
    PFT_HIPCHK(t, hipMemsetAsync(t->d_n_in, 0, sizeof(uint32_t), t->stream));
  }
  if (!t->borrow || !t->borrow->filter_alive || t->borrow_of != f) {
    release_borrow(t);
    PftBorrow* b = new PftBorrow();
    if (hipEventCreateWithFlags(&b->ev, hipEventDisableTiming) != hipSuccess) {
      delete b;
      t->err = "pft_set_input_from_filter: hipEventCreateWithFlags failed";
      return PFT_ERR_HIP;
    }
    t->borrow = b;
    t->borrow_of = f;
    pftf_attach(f, b);
  }
  t->borrow->armed = true;
  t->borrow->valid = true;
  PFT_HIPCHK(t, hipStreamWaitEvent(t->stream, v.done, 0));  // the apply, however far it has got
  t->N = (uint32_t)bound;
  t->n_on_device = true;
  t->n_src = v.n_out_dev;
  t->raw_pending = v.out;
  t->has_input = true;
  pftt_sync_dev(t);
  return PFT_OK;
}

// ---- accessors ----
extern "C" int pft_get_result(pft_tracker* t, pft_particle* out) {
  if (!t || !out) return PFT_ERR_INVALID_ARG;
  PFT_HIPCHK(t, hipMemcpyAsync(out, &t->d_hdr->rep, sizeof(pft_particle), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);  // the pose is written either way; a failed iteration makes it the unweighted mean
}

extern "C" int pft_get_fit_ratio(pft_tracker* t, double* out) {
  if (!t || !out) return PFT_ERR_INVALID_ARG;
  PFT_HIPCHK(t, hipMemcpyAsync(out, &t->d_hdr->fit_ratio, sizeof(double), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

extern "C" int pft_get_particles(pft_tracker* t, pft_particle* out, size_t cap, size_t* n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  size_t P = t->initialized ? t->prm.P_total : 0;
  if (P && t->prm.kld) {  // particle_num_ of the KLD variant lives on the device
    uint32_t pa = 0;
    pftt_sync_dev(t);
    PFT_HIPCHK(t, hipMemcpyAsync(&pa, &t->d_hdr->p_active, sizeof(pa), hipMemcpyDeviceToHost, t->stream));
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
    P = pa;
  }
  if (n) *n = P;
  if (!out || !P) return PFT_OK;
  size_t c = cap < P ? cap : P;
  pftt_sync_dev(t);
  PFT_HIPCHK(t, hipMemcpyAsync(out, t->dev.part_all, c * sizeof(pft_particle), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return pftt_check_device_error(t);
}

extern "C" int pft_set_particles(pft_tracker* t, const pft_particle* p, size_t n) {
  if (!t || !p) return PFT_ERR_INVALID_ARG;
  if (t->prm.kld ? (n == 0 || n > t->Pcap) : (n != t->prm.P_local)) return PFT_ERR_INVALID_ARG;
  PFT_HIPCHK(t, hipMemcpyAsync(t->d_part[t->cur], p, n * sizeof(pft_particle), hipMemcpyHostToDevice, t->stream));
  if (t->prm.kld) {  // particle_num_ of the KLD variant lives on the device
    const uint32_t pa = (uint32_t)n;
    PFT_HIPCHK(t, hipMemcpyAsync(&t->d_hdr->p_active, &pa, sizeof(pa), hipMemcpyHostToDevice, t->stream));
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  }
  pftk_pose_to_matrix(t->stream, t->d_part[t->cur], (uint32_t)n, t->d_mats);
  pft_particle rep;
  pft_to_state(t->trans, &rep);
  rep.weight = 1.0f / (float)t->prm.P_total;
  PFT_HIPCHK(t, hipMemcpyAsync(&t->d_hdr->rep, &rep, sizeof(rep), hipMemcpyHostToDevice, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  t->initialized = true;
  t->changed = false;
  t->tree_of_compute = false;  // the representative state was replaced: the tree is not its frame's any more
  if (t->h_stat) t->h_stat[0] = t->h_stat[1] = 0;  // the spread of the particles decides the crop: forget the builder hints
  return PFT_OK;
}

// pft_api_debug.hip -- the test and benchmark hooks of the tracker handle: pft_eval_weights, every pft_debug_* entry point
// and the checkpoint of the filter state (pft_debug_state_save / _restore with k_copy_segments).  None of this runs in a
// tracked frame.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pft_tracker.h"

// ---- test hooks ----
extern "C" int pft_debug_set_limits(pft_tracker* t, uint32_t max_words, int sorted_npass) {
  if (!t) return PFT_ERR_INVALID_ARG;
  hipStreamSynchronize(t->stream);
  if (max_words) {
    if (t->in_cap == 0 || max_words > t->in_cap * 8u + 64u) return PFT_ERR_CAPACITY;  // only ever below the allocation
    t->max_words = max_words;
  }
  t->force_npass = sorted_npass;
  pftt_sync_dev(t);
  return PFT_OK;
}
extern "C" int pft_debug_set_exact_limits(pft_tracker* t, uint32_t ec_slots) {
  if (!t || !t->cfg.exact_nearest || !ec_slots) return PFT_ERR_INVALID_ARG;
  if (ec_slots > PFT_EC_SLOTS) return PFT_ERR_CAPACITY;  // only ever below the allocation
  hipStreamSynchronize(t->stream);
  t->ec_slots_cap = ec_slots;
  pftt_sync_dev(t);
  return PFT_OK;
}
// ---- checkpoint of the filter state (between frames): the whole population with its weights, the alias prefix form the
// next resample draws from, the header (representative state, motion, KLD particle count) and the host-side schedule
// state.  Restoring is ONE kernel on the handle's stream, so a benchmark can replay the same frame again and again.
struct CopySeg {
  const uint32_t* src;
  uint32_t* dst;
  uint32_t n;  // 32-bit words
};
struct CopySegs {
  CopySeg s[5];
};
__global__ __launch_bounds__(256) void k_copy_segments(CopySegs cs) {
  const CopySeg g = cs.s[blockIdx.y];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += gridDim.x * blockDim.x) g.dst[i] = g.src[i];
}

static void state_segments(pft_tracker* t, bool save, CopySegs* cs) {
  const uint32_t P = t->Pcap;
  const void* live[5] = {t->dev.part_all, t->d_alias_list, t->d_alias_pref, t->d_alias_pos, t->d_hdr};
  void* saved[5] = {t->sv_part, t->sv_alias_list, t->sv_alias_pref, t->sv_alias_pos, t->sv_hdr};
  const uint32_t words[5] = {P * 8u, P * 2u, P * 4u, P, (uint32_t)(sizeof(PftHeader) / 4u)};
  for (int k = 0; k < 5; k++) {
    cs->s[k].src = static_cast<const uint32_t*>(save ? live[k] : saved[k]);
    cs->s[k].dst = static_cast<uint32_t*>(save ? saved[k] : const_cast<void*>(live[k]));
    cs->s[k].n = words[k];
  }
}

extern "C" int pft_debug_state_save(pft_tracker* t) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!t->initialized) {
    t->err = "pft_debug_state_save before the first compute";
    return PFT_ERR_STATE;
  }
  hipSetDevice(t->cfg.device_id);
  t->sv_valid = false;  // (until this save has completed)
  if (!t->sv_hdr) {     // (the last of the five to be allocated: null until all are there)
    const size_t P = t->Pcap;
    PFTT_GROW(t, t->sv_part.alloc(P));
    PFTT_GROW(t, t->sv_alias_list.alloc(2 * P));
    PFTT_GROW(t, t->sv_alias_pref.alloc(2 * P));
    PFTT_GROW(t, t->sv_alias_pos.alloc(P));
    PFTT_GROW(t, t->sv_hdr.alloc(1));
  }
  pftt_sync_dev(t);
  CopySegs cs;
  state_segments(t, true, &cs);
  hipLaunchKernelGGL(k_copy_segments, dim3(64, 5), dim3(256), 0, t->stream, cs);
  t->sv_cd_valid = false;
  if (t->cd_ever) {  // the change detector's state and both voxel sets
    const uint32_t cap = t->cd.b.cap;
    if (t->sv_cd_cnt[1].cap() != cap) {  // (the last of the five to be allocated: capacity 0 until all are there)
      t->sv_cd_cnt[1].reset();
      PFTT_GROW(t, t->sv_cd.alloc(1));
      for (int k = 0; k < 2; k++) {
        PFTT_GROW(t, t->sv_cd_key[k].alloc(cap));
        PFTT_GROW(t, t->sv_cd_cnt[k].alloc(cap));
      }
    }
    PFT_HIPCHK(t, hipMemcpyAsync(t->sv_cd, t->cd.b.st, sizeof(PftChangeState), hipMemcpyDeviceToDevice, t->stream));
    for (int k = 0; k < 2; k++) {
      PFT_HIPCHK(t, hipMemcpyAsync(t->sv_cd_key[k], t->cd.b.set_key[k], (size_t)cap * 8u, hipMemcpyDeviceToDevice, t->stream));
      PFT_HIPCHK(t, hipMemcpyAsync(t->sv_cd_cnt[k], t->cd.b.set_cnt[k], (size_t)cap * 4u, hipMemcpyDeviceToDevice, t->stream));
    }
    t->sv_cd_valid = true;
  }
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  t->sv_cur = t->cur;
  t->sv_epoch = t->resample_epoch;
  t->sv_changed = t->changed;
  t->sv_cd_counter = t->cd_counter;
  t->sv_valid = true;
  return pftt_check_device_error(t);
}

extern "C" int pft_debug_state_restore(pft_tracker* t) {
  if (!t) return PFT_ERR_INVALID_ARG;
  if (!t->sv_valid) {
    t->err = "pft_debug_state_restore without a saved state";
    return PFT_ERR_STATE;
  }
  if (t->sv_cd_valid != t->cd_ever || (t->sv_cd_valid && t->cd.b.cap != t->sv_cd_cnt[1].cap())) {
    // the detector was first enabled, or its sets were re-allocated for a larger input, after the save: the checkpoint
    // cannot put it back.  Checked before anything is copied, so the handle is left as it was
    t->err = "pft_debug_state_restore: the change detector was enabled or its buffers grew after pft_debug_state_save";
    return PFT_ERR_STATE;
  }
  hipSetDevice(t->cfg.device_id);
  t->tree_of_compute = false;  // the header goes back to the checkpoint's, the tree does not
  t->cur = t->sv_cur;
  t->resample_epoch = t->sv_epoch;
  t->changed = t->sv_changed;
  t->cd_counter = t->sv_cd_counter;
  pftt_sync_dev(t);
  CopySegs cs;
  state_segments(t, false, &cs);
  hipLaunchKernelGGL(k_copy_segments, dim3(64, 5), dim3(256), 0, t->stream, cs);
  if (t->sv_cd_valid) {
    const uint32_t cap = (uint32_t)t->sv_cd_cnt[1].cap();
    PFT_HIPCHK(t, hipMemcpyAsync(t->cd.b.st, t->sv_cd, sizeof(PftChangeState), hipMemcpyDeviceToDevice, t->stream));
    for (int k = 0; k < 2; k++) {
      PFT_HIPCHK(t, hipMemcpyAsync(t->cd.b.set_key[k], t->sv_cd_key[k], (size_t)cap * 8u, hipMemcpyDeviceToDevice, t->stream));
      PFT_HIPCHK(t, hipMemcpyAsync(t->cd.b.set_cnt[k], t->sv_cd_cnt[k], (size_t)cap * 4u, hipMemcpyDeviceToDevice, t->stream));
    }
  }
  return PFT_OK;
}

extern "C" int pft_debug_inject_error(pft_tracker* t, uint32_t bits) {
  if (!t) return PFT_ERR_INVALID_ARG;
  t->inject_error = bits;
  return PFT_OK;
}
extern "C" int pft_debug_get_host_stat(pft_tracker* t, uint32_t out4[4]) {
  if (!t || !out4 || !t->h_stat) return PFT_ERR_INVALID_ARG;
  for (int i = 0; i < 4; i++) out4[i] = ((volatile uint32_t*)t->h_stat)[i];
  return PFT_OK;
}

extern "C" int pft_eval_weights(pft_tracker* t, const pft_particle* particles, size_t P, float* raw_w,
                                int32_t* nn_idx, float* nn_d2) {
  int r = pftt_check_ready(t);
  if (r != PFT_OK) return r;
  if (!particles || !P) return PFT_ERR_INVALID_ARG;
  if (P > (t->prm.kld ? t->Pcap : t->prm.P_local)) {
    t->err = "pft_eval_weights: " + std::to_string(P) + " particles handed over, the handle's buffers hold " +
             std::to_string(t->prm.kld ? t->Pcap : t->prm.P_local) + " (particle_num / maximum_particle_num of this rank)";
    return PFT_ERR_CAPACITY;
  }
  const bool want_nn = nn_idx || nn_d2;
  const size_t pairs = P * (size_t)t->prm.M;
  const bool grow_nn = want_nn && pairs > t->d_nn_d2.cap();
  if (P > t->d_dbg_part.cap() || P > t->d_dbg_f.cap() || grow_nn) hipStreamSynchronize(t->stream);
  PFTT_GROW(t, t->d_dbg_part.reserve(P));
  PFTT_GROW(t, t->d_dbg_f.reserve(P));
  if (grow_nn) {
    t->d_nn_d2.reset();  // (the pair's capacity: zero until both are there)
    PFTT_GROW(t, t->d_nn_idx.alloc(pairs));
    PFTT_GROW(t, t->d_nn_d2.alloc(pairs));
  }
  pftt_sync_dev(t);
  t->tree_of_compute = false;  // the crop and the tree are rebuilt for these particles
  PftDev d = t->dev;
  d.p_active = nullptr;  // explicit particle count (a KLD handle's device-side count does not apply here)
  d.part_cur = t->d_dbg_part;
  d.part_all = t->d_dbg_part;
  d.bbox6 = t->d_bbox6;
  PFT_HIPCHK(t, hipMemcpyAsync(t->d_dbg_part, particles, P * sizeof(pft_particle), hipMemcpyHostToDevice, t->stream));
  PFT_HIPCHK(t, hipMemsetAsync(&t->d_hdr->stat_queries, 0, (2 + 32) * sizeof(unsigned long long), t->stream));
  PFT_HIPCHK(t, hipMemsetAsync(t->d_hdr->dbg_hard, 0, sizeof(t->d_hdr->dbg_hard) + sizeof(t->d_hdr->lik_layout), t->stream));
  pftk_pose_to_matrix(t->stream, t->d_dbg_part, (uint32_t)P, t->d_mats);
  pftt_stage_aabb(t, d, (uint32_t)P, false);
  pftt_stage_crop_octree_likelihood(t, d, (uint32_t)P, want_nn, true, true, true, false);
  pftk_finalize_raw(t->stream, t->prm, d, (uint32_t)P, t->d_dbg_f, nullptr);
  if (raw_w) PFT_HIPCHK(t, hipMemcpyAsync(raw_w, t->d_dbg_f, P * sizeof(float), hipMemcpyDeviceToHost, t->stream));
  if (nn_idx) PFT_HIPCHK(t, hipMemcpyAsync(nn_idx, t->d_nn_idx, pairs * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
  if (nn_d2) PFT_HIPCHK(t, hipMemcpyAsync(nn_d2, t->d_nn_d2, pairs * sizeof(float), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  // the matrices of the live particles were overwritten: restore them
  if (t->initialized) pftk_pose_to_matrix(t->stream, t->d_part[t->cur], t->prm.P_local, t->d_mats);
  PFT_HIPCHK(t, hipGetLastError());
  return pftt_check_device_error(t);
}

static int read_hdr(pft_tracker* t, PftHeader* h) {
  PFT_HIPCHK(t, hipMemcpyAsync(h, t->d_hdr, sizeof(PftHeader), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  return PFT_OK;
}

extern "C" int pft_debug_get_bbox(pft_tracker* t, float bbox[6]) {
  if (!t || !bbox) return PFT_ERR_INVALID_ARG;
  PftHeader h;
  int r = read_hdr(t, &h);
  if (r != PFT_OK) return r;
  memcpy(bbox, h.bbox, sizeof(float) * 6);
  return PFT_OK;
}

extern "C" int pft_debug_get_crop(pft_tracker* t, int32_t* idx, size_t cap, size_t* n) {
  if (!t) return PFT_ERR_INVALID_ARG;
  PftHeader h;
  int r = read_hdr(t, &h);
  if (r != PFT_OK) return r;
  if (n) *n = h.n_crop;
  size_t c = cap < h.n_crop ? cap : h.n_crop;
  if (idx && c) {
    PFT_HIPCHK(t, hipMemcpy(idx, t->d_crop_idx, c * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return PFT_OK;
}

extern "C" int pft_debug_get_input_records(pft_tracker* t, void* out, size_t first, size_t n) {
  if (!t || (!out && n)) return PFT_ERR_INVALID_ARG;
  if (first + n > t->in_cap) return PFT_ERR_CAPACITY;
  hipSetDevice(t->cfg.device_id);
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  if (n) PFT_HIPCHK(t, hipMemcpy(out, t->d_in_pts + first, n * sizeof(float4), hipMemcpyDeviceToHost));
  return PFT_OK;
}

extern "C" int pft_debug_get_octree(pft_tracker* t, int32_t* depth, double mn[3], double mx[3], uint32_t* n_leaves,
                                    uint32_t* n_nodes) {
  if (!t) return PFT_ERR_INVALID_ARG;
  PftHeader h;
  int r = read_hdr(t, &h);
  if (r != PFT_OK) return r;
  if (h.error) {
    t->err = "octree build error flag " + std::to_string(h.error);
    return PFT_ERR_CAPACITY;
  }
  if (depth) *depth = h.depth;
  if (mn) memcpy(mn, h.omin, sizeof(double) * 3);
  if (mx) memcpy(mx, h.omax, sizeof(double) * 3);
  if (n_leaves) *n_leaves = h.n_leaves;
  if (n_nodes) *n_nodes = h.n_words;
  return PFT_OK;
}

extern "C" int pft_debug_get_point_keys(pft_tracker* t, uint32_t* keys3, size_t cap_points) {
  if (!t || !keys3) return PFT_ERR_INVALID_ARG;
  PftHeader h;
  int r = read_hdr(t, &h);
  if (r != PFT_OK) return r;
  size_t c = cap_points < h.n_crop ? cap_points : h.n_crop;
  if (c) PFT_HIPCHK(t, hipMemcpy(keys3, t->d_pt_key, c * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PFT_OK;
}

extern "C" int pft_debug_get_tree(pft_tracker* t, uint32_t* info, uint32_t* words, size_t words_cap, uint32_t* leaf_order,
                                  size_t leaf_order_cap, void* leaf_pts, size_t leaf_pts_cap, void* crop_pts,
                                  size_t crop_pts_cap, uint16_t* jump, size_t jump_cap) {
  if (!t || !info) return PFT_ERR_INVALID_ARG;
  if (t->cfg.world_size != 1 || t->cfg.exact_nearest) {
    t->err = "pft_debug_get_tree: sharded handles (world_size > 1) and the exact nearest-neighbour mode build no octree";
    return PFT_ERR_INVALID_ARG;
  }
  if (t->in_cap == 0 || !t->d_words) {
    t->err = "pft_debug_get_tree before the first input cloud: no tree buffers yet";
    return PFT_ERR_STATE;
  }
  hipSetDevice(t->cfg.device_id);
  PftHeader h;
  int r = read_hdr(t, &h);  // (synchronises the stream)
  if (r != PFT_OK) return r;
  const size_t n_jump = (size_t)1 << (3 * PFT_JUMP_MAX_LEVEL);
  uint32_t f32[5];
  memcpy(&f32[0], &h.margin_cells, 4);
  memcpy(&f32[1], &h.inv_res, 4);
  memcpy(&f32[2], h.ominf, 12);
  memset(info, 0, PFT_TREE_INFO_WORDS * sizeof(uint32_t));
  info[0] = h.n_crop; info[1] = h.error; info[2] = (uint32_t)h.depth; info[3] = (uint32_t)h.use_table;
  info[4] = h.n_words; info[5] = h.n_leaves; info[6] = h.leaf_start; info[7] = (uint32_t)h.n_grow;
  info[8] = (uint32_t)h.build_path; info[9] = (uint32_t)h.leaf_indirect; info[10] = (uint32_t)h.jump_level;
  for (int k = 0; k < 5; k++) info[11 + k] = f32[k];
  info[16] = h.build_epoch; info[17] = h.build_variant;
  info[18] = ((uint32_t)pftk_max_lds_bytes() - 10240u) & ~15u;  // pftk_octree's request
  info[19] = (uint32_t)n_jump;
  static_assert(20 + PFT_MAX_DEPTH + 3 <= PFT_TREE_INFO_WORDS, "lvl_start does not fit the info block");
  for (int l = 0; l <= h.depth + 1 && l < PFT_MAX_DEPTH + 3 && h.depth > 0; l++) info[20 + l] = h.lvl_start[l];
  // (counts are bounded by the allocations whatever the header says)
  const size_t n_pts = std::min<size_t>(h.n_crop, t->in_cap);
  const size_t n_words = std::min<size_t>(h.n_words, (size_t)t->in_cap * 8u + 64u);
  auto copy = [&](void* dst, const void* src, size_t cap, size_t count, size_t elem) -> hipError_t {
    const size_t c = std::min(cap, count);
    return dst && src && c ? hipMemcpy(dst, src, c * elem, hipMemcpyDeviceToHost) : hipSuccess;
  };
  PFT_HIPCHK(t, copy(words, t->d_words, words_cap, n_words, sizeof(uint32_t)));
  PFT_HIPCHK(t, copy(leaf_order, t->d_leaf_order, leaf_order_cap, n_pts, sizeof(uint32_t)));
  PFT_HIPCHK(t, copy(leaf_pts, t->d_leaf_pts, leaf_pts_cap, n_pts, sizeof(float4)));
  PFT_HIPCHK(t, copy(crop_pts, t->d_crop_pts, crop_pts_cap, n_pts, sizeof(float4)));
  PFT_HIPCHK(t, copy(jump, t->d_jump, jump_cap, n_jump, sizeof(uint16_t)));
  return PFT_OK;
}

extern "C" int pft_debug_get_ticks(pft_tracker* t, uint64_t* ticks32) {
  if (!t || !ticks32) return PFT_ERR_INVALID_ARG;
  PftHeader h;
  int r = read_hdr(t, &h);
  if (r != PFT_OK) return r;
  for (int i = 0; i < 32; i++) ticks32[i] = h.ticks[i];
  return PFT_OK;
}

extern "C" int pft_debug_aabb_support_subset(const pft_point_xyzrgba* pts, size_t n, uint32_t* keep, size_t* n_keep) {
  if ((!pts && n) || !keep || !n_keep) return PFT_ERR_INVALID_ARG;
  std::vector<uint32_t> k;
  pft_aabb_support_subset(pts, n, k);
  for (size_t i = 0; i < k.size(); i++) keep[i] = k[i];
  *n_keep = k.size();
  return PFT_OK;
}

extern "C" int pft_debug_get_descent_stats(pft_tracker* t, uint64_t* dbg32) {
  if (!t || !dbg32) return PFT_ERR_INVALID_ARG;
  PftHeader h;
  int r = read_hdr(t, &h);
  if (r != PFT_OK) return r;
  for (int i = 0; i < 32; i++) dbg32[i] = h.dbg[i];
  dbg32[30] = t->prm.M_box;  // reference points the box is taken over (pft_hull.hip), of
  dbg32[31] = t->prm.M;
  if (t->cfg.exact_nearest) {  // the exact-NN mode's bookkeeping of the last iteration (tools/exact_nn_bench.py)
    dbg32[8] = h.ec_nslots;
    dbg32[9] = h.ec_pool_used;
    dbg32[10] = h.eq_totals & 0xffffffffull;
    dbg32[11] = h.eq_totals >> 32;
    dbg32[12] = h.eg_ncells;
    dbg32[13] = h.n_crop;
  }
  return PFT_OK;
}

// The exact-NN mode's state after the last iteration (evaluation or tracked frame): which capacity fallbacks were taken.
// The route counters are words of PftHeader::dbg that only the DEBUG_NN instantiations write (pft_eval_weights with the
// NN arrays, which zeroes them first): [24] k_eq_scatter queries placed through the probe-window-full branch, [25] its
// queries answered inline by the shell search, [26] inline as "empty list", [27] k_likelihood_exact queries sent to the
// shell search, [28] k_eq_scatter queries outside the grid; k_likelihood_exact keeps [0..6] (tools/exact_nn_bench.py: [0]
// queries, [1] served by a list, [3] outside the grid), pft_debug_get_descent_stats overlays [8..13] and [30..31] in its
// copy, -DPFT_EC_TIMING uses [16..20]
extern "C" int pft_debug_get_exact_state(pft_tracker* t, uint32_t* info, uint64_t* counters, uint32_t* ec_cells,
                                         uint32_t* ec_count, uint32_t* ec_base, size_t slots_cap, uint32_t* eg_start,
                                         size_t eg_start_cap, uint32_t* leaf_order, size_t leaf_order_cap) {
  if (!t || !info || !t->cfg.exact_nearest) return PFT_ERR_INVALID_ARG;
  if (t->in_cap == 0 || !t->d_eg_start) {
    t->err = "pft_debug_get_exact_state before the first input cloud: no grid buffers yet";
    return PFT_ERR_STATE;
  }
  hipSetDevice(t->cfg.device_id);
  PftHeader h;
  int r = read_hdr(t, &h);  // (synchronises the stream)
  if (r != PFT_OK) return r;
  memset(info, 0, PFT_EXACT_STATE_WORDS * sizeof(uint32_t));
  memcpy(&info[0], &h.eg_g, 4);
  for (int a = 0; a < 3; a++) {
    info[1 + a] = (uint32_t)h.eg_dim[a];
    memcpy(&info[4 + a], &h.eg_min[a], 4);
  }
  info[7] = h.eg_ncells; info[8] = h.n_crop; info[9] = h.ec_nslots; info[10] = h.ec_pool_used;
  info[11] = t->dev.ec_pool_cap; info[12] = (uint32_t)(h.eq_totals & 0xffffffffull); info[13] = (uint32_t)(h.eq_totals >> 32);
  info[14] = t->dev.ec_slots_cap; info[15] = t->dev.eg_cap; info[16] = t->dev.eq_tiles_cap; info[17] = t->dev.eq_cap;
  info[18] = PFT_EC_SLOTS; info[19] = PFT_EC_POOL; info[20] = PFT_EG_CAP; info[21] = PFT_EC_POOL_MIN;
  info[22] = (uint32_t)t->num_cus;
  if (counters) {
    const int words[8] = {24, 25, 26, 27, 28, 0, 1, 3};
    for (int k = 0; k < 8; k++) counters[k] = h.dbg[words[k]];
  }
  // (counts are bounded by the allocations whatever the header says)
  const size_t n_slots = std::min<size_t>(std::min(h.ec_nslots, t->dev.ec_slots_cap), PFT_EC_SLOTS);
  const size_t n_cells = h.n_crop ? std::min<size_t>(h.eg_ncells, PFT_EG_CAP) + 1u : 0u;
  const size_t n_pts = std::min<size_t>(h.n_crop, t->in_cap);
  auto copy = [&](void* dst, const void* src, size_t cap, size_t count, size_t elem) -> hipError_t {
    const size_t c = std::min(cap, count);
    return dst && src && c ? hipMemcpy(dst, src, c * elem, hipMemcpyDeviceToHost) : hipSuccess;
  };
  PFT_HIPCHK(t, copy(ec_cells, t->d_ec_cells, slots_cap, n_slots, sizeof(uint32_t)));
  PFT_HIPCHK(t, copy(ec_count, t->d_ec_count, slots_cap, n_slots, sizeof(uint32_t)));
  PFT_HIPCHK(t, copy(ec_base, t->d_ec_base, slots_cap, n_slots, sizeof(uint32_t)));
  PFT_HIPCHK(t, copy(eg_start, t->d_eg_start, eg_start_cap, n_cells, sizeof(uint32_t)));
  PFT_HIPCHK(t, copy(leaf_order, t->d_leaf_order, leaf_order_cap, n_pts, sizeof(uint32_t)));
  return PFT_OK;
}

extern "C" int pft_debug_get_likelihood_layout(pft_tracker* t, uint32_t out4[4]) {
  if (!t || !out4) return PFT_ERR_INVALID_ARG;
  PftHeader h;
  int r = read_hdr(t, &h);
  if (r != PFT_OK) return r;
  memcpy(out4, h.lik_layout, sizeof(h.lik_layout));
  return PFT_OK;
}

extern "C" int pft_debug_get_ancestor_level(pft_tracker* t, uint32_t out5[5]) {
  if (!t || !out5 || !t->h_stat) return PFT_ERR_INVALID_ARG;
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));  // (the builder's status word of the last build has arrived)
  out5[0] = ((volatile uint32_t*)t->h_stat)[5];
  out5[1] = (uint32_t)t->anc_up_last;
  out5[2] = (uint32_t)t->lik_up_last;
  out5[3] = t->anc_up_changes;
  out5[4] = t->graph_rebuilds;
  return PFT_OK;
}

extern "C" int pft_debug_get_ancestor_table(pft_tracker* t, uint32_t info10[10], uint32_t* table, size_t cap) {
  if (!t || !info10) return PFT_ERR_INVALID_ARG;
  PftHeader h;
  int r = read_hdr(t, &h);
  if (r != PFT_OK) return r;
  const bool has = t->d_anc != nullptr && h.anc_level > 0;
  info10[0] = has && h.anc_epoch == h.build_epoch ? 1u : 0u;
  info10[1] = has ? (uint32_t)h.anc_level : 0u;
  for (int a = 0; a < 3; a++) {
    info10[2 + a] = has ? h.anc_lo[a] : 0u;
    info10[5 + a] = has ? h.anc_bits[a] : 0u;
  }
  info10[8] = h.build_epoch;
  info10[9] = h.anc_epoch;
  const size_t cells = has ? (size_t)1 << (h.anc_bits[0] + h.anc_bits[1] + h.anc_bits[2]) : 0u;
  if (table && cells && cap) {
    PFT_HIPCHK(t, hipMemcpyAsync(table, t->d_anc, std::min(cap, cells) * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  }
  return PFT_OK;
}

extern "C" int pft_debug_get_hard_steps(pft_tracker* t, uint64_t out5[5]) {
  if (!t || !out5) return PFT_ERR_INVALID_ARG;
  PftHeader h;
  int r = read_hdr(t, &h);
  if (r != PFT_OK) return r;
  for (int i = 0; i < 5; i++) out5[i] = h.dbg_hard[i];
  return PFT_OK;
}

extern "C" int pft_debug_get_scan_stats(pft_tracker* t, uint64_t* queries, uint64_t* scanned) {
  if (!t) return PFT_ERR_INVALID_ARG;
  PftHeader h;
  int r = read_hdr(t, &h);
  if (r != PFT_OK) return r;
  if (queries) *queries = h.stat_queries;
  if (scanned) *scanned = h.stat_scanned;
  return PFT_OK;
}

// population stages on explicit arrays (temporary buffers; the live state is not touched)
struct DbgPop {
  DevBuf<pft_particle> part;
  DevBuf<int32_t> a;
  DevBuf<double> q;
  DevBuf<int32_t> list;
  DevBuf<double> pref;
  DevBuf<uint32_t> pos;
  DevBuf<double> rows;
};

// partial != null: the raw weights are first formed from the n x nchunk likelihood partial sums given (from_partials)
static int dbg_population(pft_tracker* t, std::vector<pft_particle>& host, int norm, int mean, int alias, DbgPop& b,
                          PftHeader* hout, const double* partial = nullptr, uint32_t nchunk = 0) {
  const size_t n = host.size();
  if (n > PFT_MAX_PARTICLES) return PFT_ERR_CAPACITY;
  if (partial) {
    PFTT_GROW(t, b.rows.alloc(n * nchunk));
    PFT_HIPCHK(t, hipMemcpyAsync(b.rows, partial, n * nchunk * sizeof(double), hipMemcpyHostToDevice, t->stream));
  }
  PFTT_GROW(t, b.part.alloc(n));
  PFTT_GROW(t, b.a.alloc(n));
  PFTT_GROW(t, b.q.alloc(n));
  PFTT_GROW(t, b.list.alloc(2 * n));
  PFTT_GROW(t, b.pref.alloc(2 * n));
  PFTT_GROW(t, b.pos.alloc(n));
  PFT_HIPCHK(t, hipMemcpyAsync(b.part, host.data(), n * sizeof(pft_particle), hipMemcpyHostToDevice, t->stream));
  PFT_HIPCHK(t, hipMemsetAsync(t->d_dbg_hdr, 0, sizeof(PftHeader), t->stream));
  pftt_sync_dev(t);
  PftDev d = t->dev;
  d.p_active = nullptr;  // explicit particle count (a KLD handle's device-side count does not apply here)
  d.part_all = b.part;
  d.alias_list = b.list;
  d.alias_pref = b.pref;
  d.alias_pos = b.pos;
  d.hdr = t->d_dbg_hdr;
  PftParams prm = t->prm;
  if (partial) {
    d.partial = b.rows;
    d.raw_w = nullptr;
    prm.nchunk = nchunk;
  }
  pftk_population(t->stream, prm, d, (uint32_t)n, partial ? 1 : 0, norm, mean, alias);
  if (alias) pftk_alias_materialize(t->stream, d, (uint32_t)n, b.a, b.q);
  PFT_HIPCHK(t, hipMemcpyAsync(host.data(), b.part, n * sizeof(pft_particle), hipMemcpyDeviceToHost, t->stream));
  if (hout) PFT_HIPCHK(t, hipMemcpyAsync(hout, t->d_dbg_hdr, sizeof(PftHeader), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  PFT_HIPCHK(t, hipGetLastError());
  return PFT_OK;
}

extern "C" int pft_debug_normalize(pft_tracker* t, float* w, size_t n, double* fit_ratio) {
  if (!t || !w || !n) return PFT_ERR_INVALID_ARG;
  std::vector<pft_particle> h(n);
  memset(h.data(), 0, n * sizeof(pft_particle));
  for (size_t i = 0; i < n; i++) h[i].weight = w[i];
  DbgPop b;
  PftHeader hd;
  int r = dbg_population(t, h, 1, 0, 0, b, &hd);
  if (r != PFT_OK) return r;
  for (size_t i = 0; i < n; i++) w[i] = h[i].weight;
  if (fit_ratio) *fit_ratio = hd.fit_ratio;
  return PFT_OK;
}

extern "C" int pft_debug_normalize_partials(pft_tracker* t, const double* partial, size_t nchunk, size_t n, float* w,
                                            double* fit_ratio) {
  if (!t || !partial || !nchunk || nchunk > 0xffffu || !w || !n) return PFT_ERR_INVALID_ARG;
  std::vector<pft_particle> h(n);
  memset(h.data(), 0, n * sizeof(pft_particle));
  DbgPop b;
  PftHeader hd;
  int r = dbg_population(t, h, 1, 0, 0, b, &hd, partial, (uint32_t)nchunk);
  if (r != PFT_OK) return r;
  for (size_t i = 0; i < n; i++) w[i] = h[i].weight;
  if (fit_ratio) *fit_ratio = hd.fit_ratio;
  return PFT_OK;
}

extern "C" int pft_debug_alias(pft_tracker* t, const float* w, size_t n, int32_t* a, double* q) {
  if (!t || !w || !n || !a || !q) return PFT_ERR_INVALID_ARG;
  std::vector<pft_particle> h(n);
  memset(h.data(), 0, n * sizeof(pft_particle));
  for (size_t i = 0; i < n; i++) h[i].weight = w[i];
  DbgPop b;
  int r = dbg_population(t, h, 0, 0, 1, b, nullptr);
  if (r != PFT_OK) return r;
  PFT_HIPCHK(t, hipMemcpy(a, b.a, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  PFT_HIPCHK(t, hipMemcpy(q, b.q, n * sizeof(double), hipMemcpyDeviceToHost));
  return PFT_OK;
}

extern "C" int pft_debug_weighted_mean(pft_tracker* t, const pft_particle* p, size_t n, pft_particle* out) {
  if (!t || !p || !n || !out) return PFT_ERR_INVALID_ARG;
  std::vector<pft_particle> h(p, p + n);
  DbgPop b;
  PftHeader hd;
  int r = dbg_population(t, h, 0, 1, 0, b, &hd);
  if (r != PFT_OK) return r;
  *out = hd.rep;
  return PFT_OK;
}

extern "C" int pft_debug_init_particles(pft_tracker* t, const pft_particle* rep, uint32_t id_offset, size_t n_local,
                                        pft_particle* out) {
  if (!t || !rep || !out || !n_local) return PFT_ERR_INVALID_ARG;
  DevBuf<pft_particle> d;
  PFTT_GROW(t, d.alloc(n_local));
  PftParams p = t->prm;
  p.id_offset = id_offset;
  p.P_local = (uint32_t)n_local;
  pftk_init_particles(t->stream, p, *rep, d, nullptr, nullptr);
  hipError_t e = hipMemcpyAsync(out, d, n_local * sizeof(pft_particle), hipMemcpyDeviceToHost, t->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  PFT_HIPCHK(t, e);
  return PFT_OK;
}

extern "C" int pft_debug_resample(pft_tracker* t, const pft_particle* old, size_t n_total, const int32_t* a,
                                  const double* q, const pft_particle* rep, uint32_t epoch, uint32_t id_offset,
                                  size_t n_local, pft_particle* out) {
  if (!t || !old || !a || !q || !rep || !out || !n_total || !n_local) return PFT_ERR_INVALID_ARG;
  DevBuf<pft_particle> d_old, d_out;
  DevBuf<int32_t> d_a;
  DevBuf<double> d_q;
  PFTT_GROW(t, d_old.alloc(n_total) && d_out.alloc(n_local) && d_a.alloc(n_total) && d_q.alloc(n_total));
  hipError_t e = hipMemcpyAsync(d_old, old, n_total * sizeof(pft_particle), hipMemcpyHostToDevice, t->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_a, a, n_total * sizeof(int32_t), hipMemcpyHostToDevice, t->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_q, q, n_total * sizeof(double), hipMemcpyHostToDevice, t->stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->d_dbg_hdr, 0, sizeof(PftHeader), t->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&t->d_dbg_hdr->rep, rep, sizeof(pft_particle), hipMemcpyHostToDevice, t->stream);
  if (e == hipSuccess) {
    PftParams p = t->prm;
    p.id_offset = id_offset;
    p.P_local = (uint32_t)n_local;
    p.P_total = (uint32_t)n_total;
    pftk_resample_table(t->stream, p, d_old, d_a, d_q, t->d_dbg_hdr, epoch, d_out);
    e = hipMemcpyAsync(out, d_out, n_local * sizeof(pft_particle), hipMemcpyDeviceToHost, t->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  PFT_HIPCHK(t, e);
  return PFT_OK;
}

// The product resample instances (prefix-form alias table, two-level search) on explicit inputs: the prefix form is
// built from old's weights as given (dbg_population, the handle's summation order), then the requested instance is
// launched through the product launchers.  instance: 0 k_resample<false>, 1 k_resample4<false, false>,
// 2 k_resample4<true, false> (needs a reference cloud whose support subset fits the fused form)
extern "C" int pft_debug_resample_prefix(pft_tracker* t, const pft_particle* old, size_t n_total, const pft_particle* rep,
                                         uint32_t epoch, uint32_t id_offset, size_t n_local, int instance,
                                         pft_particle* out, float* mats12) {
  if (!t || !old || !rep || !out || !n_total || !n_local || instance < 0 || instance > 2) return PFT_ERR_INVALID_ARG;
  if (n_local > n_total || (size_t)id_offset > n_total - n_local) return PFT_ERR_INVALID_ARG;
  if (instance == 2 && (!t->dev.ref_box || t->prm.M_box == 0u)) return PFT_ERR_STATE;
  std::vector<pft_particle> h(old, old + n_total);
  DbgPop b;
  int r = dbg_population(t, h, 0, 0, 1, b, nullptr);
  if (r != PFT_OK) return r;
  PftParams p = t->prm;
  p.id_offset = id_offset;
  p.P_local = (uint32_t)n_local;
  p.P_total = (uint32_t)n_total;
  const uint32_t nparts = (4u * p.P_local + 255u) / 256u;
  DevBuf<pft_particle> d_out;
  DevBuf<float> d_mats, d_box;
  PFTT_GROW(t, d_out.alloc(n_local) && d_mats.alloc(n_local * 12) && d_box.alloc((size_t)nparts * 6));
  hipError_t e = hipMemcpyAsync(&t->d_dbg_hdr->rep, rep, sizeof(pft_particle), hipMemcpyHostToDevice, t->stream);
  bool launched = true;
  if (e == hipSuccess) {
    PftDev d = t->dev;
    d.p_active = nullptr;
    d.gate = nullptr;  // (the ungated instances)
    d.part_all = b.part;
    d.alias_list = b.list;
    d.alias_pref = b.pref;
    d.alias_pos = b.pos;
    d.hdr = t->d_dbg_hdr;
    d.mats = d_mats;
    d.bbox_part = d_box;
    d.bbox_part_cap = nparts;
    if (instance == 2)
      launched = pftk_resample_box(t->stream, p, d, epoch, d_out) != 0u;
    else
      pftk_resample(t->stream, p, d, epoch, d_out, instance == 0);
    if (launched) e = hipMemcpyAsync(out, d_out, n_local * sizeof(pft_particle), hipMemcpyDeviceToHost, t->stream);
    if (launched && e == hipSuccess && mats12)
      e = hipMemcpyAsync(mats12, d_mats, n_local * 12 * sizeof(float), hipMemcpyDeviceToHost, t->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if (e == hipSuccess) e = hipGetLastError();
  PFT_HIPCHK(t, e);
  return launched ? PFT_OK : PFT_ERR_STATE;
}

extern "C" int pft_debug_pose_to_matrix(pft_tracker* t, const pft_particle* p, size_t n, float* m12) {
  if (!t || !p || !n || !m12) return PFT_ERR_INVALID_ARG;
  DevBuf<pft_particle> d;
  DevBuf<float> dm;
  PFTT_GROW(t, d.alloc(n) && dm.alloc(n * 12));
  hipError_t e = hipMemcpyAsync(d, p, n * sizeof(pft_particle), hipMemcpyHostToDevice, t->stream);
  if (e == hipSuccess) {
    pftk_pose_to_matrix(t->stream, d, (uint32_t)n, dm);
    e = hipMemcpyAsync(m12, dm, n * 12 * sizeof(float), hipMemcpyDeviceToHost, t->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  PFT_HIPCHK(t, e);
  return PFT_OK;
}

// k_pack_reference (the reference side's RGB2HSV and its float triples) on buffers of its own: the handle's reference cloud
// is not touched and no hull is taken
extern "C" int pft_debug_pack_reference(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n, float* hsv_out) {
  if (!t || !pts || !n || !hsv_out) return PFT_ERR_INVALID_ARG;
  if (n > 0x7fffffffu) return PFT_ERR_CAPACITY;
  hipSetDevice(t->cfg.device_id);
  DevBuf<pft_point_xyzrgba> d_pts;
  DevBuf<float4> d_xyz, d_hsv;
  PFTT_GROW(t, d_pts.alloc(n) && d_xyz.alloc(n) && d_hsv.alloc(n));
  hipError_t e = hipMemcpyAsync(d_pts, pts, n * sizeof(pft_point_xyzrgba), hipMemcpyHostToDevice, t->stream);
  if (e == hipSuccess) {
    pftk_pack_reference(t->stream, d_pts, (uint32_t)n, t->prm.hsv_argorder, d_xyz, d_hsv);
    e = hipMemcpyAsync(hsv_out, d_hsv, n * sizeof(float4), hipMemcpyDeviceToHost, t->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if (e == hipSuccess) e = hipGetLastError();
  PFT_HIPCHK(t, e);
  return PFT_OK;
}

// mats12 != null: the launch also writes the 3x4 matrix of every candidate (the pose -> matrix step the kernel fuses, as
// in pft_compute); the first n_out of them are returned
static int dbg_kld_resample(pft_tracker* t, const pft_particle* old, size_t n_old, const int32_t* a, const double* q,
                            const pft_particle* motion, uint32_t epoch, pft_particle* out, int32_t* bins6,
                            uint32_t* n_out, uint32_t* k_out, float* mats12) {
  if (!t || !old || !n_old || (!a) != (!q) || !motion || !out || !n_out) return PFT_ERR_INVALID_ARG;
  if (!t->prm.kld) return PFT_ERR_STATE;
  const uint32_t maxn = t->prm.kld_max;
  const bool table = a != nullptr;
  // without a table: the prefix form of old's weights as given (dbg_population, the handle's summation order) and the
  // product instance k_resample_kld<false, false>
  DbgPop b;
  if (!table) {
    std::vector<pft_particle> ho(old, old + n_old);
    int r = dbg_population(t, ho, 0, 0, 1, b, nullptr);
    if (r != PFT_OK) return r;
  }
  DevBuf<pft_particle> d_old, d_out;  // (d_old, d_a, d_q stay null without a table)
  DevBuf<int32_t> d_a, d_bins;
  DevBuf<double> d_q;
  DevBuf<float> d_mats;
  PFTT_GROW(t, d_out.alloc(maxn) && d_bins.alloc((size_t)6 * maxn));
  if (table) PFTT_GROW(t, d_old.alloc(n_old) && d_a.alloc(n_old) && d_q.alloc(n_old));
  if (mats12) PFTT_GROW(t, d_mats.alloc((size_t)12 * maxn));
  PftHeader* h = new PftHeader();
  memset(h, 0, sizeof(*h));
  h->p_active = (uint32_t)n_old;
  h->motion = *motion;
  hipError_t e = hipSuccess;
  if (table) {
    if (e == hipSuccess) e = hipMemcpyAsync(d_old, old, n_old * sizeof(pft_particle), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_a, a, n_old * sizeof(int32_t), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_q, q, n_old * sizeof(double), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_dbg_hdr, h, sizeof(PftHeader), hipMemcpyHostToDevice, t->stream);
  } else {  // (the debug header holds alias_m / alias_nh of the prefix form: only the count and the motion are added)
    if (e == hipSuccess)
      e = hipMemcpyAsync(&t->d_dbg_hdr->p_active, &h->p_active, sizeof(uint32_t), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(&t->d_dbg_hdr->motion, &h->motion, sizeof(pft_particle), hipMemcpyHostToDevice, t->stream);
  }
  if (e == hipSuccess) {
    PftDev d = t->dev;
    d.part_all = table ? d_old.get() : b.part.get();
    d.hdr = t->d_dbg_hdr;
    d.mats = mats12 ? d_mats.get() : nullptr;
    if (!table) {
      d.gate = nullptr;  // (the ungated instance)
      d.alias_list = b.list;
      d.alias_pref = b.pref;
      d.alias_pos = b.pos;
    }
    pftk_resample_kld(t->stream, t->prm, d, epoch, d_out, d_a, d_q, d_bins);
    e = hipMemcpyAsync(h, t->d_dbg_hdr, sizeof(PftHeader), hipMemcpyDeviceToHost, t->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if (e == hipSuccess) {
    *n_out = h->p_active;
    if (k_out) *k_out = h->kld_k;
    e = hipMemcpy(out, d_out, (size_t)h->p_active * sizeof(pft_particle), hipMemcpyDeviceToHost);
    if (e == hipSuccess && bins6) e = hipMemcpy(bins6, d_bins, (size_t)h->p_active * 6 * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && mats12) e = hipMemcpy(mats12, d_mats, (size_t)h->p_active * 12 * sizeof(float), hipMemcpyDeviceToHost);
  }
  delete h;
  PFT_HIPCHK(t, e);
  return PFT_OK;
}

extern "C" int pft_debug_kld_resample(pft_tracker* t, const pft_particle* old, size_t n_old, const int32_t* a,
                                      const double* q, const pft_particle* motion, uint32_t epoch, pft_particle* out,
                                      int32_t* bins6, uint32_t* n_out, uint32_t* k_out) {
  return dbg_kld_resample(t, old, n_old, a, q, motion, epoch, out, bins6, n_out, k_out, nullptr);
}

extern "C" int pft_debug_kld_resample_mats(pft_tracker* t, const pft_particle* old, size_t n_old, const int32_t* a,
                                           const double* q, const pft_particle* motion, uint32_t epoch,
                                           pft_particle* out, int32_t* bins6, uint32_t* n_out, uint32_t* k_out,
                                           float* mats12) {
  if (!mats12) return PFT_ERR_INVALID_ARG;
  return dbg_kld_resample(t, old, n_old, a, q, motion, epoch, out, bins6, n_out, k_out, mats12);
}

// ---- change detection: the hooks (the settings are in pft_api_features.hip) ----
extern "C" int pft_debug_change_state(pft_tracker* t, int which, uint32_t* gate, uint32_t* counter, double box[6],
                                      int32_t* depth, uint32_t* ring, uint32_t* n_calls) {
  if (!t || (which != 0 && which != 1)) return PFT_ERR_INVALID_ARG;
  PftChangeState st;
  memset(&st, 0, sizeof(st));
  const CdInst& c = which ? t->cd_dbg : t->cd;
  if (c.b.st) {
    PFT_HIPCHK(t, hipMemcpyAsync(&st, c.b.st, sizeof(st), hipMemcpyDeviceToHost, t->stream));
    PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  } else if (which == 0) {  // not enabled yet: the host's bookkeeping
    st.counter = t->cd_counter;
    st.gate = t->changed ? 1u : 0u;
  }
  if (gate) *gate = st.gate;
  if (counter) *counter = st.counter;
  if (box)
    for (int k = 0; k < 3; k++) {
      box[k] = st.mn[k];
      box[3 + k] = st.mx[k];
    }
  if (depth) *depth = st.depth;
  if (n_calls) *n_calls = st.n_calls;
  if (ring) {
    const uint32_t m = st.n_calls < PFT_CD_RING ? st.n_calls : PFT_CD_RING;
    for (uint32_t i = 0; i < m; i++) {
      const uint32_t* r = st.ring[(st.n_calls - m + i) % PFT_CD_RING];
      for (int k = 0; k < 5; k++) ring[5 * i + k] = r[k];
    }
  }
  return pftt_check_device_error(t);
}

extern "C" int pft_debug_change_detect(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n, int min_points,
                                       double resolution, int reset, uint32_t* new_idx, size_t cap, size_t* n_new) {
  if (!t || (!pts && n) || min_points < 0 || !(resolution > 0)) return PFT_ERR_INVALID_ARG;
  if (n > 0x7fffffffu) return PFT_ERR_CAPACITY;
  hipSetDevice(t->cfg.device_id);
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  if (reset || !t->cd_dbg.b.st) {
    pftt_cd_free(t->cd_dbg);
    t->cd_dbg_res = resolution;
  }
  int r = pftt_cd_reserve(t, t->cd_dbg, (uint32_t)n, true);
  if (r != PFT_OK) return r;
  std::vector<float4> xyz(n);
  for (size_t i = 0; i < n; i++) xyz[i] = make_float4(pts[i].x, pts[i].y, pts[i].z, 0.0f);
  if (n) PFT_HIPCHK(t, hipMemcpyAsync(t->cd_dbg.pts, xyz.data(), n * sizeof(float4), hipMemcpyHostToDevice, t->stream));
  PftChangeArgs a;
  a.res = t->cd_dbg_res;
  a.use = 1u;
  a.interval = 0u;
  a.min_points = (uint32_t)min_points;
  a.force = 1u;
  pftk_change_detect(t->stream, t->cd_dbg.b, t->cd_dbg.pts, nullptr, (uint32_t)n, a, t->h_stat);
  std::vector<uint32_t> mark(n);
  if (n) PFT_HIPCHK(t, hipMemcpyAsync(mark.data(), t->cd_dbg.b.mark, n * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
  PFT_HIPCHK(t, hipStreamSynchronize(t->stream));
  PFT_HIPCHK(t, hipGetLastError());
  size_t k = 0;
  for (size_t i = 0; i < n; i++)
    if (mark[i]) {
      if (new_idx && k < cap) new_idx[k] = (uint32_t)i;
      k++;
    }
  if (n_new) *n_new = k;
  return pftt_check_device_error(t);
}

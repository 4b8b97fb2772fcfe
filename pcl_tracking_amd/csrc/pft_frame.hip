// pft_frame.hip -- the frame: the A12 schedule (ParticleFilterOMPTracker::computeTracking) as a chain of kernel launches
// on the handle's stream.  The stages, the choice of the ancestor table's level, pft_compute with its graph capture, and
// the pft_dist_* phases of a sharded handle.  No CPU compute path exists here: every stage is a kernel.
#include <string>

#include "pft_tracker.h"

// ---- the stages ----
static void stage_init_particles(pft_tracker* t) {
  pft_particle rep;
  pft_to_state(t->trans, &rep);
  rep.weight = 1.0f / (float)t->prm.P_total;
  pftt_sync_dev(t);
  ProfScope ps(t, PFT_K_RESAMPLE);
  pftk_init_particles(t->stream, t->prm, rep, t->d_part[t->cur], t->d_mats, t->d_hdr);
  t->initialized = true;
  t->changed = false;
  t->resample_epoch = 0;
}

static void stage_resample(pft_tracker* t) {
  pftt_sync_dev(t);
  pft_particle* out = t->d_part[1 - t->cur];
  {
    ProfScope ps(t, PFT_K_RESAMPLE);
    if (t->prm.kld)
      pftk_resample_kld(t->stream, t->prm, t->dev, t->resample_epoch, out, nullptr, nullptr, nullptr);
    else
      pftk_resample(t->stream, t->prm, t->dev, t->resample_epoch, out, t->sw.resample_one_lane);
  }
  t->resample_epoch++;
  t->cur = 1 - t->cur;
  pftt_sync_dev(t);
}

// A2+A3 (fused; transformed clouds are never materialised)
void pftt_stage_aabb(pft_tracker* t, const PftDev& d, uint32_t np, bool finalize) {
  ProfScope ps(t, PFT_K_AABB);
  pftk_aabb(t->stream, t->prm, d, np, finalize);
}
// A11 + A1 + A2 + A3 of a steady-state iteration of the fixed-size tracker: ONE launch when the box's support subset is
// small (pft_hull.hip), the quads that draw the particles fold their boxes; PFT_SPLIT_RESAMPLE=1 keeps the two launches
// (cross-check -- identical bits --, A/B timing).  The KLD variant, whose resample is a grid-wide loop of its own, and the
// first iteration after pft_set_particles / init take the separate kernels.
static void stage_resample_aabb(pft_tracker* t, bool finalize) {
  if (!t->prm.kld && t->changed && !t->sw.split_resample) {
    pftt_sync_dev(t);
    uint32_t nparts;
    {
      ProfScope ps(t, PFT_K_RESAMPLE);
      nparts = pftk_resample_box(t->stream, t->prm, t->dev, t->resample_epoch, t->d_part[1 - t->cur]);
    }
    if (nparts) {
      t->resample_epoch++;
      t->cur = 1 - t->cur;
      pftt_sync_dev(t);
      t->dev.bbox_grid = nparts;  // (the consumers of the partials: the crop kernel, k_bbox_final)
      if (finalize) pftk_bbox_final(t->stream, t->dev);
      return;
    }
  }
  if (t->changed) stage_resample(t);
  pftt_sync_dev(t);
  pftt_stage_aabb(t, t->dev, t->prm.kld ? t->Pcap : t->prm.P_local, finalize);
}
// A4, A5, A6+A7
__global__ void k_inject_error(PftHeader* hdr, uint32_t bits) { hdr->error |= bits; }

// The ancestor table's level for the next build, depth - anc_up: 1 when the D - 1 window of the PREVIOUS
// build fitted the table, else 2 when its D - 2 window did, else 0 -- read from the pinned status block without
// synchronising, like the builder choice; a wrong guess costs time (the builder fills nothing when the window does not fit,
// and the likelihood instance runs table-less on a tree whose table is not at its level, ~15 us dearer than either table),
// never the result.  So D - 1 is asked for only after PFT_ANC_UP_CONFIRM builds in a row have seen a fitting D - 1 window:
// a window that hovers at the cap (the free-running filter's does, from frame to frame) stays at D - 2.  Before the
// first build's word has arrived: D - 2.  own_population false (pft_eval_weights): never D - 1 unless forced -- its
// DEBUG_NN form has the level D - 2 code only, and the two forms of one evaluation walk the same table.
#define PFT_ANC_UP_CONFIRM 8u
static int pick_anc_up(pft_tracker* t, bool own_population, bool gather) {
  // (gather false: the builder copies the few leaf records itself and no launch behind it fills a table)
  if (!t->d_anc || !t->sw.ancestor_table || t->leaf_indirect || !gather) return 0;
  if (t->sw.anc_up_force >= 0) return t->sw.anc_up_force;
  const volatile uint32_t* hs = t->h_stat;
  const uint32_t w = hs ? hs[5] : 0u;
  if (!(w & 0x80000000u)) return 2;
  if (own_population) {
    t->anc_fit_streak = (w & 0xffu) <= PFT_ANC_CAP_BITS ? t->anc_fit_streak + 1u : 0u;
    if (t->anc_fit_streak >= PFT_ANC_UP_CONFIRM) return 1;
  }
  return ((w >> 8) & 0xffu) <= PFT_ANC_CAP_BITS ? 2 : 0;
}

void pftt_stage_crop_octree_likelihood(pft_tracker* t, const PftDev& d, uint32_t np, bool debug_nn,
                                       bool bbox_from_partials, bool keep_point_keys, bool likelihood, bool own_population) {
  {
    ProfScope ps(t, PFT_K_CROP);
    if (++t->crop_epoch == 0) t->crop_epoch = 1;
    const bool from_filter = t->n_on_device && t->raw_pending;
    pftk_crop(t->stream, t->prm, d, bbox_from_partials, t->crop_epoch, t->raw_pending, t->sw.crop_two_pass,
              from_filter ? t->n_src : nullptr);
    t->raw_pending = nullptr;
    if (from_filter && t->borrow) {  // the filter's output and count word have been read: its next apply waits for this
      hipEventRecord(t->borrow->ev, t->stream);
      t->borrow->recorded = true;
      t->borrow->armed = false;
    }
    if (t->inject_error & ~16u) {  // test hook: what a failing crop / builder would leave behind (bit 4 belongs to the
                                   // population launch: pft_compute raises it there)
      hipLaunchKernelGGL(k_inject_error, dim3(1), dim3(1), 0, t->stream, t->d_hdr.get(), t->inject_error & ~16u);
      t->inject_error &= 16u;
    }
    if (t->gate_on) {  // weight()'s change-detector test on this crop: writes the gate the launches below read
      PftChangeArgs a;
      a.res = t->cd_res_latched;
      a.use = t->cd_use ? 1u : 0u;
      a.interval = t->cd_interval;
      a.min_points = t->cd_min_points;
      a.force = 0u;
      pftk_change_detect(t->stream, t->cd.b, t->d_crop_pts, &t->d_hdr->n_crop, 0u, a, t->h_stat);
    }
  }
  if (t->cfg.exact_nearest) {  // NearestPairPointCloudCoherence: uniform grid + true nearest neighbour, no octree
    PftDev dq = d;
    {
      // the cell-sorted query arrays grow to the largest evaluation seen (16 + 8 bytes per query, up to 2^30 queries;
      // beyond that, or if the allocation fails, the per-query kernel serves)
      const unsigned long long nq = (unsigned long long)np * t->prm.M;
      if (nq > t->eq_cap && nq <= (1ull << 30)) {
        t->eq_cap = t->eq_blk_cap = t->eq_tiles_cap = 0;
        t->d_eq_tiles.reset();
        const size_t nblk = (size_t)(nq / 64u) + PFT_EC_SLOTS + 64u;
        size_t ppw = ((size_t)np + (size_t)t->num_cus - 1u) / (size_t)t->num_cus;  // as pftk_likelihood_exact tiles the particles
        ppw = ppw < 1u ? 1u : (ppw > 32u ? 32u : ppw);
        const size_t ntiles = ((size_t)np + ppw - 1u) / ppw + 1u;
        if (t->d_eq_sorted.alloc((size_t)nq) && t->d_eq_out.alloc((size_t)nq) && t->d_eq_blk.alloc(nblk)) {
          t->eq_cap = (uint32_t)nq;
          t->eq_blk_cap = (uint32_t)nblk;
          // the per-tile count tables are optional (k_eq_scatter counts its tile again without them)
          const size_t want = ntiles < 4096u ? ntiles : 4096u;
          if (t->d_eq_tiles.alloc(want * 2u * 8192u)) t->eq_tiles_cap = (uint32_t)want;
        } else {
          t->d_eq_sorted.reset();
          t->d_eq_out.reset();
          t->d_eq_blk.reset();
        }
      }
      // the candidate pool follows the demand of the previous iteration (pinned status word 4, read without
      // synchronising; a pool that is too small costs time -- its overflow cells keep the ring search -- never the result)
      {
        const volatile uint32_t* hs = t->h_stat;
        const uint32_t demand = hs ? hs[4] : 0u;
        const uint32_t pool_cap = (uint32_t)t->d_ec_list.cap();
        if (demand > pool_cap && pool_cap < PFT_EC_POOL) {
          unsigned long long want = (unsigned long long)demand + demand / 4u;  // a quarter of head-room
          uint32_t cap = pool_cap;
          while (cap < want && cap < PFT_EC_POOL) cap <<= 1;
          hipStreamSynchronize(t->stream);
          DevBuf<float4> grown;
          if (grown.alloc((size_t)cap)) t->d_ec_list.swap(grown);  // (else: keep the smaller pool)
        }
        dq.ec_list = t->d_ec_list;
        dq.ec_pool_cap = (uint32_t)t->d_ec_list.cap();
        t->dev.ec_list = dq.ec_list;
        t->dev.ec_pool_cap = dq.ec_pool_cap;
      }
      dq.eq_sorted = t->d_eq_sorted;
      dq.eq_out = t->d_eq_out;
      dq.eq_blk = t->d_eq_blk;
      dq.eq_cap = t->eq_cap;
      dq.eq_blk_cap = t->eq_blk_cap;
      dq.eq_tiles = t->d_eq_tiles;
      dq.eq_tiles_cap = t->eq_tiles_cap;
      // (t->dev is not formed anew here -- `d` may be t->dev itself, with this iteration's bbox_grid --: the fields that
      // can have moved are carried over by hand, so that it never keeps a freed address)
      t->dev.eq_sorted = dq.eq_sorted;
      t->dev.eq_out = dq.eq_out;
      t->dev.eq_blk = dq.eq_blk;
      t->dev.eq_cap = dq.eq_cap;
      t->dev.eq_blk_cap = dq.eq_blk_cap;
      t->dev.eq_tiles = dq.eq_tiles;
      t->dev.eq_tiles_cap = dq.eq_tiles_cap;
    }
    {
      ProfScope ps(t, PFT_K_OCTREE);
      pftk_exact_grid(t->stream, t->prm, dq);  // (dq: the copy that carries the current candidate pool)
    }
    ProfScope ps(t, PFT_K_LIKELIHOOD);
    pftk_likelihood_exact(t->stream, t->prm, dq, np, debug_nn, t->num_cus, t->sw.exact_path);
    return;
  }
  int anc_up = 0;  // the ancestor table's level asked of this build (pick_anc_up), and the likelihood instance with it
  {
    ProfScope ps(t, PFT_K_OCTREE);
    PftDev db = d;
    if (!keep_point_keys) db.pt_key = nullptr;  // the per-point keys are a test hook (pft_debug_get_point_keys after pft_eval_weights)
    // the single-workgroup builder is fastest for small crops, the sorted many-workgroup builder scales; both
    // are correct for any size.  The choice uses the crop size / depth of the PREVIOUS iteration, read from
    // pinned memory without synchronising.
    const volatile uint32_t* hs = t->h_stat;
    const uint32_t last_n = hs ? hs[0] : 0u, last_depth = hs ? hs[1] : 0u;
    bool sorted = last_n > PFT_SORTED_BUILD_MIN;
    if (t->sw.builder == 1) sorted = false;
    if (t->sw.builder == 2) sorted = true;
#ifdef PFT_DIAG
    // diagnostic build only (results are wrong while set): PFT_DEBUG_SKIP_OCTREE=1 reuses the tree of the
    // previous build after the first 8 builds, to measure the builder's true share of a frame
    if (t->sw.skip_octree && ++t->dbg_builds > 8) {
    } else
#endif
    if (sorted) {
      // 8-bit passes for 3 bits per level; one level of head-room over the last depth (k_so_scan flags an error
      // if the tree turned out deeper than the passes cover)
      // (a deeper tree than the passes cover is rebuilt by the rescue launch behind the sorted builder: the guess
      // costs time when it is wrong, never the iteration)
      int npass = last_depth > 0u ? (int)((3u * (last_depth + 1u) + 7u) / 8u) : 8;
      if (t->force_npass > 0) npass = t->force_npass;
      if (npass > 8) npass = 8;
      pftk_octree_sorted(t->stream, t->prm, db, t->sort, d.N, npass);
      t->leaf_indirect = false;  // (the sorted builder and the rescue launch behind it always write the leaf records)
    } else {
      // leaf records followed through leaf_order by the likelihood kernel instead of being copied: +0.32 ps per query
      // there (5.4 us at 8 192 x 2 048), -3 us per build and one launch less here: pays below ~9 million queries (the
      // reference's own 400-500 particles: 0.202 -> 0.196 ms per frame)
      t->leaf_indirect = t->sw.leaf_indirect >= 0 ? t->sw.leaf_indirect == 1 : (unsigned long long)np * t->prm.M <= 8000000ull;
      anc_up = pick_anc_up(t, own_population, last_n > PFT_GATHER_MIN);
      pftk_octree(t->stream, t->prm, db, last_n, t->leaf_indirect, anc_up);
    }
    if (t->anc_up_last >= 0 && anc_up != t->anc_up_last) t->anc_up_changes++;
    t->anc_up_last = anc_up;
  }
  if (!likelihood) return;  // pft_reacquire: crop and tree only, its own kernel reads the tree
  {
    ProfScope ps(t, PFT_K_LIKELIHOOD);
    const int flags = (t->sw.generic_descent ? 0 : 1) | (t->sw.ancestor_table ? 2 : 0) | (t->sw.ablate << 8);
    t->lik_up_last = pftk_likelihood(t->stream, t->prm, d, np, debug_nn, t->num_cus, t->leaf_indirect, flags, anc_up);
  }
}

int pftt_check_ready(pft_tracker* t) {
  if (!t) return PFT_ERR_INVALID_ARG;
  hipSetDevice(t->cfg.device_id);
  if (!t->has_input || t->N == 0) return PFT_ERR_NO_INPUT;  // PCL: PCL_ERROR + early return
  if (t->n_on_device && t->raw_pending && !(t->borrow && t->borrow->valid)) {
    // the filter was applied again, grew or was destroyed before this frame's first crop: its output is not this frame's
    t->err = "the filter handed over by pft_set_input_from_filter was applied again or destroyed before the frame's first crop";
    t->has_input = false;
    t->raw_pending = nullptr;
    return PFT_ERR_NO_INPUT;
  }
  if (!t->has_ref) return PFT_ERR_NO_REFERENCE;
  return PFT_OK;
}

extern "C" int pft_compute(pft_tracker* t) {
  int r = pftt_check_ready(t);
  if (r != PFT_OK) return r;
  if (t->cfg.world_size != 1) {
    t->err = "pft_compute on a sharded handle: drive the pft_dist_* phases instead";
    return PFT_ERR_STATE;
  }
  t->tree_of_compute = false;
  t->match_of_compute = false;
  if (!t->initialized) stage_init_particles(t);
  if (!t->cd_latched) {  // initCompute() creates the change detector at the resolution in force now
    t->cd_res_latched = t->cd_res;
    t->cd_latched = true;
  }
  t->gate_on = t->cd_ever;
  pftt_sync_dev(t);
  // Steady-state frames as ONE graph launch (opt-in): every launch below is recorded instead of issued, and the recorded
  // graph updates the instantiated one in place (kernel arguments such as the epochs and the particle-buffer parity
  // change from frame to frame, the node sequence only when the builder choice does: then it is instantiated anew).
  // The first frames run directly: they set the kernels' one-time attributes, which must not happen during capture.
  // Nothing that allocates or sets a one-time kernel attribute may run during capture: the exact-NN mode (its query
  // arrays grow with np * M inside the stage) is never captured, and a capture that fails for any other reason -- a
  // builder or rescue kernel whose attribute is set on first use, say -- switches the handle back to direct launches
  // and runs THIS frame directly: the host-side state the recorded pass advanced is put back first.
  int lik_sig = 0;  // the likelihood instances of this frame's iterations (ANC_UP + 1, two bits each)
  auto run_iterations = [&]() {
    lik_sig = 0;
    for (int it = 0; it < t->cfg.iteration_num; it++) {
      stage_resample_aabb(t, false);
      // KLD variant: launches are sized for the capacity, the kernels take particle_num_ from PftHeader::p_active
      const uint32_t np = t->prm.kld ? t->Pcap : t->prm.P_local;
      pftt_stage_crop_octree_likelihood(t, t->dev, np, false, true);
      lik_sig = ((lik_sig << 2) | (t->lik_up_last + 1)) & 0xffffff;
      if (t->inject_error & 16u) {  // test hook: a population barrier that timed out in some workgroup
        hipLaunchKernelGGL(k_inject_error, dim3(1), dim3(1), 0, t->stream, t->d_hdr.get(), 16u);
        t->inject_error &= ~16u;
      }
      {
        ProfScope ps(t, PFT_K_POPULATION);
        // raw weights from the partial sums, then weight()'s normalizeWeight(); use_change_detector_ == false
        // => changed_ = true => update(); the alias prefix form feeds the next resample: one launch
        pftk_population(t->stream, t->prm, t->dev, t->prm.kld ? t->Pcap : t->prm.P_total, 1, 1, 1, 1);
      }
      t->changed = true;  // (the launches of the next iteration; with a detector the device gate decides what they do)
      if (!t->cd_ever) t->cd_counter = t->cd_counter == 0u ? t->cd_interval : t->cd_counter - 1u;
    }
  };
  // (a frame whose input count lives on the device is launched directly: its first crop carries the filter's pointers
  // and is followed by an event record, neither of which belongs into the replayed graph)
  const bool graphed = t->use_graph && !t->cfg.exact_nearest && t->changed && !t->prof && !t->n_on_device &&
                       t->graph_frames++ >= 2u;
  if (!graphed) {
    run_iterations();
  } else {
    const int cur0 = t->cur;
    const uint32_t epoch0 = t->resample_epoch, crop0 = t->crop_epoch, grid0 = t->dev.bbox_grid;
    const pft_point_xyzrgba* raw0 = t->raw_pending;
    const uint32_t cdc0 = t->cd_counter;
    hipError_t ge = hipStreamBeginCapture(t->stream, hipStreamCaptureModeThreadLocal);
    hipGraph_t g = nullptr;
    if (ge == hipSuccess) {
      run_iterations();
      ge = hipStreamEndCapture(t->stream, &g);
    }
    if (ge == hipSuccess && g) {
      bool ready = false;
      // another likelihood instance than the instantiated graph holds (the ancestor table's level changed): a change of
      // the node sequence like the builder's -- instantiated anew, not updated in place
      if (t->graph_exec && t->graph_lik_up != lik_sig) {
        hipGraphExecDestroy(t->graph_exec);
        t->graph_exec = nullptr;
      }
      t->graph_lik_up = lik_sig;
      if (t->graph_exec) {
        hipGraphNode_t bad = nullptr;
        hipGraphExecUpdateResult res;
        ready = hipGraphExecUpdate(t->graph_exec, g, &bad, &res) == hipSuccess;
        if (!ready) {
          (void)hipGetLastError();
          hipGraphExecDestroy(t->graph_exec);
          t->graph_exec = nullptr;
        }
      }
      if (!ready) {
        ge = hipGraphInstantiate(&t->graph_exec, g, nullptr, nullptr, 0);
        t->graph_rebuilds++;
        ready = ge == hipSuccess;
      }
      if (ready) ge = hipGraphLaunch(t->graph_exec, t->stream);
    } else if (ge == hipSuccess) {
      ge = hipErrorUnknown;
    }
    if (g) hipGraphDestroy(g);
    if (ge != hipSuccess) {  // none of the frame's work was issued: back to direct launches, for this frame and for good
      (void)hipGetLastError();
      if (t->graph_exec) {
        hipGraphExecDestroy(t->graph_exec);
        t->graph_exec = nullptr;
      }
      t->use_graph = false;
      t->cur = cur0;
      t->resample_epoch = epoch0;
      t->crop_epoch = crop0;
      t->dev.bbox_grid = grid0;
      t->raw_pending = raw0;
      t->cd_counter = cdc0;
      pftt_sync_dev(t);
      run_iterations();
    }
  }
  t->gate_on = false;  // (no other entry point reads the gate: pft_eval_weights and the debug hooks evaluate)
  pftt_sync_dev(t);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    t->err = std::string("kernel launch: ") + hipGetErrorString(e);
    return PFT_ERR_HIP;
  }
  t->tree_of_compute = true;  // (pft_match: cleared by whatever rebuilds the tree for other particles)
  return PFT_OK;
}

// ---- multi-GPU phases ----
extern "C" int pft_dist_bind(pft_tracker* t, void* bbox6_dev, void* shard_dev, void* gathered_dev) {
  if (!t || !bbox6_dev || !shard_dev || !gathered_dev) return PFT_ERR_INVALID_ARG;
  t->bound_bbox6 = bbox6_dev;
  t->bound_shard = shard_dev;
  t->bound_gathered = gathered_dev;
  pftt_sync_dev(t);
  return PFT_OK;
}

extern "C" int pft_dist_begin_frame(pft_tracker* t) {
  int r = pftt_check_ready(t);
  if (r != PFT_OK) return r;
  if (!t->bound_gathered) {
    t->err = "pft_dist_bind not called";
    return PFT_ERR_STATE;
  }
  if (!t->initialized) stage_init_particles(t);
  return PFT_OK;
}

extern "C" int pft_dist_phase_a(pft_tracker* t, int iteration) {
  (void)iteration;
  int r = pftt_check_ready(t);
  if (r != PFT_OK) return r;
  if (!t->initialized) return PFT_ERR_STATE;
  stage_resample_aabb(t, true);
  return PFT_OK;
}

extern "C" int pft_dist_phase_b(pft_tracker* t) {
  int r = pftt_check_ready(t);
  if (r != PFT_OK) return r;
  pftt_sync_dev(t);
  pftt_stage_crop_octree_likelihood(t, t->dev, t->prm.P_local, false, false);
  {
    ProfScope ps(t, PFT_K_POPULATION);
    // raw weights from the partial sums, written with their particles straight into the all-gather's send buffer
    pftk_finalize_raw(t->stream, t->prm, t->dev, t->prm.P_local, nullptr, static_cast<pft_particle*>(t->bound_shard));
  }
  return PFT_OK;
}

extern "C" int pft_dist_phase_c(pft_tracker* t) {
  int r = pftt_check_ready(t);
  if (r != PFT_OK) return r;
  pftt_sync_dev(t);
  {
    ProfScope ps(t, PFT_K_POPULATION);
    pftk_population(t->stream, t->prm, t->dev, t->prm.P_total, 0, 1, 1, 1);
  }
  t->changed = true;
  return PFT_OK;
}

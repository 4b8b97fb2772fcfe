// pft_tracker.h -- the tracker handle behind include/pft.h and the host helpers its translation units share:
//   pft_api.hip           names, config, profiling, create / destroy, reference, input, hand-offs, particles, result
//   pft_frame.hip         the stages of a frame, pft_compute with its graph capture, the pft_dist_* phases
//   pft_api_debug.hip     pft_eval_weights, the pft_debug_* hooks, the state checkpoint
//   pft_api_features.hip  change-detector settings, report, match, spread, visibility, re-acquisition, refinement
//   pft_view.hip          the view-dependent reference: its kernels and its part of the C ABI (include/pft_view.h)
// Internal: nothing outside csrc/ includes this.
//
// Device memory: every buffer the handle owns is a DevBuf (pft_devbuf.h), so deleting the handle frees it and no list of
// buffers exists anywhere.  A buffer that grows alone is its own capacity (cap()).  Buffers that grow as a group share a
// capacity word (in_cap, ref_cap, rq_cap, eq_*, rf.g_cap, CdInst::b.cap), and every group follows one rule: the word is
// set to 0, and the state flags that depend on the group are cleared, BEFORE the first free, and the word is set again
// after the last successful allocation.  A failed growth goes through PFTT_GROW, which forms PftDev anew, so neither the
// handle nor t->dev ever holds a freed address or a capacity over a null buffer.
#pragma once
#include <string>
#include <vector>

#include "pft_devbuf.h"
#include "pft_internal.h"

// a DevBuf growth of the tracker's: the failing call's text as the message, PftDev formed anew, PFT_ERR_HIP
#define PFTT_GROW(t, call)                                                                    \
  do {                                                                                        \
    if (!(call)) {                                                                            \
      (t)->err = std::string(#call) + ": " + pft_dev_alloc_error();                           \
      pftt_sync_dev(t);                                                                       \
      return PFT_ERR_HIP;                                                                     \
    }                                                                                         \
  } while (0)

struct EvPair {
  hipEvent_t a, b;
};

// one change-detector instance: the device state and its buffers (pft_change.hip).  b is the kernel argument, formed from
// the buffers by pftt_cd_reserve
struct CdInst {
  PftChangeBufs b = {};
  DevBuf<PftChangeState> st;
  DevBuf<unsigned long long> set_key[2], tab_key, pt_key;
  DevBuf<uint32_t> set_cnt[2], tab_cnt, mark;
  DevBuf<float4> pts;  // pft_debug_change_detect: the explicit cloud
};

struct pft_tracker {
  pft_config cfg;
  PftParams prm;
  PftDev dev;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int num_cus = 256;
  std::string err;

  // buffers
  DevBuf<pft_point_xyzrgba> d_ref_raw;
  DevBuf<float4> d_ref_xyz, d_ref_hsv, d_ref_box;
  uint32_t ref_cap = 0;
  DevBuf<pft_point_xyzrgba> d_in_raw;
  DevBuf<float4> d_in_pts;
  uint32_t in_cap = 0, N = 0;
  const pft_point_xyzrgba* raw_pending = nullptr;  // input handed over but not yet packed: the next crop does it
  // pft_set_input_from_filter: the frame's input count lives on the device.  N is then its bound; the first crop reads
  // the count from n_src (the filter's word), latches it into d_n_in for the later crops and records borrow->ev
  bool n_on_device = false;
  const uint32_t* n_src = nullptr;
  DevBuf<uint32_t> d_n_in;
  PftBorrow* borrow = nullptr;  // the link to the filter last borrowed from (shared with it)
  const pft_filter* borrow_of = nullptr;
  DevBuf<pft_particle> d_part[2];
  int cur = 0;
  DevBuf<float> d_mats;
  DevBuf<float> d_bbox_part;  // six floats per partial box
  DevBuf<float> d_bbox6;
  DevBuf<uint32_t> d_crop_counts;
  DevBuf<unsigned long long> d_crop_slots;
  uint32_t crop_epoch = 0;  // tag of the last one-pass crop launch (0 = what freshly allocated slots hold)
  DevBuf<float4> d_crop_pts;
  DevBuf<int32_t> d_crop_idx;
  DevBuf<uint32_t> d_words;
  uint32_t max_words = 0;
  DevBuf<uint16_t> d_jump;
  DevBuf<uint32_t> d_anc;    // ancestor table (PFT_ANC_CAP entries; null with PFT_ANCESTOR_TABLE=0)
  DevBuf<uint32_t> d_ref_perm;
  DevBuf<float4> d_leaf_pts;
  DevBuf<uint32_t> d_leaf_order, d_pt_node, d_pt_key, d_pt_tmp;
  DevBuf<unsigned long long> d_pt_key64;
  SortBufs sort = {};  // the sorted builder's argument, formed from the buffers below by ensure_input_capacity
  DevBuf<unsigned long long> d_sort_keys[2];
  DevBuf<uint32_t> d_sort_vals[2], d_sort_hist, d_sort_tile_cnt;
  DevBuf<float> d_sort_tile_box;
  uint32_t* h_stat = nullptr;   // pinned, device-visible (freed by the destructor)
  PftSwitches sw = {};          // the path switches, read once by pft_create
  bool leaf_indirect = false;   // leaf-record form of the last tree built (PftSwitches::leaf_indirect and the size rule)
  int force_npass = 0;          // test hook (pft_debug_set_limits): radix passes of the sorted builder, 0 = from the last depth
  uint32_t inject_error = 0;    // test hook (pft_debug_inject_error): bits OR-ed into PftHeader::error after the next crop
  DevBuf<double> d_partial;
  DevBuf<int32_t> d_alias_list;
  DevBuf<double> d_alias_pref;
  DevBuf<double> d_pop_part;
  DevBuf<uint32_t> d_eg_start, d_eg_cnt, d_eg_tile;
  DevBuf<uint32_t> d_ec_slot, d_ec_cells, d_ec_count, d_ec_base;
  DevBuf<float4> d_ec_list;  // the candidate pool: cap() entries
  // exact-NN mode, cell-sorted queries (sized by the largest particle count x reference size evaluated so far)
  DevBuf<uint32_t> d_eq_cellq, d_eq_nq, d_eq_qbase, d_eq_bbase, d_eq_fill, d_eq_blk, d_eq_tiles;
  DevBuf<float4> d_eq_sorted;
  DevBuf<double> d_eq_out;
  uint32_t eq_cap = 0, eq_blk_cap = 0, eq_tiles_cap = 0;
  uint32_t ec_slots_cap = PFT_EC_SLOTS;  // test hook (pft_debug_set_exact_limits): list slots handed out, never above the allocation
  DevBuf<uint32_t> d_kld_table;
  DevBuf<int32_t> d_kld_bins;
  uint32_t dbg_builds = 0;
  uint32_t Pcap = 0;  // particle capacity of the buffers (== P_total unless KLD-adaptive)
  DevBuf<uint32_t> d_alias_pos;
  DevBuf<float> d_raw_w;
  DevBuf<PftHeader> d_hdr;
  DevBuf<int32_t> d_nn_idx;
  DevBuf<float> d_nn_d2;  // (allocated after d_nn_idx: its cap() is the pairs both have room for)
  // debug scratch
  DevBuf<pft_particle> d_dbg_part;
  DevBuf<PftHeader> d_dbg_hdr;
  DevBuf<float> d_dbg_f;
  // dist binding
  void *bound_bbox6 = nullptr, *bound_shard = nullptr, *bound_gathered = nullptr;

  // pft_debug_state_save / _restore: a checkpoint of the filter state in HBM (bench.py's stationary workload, tests)
  DevBuf<pft_particle> sv_part;
  DevBuf<int32_t> sv_alias_list;
  DevBuf<double> sv_alias_pref;
  DevBuf<uint32_t> sv_alias_pos;
  DevBuf<PftHeader> sv_hdr;
  int sv_cur = 0;
  uint32_t sv_epoch = 0;
  bool sv_changed = false, sv_valid = false;

  // change detection (pft_set_change_detector): PCL's settings, read on every call except the resolution, which the first
  // pft_compute latches.  Until the detector is first enabled no detector launch exists and the host keeps
  // change_counter_ (every iteration evaluates then); from then on the counter and changed_ live on the device
  int cd_use = 0;
  uint32_t cd_interval = 10, cd_min_points = 10;
  double cd_res = 0.01, cd_res_latched = 0.01;
  bool cd_latched = false, cd_ever = false, gate_on = false;
  uint32_t cd_counter = 0;
  CdInst cd, cd_dbg;
  double cd_dbg_res = 0.01;  // resolution of pft_debug_change_detect's instance since its last reset
  DevBuf<PftChangeState> sv_cd;
  DevBuf<unsigned long long> sv_cd_key[2];
  DevBuf<uint32_t> sv_cd_cnt[2];  // (sv_cd_cnt[1] is allocated last: its cap() is the checkpoint's capacity in points)
  bool sv_cd_valid = false;
  uint32_t sv_cd_counter = 0;

  // object report (pft_set_report_cloud / pft_report): the report cloud, its tracked copy and the report itself
  DevBuf<pft_point_xyzrgba> d_rep_pts;
  DevBuf<pft_point_xyzrgba> d_rep_tracked;  // (allocated after d_rep_pts: its cap() is the points both have room for)
  DevBuf<pft_object_report> d_report;
  uint32_t rep_n = 0;
  uint32_t rep_tracked_n = 0;  // points of the tracked cloud the last pft_report wrote (0: none, or the buffer was replaced)
  bool rep_issued = false;     // a pft_report has been enqueued: d_report holds (or will hold) its result

  // match statistics (pft_match): the result block with the lost rule's state, and the pairs in the caller's order
  DevBuf<pft_match_stats> d_match;
  DevBuf<int32_t> d_match_idx;
  DevBuf<float> d_match_d2;      // (allocated after d_match_idx: its cap() is the reference points both have room for)
  uint32_t match_n = 0;          // reference points of the last pft_match (0: none since the reference was last set)
  bool match_issued = false;     // a pft_match has been enqueued: d_match holds (or will hold) its result
  bool tree_of_compute = false;  // the tree, crop and result on the device are those of the last pft_compute
  double match_min_ratio = 0.0;
  int match_lost_after = 1;

  // population statistics (pft_spread): the result block with the spread rule's state, and the per-block roots of the
  // two-launch reduction (sized once for the handle's particle capacity)
  DevBuf<pft_population_stats> d_spread;
  DevBuf<double> d_spread_part;
  DevBuf<uint32_t> d_spread_zero, d_spread_imax;
  DevBuf<float> d_spread_wmax;
  bool spread_issued = false;    // a pft_spread has been enqueued: d_spread holds (or will hold) its result
  double spread_max_pos_sigma = INFINITY, spread_min_n_eff = 0.0;
  int spread_after = 1;

  // visibility (pft_visibility): the camera, the rule's settings, the result block with the rule's state, the two depth
  // images (one buffer, sized for the largest camera used), the moved points and the per-point results
  pft_visibility_config vis_cam;     // (set by pft_create: pft_visibility_config_default)
  double vis_min_visible_ratio = 0.25, vis_min_ratio = 0.0;
  int vis_lost_after = 1;
  DevBuf<pft_visibility_stats> d_vis;
  DevBuf<PftVisCtl> d_vis_ctl;
  DevBuf<uint32_t> d_vis_z;
  DevBuf<uint2> d_vis_q;
  DevBuf<uint8_t> d_vis_state;
  DevBuf<float> d_vis_sgap, d_vis_mgap;  // (d_vis_mgap is allocated last of the four: its cap() is the points all have room for)
  uint32_t vis_n = 0;                // reference points of the last pft_visibility (0: none since the reference was last set)
  bool vis_issued = false;           // a pft_visibility has been enqueued: d_vis holds (or will hold) its result
  bool match_of_compute = false;     // a pft_match has been enqueued since the last pft_compute

  // the view-dependent reference (pft_view_select): the result block, the depth image (sized for the largest camera used),
  // the copy of a host model, and the per-record group that grows with the model
  DevBuf<pft_view_stats> d_view;
  DevBuf<PftViewCtl> d_view_ctl;
  DevBuf<uint32_t> d_view_z;
  DevBuf<pft_point_xyzrgba> d_view_model;
  DevBuf<uint2> d_view_q;
  DevBuf<uint8_t> d_view_state;
  DevBuf<float> d_view_gap;
  DevBuf<uint4> d_view_tile;
  DevBuf<uint32_t> d_view_base, d_view_idx;
  DevBuf<pft_point_xyzrgba> d_view_cloud;  // (allocated last of the group: its cap() is the records all have room for)
  uint32_t view_grid = 0;            // test hook (pft_debug_set_view_grid): workgroups of every pass, 0 = sized from the model
  bool view_issued = false;          // a select has been enqueued: d_view holds (or will hold) its result
  bool view_fresh = false;           // ... and pft_set_reference_from_view has not consumed it

  // re-acquisition (pft_reacquire): buffers of the feature's own, sized for the largest K seen (never the handle's
  // particle_num-sized ones): candidates, their matrices, the scores, the partial boxes of k_aabb, the result block
  DevBuf<pft_particle> d_rq_part;
  DevBuf<float> d_rq_mats;
  PftRqScores rq_sc = {};        // the scoring launches' argument, formed from the five buffers below by rq_reserve
  DevBuf<uint32_t> d_rq_n_inliers, d_rq_n_matched;
  DevBuf<double> d_rq_coherence, d_rq_sum_sq_dist, d_rq_inlier_sq_dist;
  uint32_t rq_cap = 0;           // candidates the arrays above have room for
  DevBuf<float> d_rq_centres;
  DevBuf<uint32_t> d_rq_first, d_rq_count;  // the segmenter form: every cluster's first point and size (d_rq_count is
                                            // allocated last of the three: its cap() is the centres all have room for)
  DevBuf<float> d_rq_bbox_part;  // num_cus partial boxes
  DevBuf<pft_reacquire_result> d_rq_result;
  uint32_t rq_n = 0;             // candidates of the last call
  bool rq_valid = false;         // a call has completed: the arrays hold its candidates and scores
  std::vector<float> rq_centres;  // the last call's centres (host copy)
  // pose refinement (pft_refine): buffers of the feature's own; rf is the launches' argument, formed by rf_reserve
  PftRefineDev rf = {};
  DevBuf<unsigned char> d_rf_ctl;   // pftk_refine_ctl_bytes() bytes: the control block is defined in pft_refine.hip
  DevBuf<double> d_rf_part;
  DevBuf<uint32_t> d_rf_part_n;
  DevBuf<pft_refine_result> d_rf_result;
  DevBuf<pft_refine_trace_entry> d_rf_trace;
  DevBuf<float> d_rf_mats;          // the eight shifted copies of the start the crop box is taken over
  uint32_t rf_n = 0;                // trace entries of the last completed call
  bool rf_valid = false;

  // state
  bool has_ref = false, has_input = false, initialized = false, changed = false;
  uint32_t resample_epoch = 0;
  float trans[16];

  // frame graph (PFT_GRAPH=1, own stream only): the launches of a steady-state frame are captured and replayed as one
  // hipGraph; the instantiated graph is updated in place while the launch sequence keeps its shape
  bool use_graph = false;
  hipGraphExec_t graph_exec = nullptr;
  uint32_t graph_frames = 0, graph_rebuilds = 0;
  // ancestor table level: what the last build was asked for, the ANC_UP of the last likelihood instance
  // launched, how often the request changed from one build to the next, and the instance the replayed graph holds
  int anc_up_last = -1, lik_up_last = -1, graph_lik_up = -1;
  uint32_t anc_up_changes = 0;
  uint32_t anc_fit_streak = 0;  // consecutive builds whose look at the status word found a D - 1 window that fits

  // profiling
  bool prof = false;
  std::vector<EvPair> ev[PFT_K_COUNT];
  std::vector<EvPair> ev_free;
  double prof_ms[PFT_K_COUNT] = {0};
  uint64_t prof_n[PFT_K_COUNT] = {0};

  // everything that is no DevBuf: the filter link, the graph, the events, h_stat, an own stream (pft_api.hip).  The
  // stream has been drained by pft_destroy
  ~pft_tracker();
};

// ---- profiling helpers ----
struct ProfScope {
  pft_tracker* t;
  int id;
  EvPair p;
  bool on;
  ProfScope(pft_tracker* t_, int id_) : t(t_), id(id_), on(t_->prof) {
    if (!on) return;
    if (!t->ev_free.empty()) {
      p = t->ev_free.back();
      t->ev_free.pop_back();
    } else {
      hipEventCreate(&p.a);
      hipEventCreate(&p.b);
    }
    hipEventRecord(p.a, t->stream);
  }
  ~ProfScope() {
    if (!on) return;
    hipEventRecord(p.b, t->stream);
    t->ev[id].push_back(p);
  }
};

// ---- host helpers used from more than one of the four files ----
// pft_api.hip
void pftt_sync_dev(pft_tracker* t);            // the one place that forms PftDev from the handle
int pftt_check_device_error(pft_tracker* t);   // after the stream has drained: PftHeader::error as a status
int pftt_match_clear_streak(pft_tracker* t);
// pft_set_reference; same_object (pft_set_reference_from_view): the streaks and flags of the three rules are kept
int pftt_set_reference(pft_tracker* t, const pft_point_xyzrgba* pts, size_t n, bool same_object);
void pftt_cd_free(CdInst& c);
int pftt_cd_reserve(pft_tracker* t, CdInst& c, uint32_t cap, bool debug);
// pft_frame.hip
int pftt_check_ready(pft_tracker* t);
void pftt_stage_aabb(pft_tracker* t, const PftDev& d, uint32_t np, bool finalize);
void pftt_stage_crop_octree_likelihood(pft_tracker* t, const PftDev& d, uint32_t np, bool debug_nn, bool bbox_from_partials,
                                       bool keep_point_keys = false, bool likelihood = true, bool own_population = true);

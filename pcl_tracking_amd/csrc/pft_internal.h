// pft_internal.h -- device-side data layout + kernel launch prototypes (gfx950 only).
//
// HBM layout of one tracker (all arrays allocated once, resident for the handle's lifetime):
//   ref_xyz / ref_hsv   float4[M]   reference points {x,y,z,-} and precomputed {fh,fs,fv,-}   (A7b, once)
//   in_pts              float4[N]   input cloud {x,y,z,rgba-bits}                              (per frame)
//   part[2]             particle[P_local] double-buffered shard; part_all = all P (gathered)
//   mats                float[12*P_local] row-major 3x4 per particle                           (A1)
//   bbox_part           float[6*grid] per-workgroup AABB partials -> bbox6 {-min xyz, max xyz}  (A3)
//   crop_pts            float4[N]   cropped points {x,y,z,h|s<<8|v<<16}, input order            (A4)
//   words               u32[]       linearised octree: branch = mask | child_base<<8, levels contiguous,
//                                   leaf = start offset into leaf_pts (+ one sentinel)          (A5)
//   (per-level per-axis voxel-centre tables: formed in LDS by the likelihood kernel from depth + box)      (A6)
//   leaf_pts            float4[N]   cropped points in leaf order (insertion order inside a leaf)
//   partial             double[P_local*nchunk] per (particle, reference chunk) likelihood sums   (A7)
//   alias_list/pref/pos prefix-sum form of the Walker alias table over all P particles          (A9)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pft.h"
#include "../../include/pft_visibility.h"
#include "../../include/pft_view.h"

#define PFT_MAX_DEVICES 64      // per-device caches of one-time kernel attributes
#define PFT_MAX_DEPTH 30
#define PFT_TABLE_MAX_DEPTH 10
#define PFT_MAX_GROW 40
#define PFT_JUMP_MAX_LEVEL 4     // 2^12 cells x u16 = 8 KiB of LDS in the likelihood kernel
#ifndef PFT_ANC_CAP_BITS
#define PFT_ANC_CAP_BITS 18      // ancestor table: log2 of the entries per handle (1 MiB); a larger window has no table
#endif
#define PFT_ANC_CAP (1u << PFT_ANC_CAP_BITS)
#define PFT_REF_CHUNK 256        // reference points per likelihood work item (upper limit; PftParams::ref_chunk)
#ifndef PFT_BUILD_THREADS
#define PFT_BUILD_THREADS 1024
#endif
#ifndef PFT_LIK_GROUPS
#define PFT_LIK_GROUPS 64        // likelihood kernel: groups of workgroups that share a dynamic work-item counter
#endif
#ifndef PFT_LIK_CTR_STRIDE
#define PFT_LIK_CTR_STRIDE 16u    // uint32 between two groups' counters
#endif
#ifndef PFT_LIK_THREADS
#define PFT_LIK_THREADS 1024   // likelihood workgroup size
#endif
#ifndef PFT_LIK_WGS_PER_CU
#define PFT_LIK_WGS_PER_CU 2    // resident likelihood workgroups per CU (each gets 1/N of the LDS)
#endif
#define PFT_POP_THREADS 1024
#define PFT_GATHER_MIN 5000u       // cropped points (last iteration) up to which the single-workgroup builder copies the leaf records itself
#define PFT_SORTED_BUILD_MIN 18000  // cropped points (last iteration) above which the sorted builder is used
#define PFT_EG_CAP (1u << 21)     // exact-NN mode: grid cells (8 MB of cell starts)
#define PFT_EC_SLOTS (1u << 19)  // exact-NN mode: candidate lists per iteration (cells hit by queries)
#define PFT_EC_POOL (1u << 24)   // exact-NN mode: candidate entries of all lists together (16 B each), upper limit
#define PFT_EC_POOL_MIN (1u << 20)  // first allocation (16 MB); the pool then follows the demand of the previous iteration
#define PFT_POPM_THREADS 256
#define PFT_POPM_ITEMS 16   // many-workgroup population path: 4096 particles per workgroup
#define PFT_POPM_MAX_WGS 256
#define PFT_POPM_MIN (16 * PFT_POP_THREADS + 1)  // above the register-resident single-workgroup range
#define PFT_MAX_PARTICLES (PFT_POPM_MAX_WGS * PFT_POPM_THREADS * PFT_POPM_ITEMS)  // 1 048 576

struct PftParams {  // immutable per handle, passed by value to kernels
  double alpha;
  double maxd2;          // max_distance * max_distance (double, as PCL compares)
  double res;            // octree resolution
  double dist_w, hsv_w;
  float h_w, s_w, v_w;
  int hsv_argorder;
  double step_sigma[6], init_sigma[6], init_mean[6];
  uint32_t seed_lo, seed_hi;
  uint32_t P_total, P_local, id_offset;
  uint32_t M, nchunk;
  uint32_t M_box;      // reference points that can be extreme in a rigidly transformed coordinate (pft_hull.hip): the box's input
  uint32_t ref_chunk;  // reference points per likelihood work item: 64 .. PFT_REF_CHUNK, smaller when there are few particles
  uint32_t split_last;  // s > 0: the last ref_chunk points of the cloud form s items of ref_chunk / s points, handed out last (shorter tail)
  // KLD-adaptive variant (KLDAdaptiveParticleFilterOMPTracker, auto_tracking.cpp:207-222)
  uint32_t kld;          // 1: the particle count changes at every resample and lives in PftHeader::p_active
  uint32_t kld_max;      // maximum_particle_number_
  double kld_z;          // normalQuantile(delta_), evaluated on the host
  double kld_eps;        // epsilon_
  float kld_bin[6];      // bin_size_ (a ParticleXYZRPY upstream: floats)
  double motion_ratio;   // motion_ratio_
  int32_t sum_order;     // pft_config::sum_order: PFT_SUM_TREE (k_population) or PFT_SUM_PCL (k_population_seq)
};

struct PftHeader {  // lives in HBM; written by kernels, read by later kernels (and by the host for debug)
  float bbox[6];    // x_min,x_max,y_min,y_max,z_min,z_max
  uint32_t n_crop;
  uint32_t error;   // per iteration (cleared by the crop kernel): bit0 octree capacity exceeded, bit1 depth / growth steps
                    // exceeded, bit2 one-pass crop gave up waiting, bit3 (internal, transient) sorted builder's radix passes
                    // too few -> the rescue launch rebuilds, bit4 a device-scope barrier of the population kernel timed out,
                    // bit5 the change detector's depth (21) or growth steps exceeded -- raised in the pinned status block
                    // only (host_stat[2..3]): every stage reads a non-zero word here as "no target", and that iteration
                    // evaluates; bit6 / bit7 a device-side input count above its bound / of zero (first crop of a frame),
                    // in the pinned status block only as well
  double omin[3], omax[3];
  int32_t depth;
  int32_t use_table;
  uint32_t n_words;   // words used incl. leaf level + sentinel
  uint32_t n_leaves;
  uint32_t leaf_start;  // index of first leaf word
  uint32_t lvl_start[PFT_MAX_DEPTH + 3];
  int32_t n_grow;
  int32_t build_path;   // 1 = register/LDS-resident builder, 0 = generic builder (diagnostic)
  // which builder instance produced the tree (read by the test hook pft_debug_get_tree only).  k_octree_build: bits 0-2 the
  // per-point store (1 RegStore<4>, 2 RegStore<8>, 3 RegStore<14>, 4 HybridStore<8>, 5 GlobStore), bit 3 the node words
  // ended in LDS, bit 4 the leaf scratch was in LDS, bit 5 an LDS attempt was abandoned and the tree rebuilt in HBM, bit 6
  // dense top levels (J > 0), bit 7 the rescue launch did the build, bits 8-9 copy_leaf_pts.  Sorted builder: 6 | npass << 10
  uint32_t build_variant;
  int32_t leaf_indirect;  // 1: leaf_pts was NOT written for this tree; the likelihood kernel reads crop_pts[leaf_order[pos]]
  // fast descent (pft_likelihood.hip): direct-index table of the level-J nodes and the safety margin
  int32_t jump_level;   // J (0 = no table): jump[kx | ky<<J | kz<<2J] = 1 + index of the node inside level J
  float margin_cells;   // a query closer than this (in leaf cells) to a cell face takes the exact generic step
  float ominf[3];       // (float) omin
  float inv_res;        // (float)(1/res)
  // ancestor table of the fast descent (PftDev::anc): entry (a << 27) | node for every level-anc_level cell c of the window
  // anc_lo + [0, 2^anc_bits) (index cx | cy << bx | cz << (bx + by)): node is the deepest existing ancestor of c at a level
  // a <= anc_level.  Written by the builders (window) and the fill (entries); used only while anc_epoch == build_epoch
  int32_t anc_level;     // L = depth - 1 or depth - 2, as the host asked and the window allowed (0: no table for this tree)
  uint32_t anc_lo[3], anc_bits[3];
  uint32_t build_epoch;  // bumped by every tree build
  uint32_t anc_epoch;    // the build_epoch the entries were filled for
  // growth history of the box replay (read by the key kernel of the sorted builder)
  uint32_t grow_idx[PFT_MAX_GROW];
  uint32_t grow_shift[PFT_MAX_GROW];      // bit a set: min of axis a lowered by the old side
  uint32_t grow_old_depth[PFT_MAX_GROW];
  double grow_min[PFT_MAX_GROW + 1][3];   // [e] = box minimum valid for points inserted in epoch e
  double fit_ratio;
  pft_particle rep;
  pft_particle motion;
  uint32_t alias_m, alias_nh;   // sizes of the small / large lists
  // exact-nearest-neighbour mode (pft_exact_nn.hip): uniform grid over the crop box
  float eg_g, eg_inv_g, eg_min[3];
  int32_t eg_dim[3];
  uint32_t eg_ncells;
  uint32_t p_active;            // KLD variant: current particle_num_ (written by init / k_resample_kld)
  uint32_t kld_k;               // KLD variant: distinct bins of the last resample (diagnostic)
  unsigned long long stat_queries, stat_scanned;
  unsigned long long dbg[32];    // debug-variant likelihood statistics (tools/descent_stats.py)
  unsigned long long ticks[32];  // wall_clock64() (100 MHz) at phase boundaries: [0..15] octree, [16..31] population
  // likelihood kernel: per group of workgroups, the next work item of the group's range (one counter per 64-byte line;
  // reset by the crop kernel of the same iteration)
  alignas(128) uint32_t lik_ctr[PFT_LIK_GROUPS * PFT_LIK_CTR_STRIDE];
  // exact-NN mode: running totals taken with returning atomics by every wave of k_ec_slots / k_ec_build.  In a cache line
  // of their own: next to the grid geometry, which the same waves READ, 22 000 atomics cost 540 us (25 ns each)
  alignas(128) uint32_t ec_nslots;  // grid cells hit by at least one query this iteration (candidate lists)
  uint32_t ec_pool_used;            // candidate entries allotted so far
  unsigned long long eq_totals;     // (64-query blocks << 32) | queries of the cells allotted so far (k_ec_slots)
  alignas(128) uint32_t crop_ticket;  // one-pass crop: workgroups take their logical index here (the last one resets it)
  uint32_t pop_bar[4];   // population kernel: arrival counters of its three device-scope barriers + "done" (self-resetting)
  // DEBUG_NN likelihood instance: queries by number of "hard" generic steps (0, 1, 2, 3, >= 4), then (directly after it:
  // pft_eval_weights clears both with one memset) the instance's choice (workgroup 0, thread 0; cleared by pft_eval_weights, read by
  // pft_debug_get_likelihood_layout): [0] bit 0 valid, bits 1-2 layout (0 node words + u16 leaf starts, 1 u32 node words,
  // 2 branch levels only, 3 hybrid), bits 3-4 descent (0 fast, 1 table generic, 2 no table), bit 5 INDIRECT instance,
  // bit 6 leaf_indirect, bit 7 the jump table dropped to make the words fit, bits 8-11 J used; [1] n_lds_words (hybrid);
  // [2] lds_bytes; [3] margin_cells (float bits)
  unsigned long long dbg_hard[5];
  uint32_t lik_layout[4];
};

struct PftDev {  // device pointers (host-side struct, passed by value)
  const float4* ref_xyz;
  const float4* ref_hsv;
  const float4* ref_box;    // [M_box] {x, y, z, .} of the box's support subset
  const float4* in_pts;
  uint32_t N;               // input points; with n_dev an upper bound on them (grids and buffers are sized by it)
  const uint32_t* n_dev;    // the input count lives on the device (pft_set_input_from_filter): the handle's own copy of it,
                            // latched by the first crop of the frame; else null
  pft_particle* part_cur;   // shard being evaluated
  pft_particle* part_all;   // all P particles (== part_cur when world_size == 1)
  float* mats;
  float* bbox_part;
  uint32_t bbox_grid;
  uint32_t bbox_part_cap;   // partial boxes bbox_part has room for
  float* bbox6;             // {-xmin,-ymin,-zmin,xmax,ymax,zmax}: max-reducible across ranks
  uint32_t* crop_counts;
  unsigned long long* crop_slots;  // one-pass crop: per workgroup (launch epoch << 32) | kept points, published with atomics
  float4* crop_pts;
  int32_t* crop_idx;
  uint32_t* words;
  uint32_t max_words;
  uint16_t* jump;           // [2^(3*PFT_JUMP_MAX_LEVEL)]
  uint32_t* anc;            // [PFT_ANC_CAP] ancestor table (PftHeader::anc_level), or null: no table for this handle
  const uint32_t* ref_perm; // sorted reference position -> index in the caller's reference cloud
  float4* leaf_pts;
  uint32_t* leaf_order;
  uint32_t* pt_node;
  uint32_t* pt_key;     // 3 per point (final-frame keys; read back by the debug hook)
  unsigned long long* pt_key64;  // packed keys of the generic (HBM-resident) builder path
  uint32_t* pt_tmp;
  double* partial;
  int32_t* alias_list;   // [0,P): small list, [P,2P): large list
  double* alias_pref;    // [0,P): running deficit, [P,2P): running excess
  uint32_t* alias_pos;   // [P]
  float* raw_w;          // [P_local] raw likelihood weights, w = -(float) sum of the particle's partial sums (k_finalize_raw)
  double* pop_part;      // [PFT_POPM_MAX_WGS][16] per-workgroup values that cross workgroups in the population kernel
  PftHeader* hdr;
  const uint32_t* p_active;  // KLD variant: &hdr->p_active (kernels take the particle count from here), else null
  uint32_t* eg_start;        // exact-NN mode: [eg_cap + 1] first slot of every grid cell
  uint32_t* eg_cnt;          // exact-NN mode: [eg_cap] cell counts / fill cursors
  uint32_t* eg_tile;         // exact-NN mode: per-2048-cell tile sums
  uint32_t eg_cap;           // exact-NN mode: cells available
  uint32_t* ec_slot;         // exact-NN mode: [eg_cap] 0 = no query in this cell, 1 = hit (before the slots are allotted), 0xffffffff = no list, else list slot + 2
  uint32_t* ec_cells;        // exact-NN mode: [PFT_EC_SLOTS] cell of every list slot
  uint32_t* ec_count;        // exact-NN mode: [PFT_EC_SLOTS] candidates of the list (0xffffffff: the pool was full, no list)
  uint32_t* ec_base;         // exact-NN mode: [PFT_EC_SLOTS] first entry of the list in ec_list
  float4* ec_list;           // exact-NN mode: [ec_pool_cap] candidates {x, y, z, position in leaf_pts}
  uint32_t ec_pool_cap;      // entries of ec_list: grows with the demand of the previous iteration, at most PFT_EC_POOL
  uint32_t ec_slots_cap;     // exact-NN mode: list slots handed out, PFT_EC_SLOTS (the allocation) unless pft_debug_set_exact_limits lowered it
  // exact-NN mode, queries sorted by grid cell (one wave then walks ONE candidate list for 64 queries):
  uint32_t* eq_cellq;        // [eg_cap] queries per grid cell this iteration
  uint32_t* eq_nq;           // [PFT_EC_SLOTS] queries of the slot's cell that are searched through its list
  uint32_t* eq_qbase;        // [PFT_EC_SLOTS] first sorted query of the slot
  uint32_t* eq_bbase;        // [PFT_EC_SLOTS] first 64-query block of the slot
  uint32_t* eq_fill;         // [PFT_EC_SLOTS] fill cursor of the scatter
  uint32_t* eq_blk;          // [eq_blk_cap] slot of every block
  float4* eq_sorted;         // [eq_cap] {qx, qy, qz, query id = particle * M + reference position}
  double* eq_out;            // [eq_cap] by query id: the point coherence of the pair (0: no neighbour inside the gate)
  uint32_t eq_cap, eq_blk_cap;  // 0: the per-query kernel is used instead
  uint32_t* eq_tiles;        // [eq_tiles_cap][2 * 8192] per tile of particles: the LDS count table of k_ec_mark (cells, counts)
  uint32_t eq_tiles_cap;
  uint32_t* kld_table;       // KLD variant: open-addressing table of first occurrences, 2 x pow2(kld_max) entries
  int32_t* kld_bins;         // KLD variant: 6 ints per candidate
  uint32_t* host_stat;  // pinned host memory, device-visible: [0] last n_crop, [1] last octree depth (read by the
                        // host WITHOUT synchronising, to pick the builder for the next iteration: a wrong guess costs
                        // time, never correctness), [2] error flags of the last failed iteration, [3] error flags
                        // accumulated since the host last looked (checked and cleared at the host's sync points),
                        // [4] exact-NN pool demand, [5] ancestor table window sizes of the last build (pft_anc_window)
  int32_t* nn_idx;      // debug only
  float* nn_d2;
  // change detection (pft_change.hip): &PftChangeState::gate while pft_compute drives a handle whose detector has ever been
  // enabled, else null.  Gate 0 (changed_ == false): the builders and the likelihood return at once, the population
  // launch only renormalises the stored weights, the resample launches copy the population through
  const uint32_t* gate;
};

// per-handle state of the change detector (OctreePointCloudChangeDetector of ParticleFilterTracker), in HBM; apart from
// PftHeader, whose per-iteration fields the crop kernel clears
struct PftChangeState {
  double mn[3], mx[3];  // the detector octree's bounding box: never reset, grows over every crop tested
  int32_t depth;
  uint32_t defined;     // bounding_box_defined_
  uint32_t counter;     // change_counter_
  uint32_t gate;        // changed_
  uint32_t n_set[2];    // voxels of the two sets (packed 3 x 21-bit key + point count)
  uint32_t prev;        // the set of the previous test
  uint32_t n_calls;     // decisions made; ring[n_calls % PFT_CD_RING] is the next
  uint32_t ring[PFT_CD_RING][5];  // tested, changed, new voxels, new points, counter after
};
struct PftChangeBufs {  // one detector instance (by value into the kernel)
  PftChangeState* st;
  unsigned long long* set_key[2];
  uint32_t* set_cnt[2];
  unsigned long long* tab_key;  // [tab_cap] open-addressing table of the test (keys)
  uint32_t* tab_cnt;            // [tab_cap] points of the current crop | bit 31: voxel of the previous set
  unsigned long long* pt_key;   // [cap] packed key of every point of the crop
  uint32_t* mark;               // [cap] debug instance: 1 for a point of a counted new voxel (null in the tracker's)
  uint32_t cap, tab_cap;        // points (and voxels per set); table entries (a power of two >= 4 cap)
};
struct PftChangeArgs {
  double res;           // latched resolution
  uint32_t use, interval, min_points;
  uint32_t force;       // debug instance: test regardless of the counter, leave the counter alone
};
// the detector launch: counter bookkeeping, and at counter 0 with use != 0 the test of pts[0 .. *n_ptr (or n)) against the
// previous test.  Writes st->gate; a depth above 21 or too many growth steps raises error bit 5 in host_stat[2..3]
void pftk_change_detect(hipStream_t s, const PftChangeBufs& b, const float4* pts, const uint32_t* n_ptr, uint32_t n,
                        const PftChangeArgs& a, uint32_t* host_stat);

// ---- device-side hand-off from an input filter to a tracker (pft_set_input_from_filter) ----
// One link per tracker and filter, shared by the two handles; the handle that finds the other one gone frees it.
struct PftBorrow {
  hipEvent_t ev = nullptr;   // recorded by the tracker right behind the first crop of a frame: the only launch that reads the
                             // filter's output and count word
  bool recorded = false;     // ev has been recorded at least once
  bool armed = false;        // handed over, that crop not enqueued yet
  bool valid = false;        // cleared when the filter overwrites or frees its output while the link is armed
  bool tracker_alive = true, filter_alive = true;
};
struct pft_filter;
struct PftFilterView {
  const pft_point_xyzrgba* out;  // the output cloud in HBM
  const uint32_t* n_out_dev;     // the device word that holds its count
  size_t n_in;                   // points the apply ran over: the count can never exceed it
  int device_id;
  hipEvent_t done;               // recorded on the filter's stream behind the apply
};
// pft_filters.hip: PFT_ERR_STATE before the first apply
int pftf_view(pft_filter* f, PftFilterView* v);
void pftf_attach(pft_filter* f, PftBorrow* b);
// ---- the depth entrance of an input filter (pft_depth.hip; include/pft_filters.h) ----
// The device copies of the two images and the pinned slots hang on the filter handle, which frees them with pftd_destroy
// (its stream drained).  pft_depth.hip reaches the handle through these calls of pft_filters.hip only:
struct PftDepthState;
void pftd_destroy(PftDepthState* s);
struct PftFilterAccess {
  hipStream_t stream;
  int device_id;
  PftDepthState** depth;  // the handle's slot for the state (null until the first depth call)
  std::string& err;      // the handle's error text: PFT_HIPCHK(&access, call) works as on a handle
};
PftFilterAccess pftf_access(pft_filter* f);
// the front half of an apply over n > 0 records the caller is about to write into the handle's own input buffer: the
// capacity, the borrowed outputs settled.  *d_in: that buffer
int pftf_begin_own_input(pft_filter* f, size_t n, pft_point_xyzrgba** d_in);
// the back half: the pipeline over the own input buffer, then the wait for the counts if asked for
int pftf_run_own_input(pft_filter* f, size_t n, bool wait);

// ---- model preparation (pft_model.hip) and its hand-off to a tracker (pft_set_object_from_model) ----
// pft_segment.hip: removeZeroPoints (RULE zero, no transform) as the ordered compaction of the segmenter.  keep_idx[0 ..
// *n_keep) = the kept input indices, ascending, keep_xyz their {x, y, z, 1}; xyz [n], flag [n], tile [ceil(n / 1024)] scratch
void pftk_remove_zero_points(hipStream_t s, const pft_point_xyzrgba* in, uint32_t n, float4* xyz, uint8_t* flag,
                             uint32_t* tile, uint32_t* keep_idx, float4* keep_xyz, uint32_t* n_keep);
// pft_segment.hip: the one-workgroup exclusive scan of the tile / scan / emit compaction (1024-element tiles), in place over
// tile[0 .. ntiles); the total goes to *out
void pftk_tile_scan(hipStream_t s, uint32_t* tile, uint32_t ntiles, uint32_t* out);
struct pft_segment;
int pftsg_device_id(const pft_segment* s);
struct pft_model;
struct PftModelView {
  const pft_point_xyzrgba* recentred;  // transed_ref, in HBM
  size_t n_recentred;
  const pft_point_xyzrgba* reference;  // transed_ref_downsampled, in HBM
  size_t n_reference;
  float trans[16];
  uint32_t first_nonfinite;            // first re-centred point with a non-finite coordinate, 0xFFFFFFFF: none
  int device_id;
};
// PFT_ERR_STATE unless the last prepare succeeded
int pftm_view(const pft_model* m, PftModelView* v);

// The result-neutral path switches (A/B timing and cross-checks; README "Environment switches").  pft_create reads them
// once, with pft_read_switches, and keeps them on the handle: the launchers take the decisions as plain arguments.
enum class PftExactPath { sorted, per_query, shells };  // exact-NN search: cell-sorted lists, lists per query, shells only
struct PftSwitches {
  bool graph;             // PFT_GRAPH=1: steady-state frames replayed as one hipGraph (handles with their own stream)
  int builder;            // PFT_FORCE_BUILDER: 0 by the last crop size, 1 single workgroup ("single"), 2 sorted ("sorted")
  int leaf_indirect;      // PFT_LEAF_INDIRECT: -1 by the launch size, 0 leaf records copied, 1 followed through leaf_order
  bool aabb_full;         // PFT_AABB_FULL: the box over every reference point instead of the hull shell
  bool split_resample;    // PFT_SPLIT_RESAMPLE or PFT_RESAMPLE_ONE_LANE: resample and box as separate launches
  bool resample_one_lane; // PFT_RESAMPLE_ONE_LANE: the one-lane-per-particle resample kernel instead of the four-lane one
  bool crop_two_pass;     // PFT_CROP_TWO_PASS: the crop as a count + a scatter launch instead of the one-pass kernel
  bool generic_descent;   // PFT_GENERIC_DESCENT=1: every octree level by the exact 8-way selection
  bool ancestor_table;    // PFT_ANCESTOR_TABLE (default 1): the fast descent starts from the ancestor table
  int anc_up_force;       // PFT_ANC_UP_FORCE=0|1|2: the table's level D - 1 / D - 2 or none, whatever the last window's size (-1: by it)
  PftExactPath exact_path;  // PFT_EXACT_SHELLS_ONLY, else PFT_EXACT_PER_QUERY, else the cell-sorted search
  int ablate;             // diagnostic build only: PFT_ABLATE, or pft_debug_set_ablate (results are wrong while set)
  bool skip_octree;       // diagnostic build only: PFT_DEBUG_SKIP_OCTREE (results are wrong while set)
};
PftSwitches pft_read_switches();

// launchers
// the object report (pft_report.hip): one workgroup reads hdr->rep, writes the tracked cloud and the report
void pftk_report(hipStream_t s, const pft_point_xyzrgba* pts, uint32_t n, const PftHeader* hdr, int sum_order,
                 pft_point_xyzrgba* tracked, pft_object_report* out);
// the match statistics of the result pose (pft_match.hip): one workgroup reads hdr->rep and the tree of the last iteration
// (d.gate: the change detector's gate word or null), writes the statistics, the lost rule's state and the pairs
void pftk_match(hipStream_t s, const PftParams& p, const PftDev& d, double min_ratio, uint32_t lost_after,
                pft_match_stats* out, int32_t* input_idx, float* sq_dist);
// population statistics (pft_spread.hip): two launches over d.part_all[0 .. n) -- n = n_max, or a KLD handle's device-side
// count (d.p_active), never above n_max -- around d.hdr->rep.  part [29][blocks], part_zero / part_wmax / part_imax [blocks]
// with blocks = pftk_spread_blocks(n_max): the per-block roots, owned by the feature.  Writes the result block and the
// spread rule's state; a failed last iteration (PftHeader::error) only clears `evaluated`
uint32_t pftk_spread_blocks(uint32_t n_max);
void pftk_spread(hipStream_t s, const PftDev& d, uint32_t n_max, double* part, uint32_t* part_zero, float* part_wmax,
                 uint32_t* part_imax, double max_pos_sigma, double min_n_eff, uint32_t after, pft_population_stats* out);
// visibility of the reference cloud at a pose (pft_visibility.hip)
struct PftVisCam {  // pft_visibility_config as the kernels take it (the margins rounded to float once)
  int W, H, splat;
  float fx, fy, cx, cy, z_near, occlusion_margin, self_margin;
};
struct PftVisArgs {
  float m[12];               // the explicit matrix (use_rep == 0)
  uint32_t use_rep;          // T = pose_to_matrix(PftHeader::rep); a failed last iteration is then not evaluated
  uint32_t match_enqueued;   // use_rep, and a pft_match for this reference cloud was enqueued after the last pft_compute
  uint32_t lost_after;
  double min_visible_ratio, min_ratio;
};
struct PftVisCtl {  // written by k_vis_model, read by the two launches behind it
  float T[12];
  uint32_t run;              // 0: nothing is evaluated
  int u0, v0, u1, v1;        // pixel rectangle of the in-view model points
  uint32_t zmax;             // bits of their largest z
  uint32_t n_in_view;
};
struct PftVisBufs {
  PftVisCtl* ctl;
  uint32_t* zbuf;            // [2 W H] depth bits: the frame's image, then the model's
  uint2* q;                  // [M] stored order: {bits of the moved z, pixel or 0xffffffff}
  uint8_t* state;            // [M] the caller's order, as scene_gap and self_gap
  float *scene_gap, *self_gap;
  pft_visibility_stats* out;
};
PftVisCam pftk_visibility_cam(const pft_visibility_config& c);
void pftk_visibility_clear(hipStream_t s, const PftVisBufs& b, uint32_t M);
// fill, model, frame (pts: N records of stride4 x 16 bytes, or *n_dev of them), classify; match / match_idx: the block and
// the pairs of pft_match (read only with a.match_enqueued)
void pftk_visibility(hipStream_t s, const PftDev& d, uint32_t M, const float4* pts, uint32_t stride4, uint32_t N,
                     const uint32_t* n_dev, const PftVisCam& cam, const PftVisArgs& a, const PftVisBufs& b,
                     const pft_match_stats* match, const int32_t* match_idx, int num_cus);
// the view-dependent reference (pft_view.hip)
struct PftViewArgs {
  float m[12];               // the explicit matrix (use_rep == 0)
  uint32_t use_rep;          // T = pose_to_matrix(PftHeader::rep); a failed last iteration is then not evaluated
  uint32_t K;                // max_points (0: no limit)
};
struct PftViewCtl {  // written by k_view_fill, read by the launches behind it
  float T[12];
  uint32_t run;              // 0: nothing is evaluated
};
struct PftViewBufs {
  PftViewCtl* ctl;
  uint32_t* zbuf;            // [W H] depth bits of the moved model
  uint2* q;                  // [N] {bits of the moved z, pixel | 0xffffffff out of view | 0xfffffffe non-finite record}
  uint8_t* state;            // [N]
  float* gap;                // [N]
  uint4* tile_cnt;           // [tiles of 256 records] {visible, self-occluded, out of view, non-finite}
  uint32_t* tile_base;       // [tiles] visible records before the tile
  uint32_t* kept_idx;        // [n_kept]
  float4* cloud;             // [2 n_kept] the kept records
  pft_view_stats* out;
};
// fill, project, classify, scan, compact over the N records at `model` (pairs of 16 bytes); grid: the workgroups of every
// pass but the one-workgroup scan, 0 = sized from N and num_cus
void pftk_view(hipStream_t s, const PftHeader* hdr, const float4* model, uint32_t N, const PftVisCam& cam,
               const PftViewArgs& a, const PftViewBufs& b, uint32_t grid, int num_cus);
// re-acquisition (pft_reacquire.hip): the orientation lattice, the per-candidate score arrays (K each, owned by the feature)
struct PftRqLattice {
  uint32_t n[3];             // roll, pitch, yaw steps (>= 1)
  float base[3], span[3];
};
struct PftRqScores {
  uint32_t *n_inliers, *n_matched;
  double *coherence, *sum_sq_dist, *inlier_sq_dist;
};
// compute3DCentroid of n_clusters runs of points (first / count per cluster, device arrays) -> centres [3 * n_clusters]
void pftk_reacquire_centroids(hipStream_t s, const pft_point_xyzrgba* pts, const uint32_t* first, const uint32_t* count,
                              uint32_t n_clusters, float* centres);
// candidate k = ((c n_roll + ir) n_pitch + ip) n_yaw + iy -> part [K], mats [12 K]
void pftk_reacquire_candidates(hipStream_t s, const float* centres, uint32_t K, const PftRqLattice& lat, pft_particle* part,
                               float* mats);
// one workgroup per candidate d.mats[k] against the tree of the last build; reads no particle, no partial box
void pftk_reacquire_score(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t K, double inlier_d2,
                          const PftRqScores& out);
// one workgroup: the best candidate (d.part_cur / d.mats are the candidates') and the result block; mirrors
// PftHeader::error into the pinned status block
void pftk_reacquire_select(hipStream_t s, const PftParams& p, const PftDev& d, const PftRqScores& sc, uint32_t K,
                           uint32_t n_centres, uint32_t per_centre, double accept_ratio, pft_reacquire_result* out);
// refinement of a pose (pft_refine.hip): the control block (state, current T, the loop's words) lives in HBM and is defined
// there; part [17][g_cap] and part_n [2 g_cap] hold the per-block roots and counts, g_cap = pftk_refine_blocks(M); trace has
// room for PFT_REFINE_MAX_ITERATIONS + 1 entries.  All owned by the feature
struct PftRefineCtl;
struct PftRefineDev {
  PftRefineCtl* ctl;
  double* part;
  uint32_t* part_n;
  uint32_t g_cap;
  pft_refine_result* result;
  pft_refine_trace_entry* trace;
};
struct PftRefineArgs {
  float start[12];
  uint32_t use_rep;     // the start is pose_to_matrix(PftHeader::rep)
  uint32_t max_iterations, min_pairs;
  double pair2, inl2, margin, trans_eps2, rot_eps2;
};
size_t pftk_refine_ctl_bytes();
uint32_t pftk_refine_blocks(uint32_t M);
// one lane: the start, its state, the eight shifted matrices (mats [8 x 12]) the crop box is taken over
void pftk_refine_init(hipStream_t s, const PftRefineArgs& a, const PftRefineDev& r, const PftHeader* hdr, float* mats);
// max_iterations + 1 passes (k_refine_pairs + k_refine_step each) against the tree of the last build
void pftk_refine_passes(hipStream_t s, const PftParams& p, const PftDev& d, const PftRefineDev& r, const PftRefineArgs& a);
void pftk_pack_reference(hipStream_t s, const pft_point_xyzrgba* d_pts, uint32_t n, int argorder, float4* xyz,
                         float4* hsv);
void pftk_pack_input(hipStream_t s, const pft_point_xyzrgba* d_pts, uint32_t n, float4* out,
                     const uint32_t* n_dev = nullptr);
void pftk_init_particles(hipStream_t s, const PftParams& p, pft_particle rep, pft_particle* out, float* mats,
                         PftHeader* hdr);
void pftk_resample(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t epoch, pft_particle* out, bool one_lane);
void pftk_bbox_final(hipStream_t s, const PftDev& d);
uint32_t pftk_resample_box(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t epoch, pft_particle* out);
// debug: resample from an explicit (a, q) table instead of the prefix-sum form
void pftk_resample_table(hipStream_t s, const PftParams& p, const pft_particle* old, const int32_t* a,
                         const double* q, const PftHeader* hdr, uint32_t epoch, pft_particle* out);
void pftk_pose_to_matrix(hipStream_t s, const pft_particle* p, uint32_t n, float* mats);
void pftk_aabb(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t n_particles, bool finalize);
void pft_aabb_support_subset(const pft_point_xyzrgba* pts, size_t n, std::vector<uint32_t>& keep);  // pft_hull.hip (host)
// NearestPairPointCloudCoherence mode: uniform grid over the cropped cloud, then the likelihood with the true NN
void pftk_exact_grid(hipStream_t s, const PftParams& p, const PftDev& d);
void pftk_likelihood_exact(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t n_particles, bool debug_nn,
                           int num_cus, PftExactPath path);
// KLD variant: draws up to p.kld_max candidates from d.part_all[0 .. p_active) (alias prefix form, or the explicit
// table a/q when given), keeps the prefix the KL bound asks for, writes particles + matrices and the new p_active
void pftk_resample_kld(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t epoch, pft_particle* out,
                       const int32_t* table_a, const double* table_q, int32_t* bins_out);
// epoch: a value that differs from the handle's previous crop launch (non-zero); tags the per-workgroup counts of the one-pass crop
// raw: the input in PCL's 32-byte layout when its 16-byte records have not been formed yet (first crop of a frame), else null
// n_src (with d.n_dev, first crop of a frame): the device word the live input count is read from; the crop latches
// min(count, d.N) into d.n_dev for the frame's later crops and raises bit 6 (count above d.N) or bit 7 (count zero) in
// the pinned status block.  Null: the count is d.n_dev's (or, without one, d.N)
void pftk_crop(hipStream_t s, const PftParams& p, const PftDev& d, bool bbox_from_partials, uint32_t epoch,
               const pft_point_xyzrgba* raw, bool two_pass, const uint32_t* n_src = nullptr);
// the single-workgroup builder; indirect: no leaf_pts copies, the likelihood kernel follows leaf_order (its INDIRECT form)
// anc_up: the ancestor table's level for this tree, depth - anc_up (1 or 2; 0: none), where its window fits
void pftk_octree(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t expected_points, bool indirect, int anc_up);
// no-op launch unless the sorted builder flagged "radix passes too few" (error bit 3): then the single-workgroup build
void pftk_octree_rescue(hipStream_t s, const PftParams& p, const PftDev& d);
struct SortBufs {
  unsigned long long* keys[2];
  uint32_t* vals[2];
  uint32_t* hist;      // [256][ntiles]
  uint32_t* tile_cnt;  // [ntiles][PFT_MAX_DEPTH + 2]
  float* tile_box;     // [ntiles][6] AABB of each 1024-point tile of the cropped cloud
  uint32_t ntiles;
};
// many-workgroup builder for large cropped clouds (pft_octree_sorted.hip); npass = 4 (depth <= 10) or 8
void pftk_octree_sorted(hipStream_t s, const PftParams& p, const PftDev& d, const SortBufs& sb, uint32_t n_pad,
                        int npass);
// flags (k_likelihood's argument): bit 0 fast descent allowed, bit 1 ancestor table allowed, bits 8+ the stage ablation
// mask of the diagnostic build; anc_up: what the tree's builder was asked for -- picks the product instance, whose ANC_UP
// is returned
int pftk_likelihood(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t n_particles, bool debug_nn,
                    int num_cus, bool leaf_indirect, int flags, int anc_up);
// shard (nullable): sharded handles -- the particles with their raw weights also go into the all-gather's send buffer
void pftk_finalize_raw(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t n_particles,
                       float* raw_out /*nullable*/, pft_particle* shard /*nullable*/);
// normalise + update + alias prefix form over part_all[0..n) in one launch, in the handle's summation order; from_partials != 0: the raw weights are
// first formed from the likelihood partial sums (single-GPU path: fuses k_finalize_raw)
void pftk_population(hipStream_t s, const PftParams& p, const PftDev& d, uint32_t n, int from_partials,
                     int do_normalize, int do_mean, int do_alias);
// debug: materialise the (a, q) table from the prefix-sum form
void pftk_alias_materialize(hipStream_t s, const PftDev& d, uint32_t n, int32_t* a, double* q);
int pftk_max_lds_bytes();
int pftk_cur_device();  // current HIP device ordinal, clamped to [0, PFT_MAX_DEVICES)
// stable LSD radix sort (pft_filters.hip) of (key, val) pairs by the low `bits` bits of the key, 8 bits per pass;
// key[cur] / val[cur] hold the input, the return value is the index of the buffers that hold the output.
// hist: >= 256 * ceil(n / 1024) + 256 words.
int pftk_radix_sort_pairs(hipStream_t s, uint32_t* key[2], uint32_t* val[2], uint32_t n, int bits, uint32_t* hist);

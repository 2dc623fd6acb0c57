// The filter behind the C ABI (include/parakeet_slam.h): struct pk_filter and what every part of the host layer needs to work on
// it.  Private to the pk_api*.hip files, which divide the ABI between them:
//   pk_api.hip          lifecycle, transfers, motion, resample, the step, new-landmark bookkeeping, options, timing, the probe
//   pk_api_observe.hip  the observe pipeline: routing, association, the one-pass stages, the colour table's host side
//   pk_api_scan.hip     how a scan gets onto the device: the staging ring, the per-scan blocks, the scan-taking calls' argument checks
//   pk_api_shard.hip    the multi-GPU protocol: host-side, device-resident and balanced
//   pk_api_path.hip     the path estimate: the ring of resampled generations, its transfers, trace and summaries, the trunk of
//                       settled rows, the best particle
//   pk_api_adaptive.hip adaptive resampling: the gated resample and step, the weight sums, the weighted pose summary
//   pk_api_mapmatch.hip the discovered landmarks: the matched moments and the finished estimate
//   pk_api_propose.hip  the measurement-informed proposal: pk_propose, pk_propose_odom, pk_proposal_download, its modes
//                       (pk_proposal_ranges, pk_proposal_grow)
//   pk_api_range.hip    range-bearing scans: pk_scan_ranges, what consumes the armed ranges, their refusals
//   pk_api_unique.hip   unique association: pk_assoc_unique, its counters, the pass behind the association, its refusals
// No kernel is defined or launched here: everything goes through the launch_* functions of pk_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "../../include/parakeet_slam.h"
#include "pk_devmem.hpp"
#include "pk_kernels.hpp"
#include "pk_pub_layout.hpp"
#include "pk_scan_block.hpp"

using namespace pk;

// the status `code`, with the message pk_last_error reports (one thread-local string, in pk_api.hip)
int fail(int code, const char* fmt, ...);

#define PK_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      (void)hipGetLastError();                                                               \
      return fail(e_ == hipErrorOutOfMemory ? PK_ERR_NOMEM : PK_ERR_HIP, "%s failed: %s (%s:%d)", #call, \
                  hipGetErrorString(e_), __FILE__, __LINE__);                                \
    }                                                                                        \
  } while (0)

// Kernel launches report configuration errors (too much dynamic LDS, bad grid) through the
// runtime's last-error slot, not through a return value: every entry point that enqueued kernels
// asks for it before it reports success.
#define PK_LAUNCH_CHECK(what)                                                                \
  do {                                                                                       \
    hipError_t e_ = hipGetLastError();                                                       \
    if (e_ != hipSuccess)                                                                    \
      return fail(PK_ERR_HIP, "%s: a kernel launch failed: %s", what, hipGetErrorString(e_)); \
  } while (0)

struct TimedSpan {
  int slot;
  hipEvent_t a, b;
};

// what the filter's memory registry (pk_devmem.hpp) allocates and frees with
struct HipRaw {
  int device_alloc(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return PK_OK;
    (void)hipGetLastError();
    return fail(PK_ERR_NOMEM, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
  }
  void device_free(void* p) { (void)hipFree(p); }
  int host_alloc(void** p, size_t bytes, unsigned flags) {
    hipError_t e = hipHostMalloc(p, bytes, flags);
    if (e == hipSuccess) return PK_OK;
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? PK_ERR_NOMEM : PK_ERR_HIP, "hipHostMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
  }
  void host_free(void* p) { (void)hipHostFree(p); }
};

// The kernels of one maximum-likelihood scan ("Routing": the table of kinds against their conditions).
// The observe's planner (pk_api_observe.hip) decides it once per scan; every stage of the observe follows it.
enum class ScanKind {
  Brute,         // k_assoc_brute + k_observe
  General,       // k_assoc_grid + k_observe
  HandoffFast,   // k_assoc_grid's hand-off + k_observe_fast
  HandoffSweep,  // ... + k_observe_sweep
  // the one-pass kinds: the association launches nothing, one kernel does gates + EKF, what it flags goes to the kernels above
  Fused,         // k_step_fused
  PubSmall,      // k_step_pub<1, 256>
  Regs,          // k_step_regs, no publish table
  PubRegs,       // k_step_pub<2, 512>, k_step_regs behind it for the scans it stands back from
  Pub,           // k_step_pub<2, 512> alone (pruned lists, growing maps)
  PubBig,        // k_step_pub_big, k_step_pub_duo in front of it with "pub_duo"
};
struct ScanPlan {
  ScanKind kind = ScanKind::Brute;
  int route = PK_ROUTE_ML_GENERAL;  // what pk_observe_route reports
  // the hand-off: slots per landmark, lists allocated (for every particle on the hand-off kinds, for the second-chance rows behind
  // k_step_regs / k_step_pub / k_step_pub_big), the second chance runs
  int slots = kFastSlots;
  bool lists = false;
  bool retry = false;
  // the reference particle's candidate lists: entries per list (0: none made), inverse lists and the publish table's layout
  // (k_cand_entries) for ecap entries, look-alikes beyond the underflow edge pruned
  int cand_slots = 0;
  bool publish = false;
  int ecap = 0;
  bool far = false;
  DuoLimits duo;            // PubBig: what k_step_pub_duo has room for (all zero: the instance is off)
  // a scan the kernel stands back from, with no stand-by kernel behind it, flags its particles for the fall-back kernels: inside
  // k_cand_entries when the launches cover every particle, else by a k_flag_range_if launch per range (3 us a step)
  bool flag_fold = false, flag_range = false;
  bool colour_table = false;  // Pub: the table-mode instance
  bool onepass() const { return kind >= ScanKind::Fused; }
  bool ranged() const { return kind >= ScanKind::Regs; }  // runs on particle ranges (pk_observe_staged_range)
};

// One uploaded maximum-likelihood scan and the kernels it gets (enqueue_association fills both)
struct AssocLaunch {
  ScanTables scan;
  ScanPlan plan;
};

// The ranges a consuming call took from the filter (ranges_take): rows [B][2] (range, variance; NaN range = none).  armed: ranges
// were named for this scan at all; any: some blob has one -- only then does the scan stage them and take the range kernels.
struct RangeScan {
  bool armed = false, any = false;
  std::vector<double> rv;
};

// What pk_set_option sets: every tuning knob with its default.  (Protocol state that an option name also reaches -- the loopback
// bounds of the sharded tests -- stays with the shard fields of pk_filter.)
struct Options {
  int assoc_kernel = 0;  // 0 = colour-grid kernel, 1 = brute-force reference kernel
  int assoc_dup = 1;     // grid kernel: use the 9x column-duplicated index list when it fits in LDS
  int fast_observe = 1;  // association hand-off + k_observe_fast (L <= 512) / k_observe_sweep; 2 = always the sweep kernel
  int timing_stride = 1; // a timing slot that is switched on (timing_mask) is bracketed every timing_stride-th time it comes up (sampling keeps the probe cheap)
  int upload_kernel = 1; // per-scan block: read from pinned host memory by a kernel (1) or hipMemcpyAsync (0)
  int fused_step = 1;    // L <= 512 and small scan tables: k_step_fused instead of hand-off + k_observe_fast
  int cand_lists = 1;    // k_step_regs: gates against the reference particle's candidate lists (k_candidates) instead of the grid walk
  int pub_step = 1;      // ... with the contested blobs settled by static publish / subscribe (k_step_pub) while the publish table fits LDS
  int pub_small = -1;    // L <= 512: k_step_pub<256 lanes> instead of k_step_fused -- 1 / 0, or -1 (default): where it is measured faster
                         // (kPubSmallAutoWork, pk_api_observe.hip)
  int pub_lean = 1;      // k_step_pub<2, 512>: the (wave, pair) groups of simple landmarks take the lean body (pub_lean_pair); 0: the usual one
  int far_prune = 1;             // look-alikes certainly beyond the underflow edge leave the candidate lists once per scan (0: as round 4)
  int duo_on = 0;        // "pub_duo" (measured, off: DESIGN.md section 4): 2 048 < L <= 5 120, scans whose publish table fits its share of a CU's LDS go to
                         // k_step_pub_duo -- 1: two 512-lane workgroups per CU (<= 128 VGPRs), 2: three 256-lane workgroups (<= 168) -- the others to k_step_pub_big
  int duo_park_limit = -1;  // >= 0: k_step_pub_duo's overflow area is treated as this small (tests: particles that need more go to the fall-back kernels)
  int pub_entry_limit = 0;  // > 0: the publish table is treated as this small (tests: scans whose table "does not fit" fall back to k_step_regs)
  int regs_step = 1;     // 512 < L <= 2048 and scan tables that fit LDS: k_step_regs (one pass, map in registers)
  int regs_retry = 1;    // k_step_regs: 1 = the particles it flags get a second chance (eight-slot hand-off + k_observe_sweep) before the general kernels
  int regs_warm = 1;     // k_step_regs: L2 warming of the next particle's slot: 0 none, 1 its mean rows (default), 2 the whole slot (measured slower)
  int split_reserve_cus = 16;  // CUs the first part of a split step leaves free for the all-to-all's kernels
  int colour_table_depth = 1024;  // option: levels of the table
  int colour_table_margin = -1;   // option: the host leaves the mode this many levels short of the table's end; -1: min(16, depth / 2); 0: never
  int colour_table = -1;          // option: -1 auto, 0 off, 1 as auto
  int map_sum_groups = 0;         // the map estimate's particle groups: 0 = map_sum_groups(P, Ls) (pk_kernels.hpp), else forced (tests: many particles per group, ragged last groups)
  int map_match_groups = 0;       // the discovered landmarks' particle groups: 0 = map_match_groups(P, rows), else forced (tests)
};

// One row per knob: the name a caller gives, the member, how the value is taken, the inclusive range, the refusal outside it.
enum class Take {
  Range,  // as given, inside [lo, hi]
  Flag,   // value != 0
  Tri,    // "pub_small": negative -> -1 (automatic), else value != 0
};
struct OptionRow {
  const char* name;
  int Options::*member;
  Take take;
  int64_t lo, hi;
  const char* refusal;
};
inline constexpr OptionRow kOptionTable[] = {
    {"assoc_kernel", &Options::assoc_kernel, Take::Range, 0, 1, "assoc_kernel: 0 (colour grid) or 1 (brute force)"},
    {"assoc_dup", &Options::assoc_dup, Take::Flag, 0, 0, nullptr},
    {"fast_observe", &Options::fast_observe, Take::Range, 0, 3,
     "fast_observe: 0 (general kernels), 1 (default), 2 (always the sweep kernel) or 3 (... with eight slots)"},
    {"timing_stride", &Options::timing_stride, Take::Range, 1, 1000000, "timing_stride: 1 .. 1000000"},
    {"upload_kernel", &Options::upload_kernel, Take::Flag, 0, 0, nullptr},
    {"fused_step", &Options::fused_step, Take::Flag, 0, 0, nullptr},
    {"cand_lists", &Options::cand_lists, Take::Flag, 0, 0, nullptr},
    {"pub_step", &Options::pub_step, Take::Flag, 0, 0, nullptr},
    {"pub_small", &Options::pub_small, Take::Tri, 0, 0, nullptr},
    {"far_prune", &Options::far_prune, Take::Flag, 0, 0, nullptr},
    {"pub_lean", &Options::pub_lean, Take::Flag, 0, 0, nullptr},
    {"pub_duo", &Options::duo_on, Take::Range, 0, 2,
     "pub_duo: 0 (off), 1 (two 512-lane workgroups per CU) or 2 (three 256-lane workgroups per CU)"},
    {"pub_duo_park_limit", &Options::duo_park_limit, Take::Range, -1, 65535, "pub_duo_park_limit: -1 (what LDS holds) .. 65535"},
    {"pub_entry_limit", &Options::pub_entry_limit, Take::Range, 0, 65534, "pub_entry_limit: 0 (what LDS holds) .. 65534"},
    {"regs_step", &Options::regs_step, Take::Flag, 0, 0, nullptr},
    {"regs_retry", &Options::regs_retry, Take::Range, 0, 1, "regs_retry: 0 or 1"},
    {"regs_warm", &Options::regs_warm, Take::Range, 0, 2, "regs_warm: 0 (off), 1 (mean rows) or 2 (whole slot)"},
    {"split_reserve_cus", &Options::split_reserve_cus, Take::Range, 0, 128, "split_reserve_cus: 0..128"},
    // (takes effect when the table is next built: at the first table-mode scan behind a pk_upload_map)
    {"colour_table_depth", &Options::colour_table_depth, Take::Range, 8, 32768,
     "colour_table_depth: 8 .. 32768 levels (the table stays below 4 GB: 32-bit offsets)"},
    {"colour_table_margin", &Options::colour_table_margin, Take::Range, -1, 32768,
     "colour_table_margin: -1 (auto), 0 (the host never leaves the mode for the table's end) or levels"},
    {"map_sum_groups", &Options::map_sum_groups, Take::Range, 0, 1024, "map_sum_groups: 0 (chosen from the shape) .. 1024"},
    {"map_match_groups", &Options::map_match_groups, Take::Range, 0, 1024, "map_match_groups: 0 (chosen from the shape) .. 1024"},
    // "colour_table" itself is taken by pk_set_option in code: switching it off in mid-run gives the slots their colour rows back
};

struct pk_filter {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  DeviceState d{};
  NoiseD qt{0.1, 0.1, 0.0, 0.0, 0.1, 0.0, 0.1};
  double qt16[16] = {0.1, 0, 0, 0, 0, 0.1, 0, 0, 0, 0, 0.1, 0, 0, 0, 0, 0.1};  // the same, dense (prkt_core_v2.py:50-53)
  int model = PK_MODEL_REFERENCE;  // pk_set_measurement_model: what the observes compute (pk_math.hpp: kModelReference / kModelBearing)
  bool qt_dense = false;   // Qt couples bearing and colour or is not symmetric: only the dense kernels take it
  bool dense = false;      // maps in the dense 30-row layout (pk_layout.hpp): the general dense kernels run the observes
  std::vector<double> dense_staged;  // pk_stage_scan in dense mode: the blobs, kept on the host
  bool map_loaded = false;
  bool src_identity = true;
  int64_t nblocks = 0;  // weight-scan blocks
  DevMem<HipRaw> mem;   // owns every device and pinned block below and in d, fh, grow, bal (dev_alloc / dev_reserve / host_alloc)
  // workspaces
  double* z_dev = nullptr;        // P x 3
  unsigned char* scan_dev = nullptr;  // per-scan block (pk_scan_block.hpp)
  size_t scan_cap = 0;
  bool gmax_fused = false;  // ctl holds the max of the current log-weights (set by observe)
  int32_t* ids_dev = nullptr;     // P x B
  int64_t ids_cap = 0;
  double* g_totals = nullptr;   // sharded resample: every shard's block totals
  double* g_offsets = nullptr;
  int64_t gblocks_cap = 0;
  double* gl_clocal = nullptr;  // global-scan mode of the sharded resample: block-local scans of ALL particles' weights
  double* gl_totals = nullptr;
  double* gl_offsets = nullptr;
  int64_t gl_cap = 0;
  int64_t* hi_dev = nullptr;    // P + 1
  unsigned* plan_ticket = nullptr;  // workgroup counter of the one-launch shard plan
  int64_t* idx_dev = nullptr;   // P
  int64_t* srcs_dev = nullptr;  // P
  int64_t* rlohi_dev = nullptr; // (lo, hi) of the received records
  int64_t rlohi_cap = 0;
  BalancedBuffers bal{};        // balanced placement of the sharded filter: the plan's tables (every rank holds the whole plan)
  int64_t bal_m = -1;           // slots this rank's own children fill in the plan that is being carried out (-1: none)
  int64_t bal_loop_keep = -1;   // "balanced_loopback_keep" (debug, one-rank tests of the exchange): the next balanced adoption fills only the
                                // slots [0, keep) with this rank's own children; the slots [keep, P) come from records -- which the caller
                                // packs with pk_shard_pack_balanced_loop_dev and sends through the all-to-all to itself
  int64_t loop_lo = INT64_MIN, loop_hi = INT64_MAX;  // "split_loopback_lo/hi" (debug): local slots outside come from records
  Options opt;                  // the tuning knobs (pk_set_option)
  // host half of an ML scan upload done ahead of time (pk_stage_scan): tables built in a staging slot
  struct Staged {
    bool valid = false;
    int B = 0;
    unsigned char* st = nullptr;
    int slot = 0;
    BlobGrid g{};
    int n9 = 0;
    bool use_grid = false;
    MlScanLayout lay{};  // where everything lies in st (pk_scan_block.hpp); lay.upload_bytes: what the device needs of it
    bool uploaded = false;  // pk_step sent the block to the device together with the motion kernel
    bool with_ranges = false;  // the scan was staged with ranges named for it (pk_scan_ranges) ...
    bool ranged = false;       // ... of which at least one is finite: 32 B bytes of range rows lie behind the block (lay.rng)
  } staged;
  // pk_scan_ranges: the ranges of the next scan, on the host until a call that takes blobs consumes them (pk_api_range.hip)
  struct Ranges {
    bool armed = false, any = false;
    int32_t B = 0;
    std::vector<double> rv;  // [B][2] range, variance
  } rng;
  int route = PK_ROUTE_NONE;  // kernels used by the last observe
  unsigned* bcnt_dev = nullptr;  // [bcand_cap] entries of the blobs' inverse candidate lists
  uint4* brec_dev = nullptr;     // [bcand_cap] the lists
  int64_t bcand_cap = 0;
  uint4* cand_dev = nullptr;  // [Lp + kCandSpare][3] candidate records (two or three uint4 per landmark in use)
  uint4* erec_dev = nullptr;     // [Lp] publish entries of every landmark's candidates (k_cand_entries)
  uint4* erec_dev2 = nullptr;    // [Lp][2] the same for sixteen-entry lists (k_step_pub_big)
  unsigned* binfo_dev = nullptr; // [bcand_cap] per blob: first entry | contenders << 16
  unsigned char* npass_dev = nullptr; // [Lp + kCandSpare] per landmark: blobs inside the reference particle's own gates (k_candidates)
  unsigned* unm_dev = nullptr;   // growing maps on the publish / subscribe routes: [P][unm_words] every particle's unmatched blobs, bits in scan order
  int unm_words = 0;
  int64_t unm_cap = 0;
  bool grow_bits = false;        // the last observe's one-pass kernel left those rows (k_new_landmarks reads them where the particle was not handed on)
  uint4* prim_dev = nullptr;     // the two-pass kernels' primary-blob table: every landmark's first candidate in landmark order (prim_table_uint4; k_cand_entries)
  float4* gate4_dev = nullptr;   // [bcand_cap] every blob's bearing and colour as float: k_step_pub_big's first look (k_cand_entries)
  uint4* far_dev = nullptr;      // [Lp + kCandSpare][3] per landmark: the bound its list was pruned with | its far list (k_candidates, pk_pub_math.hpp)
  unsigned* glist_dev = nullptr; // [bcand_cap + 1 + 256] the same for the blobs several landmarks list, compacted; then their number; then the octet orders of k_step_pub (128 u16) and k_step_pub_big (384 u16)
  // a split observe in progress (pk_observe_staged_range): what the first call set up for the later ones
  struct Split {
    bool active = false;
    AssocLaunch al;
    PubTables pub;
    bool reset = false;
  } split;
  // The colour table (pk_colour.hpp): while every map descends from one pk_upload_map the colour block of a landmark is
  // a function of (landmark, update count), and k_step_pub's 512-lane instances take it from ct_tab instead of streaming six rows per
  // landmark in and out of every slot.  The slots' colour rows go stale then (colour_rows_valid) and are written back from the table
  // whenever anything else wants them (ensure_colour_rows).
  bool ct_eligible = false;       // the maps came from pk_upload_map and nothing has ended the mode since
  bool ct_updated = false;        // some landmark may be off level 0: an observe has run since that upload (pk_set_measurement_noise clears
                                  // it again where ct_maps_untouched finds every count of the live buffer at 0 still)
  bool ct_sharded = false;        // a shard / pack / adopt call was made on this filter: never
  bool ct_built = false;          // ct_tab holds the levels of ct_base under ct_qt
  bool ct_engaged = false;        // the last observe did, and nothing has ended the mode since
  bool colour_rows_valid = true;
  double* ct_base = nullptr;      // [6][Lp] the uploaded colour rows
  double* ct_tab = nullptr;       // [ct_depth][6][Lp]
  int ct_depth = 0;
  NoiseD ct_qt{};
  unsigned* ct_max_dev = nullptr; // word 0: the highest level a table-mode kernel has read since the upload; word 1: ct_maps_untouched's
                                  // flag (some count of the live buffer is not 0); words 2, 3 free
  unsigned* ct_seen = nullptr;    // pinned host words.  0: that figure, copied behind every table-mode scan (the last finished scan's, or the
                                  // one before); 1: ct_maps_untouched's flag, read behind a synchronisation
  int64_t ct_scans = 0, ct_whole = 0;  // scans taken in the mode, whole-buffer materialisations
  bool adopt_local_done = false;  // pk_shard_adopt_local_dev made the new generation current; pk_shard_adopt_remote_dev may fill it
  int pub_ecap = 0;       // k_step_pub was prepared for the current scan with this many publish entries (0: not prepared)
  uint4* sweep_results = nullptr;  // k_observe_sweep: per-workgroup result lists
  size_t sweep_cap = 0;
  unsigned* retry_seen = nullptr;  // pinned host word: second-chance rows the last scan WANTED (copied behind every second chance)
  int64_t retry_rows_min = 0;      // what retry_rows() grows to when a scan wanted more rows than there were
  FastHandoff fh{};      // device buffers of the hand-off
  int64_t fh_cap_l = 0, fh_cap_b = 0;
  // pinned host staging ring for the per-scan uploads (blobs, ray directions, chains):
  // lets pk_observe/pk_step return without synchronising the stream
  static constexpr int kRing = 8;
  unsigned char* stage[kRing] = {nullptr};
  hipEvent_t stage_done[kRing] = {nullptr};
  // which enqueued upload last read each slot, and up to which upload each slot's event covers
  // (an event is recorded behind every 4th upload only; a slot whose covering record never came --
  // its scan was staged and then discarded -- gets one when the slot is next handed out)
  uint64_t upload_seq = 0;
  uint64_t slot_seq[kRing] = {0};
  uint64_t event_seq[kRing] = {0};
  size_t stage_cap = 0;
  int stage_next = 0;
  double* partial = nullptr;  // 4 * 1024
  double* gmax = nullptr;
  double* clocal = nullptr;   // P
  double* totals = nullptr;   // nblocks
  double* offsets = nullptr;  // nblocks
  double* sum = nullptr;
  double* out4 = nullptr;
  double* pose_part = nullptr;   // [motion_pose_blocks(P)][4]: per-block sums of x, y, sin h, cos h the last whole-filter motion launch left
  bool pose_part_ok = false;     // ... and nothing has touched the poses since
  // the map estimate (pk_map_moments / pk_map_summary): nothing until the first call
  double* ms_part = nullptr;     // [groups][kMapSums][tiles x kMapSumLanes] k_map_partials' sums
  double* ms_res = nullptr;      // the handle's own maximum log-weight (2 words) | [kMapSumMaxGroups][2] the groups' weight sums | [2 + 30 L] the moments
  size_t ms_cap = 0;             // doubles of ms_part
  // the discovered landmarks (pk_map_match_moments / pk_map_discovered; pk_api_mapmatch.hip): nothing until the first call
  double* mm_ref = nullptr;      // [mm_rows][5] the reference features
  int32_t* mm_refi = nullptr;    // [4 + 2 mm_rows] launch_match_reference's integers
  double* mm_res = nullptr;      // a maximum log-weight (2 words) | [kMatchMaxGroups][2] the groups' weight sums | k_match_finish's result
  size_t mm_rows = 0;
  double* mm_part = nullptr;     // k_match_partials' sums
  size_t mm_part_cap = 0;        // doubles of mm_part
  int32_t* mm_match = nullptr;   // [P][n_ref] the match table, for the calls that ask for it
  size_t mm_match_cap = 0;
  // the path estimate (pk_path_enable; pk_api_path.hip): the ring, and pk_path_trace's / pk_path_summary's scratch -- nothing until first asked for
  PathRing path{};
  int64_t* pt_idx = nullptr;     // [pt_cap] the particles of one pk_path_trace chunk
  double* pt_out = nullptr;      // [pt_cap][rows][3] their paths
  int64_t pt_cap = 0, pt_out_cap = 0;
  unsigned* ps_cnt = nullptr;    // [3][P] descendant counts of three consecutive rows
  double* ps_ref = nullptr;      // [ps_rows][3] particle 0's lineage
  double* ps_part = nullptr;     // [ps_rows][path_blocks(P)][kPathSums]
  double* ps_res = nullptr;      // [ps_rows][kPathSums]
  int64_t ps_rows = 0;
  // pk_path_summary_weighted's scratch (nothing until it is first called; path_release gives it back with the ring)
  int32_t* pw_idx = nullptr;     // [P] every current particle's lineage index in the row being reduced
  double* pw_wgt = nullptr;      // [P] its weight
  double* pw_ref = nullptr;      // [pw_rows][3] particle 0's lineage
  double* pw_part = nullptr;     // [pw_rows][path_blocks(P)][kPathSums]
  double* pw_res = nullptr;      // [pw_rows][kPathWRes], then the call's own maximum log-weight (1 word)
  int64_t pw_rows = 0;
  // the trunk (pk_path_trunk_enable): the settled rows; settling works in pk_path_summary_weighted's scratch, which
  // pk_path_trunk_enable reserves for the whole ring, so that no step allocates.  The rows start at max(4 batch, 1024) and grow by
  // doubling -- allocate, device-to-device copy, free -- which is the ONLY synchronisation a settling step can ever meet.
  PathTrunk trunk{};
  // adaptive resampling and the weighted pose summary (pk_api_adaptive.hip): nothing until one of its entry points is first called
  double* ad_s2 = nullptr;          // [nblocks] sum w^2 of every scan block
  double* ad_words = nullptr;       // [kAdWords] the scan's shift | the plan beyond kAncestorsScanMaxBlocks blocks | a maximum log-weight | the pose summary
  double* ad_part = nullptr;        // [path_blocks(P)][kPathSums] k_pose_moments' partials
  GateOutcome* ad_out = nullptr;    // what the last gated call decided, and the counters since pk_create
  int64_t ad_calls = 0;             // gated calls enqueued (pk_resample_stats: 0 -> nothing to report)
  GrowState grow{};                 // section 8(f4) on the device (pk_grow_enable): per-particle new-landmark bookkeeping
  GrowInit grow_init{};             // pk_grow_init: where and how surely the bookkeeping places a new feature (no per-particle state)
  bool grow_on = false;
  bool grow_ranges = false;         // pk_grow_ranges: a ranged scan is taken, and one ranged sighting places a new feature (no per-particle state)
  RetireState retire{};            // pk_grow_retire (pk_api_retire.hip): the clocks of the retirement rule -- nothing until it is switched on
  RetireView view{};               // pk_grow_view (pk_api_retire.hip): the field of view of that rule -- off, and 32 bytes of counters once asked for
  // the measurement-informed proposal (pk_propose / pk_propose_odom; pk_api_propose.hip): nothing until the first call, then
  // 84 P bytes -- ten rows of P doubles and one of P int32
  struct Proposal {
    double* pose = nullptr;         // [3][P] the poses before the move (x | y | h)
    double* zero = nullptr;         // [P][3] the normals of the predicted pose: zeros
    double* xi = nullptr;           // [P][3] k_propose's normals
    double* dlogw = nullptr;        // [P] its weight increments
    int32_t* used = nullptr;        // [P] the matches it used
    bool valid = false;             // the last call's results are there (pk_proposal_download)
    bool ranges = false;            // pk_proposal_ranges: armed ranges (pk_scan_ranges) are consumed by the step, not refused
    bool grow = false;              // pk_proposal_grow: the step runs on a growing filter, the bookkeeping and retirement behind it (no device state)
  } prop;
  // unique association (pk_assoc_unique; pk_api_unique.hip): configuration, and 64 bytes of counters from the first time it is switched on
  struct Unique {
    bool on = false;
    bool last = false;                    // the last scan's association went through k_assoc_unique: its counters are that scan's
    unsigned long long* stats = nullptr;  // [kAssocUniqueWords] on the device; word 4 (the bound was reached) stays up until it is reported
    unsigned long long* seen = nullptr;   // the same words in pinned host memory, copied behind every pass
  } uq;
  int32_t* anc = nullptr;           // P
  unsigned char* slot_tmp = nullptr;  // one slot
  // timing
  uint32_t timing_mask = 0;  // bit i: PK_T_* slot i is bracketed by hipEvents
  int64_t timing_seen[PK_T_COUNT] = {0};
  std::vector<TimedSpan> pending;
  std::vector<hipEvent_t> pool;
  double ms[PK_T_COUNT] = {0};
  int64_t launches[PK_T_COUNT] = {0};
};

// A filter's device and pinned memory comes from these alone ("Memory"): f->mem records every block, and
// pk_destroy frees what it holds.
template <typename T>
int dev_alloc(pk_filter* f, T** p, size_t n) { return f->mem.alloc(p, n ? n : 1); }
template <typename T>
void dev_free(pk_filter* f, T** p) {
  f->mem.release(*p);
  *p = nullptr;
}
// a buffer allocated once, when something first wants it (no synchronisation: nothing is freed)
template <typename T>
int dev_lazy(pk_filter* f, T** p, size_t n) { return *p ? PK_OK : dev_alloc(f, p, n); }
// The grow pattern: nothing while need <= *cap; else the stream is synchronised, the members are freed and allocated afresh, and
// *cap = new_cap last (a failure leaves *cap == 0).  dev_reserve: one buffer of new_cap elements; dev_reserve_group: several
// buffers behind one capacity, each want(&p, n) with its own element count.
template <typename C, typename... T>
int dev_reserve_group(pk_filter* f, C* cap, C need, C new_cap, Want<T>... w) {
  auto idle = [f]() -> int {
    PK_HIP(hipStreamSynchronize(f->stream));
    return PK_OK;
  };
  return f->mem.reserve(cap, need, new_cap, idle, w...);
}
template <typename T, typename C>
int dev_reserve(pk_filter* f, T** p, C* cap, C need, C new_cap) { return dev_reserve_group(f, cap, need, new_cap, want(p, (size_t)new_cap)); }
// pinned host memory (registered, not counted in pk_device_bytes)
template <typename T>
int host_alloc(pk_filter* f, T** p, size_t n, unsigned flags) { return f->mem.alloc_host(p, n, flags); }

struct Span {
  pk_filter* f;
  int slot;
  hipEvent_t a = nullptr, b = nullptr;
  Span(pk_filter* f_, int slot_) : f(f_), slot(slot_) {
    if (!((f->timing_mask >> slot_) & 1u)) return;
    if (f->timing_seen[slot_]++ % f->opt.timing_stride != 0) return;
    a = take();
    b = take();
    if (a) (void)hipEventRecord(a, f->stream);
  }
  hipEvent_t take() {
    if (!f->pool.empty()) {
      hipEvent_t e = f->pool.back();
      f->pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
  ~Span() {
    if (!a || !b) return;
    (void)hipEventRecord(b, f->stream);
    f->pending.push_back(TimedSpan{slot, a, b});
  }
};

inline int use_device(pk_filter* f) {
  PK_HIP(hipSetDevice(f->device));
  return PK_OK;
}

// (the poses change: the motion launch's pose sums are no longer theirs) -- ahead of the argument checks, on any handle
inline void poses_change(pk_filter* f) {
  if (f) f->pose_part_ok = false;
}

// the control words at the head of the per-scan block (kCtlBytes, pk_scan_block.hpp)
inline unsigned long long* ctl_gmax_key(pk_filter* f) { return reinterpret_cast<unsigned long long*>(f->scan_dev); }
inline unsigned* ctl_n_flagged(pk_filter* f) { return reinterpret_cast<unsigned*>(f->scan_dev + 8 * kGmaxKeys); }
inline unsigned* ctl_cand_over(pk_filter* f) { return reinterpret_cast<unsigned*>(f->scan_dev + 8 * kGmaxKeys + 4); }
inline unsigned* ctl_n_stray(pk_filter* f) { return reinterpret_cast<unsigned*>(f->scan_dev + 8 * kGmaxKeys + 8); }
// written by k_cand_entries: != 0 -> k_step_pub stands back (a candidate list overflowed, or the publish table does not fit LDS)
inline unsigned* ctl_skip_pub(pk_filter* f) { return reinterpret_cast<unsigned*>(f->scan_dev + 8 * kGmaxKeys + 12); }
// != 0 -> the candidate-list instance of k_step_regs stands back (k_step_pub runs, or the grid walk does)
inline unsigned* ctl_skip_cand(pk_filter* f) { return reinterpret_cast<unsigned*>(f->scan_dev + 8 * kGmaxKeys + 16); }
// rows of the second-chance hand-off lists dealt out so far (FastHandoff::row_next)
inline unsigned* ctl_retry_rows(pk_filter* f) { return reinterpret_cast<unsigned*>(f->scan_dev + 8 * kGmaxKeys + 20); }
// written by k_cand_entries: != 0 -> the two-workgroups-per-CU instance of the two-pass kernel (k_step_pub_duo) stands back and
// k_step_pub_big takes the scan (the publish table, the contested blobs or the landmarks with several blobs exceed its share of LDS)
inline unsigned* ctl_skip_duo(pk_filter* f) { return reinterpret_cast<unsigned*>(f->scan_dev + 8 * kGmaxKeys + 24); }
// ... != 0 -> k_step_pub_big stands back (no publish / subscribe kernel takes the scan, or k_step_pub_duo does)
inline unsigned* ctl_skip_big(pk_filter* f) { return reinterpret_cast<unsigned*>(f->scan_dev + 8 * kGmaxKeys + 28); }
// what the scan's publish table came to (k_cand_entries; pk_observe_pub_stats): entries, contested blobs, landmarks of the reference
// particle with two or more blobs inside their gates, the longest candidate list; then (pk_observe_lean_stats) the groups marked lean and
// the groups in use, and -- counted by k_step_pub<2, 512> -- the pairs of lean groups that fell back to the usual body: seven words
inline unsigned* ctl_pub_stats(pk_filter* f) { return reinterpret_cast<unsigned*>(f->scan_dev + 8 * kGmaxKeys + 32); }

// ---- helpers that more than one file calls
// pk_api.hip
int materialise(pk_filter* f);
// What moves the particles in a step: the commanded twist (pk_step, pk_step_adaptive) or an odometry delta with its sigmas
// (pk_step_odom, which has checked both).
struct StepMotion {
  bool odom = false;
  double v = 0.0, w = 0.0, dt = 0.0;                             // the twist
  double delta[3] = {0.0, 0.0, 0.0}, sigma[3] = {0.0, 0.0, 0.0};  // the delta (rot1, trans, rot2) and its sigmas
  static StepMotion twist(double v, double w, double dt) {
    StepMotion m;
    m.v = v;
    m.w = w;
    m.dt = dt;
    return m;
  }
  bool finite() const { return odom || (std::isfinite(v) && std::isfinite(w) && std::isfinite(dt)); }
};
// the body of pk_step, pk_step_adaptive and pk_step_odom.  gate == NULL: the weights restart from 1 and pk_resample ends the step;
// else they carry over and pk_resample_adaptive ends it with the threshold *gate
int step_impl(pk_filter* f, const StepMotion& m, const double* z, uint64_t seed, uint64_t draw, const double* blobs,
              int32_t B, const int32_t* ids, double u, int32_t weight_domain, const double* gate);
// the staged scan's own copy of its blobs, and "these blobs are the staged scan": neither staged nor (pk_step) uploaded again
inline const double* staged_blobs(const pk_filter::Staged& sg) { return reinterpret_cast<const double*>(sg.st + sg.lay.blobs); }
inline bool is_staged_scan(const pk_filter* f, const double* blobs, int32_t B) {
  return f->staged.valid && B > 0 && f->staged.B == B && blobs == staged_blobs(f->staged);
}
// the body pk_motion and pk_motion_odom share behind their argument checks: the copy of a supplied z, the PK_T_MOTION span, the
// staged scan that rides the launch, pose_part_ok.  launch(z_dev, up_dst_dev, up_src_host_mapped, up_bytes) is the kernel's.
using MotionLaunch = std::function<void(const double*, void*, const void*, size_t)>;
int motion_impl(pk_filter* f, const char* who, const double* z, const MotionLaunch& launch);
// pk_api_adaptive.hip
int bad_threshold(const char* who, double threshold);  // a gate's threshold: finite and >= 0, else PK_ERR_INVALID
// pk_api_odom.hip
// pk_motion_odom behind its argument checks (what step_impl runs for an odometry step that cannot ride the fused launch)
int motion_odom_checked(pk_filter* f, const double delta[3], const double sigma[3], const double* z, uint64_t seed, uint64_t draw);
// pk_api_scan.hip
// the staging ring: the next pinned block (and room for it on the device), ids_dev's capacity, one block host -> device, "slot `slot` rides an upload"
int take_stage(pk_filter* f, size_t bytes, unsigned char** out, int* slot);
int ensure_ids_capacity(pk_filter* f, int B);
int upload_scan(pk_filter* f, const unsigned char* st, size_t bytes, int slot);
int note_upload(pk_filter* f, int slot);
int stage_ml_scan(pk_filter* f, const double* blobs, int B, const RangeScan* rs = nullptr);
// a scan with supplied ids (first / next: the landmark -> blob chains all particles share, prkt_core_v2.py:88; with_ids: the id row too, for k_propose)
struct KnownScan {
  KnownScanLayout lay{};
  int n_unmatched = 0;            // blobs with id 0
  bool single_sightings = true;   // no landmark is matched by more than one blob
};
int upload_known_scan(pk_filter* f, const double* blobs, int32_t B, const int32_t* ids, bool with_ids, KnownScan* out, const RangeScan* rs = nullptr);
ScanTables known_scan_tables(const pk_filter* f, const KnownScan& ks, int B);
KnownChains known_chains(const pk_filter* f, const KnownScan& ks);
// What the scan-taking calls check of their arguments, sliced so that each call keeps its own order of refusals around them: B < 0
// or no blobs, then no map | a blob that is not finite, then (a call with ids) the empty id row for an empty scan without ids -- no
// association: every landmark keeps its state -- and an id outside 0..L | supplied ids on a growing filter
int check_scan_shape(const pk_filter* f, const char* who, const double* blobs, int32_t B);
int check_scan_values(const pk_filter* f, const char* who, const double* blobs, int32_t B, const int32_t** ids = nullptr);
int refuse_grow_ids(const char* who);
// the ids back to the caller, [P][B] (ids_out == NULL, an empty scan: nothing): the supplied row P times, or ids_dev behind a synchronisation
int return_ids(pk_filter* f, int32_t* ids_out, int32_t B, const int32_t* supplied);
// pk_api_observe.hip
int colour_rows_for_download(pk_filter* f, int64_t p0, int64_t p1);
int ct_end(pk_filter* f);
int ct_maps_untouched(pk_filter* f, bool* untouched);
int observe_impl(pk_filter* f, const double* blobs, int32_t B, const int32_t* ids, int32_t* ids_out, bool reset);
// a proposal step's scan on the device (pk_api_propose.hip): where its parts lie.  known: supplied ids' chains (the ids are
// final); scan.dir: the rays that settle tentative ids; ids: one row of B (supplied) or ids_dev's [P][B]; rng: the range rows
// ([B][2], scan order) of a scan in which some blob has a range (rs->any), else NULL
struct ProposalScan {
  ScanTables scan;
  KnownChains known;
  int32_t* ids = nullptr;
  const double* rng = nullptr;
};
int proposal_scan(pk_filter* f, const double* blobs, int32_t B, const int32_t* ids, ProposalScan* out, const RangeScan* rs = nullptr,
                  bool grow = false);
void proposal_observed(pk_filter* f, bool known);
// the tail of a growing filter's non-empty scan, behind its observe launches: new landmarks at the live poses on the ids in ids_dev
// (or the last one-pass kernel's bit rows), retirement's pass with its clock advanced, the launch check ("<who> (new landmarks)")
int grow_bookkeeping(pk_filter* f, const char* who, const ScanTables& scan, int32_t B);
// what the bearing model (pk_set_measurement_model) has no kernels for, refused while it is on (a NULL handle passes)
int refuse_bearing(const pk_filter* f, const char* who, const char* what);
// pk_api_range.hip: the armed ranges of the next scan (pk_scan_ranges).  ranges_take: what every call that takes blobs starts
// with -- the ranges leave the filter whatever follows, and come back in *out unless the call is refused (refuse_ranges: the
// refusals and their precedence); ranges_check: the refusals alone, ahead of a step's motion (the ranges stay unless it refuses)
int refuse_ranges(const pk_filter* f, const char* who, int32_t B, int32_t armed_B);
int ranges_take(pk_filter* f, const char* who, int32_t B, RangeScan* out);
int ranges_check(pk_filter* f, const char* who, int32_t B);
void ranges_disarm(pk_filter* f);
int refuse_ranges_proposal(pk_filter* f, const char* who);  // (only while pk_proposal_ranges is off)
// pk_api_unique.hip: unique association (pk_assoc_unique).  unique_refuse: what the mode has no kernels for, refused while it is on;
// unique_fits: the pass's LDS tables against the workgroup's, before anything is enqueued; unique_settle: the pass itself on ids_dev,
// behind an association that FINALISED its ids, inside the caller's PK_T_ASSOC span; unique_error: behind a synchronisation, a
// particle that reached the bound of B + 1 passes since the last report fails the call (once)
int unique_refuse(const pk_filter* f, const char* who, const char* what);
int unique_fits(const pk_filter* f, const char* who, int32_t B);
// both for a maximum-likelihood scan of B > 0 blobs while the mode is on (PK_OK while it is off): the dense layout, then the tables
int unique_check(const pk_filter* f, const char* who, int32_t B);
int unique_settle(pk_filter* f, const ScanTables& scan);
int unique_error(pk_filter* f, const char* who);
// pk_api_shard.hip
int refuse_balanced(const pk_filter* f, const char* who);
int refuse_path(const pk_filter* f, const char* who);
int refuse_retire(const pk_filter* f, const char* who);
// pk_api_retire.hip
int retire_restart(pk_filter* f, int64_t p0, int64_t p1);  // pk_grow_upload wrote these particles: their clocks restart
// pk_api_path.hip
// behind pk_resample's kernels while the ring is on; weighting: what a trunk settles by when this record fills the ring
// (PK_PATH_UNIFORM, or the gated call's weight domain over the new generation's log-weights)
int path_record(pk_filter* f, int weighting = PK_PATH_UNIFORM);
inline void path_clear(pk_filter* f) {  // the history ends: the population was replaced
  if (!f) return;
  f->path.held = f->path.first = 0;
  f->trunk.length = 0;  // (the trunk's memory stays)
  f->trunk.first_step = f->path.recorded;
}

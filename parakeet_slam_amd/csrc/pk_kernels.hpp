// Host-visible launchers of the gfx950 kernels (defined in the twenty-one pk_k_*.hip files; pk_k_step_duo.inl is part of pk_k_step_pub.hip).
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pk_layout.hpp"

namespace pk {

struct NoiseD {
  double q00, rr, rg, rb, gg, gb, bb;
};

// Device-side view of one filter shard.
struct DeviceState {
  int64_t P;
  MapLayout lay;
  // pose SoA, double-buffered for the resample gather: [cur] is live
  double* x[2];
  double* y[2];
  double* h[2];
  double* logw[2];
  int32_t* src[2];  // map slot holding the particle's landmarks (in map[mcur])
  int cur;          // live pose buffer
  unsigned char* map[2];
  int mcur;  // live map buffer
  unsigned char* immutable;  // [L]
  // Particles adopted from another shard (multi-GPU resample) are read in place from the
  // receive buffer until the next observe rewrites them: src[p] < 0 means record -src[p]-1 of
  // `alt`, whose map slot starts alt_off bytes into a record of alt_stride bytes.
  const unsigned char* alt = nullptr;
  size_t alt_stride = 0, alt_off = 0;
  int64_t global_offset = 0;  // index of local particle 0 in the whole filter (Philox counters)
  // balanced placement of the sharded filter: the LOGICAL index of the particle in every physical slot
  // (its index in one filter holding all particles -- what keys the Philox counters and orders the weight scan), double-buffered
  // with the poses; NULL until the balanced exchange is first used (the logical index is global_offset + slot then)
  int64_t* logical[2] = {nullptr, nullptr};
};

// section 8(f4) on the device (pk_k_grow.hip): the per-particle bookkeeping of the new-landmark machinery, double-buffered like the
// poses (the resample gathers it by ancestors)
struct GrowState {
  double* hyp[2] = {nullptr, nullptr};       // [P][R][8] stored readings: id, x, y, heading, bearing, r, g, b
  int32_t* cnt[2] = {nullptr, nullptr};      // [P][4]: readings stored, spare slots in use, next_id, readings dropped (ring full)
  int32_t* slot_id[2] = {nullptr, nullptr};  // [P][S] feature id of every spare slot in use
  int cur = 0;
  int L0 = 0, S = 0, R = 0;                  // preset landmarks, spare slots, ring capacity
  double pair_threshold = 0.0;
};
// how the bookkeeping kernel places a new feature (pk_grow_init; DESIGN.md section 9, "Parallax-gated pairing"): kept beside
// GrowState, not in it -- it holds nothing per particle, and the kernels that take GrowState by value keep their arguments
constexpr int kGrowInitReference = 0;     // any crossing, identity position covariance: the reference's rule
constexpr int kGrowInitTriangulated = 1;  // crossings at min_parallax or more, the triangulation's own covariance
struct GrowInit {
  int mode = kGrowInitReference;
  double min_parallax = 0.0;  // as pk_grow_init received it
  double sin_min = 0.0;       // sin(min_parallax), formed once on the host
};
// the bookkeeping of one particle behind its record in the sharded exchange: counters (16 B) | slot ids | readings
__host__ __device__ inline size_t grow_tail_readings_off(int S) { return 16 + (((size_t)S * 4 + 15) & ~(size_t)15); }
inline size_t grow_tail_bytes(const GrowState& g) { return g.R > 0 ? grow_tail_readings_off(g.S) + (size_t)g.R * 64 : 0; }
// retirement of stale readings and unconfirmed features (pk_grow_retire; pk_k_grow_retire.hip): the per-particle clocks, beside
// GrowState's arrays and double-buffered with them (GrowState::cur indexes both).  Nothing is allocated until it is switched on.
struct RetireState {
  uint32_t* scan[2] = {nullptr, nullptr};  // [P][R] the scan at which every stored reading was filed
  int32_t* seen[2] = {nullptr, nullptr};   // [P][S] count word of every spare slot in use at the last pass
  int32_t* idle[2] = {nullptr, nullptr};   // [P][S] consecutive passes it did not change
  int32_t* cnt[2] = {nullptr, nullptr};    // [P][4]: covered readings, covered slots, readings retired, features retired
  uint32_t t = 0;                          // scans that ran the bookkeeping since retirement was switched on (wraps)
  int A = 0, M = 0;                        // reading_max_age, potential_max_idle (0: never)
  bool on() const { return cnt[0] != nullptr; }
};
// the sensor's perceptual field for the retirement pass (pk_grow_view; DESIGN.md section 9, "A field of view for retirement"): kept
// beside RetireState, not in it -- it holds nothing per particle, and the kernels that take RetireState by value keep their arguments
constexpr int kRetireViewWords = 4;  // unchanged slots of the last pass | those in view | potential retired | confirmed retired
struct RetireView {
  bool on = false;
  int C = 0;                                     // confirmed_max_misses (0: a promoted feature is never retired)
  double half_fov = 0.0, r_min = 0.0, r_max = 0.0;  // as pk_grow_view received them
  double rmin2 = 0.0, rmax2 = 0.0;               // r_min^2, r_max^2, formed once on the host
  unsigned long long* stats = nullptr;           // [kRetireViewWords] on the device, from the first pk_grow_view until the clocks go
};

// Where the landmark slot of a particle lives: its own map buffer or the adoption buffer.
struct SlotSource {
  const unsigned char* map;
  size_t slot_bytes;
  const unsigned char* alt;
  size_t alt_stride, alt_off;
  __host__ __device__ const unsigned char* at(int32_t src) const {
    return src >= 0 ? map + (size_t)src * slot_bytes : alt + (size_t)(-(src + 1)) * alt_stride + alt_off;
  }
};
inline SlotSource slot_source(const DeviceState& d) {
  return SlotSource{d.map[d.mcur], d.lay.slot_bytes, d.alt, d.alt_stride, d.alt_off};
}

constexpr int kScanBlock = 1024;  // particles per weight-scan block (256 threads x 4)

// K1
// up_dst_dev != NULL: the same launch also pulls the per-scan block (up_bytes from the pinned,
// device-mapped staging slot) into HBM with a few extra workgroups -- one launch less per step
void launch_motion(hipStream_t s, DeviceState& d, double v, double w, double dt, const double* z_dev,
                   uint64_t seed, uint64_t draw, int64_t global_offset, void* up_dst_dev = nullptr,
                   const void* up_src_host_mapped = nullptr, size_t up_bytes = 0, double* pose_part_dev = nullptr);
// The twist model's sigmas of (v, w) (prkt_core_v2.py:185, :190, :193): drive, and the one both heading noises share.  The one place
// that forms them: the motion launches and pk_propose (whose normals only give pk_motion's poses while the two agree to the bit).
inline void motion_sigmas(double v, double w, double* sd, double* sh) {
  *sd = fabs(.05 * v) + fabs(.005 * w) + .0005;   // :185
  *sh = fabs(.025 * w) + fabs(.005 * v) + .0005;  // :190,:193
}
// pose_part_dev != NULL: the launch also leaves, per block of 256 particles, the sums of x, y, sin h, cos h of the moved particles
// ([4] doubles per block, motion_pose_blocks(P) blocks): k_candidates reduces them to the particles' mean pose
inline int64_t motion_pose_blocks(int64_t P) { return (P + 255) / 256; }
void launch_motion_range(hipStream_t s, DeviceState& d, double v, double w, double dt, uint64_t seed, uint64_t draw,
                         int64_t p0, int64_t p1);
// K1 for an odometry delta (rot1, trans, rot2) with its sigmas (pk_k_motion_odom.hip): launch_motion's draws, upload workgroups
// and pose sums
void launch_motion_odom(hipStream_t s, DeviceState& d, const double delta[3], const double sigma[3], const double* z_dev,
                        uint64_t seed, uint64_t draw, void* up_dst_dev = nullptr, const void* up_src_host_mapped = nullptr,
                        size_t up_bytes = 0, double* pose_part_dev = nullptr);
void launch_motion_odom_range(hipStream_t s, DeviceState& d, const double delta[3], const double sigma[3], uint64_t seed,
                              uint64_t draw, int64_t p0, int64_t p1);
void launch_reset_weights(hipStream_t s, DeviceState& d);
// K2: maximum-likelihood association -> ids[P*B]
// (a) reference kernel: every (landmark, blob) pair is gate-tested (launch_assoc_brute, below the scan's tables)
// (b) production kernel: blobs bucketed on the host into a 3-D colour grid whose cell edge
// exceeds the colour gate radius sqrt(300), so a landmark only meets the blobs of its 27
// neighbouring cells (the tables and the exact records: pk_scan_block.hpp).  With n9 > 0, idx9 lists for every (r, g) column the
// blobs within one cell in r and g, ordered by b cell: a landmark's whole 27-cell neighbourhood is then one contiguous range.
struct BlobGrid {
  double lo[3];
  double inv_h;
  int G[3];
  int ncell;
  float thr32;   // conservative fp32 pre-filter threshold for the colour gate (300)
  float thrb32;  // conservative fp32 pre-filter threshold for the bearing gate (0.5)
  float thrb32w; // ... for the bearing model's gate, whose fp32 screen wraps the difference (the wrap's own error on top)
};
constexpr double kGridCell = 17.5;  // > sqrt(300) = 17.3205 (prkt_core_v2.py:441)
constexpr int kGridMax = 16;
__host__ __device__ inline size_t grid_cs_bytes(int ncell) { return ((size_t)(ncell + 1) * 2 + 15) & ~(size_t)15; }
size_t blob_grid_table_bytes(int ncell, int B, int n9);
size_t assoc_grid_lds_bytes(int ncell, int B, int n9);
constexpr size_t kMaxDynLds = 156 * 1024;
// Per-device "already done" flag for one-time function attributes (hipFuncSetAttribute is per
// device; one process may hold filters on several GPUs).  Returns true the first time it is asked
// for the CURRENT device.
constexpr int kMaxDevices = 64;
inline bool first_time_on_this_device(bool (&done)[kMaxDevices]) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return true;
  if (done[dev]) return false;
  done[dev] = true;
  return true;
}  // 160 KiB per workgroup minus the kernels' static __shared__
// Compute units of the CURRENT device (what sizes the persistent grids), cached per device: a process may drive filters on
// devices with different CU counts.
inline int device_cu_count() {
  static int n_cu[kMaxDevices] = {0};
  int dev = 0;
  const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDevices;
  if (known && n_cu[dev] > 0) return n_cu[dev];
  int n = 256;
  hipDeviceProp_t prop;
  if (known && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) n = prop.multiProcessorCount;
  (void)hipGetLastError();
  if (known) n_cu[dev] = n;
  return n;
}
// The device view of one uploaded scan.  A maximum-likelihood scan (the observe's enqueue_association fills it, nobody else): the
// blobs and their rays in scan order, the colour grid with its tables, the exact records and the order table in cell order, and --
// only for a scan in which some blob has a range (pk_scan_ranges) -- the range rows [B][2] (range, variance) in scan order and in
// cell order.  A scan with supplied ids has B and the blobs alone.
struct ScanTables {
  int B = 0;
  const double* blobs = nullptr;  // [B][4]
  const double* dir = nullptr;    // [B][2]
  BlobGrid grid{};
  int n9 = 0;
  const unsigned char* tables = nullptr;
  const double* exact = nullptr;  // [B][6]
  const unsigned short* order = nullptr;
  const double* rng = nullptr;
  const double* rng_cell = nullptr;
};
// The particles [p0, p1) of a launch (p1 < 0: up to the last one), and how many CUs a persistent kernel leaves without a
// workgroup: its workgroups hold their CUs for the whole launch, and a collective that is to run meanwhile (the all-to-all of the
// sharded filter's split step) needs somewhere to run.
struct ParticleRange {
  int64_t p0 = 0, p1 = -1;
  int reserve_cus = 0;
  int64_t end(int64_t P) const { return p1 < 0 ? P : p1; }
};
// Workgroups of a persistent kernel that keeps per_cu of them on a CU, over the particles `r` of P: the ones resident at once (a
// reserve outside (0, n_cu) is ignored), never more than particles; 0: the range is empty, nothing to launch.
inline int64_t persistent_grid(int n_cu, int per_cu, const ParticleRange& r, int64_t P) {
  const int64_t n = r.end(P) - r.p0;
  if (P <= 0 || n <= 0) return 0;
  const int64_t grid = (int64_t)(n_cu - (r.reserve_cus > 0 && r.reserve_cus < n_cu ? r.reserve_cus : 0)) * per_cu;
  return grid > n ? n : grid;
}
void launch_assoc_brute(hipStream_t s, DeviceState& d, const ScanTables& scan, int32_t* ids_dev, int model = 0, double q00 = 0.0);
// Hand-off from the association kernel to k_observe_fast (lmpass NULL and flags_only false, as a default-constructed one has
// them = not used: the association's general instance takes every particle).
struct FastHandoff {
  uint4* lmpass = nullptr;          // [rows][Lp] (slots = 4) or [rows][Lp][2] (slots = 8): see k_assoc_grid; rows = P, or with
                                    // `retry` the capped number of second-chance rows (row_of / row_next / row_cap below)
  int slots = 4;                    // gate-passing blobs a landmark can hand over: kFastSlots or kSweepSlots
  bool flags_only = false;          // pflag / n_flagged come from k_step_fused: run the general instance on the flagged only
  unsigned char* bcount = nullptr;  // [P][B]
  unsigned char* pflag = nullptr;   // [P] 0: done by the fast kernel, 1: for the general kernels, 2: handed off on the second chance
  unsigned* n_flagged = nullptr;    // number of flagged particles of this scan
  // second chance only: the hand-off rows are dealt out in order of arrival, row_cap of them (a fraction of P: what a scan
  // flags is a few percent at worst) -- row_of[p] = the row of particle p, *row_next = rows dealt so far (zeroed by the scan
  // upload); a particle that finds none left keeps flag 1 and goes to the general kernels
  int32_t* row_of = nullptr;
  unsigned* row_next = nullptr;
  int64_t row_cap = 0;
  // Second chance for the particles a one-pass kernel flagged (a landmark passing more than its four register slots): the
  // hand-off instance with eight slots works on the particles whose flag is 1 only and leaves 2 where it succeeded (for
  // k_observe_sweep, ObserveExtras::sweep_only_value) and 1 where not even eight slots do (general kernels).
  bool retry = false;
};
constexpr int kGmaxKeys = 256;  // the running max of the log-weights is kept in this many keys (one scan-block thread each)
// Optional behaviour of one observe launch.
struct ObserveExtras {
  const unsigned char* only_flagged = nullptr;  // general kernel: only the particles flagged by the fast path (flag == 1)
  const unsigned* n_flagged = nullptr;
  int sweep_only_value = 0;                     // k_observe_sweep: 0 = the particles whose flag is 0, else only those with this flag
  bool flip = true;                             // swap the map buffers after this launch
  bool reset = false;                           // weights restart from 1 (fused pk_reset_weights)
  unsigned long long* gmax_key = nullptr;       // keep the running max of the new log-weights here
  bool single_sightings = false;                // known ids: no landmark is matched by more than one blob
  unsigned* unm = nullptr;                      // growing maps on the publish / subscribe routes: out [P][unm_words] -- every particle's unmatched
  int unm_words = 0;                            //   blobs as a bit row in scan order (pk_k_step_pub.hip: pub_note_unmatched)
  const double* ctab = nullptr;                 // k_step_pub's 512-lane instances in table mode: the colour table (ColourTable below), its
  int ctab_depth = 0;                           //   depth, and where the kernel leaves the highest level it read
  unsigned* ctab_max = nullptr;
  int model = 0;                                // launch_observe: the measurement model (pk_math.hpp: kModelReference / kModelBearing)
  int lean = 0;                                 // k_step_pub<2, 512>: lean groups take the lean body (option "pub_lean"); the scan's
  unsigned* lean_stats = nullptr;               //   figures (k_cand_entries), where the kernel counts the pairs that fell back: [6]
  const double* rng = nullptr;                  // launch_observe, bearing model: the scan's range rows ([B][2] range, variance, scan order;
                                                //   pk_scan_ranges) -- set only when some blob has a range: k_observe_range
  const double* dlogw = nullptr;                // launch_observe, bearing model: k_observe_proposed -- the ids are FINAL (k_propose settled
                                                //   them) and the log-weight takes dlogw[p], not the updates' own importance factors;
                                                //   with rng set as well: k_observe_proposed_range
};
// The colour table (pk_k_colour.hip): tab[k][6][Lp], rows crr crg crb cgg cgb cbb as in a slot -- landmark l's
// colour block after k updates from the one pk_upload_map broadcast (base[6][Lp]; the uploaded counts are 0, so a landmark's level is
// its update count / 2).  Null tab: not in use.
struct ColourTable {
  const double* tab = nullptr;
  int depth = 0;
};
void launch_colour_table(hipStream_t s, const double* base_dev, double* tab_dev, int depth, int Lp, const NoiseD& qt);
// The six colour rows of map slots written from the table at the slots' counts (levels beyond the table: the recurrence from its last
// level).  pflag_dev == NULL: every slot of the live buffer; else the SOURCE slots of the particles whose flag is set, and nothing at
// all while *n_flagged_dev == 0.  range: the slots (or, with pflag_dev, the particles) covered (its reserve_cus is not looked at).
void launch_colour_rows(hipStream_t s, DeviceState& d, const ColourTable& ct, const NoiseD& qt, const ParticleRange& range = ParticleRange(),
                        const unsigned char* pflag_dev = nullptr, const unsigned* n_flagged_dev = nullptr);
// *any_dev |= 1 when some landmark of some slot of the live buffer has a count other than 0.
void launch_colour_counts_any(hipStream_t s, DeviceState& d, unsigned* any_dev);
constexpr int kFastSlots = 4;   // gate-passing blobs a landmark can hand over to k_observe_fast; more -> general path
constexpr int kSweepSlots = 8;  // ... to k_observe_sweep (large maps: a landmark's colour neighbourhood is busier)
constexpr int kFastMaxL = 512;  // k_observe_fast / k_step_fused keep a particle's whole map in registers (one landmark per lane, 512 lanes)
// the bearing model's association (pk_math.hpp: kModelBearing): the general instance alone, every particle; a scan with
// scan.rng_cell takes the range instances
void launch_assoc_grid_bearing(hipStream_t s, DeviceState& d, const ScanTables& scan, int32_t* ids_dev, bool finalize, double q00 = 0.0);
// ML observe for L <= kFastMaxL straight from the hand-off: contested blobs are settled here,
// with the landmark state in registers.  Particles flagged in fh.pflag are skipped (the general
// k_observe, launched with only_flagged, takes them).
size_t observe_fast_lds_bytes(int B);  // dynamic LDS of k_observe_fast: must fit kMaxDynLds
void launch_observe_fast(hipStream_t s, DeviceState& d, const ScanTables& scan, const FastHandoff& fh, const NoiseD& qt,
                         const ObserveExtras& ex = ObserveExtras());
// K3: EKF update + log-weight, from scan.blobs.  Supplied ids: the landmark -> blob chains shared by all particles (device arrays,
// built on the host).  Otherwise ids_dev [P][B], from which the chains are built per particle in LDS: ML ids are TENTATIVE --
// k_observe keeps a match only if its probability is > 0 (needs scan.dir) --, k_propose's are final (ex.dlogw).
struct KnownChains {
  const int32_t* first = nullptr;  // [Lp] first blob matched to landmark l, or -1
  const int32_t* next = nullptr;   // [B] next blob matched to the same landmark, or -1
  int n_unmatched = 0;             // blobs with id 0
};
void launch_observe(hipStream_t s, DeviceState& d, const ScanTables& scan, const KnownChains& known, const NoiseD& qt,
                    const ObserveExtras& ex = ObserveExtras());
void launch_observe(hipStream_t s, DeviceState& d, const ScanTables& scan, int32_t* ids_dev, const NoiseD& qt,
                    const ObserveExtras& ex = ObserveExtras());
// The measurement-informed proposal (pk_k_propose.hip): for every particle at its predicted pose (the live pose
// arrays) the normals xi, the weight increment and the matches used; tentative ids (blobdir_dev != NULL) are settled in place.
struct ProposeLaunch {
  const double* blobs_dev = nullptr;
  const double* blobdir_dev = nullptr;  // NULL: the ids are final
  const double* rng_dev = nullptr;      // the scan's range rows ([B][2] range, variance, scan order; pk_proposal_ranges) -- set only
                                        //   when some blob has a range: k_propose_range
  int B = 0;
  int32_t* ids_dev = nullptr;           // [P][B], or one row of B for every particle (ids_shared; not written)
  bool ids_shared = false;
  const double* z_dev = nullptr;        // [P][3], or NULL: the Philox draws of (particle, seed, draw)
  uint64_t seed = 0, draw = 0;
  bool odom = false;
  double u[3] = {0, 0, 0};              // (v, w, dt) or (rot1, trans, rot2)
  double sigma[3] = {0, 0, 0};
  NoiseD qt{};
  double* xi_dev = nullptr;             // out [P][3]
  double* dlogw_dev = nullptr;          // out [P]
  int32_t* used_dev = nullptr;          // out [P]
};
void launch_propose(hipStream_t s, DeviceState& d, const ProposeLaunch& q);
// ML observe for any L from the same hand-off, two sweeps over the particle's landmarks in
// chunks (persistent workgroups; see k_observe_sweep).  plan.grid == 0: scan too large for its LDS tables.
struct SweepPlan {
  int grid = 0;               // persistent workgroups
  size_t lds = 0;             // dynamic LDS per workgroup
  int qcap = 0;               // entries of the LDS probability queue
  size_t results_per_wg = 0;  // uint4 entries of global scratch per workgroup
};
SweepPlan observe_sweep_plan(const DeviceState& d, int B);
void launch_observe_sweep(hipStream_t s, DeviceState& d, const ScanTables& scan, const FastHandoff& fh, const NoiseD& qt,
                          const ObserveExtras& ex, const SweepPlan& plan, uint4* results_dev);
// K2 + K3 fused for L <= kFastMaxL and scan tables small enough for two workgroups per CU: gates,
// settling and EKF update of a particle in one workgroup, no hand-off through HBM.  Writes fh.pflag /
// fh.n_flagged (particles left to the general kernels).
size_t fused_lds_bytes(int ncell, int B, int n9, bool exact_lds = false);
constexpr size_t kFusedMaxLds = 78 * 1024;
void launch_step_fused(hipStream_t s, DeviceState& d, const ScanTables& scan, const FastHandoff& fh, const NoiseD& qt,
                       const ObserveExtras& ex, const unsigned* pub_skipped_dev = nullptr);
// Candidate lists from a reference particle (k_candidates).  All particles of a filter see the same scan and hold
// nearly the same map (same initial map, same blobs matched), so the blobs that can pass a landmark's two gates
// (prkt_core_v2.py:433, :441) are nearly the same for every particle.  Once per scan, for every landmark of ONE
// reference particle, the blobs within the gates WIDENED by (kCandBearing, kCandColour) are listed; a particle whose
// own expected bearing and colour of that landmark lie within those margins of the reference's can only match blobs of
// that list (triangle inequality), and tests them with the exact float64 gates -- no walk through the colour grid.
// The expected bearing is unwrapped in the reference (:408-423), so "within the margin" is taken modulo one turn of
// 2 pi either way, and the list holds the blobs of all three centres.
// A particle that breaks a margin anywhere is flagged and goes the general way; a landmark with more than kCandSlots
// candidates switches the whole scan back to the grid walk (cand_over).  Record per landmark, 32 B:
//   float ebref, r, g, b  |  kCandSlots x u16 blob (cell order) or 0xFFFF
constexpr int kCandSlots = 8;
// Every candidate / entry table carries kCandSpare records with EMPTY lists behind its Lp landmarks: the lanes of k_step_pub /
// k_step_pub_big that stand beyond the map read those (index Lp), so they never see a real landmark's candidates.
constexpr int kCandSpare = 2;
constexpr double kCandBearing = 0.2;   // rad: |expected bearing - reference's| of every particle, else flagged (the particles' HEADING spread goes here: sigma 0.02 rad after 25 steps of the bench)
constexpr double kCandColour = 1.5;    // per channel: |colour mean - reference's|
// The inverse lists, blob -> the (<= kCandSlots) landmarks that list it, 16 B per blob (8 x u16, 0xFFFF = empty, filled from
// the front in arbitrary order), are what k_cand_entries lays the publish table of k_step_pub out from.
struct CandTable {
  const uint4* rec = nullptr;         // [Lp][2] landmark records
  const uint4* brec = nullptr;        // [B] blob records (the inverse lists), or NULL
  const unsigned* over = nullptr;     // != 0: some list has more entries than slots -> grid walk for this scan
  const unsigned* skip_cand = nullptr; // k_step_regs' candidate-list instance stands back when != 0 (NULL: when *over != 0)
  const unsigned* n_stray = nullptr;  // blobs on no landmark's list
  const uint4* far = nullptr;         // [Lp][1 + slots / 8] (Kb, Ib, n, 0) | far list: look-alikes k_candidates took off the lists (pk_pub_math.hpp), or NULL
  int slots = kCandSlots;             // entries per list: kCandSlots ([Lp][2] records) or twice that ([Lp][3]; no inverse lists)
};
// the grid kernel ((b) above); with cand.rec its hand-off instance takes its gates from the candidate lists (while no list overflowed)
void launch_assoc_grid(hipStream_t s, DeviceState& d, const ScanTables& scan, int32_t* ids_dev, bool finalize, const FastHandoff& fh,
                       const CandTable& cand = CandTable());
// One launch of k_candidates.  rec and over have no default: without them there is nothing to launch.
struct CandidatesLaunch {
  uint4* rec;                           // out: the lists, [Lp + kCandSpare][2] or [..][3] (what CandTable::rec reads)
  unsigned* over;                       // out: CandTable::over
  int slots = kCandSlots;               // entries per list
  int64_t ref_particle = 0;             // the particle whose map the lists are made from
  const double* pose_sums4 = nullptr;   // the reference pose is the particles' mean: from launch_summary_partials' four sums,
  const double* pose_part = nullptr;    //   or from the per-block sums the motion launch left (motion_pose_blocks)
  unsigned* bcnt = nullptr;             // the inverse lists, u32[B] / u16[B][slots]: empty (0 / 0xFF) at the call, and emptied again
  uint4* brec = nullptr;                //   by k_cand_entries behind its last read; both NULL: none are made
  unsigned char* npass = nullptr;       // out [Lp + kCandSpare], or NULL
  uint4* far = nullptr;                 // out: CandTable::far; NULL: no look-alike is taken off the lists
  ColourTable ct;                       // ct.tab, and qt, the noise the table was built with: the reference's colour blocks come
  const NoiseD* qt = nullptr;           //   from the table (its slot's rows may be stale); either missing: from its slot
};
void launch_candidates(hipStream_t s, DeviceState& d, const ScanTables& scan, const CandidatesLaunch& c);
// K2 + K3 in one pass (pk_k_observe_ml.hip, pk_k_step_pub.hip).  (k_step_owner, a barrier-free variant in which every
// landmark settled its blobs against the rivals named by the two-way lists, was measured at 56 ms against 13 and removed
// in round 3: DESIGN.md section 4.)
// 512 < L <= kRegsMaxL: persistent 1024-lane workgroups, a particle's whole map in registers (two
// landmarks per lane), state read once; warm: how much of the next particle's slot is pulled into L2 ahead of time.
constexpr int kRegsMaxL = 2048;
size_t regs_lds_bytes(int ncell, int B, int n9);
size_t regs_cand_lds_bytes(int Lp, int B);
// cand.rec != NULL: the candidate-list instance (returns at once when *cand.skip_cand != 0), and a scan in which a list
// overflowed hands all its particles to the fall-back kernels (the grid-walk instance -- cand.rec == NULL, option
// "cand_lists" = 0 -- still spills eight registers and is no default route's kernel any more)
void launch_step_regs(hipStream_t s, DeviceState& d, const ScanTables& scan, const FastHandoff& fh, const NoiseD& qt,
                      const ObserveExtras& ex, int warm, const CandTable& cand = CandTable(), const ParticleRange& range = ParticleRange());
// K2 + K3 in one pass with STATIC publish / subscribe settling (pk_k_step_pub.hip): 512 < L <= kRegsMaxL, candidate lists
// both ways (cand.rec, and the inverse lists that launch_cand_entries turns into the publish table's layout: erec, binfo).
// 512-lane persistent workgroups, four landmarks per lane, two barriers per particle.  Returns at once when *skip != 0.
int step_pub_entry_capacity(int B);  // publish-table entries that fit LDS beside the scan's tables (0: the scan does not fit)
int step_pub_entry_capacity_small(int B);  // ... with three 256-lane workgroups per CU (the L <= 512 instance)
size_t step_pub_lds_bytes(int B, int ecap, bool small = false);
// What k_step_pub_duo (the two-workgroups-per-CU instance of the two-pass kernel) has room for: entries of the publish table,
// contested blobs, landmarks with several gate-passing blobs (ecap = 0: the instance is not in use)
struct DuoLimits {
  int tbytes = 0;  // bytes of LDS the publish table (8 per entry) and the overflow area (16 per landmark with several blobs) share; 0: off
  int ecap = 0;    // entries at most (the option "pub_entry_limit")
  int gcap = 0;    // contested blobs at most
  int nl = 1;      // landmarks per lane and turn: 1 (512 lanes, two workgroups per CU) or 2 (256 lanes with a pair each, three per CU)
  int park_limit = -1;  // >= 0 (tests, option "pub_duo_park_limit"): the kernel treats its overflow area as this many places
};
// What the publish / subscribe route shares: k_candidates and k_cand_entries write it once per scan (the observe's onepass_prepare
// fills this, and decides there which members a scan's kernels get), the three k_step_pub* launchers read it.  A member that is
// NULL switches its part off.
struct PubTables {
  CandTable cand;                    // the lists (every one-pass kind with lists has these; the rest: publish / subscribe alone)
  uint4* erec = nullptr;             // [Lp + kCandSpare] ([..][2] with sixteen-entry lists): the publish entries of every list's blobs
  unsigned* glist = nullptr;         // the blobs several landmarks list, compacted; their number; the octet orders
  unsigned* bcnt = nullptr;          // the inverse lists (CandidatesLaunch::bcnt, brec) and k_cand_entries' scratch per blob
  uint4* brec = nullptr;
  unsigned* binfo = nullptr;
  unsigned char* npass = nullptr;    // [Lp + kCandSpare] blobs inside the reference particle's own gates
  unsigned* stats = nullptr;         // [7] k_cand_entries' figures of the scan
  unsigned* skip_pub = nullptr;      // != 0 after k_cand_entries: k_step_pub stands back from this scan (a list overflowed, the table does not fit)
  unsigned* skip_cand = nullptr;     // ... k_step_regs' candidate-list instance does
  int ecap = 0;                      // entries of the publish table that fit LDS
  // the two-pass kernels (sixteen-entry lists) alone, else NULL:
  float4* gate4 = nullptr;           // [B] every blob's bearing and colour as float (with it k_cand_entries reads the scan's exact records)
  uint4* prim = nullptr;             // the primary-blob table (prim_table_uint4)
  unsigned* skip_duo = nullptr;      // != 0: k_step_pub_duo stands back / k_step_pub_big does (one of the two takes the scan, or neither)
  unsigned* skip_big = nullptr;
  DuoLimits duo;                     // what k_step_pub_duo has room for (tbytes 0: the instance is off)
};
// One launch of k_cand_entries: the publish table's layout from the lists both ways.  pub.cand.rec, cand.over, erec, bcnt, brec,
// binfo, glist, skip_pub and skip_cand are needed whatever the scan.
struct CandEntriesLaunch {
  PubTables pub;
  bool pruned = false;                // the lists have had their far look-alikes taken off (CandidatesLaunch::far)
  unsigned char* flag_all = nullptr;  // [P] with n_flagged: a scan nobody takes flags every particle in this very launch
  unsigned* n_flagged = nullptr;
};
void launch_cand_entries(hipStream_t s, const DeviceState& d, const ScanTables& scan, const CandEntriesLaunch& c);
// The primary-blob table of the two-pass kernels (k_cand_entries writes it, once per scan): for every landmark l (and the kCandSpare
// spare records) the records of the FIRST blob of its candidate list, in landmark order -- four planes of Lp + kCandSpare uint4
// (bearing, r, g, b as float | exact bearing, r | exact g, b | ray direction ux, uy), then the blob's index per landmark (u32;
// 0xFFFF: the list is empty)
inline size_t prim_table_uint4(int Lp) { const size_t Lpp = (size_t)Lp + kCandSpare; return 4 * Lpp + (Lpp + 3) / 4; }
void launch_step_pub(hipStream_t s, DeviceState& d, const ScanTables& scan, const FastHandoff& fh, const NoiseD& qt,
                     const ObserveExtras& ex, const PubTables& pub, const ParticleRange& range = ParticleRange());
// every particle of [p0, p1) flagged for the fall-back kernels when *over != 0 (a candidate list overflowed)
void launch_flag_range_if(hipStream_t s, const unsigned* over_dev, unsigned char* pflag_dev, unsigned* n_flagged_dev, int64_t p0, int64_t p1);
// The same for maps beyond kRegsMaxL landmarks (up to kPubBigMaxL), in two passes over the map (the second from L2 / Infinity
// Cache); candidate and inverse lists of 2 kCandSlots entries: cand.rec [Lp][3], erec [Lp][2].
constexpr int kPubBigMaxL = 6144;  // six pairs per lane: beyond that the slot words of a lane no longer fit its registers
int step_pub_big_entry_capacity(int B);
size_t step_pub_big_lds_bytes(int B, int ecap);
void launch_step_pub_big(hipStream_t s, DeviceState& d, const ScanTables& scan, const FastHandoff& fh, const NoiseD& qt,
                         const ObserveExtras& ex, const PubTables& pub, const ParticleRange& range = ParticleRange());
// The two-workgroups-per-CU instance of the two-pass kernel (pk_k_step_duo.hip): ONE landmark per lane and turn, one carried word
// per landmark, the expected bearing worked out again in pass 2 -- at most 128 VGPRs, so that two 512-lane workgroups share a CU
// (four waves per SIMD) and one's row latency is the other's float64 issue.  Each has half the CU's LDS: k_cand_entries decides per
// scan whether the publish table fits (step_pub_duo_limits -> DuoLimits; *skip_duo), k_step_pub_big takes the scans that do not.
void step_pub_duo_limits(int B, int Lp, int nl, DuoLimits* out);
size_t step_pub_duo_lds_bytes(int B, const DuoLimits& lim);
// (nothing is launched while pub.duo.tbytes is 0, or without pub.prim and pub.stats)
void launch_step_pub_duo(hipStream_t s, DeviceState& d, const ScanTables& scan, const FastHandoff& fh, const NoiseD& qt,
                         const ObserveExtras& ex, const PubTables& pub, const ParticleRange& range = ParticleRange());
extern int g_observe_nv;
// dynamic LDS of the general ML instance of k_observe (per-particle chains first[Lp], next[B], ids[B]) and of
// k_assoc_brute (best[B] u64 + bid[B]): callers check them against kMaxDynLds BEFORE anything is enqueued
inline size_t observe_general_lds_bytes(int Lp, int B) { return sizeof(int32_t) * ((size_t)Lp + 2 * (size_t)B); }
inline size_t assoc_brute_lds_bytes(int B) { return (size_t)B * 12; }
// K2'': unique association (pk_k_assoc_unique.hip; DESIGN.md section 4, "Unique association"): behind either association kernel,
// on FINAL maximum-likelihood ids, every particle's ids are settled in place so that no landmark keeps more than one blob of the scan
// -- the greedy matching by (p descending, blob ascending, landmark ascending).  A particle whose ids claim no landmark twice is not
// written.  scan: B, blobs, dir and (a scan with ranged blobs) rng, all in scan order.
constexpr int kAssocUniqueWords = 8;  // stats_dev: particles with a conflict, blobs whose id changed, of those re-matched, the most
                                      // passes any particle took, != 0: a particle reached the bound of B + 1 passes; three spare
struct AssocUniqueLaunch {
  int32_t* ids_dev = nullptr;               // [P][B], in and out
  unsigned long long* stats_dev = nullptr;  // [kAssocUniqueWords], added to (the caller zeroes them per scan)
  int model = 0;                            // pk_math.hpp: kModelReference / kModelBearing
  double q00 = 0.0;                         // Qt[0][0], for the blobs with a range
};
// dynamic LDS: best u64[Lp] | cur_p u64[B] | win i32[Lp] | cur_id i32[B] | the losers' queue u16[B] -- callers check it against kMaxDynLds
inline size_t assoc_unique_lds_bytes(int Lp, int B) { return (12 * (size_t)Lp + 14 * (size_t)B + 15) & ~(size_t)15; }
void launch_assoc_unique(hipStream_t s, DeviceState& d, const ScanTables& scan, const AssocUniqueLaunch& q);
// K4: weights -> block totals / local scans
void launch_block_max(hipStream_t s, DeviceState& d, double* partial_dev, double* gmax_dev);
void launch_keys_max(hipStream_t s, const unsigned long long* keys_dev, double* gmax_dev);
void launch_scan_local(hipStream_t s, DeviceState& d, const double* gmax_dev, int domain,
                       double* clocal_dev, double* totals_dev, const unsigned long long* gmax_key_dev = nullptr);
// exclusive scan of the (global) block totals, sequential in block order: offsets[nb], sum[1]
void launch_scan_blocks(hipStream_t s, const double* totals_dev, int64_t nb, double* offsets_dev,
                        double* sum_dev);
// ancestors of the local output slots [slot0, slot0 + n); offsets_dev == sum_dev == NULL with
// nb <= kAncestorsScanMaxBlocks: the kernel scans the block totals itself (same order, same bits)
constexpr int64_t kAncestorsScanMaxBlocks = 256;
void launch_ancestors(hipStream_t s, const double* clocal_dev, const double* totals_dev,
                      const double* offsets_dev, const double* sum_dev, int64_t nb, int64_t P_global,
                      int64_t P_scan, double u, int64_t slot0, int64_t n, int32_t* anc_dev,
                      DeviceState* gather = nullptr);  // gather: also gather the poses (fused K5)
// K6
void launch_summary_partials(hipStream_t s, DeviceState& d, double* partial_dev, double* out4_dev);
// The map estimate (pk_k_mapsum.hip): per-landmark moments over the particles, landmarks [0, Ls).  k_map_partials, grid
// (landmark tiles, particle groups), leaves part[groups][kMapSums][tiles x kMapSumLanes] (5 first moments, 15 second moments --
// both of mu - the first local particle's mean rows --, 9 within, 1 count) and wpart[groups][2] (sum w, sum w^2); k_map_fold adds them in
// group order (in place, into group 0's), k_map_finish un-shifts into res[2 + 30 L]: wsum[2] | mean[L][5] | m2[L][15] | within[L][9] | counts[L], rows l >= Ls NaN.
// weighted: w = exp(logw - gmax), else 1.  The particles are read through src[] where they are: nothing is moved or written.
constexpr int kMapSumLanes = 256;
constexpr int kMapSums = 30;
constexpr int kMapSumMaxGroups = 1024;
inline int map_sum_tiles(int Ls) { return Ls > 0 ? (Ls + kMapSumLanes - 1) / kMapSumLanes : 1; }
int map_sum_groups(int64_t P, int Ls, int forced);  // a function of (P, Ls) alone unless forced (option "map_sum_groups") > 0
inline size_t map_sum_part_doubles(int Ls, int groups) { return (size_t)groups * kMapSums * map_sum_tiles(Ls) * kMapSumLanes; }
void launch_map_moments(hipStream_t s, const DeviceState& d, int Ls, int weighted, double gmax, int groups, double* part_dev,
                        double* wpart_dev, double* res_dev);
// k_map_fold alone: part_dev[groups][n] added in group order into group 0's, wpart_dev[groups][2] into wpart_dev[0 .. 1]
void launch_map_fold(hipStream_t s, int groups, size_t n, double* part_dev, double* wpart_dev);
// The discovered landmarks (pk_k_mapmatch.hip): per reference feature the spare slot of every particle that
// holds it (inside both radii, the smallest score, the lowest slot among equals) and the moments of the matched slots about the
// reference feature.  k_match_partials, grid (tiles of kMatchLanes features, particle groups), one wave a workgroup, leaves
// part[groups][kMatchSums][tiles x kMatchLanes] (sum w, sum w^2, sum w[potential] of the matches | 5 first, 15 second moments of
// mu - r | 9 within | 1 count) and wpart[groups][2]; k_map_fold adds them; k_match_finish un-shifts by every feature's own sum w into
// res[2 + kMatchSums rows + 3 + 2 rows]: wsum[2] | support[rows][3] | mean[rows][5] | m2[rows][15] | within[rows][9] | counts[rows] |
// the maximum log-weight used, the number of reference features, the reference particle | its count words [rows] | its ids [rows].
constexpr int kMatchLanes = 64;
constexpr int kMatchSums = 33;
constexpr int kMatchMaxGroups = 1024;
constexpr int kMatchMaxRef = 4096;
inline int map_match_tiles(int rows) { return rows > 0 ? (rows + kMatchLanes - 1) / kMatchLanes : 1; }
int map_match_groups(int64_t P, int rows, int forced);  // a function of (P, rows) alone unless forced (option "map_match_groups") > 0
inline size_t map_match_part_doubles(int rows, int groups) { return (size_t)groups * kMatchSums * map_match_tiles(rows) * kMatchLanes; }
inline size_t map_match_res_doubles(int rows) { return 2 + (size_t)kMatchSums * rows + 3 + 2 * (size_t)rows; }
struct MatchJob {
  int rows = 0;                      // rows of the result: the reference features (pk_map_match_moments) or the spare slots (pk_map_discovered)
  int nref = 0;                      // reference features when refi_dev == NULL, else word 0 of refi_dev says
  int groups = 1;
  int weighted = 0;
  double gmax = 0.0;                 // the shift of the log-weights when gmax_dev == NULL
  const double* gmax_dev = nullptr;
  double rho2 = 0.0, kap2 = 0.0, irho2 = 0.0, ikap2 = 0.0;  // squared radii and their reciprocals (0 for an infinite radius)
  const double* ref_dev = nullptr;   // [rows][5]
  const int32_t* refi_dev = nullptr; // launch_match_reference's integers, or NULL
  double* part_dev = nullptr;
  double* wpart_dev = nullptr;
  double* res_dev = nullptr;
  int32_t* matches_dev = nullptr;    // [P][nref] or NULL
};
// the reference particle's (best_dev != NULL: k_best_particle_fold's out[2], else `particle`) spare slots in use into ref_dev[S][5]
// and refi_dev[4 + 2 S] = their number, the particle, 0, 0 | count words | feature ids
void launch_match_reference(hipStream_t s, const DeviceState& d, const GrowState& g, const double* best_dev, int64_t particle,
                            double* ref_dev, int32_t* refi_dev);
void launch_map_match(hipStream_t s, const DeviceState& d, const GrowState& g, const MatchJob& m);
// The path estimate (pk_k_path.hip): a ring of the last `cap` resampled generations.  Row r of the ring:
// pose[r][3][P] (x, y, heading, structure of arrays like the live poses) and anc[r][P]; the held rows are first, first + 1, ...
// modulo cap, oldest first.
struct PathRing {
  double* pose = nullptr;  // [cap][3][P]
  int32_t* anc = nullptr;  // [cap][P]
  int cap = 0;             // rows (0: recording is off)
  int held = 0;            // rows in use
  int first = 0;           // ring row of the oldest one
  int64_t recorded = 0;    // rows ever recorded
  int row(int t) const { return (int)(((int64_t)first + t) % cap); }  // ring row of held row t
};
constexpr int kPathLanes = 256;
constexpr int kPathMaxBlocks = 256;  // workgroups of a summary launch: the partials of a row are this many at most
constexpr int kPathSums = 10;        // per (row, workgroup): n, mean dx, mean dy, centred xx, xy, yy, sum c sin h, sum c cos h, lineages alive, 0
constexpr int kPathRes = 8;          // per row: mean x, mean y, sum sin h, sum cos h, var x, cov xy, var y, survivors
inline int path_blocks(int64_t P) { const int64_t nb = (P + kPathLanes - 1) / kPathLanes; return nb > kPathMaxBlocks ? kPathMaxBlocks : (int)nb; }
// behind k_ancestors' gather (d.cur is the NEW generation): the old half of the pose buffers and anc_dev into ring row `row`
void launch_path_record(hipStream_t s, const DeviceState& d, const int32_t* anc_dev, const PathRing& ring, int row);
// out[n][held + 1][3]: the lineages of particles_dev[0 .. n) (NULL: of the particles 0 .. n - 1)
void launch_path_trace(hipStream_t s, const DeviceState& d, const PathRing& ring, const int64_t* particles_dev, int64_t n, double* out_dev);
// held + 3 launches: particle 0's lineage into ref_dev[held + 1][3]; one launch per row, newest first, that reduces the finished
// row about its reference pose into part_dev[row][path_blocks(P)][kPathSums], scatters its descendant counts (cnt_dev[3][P], integer
// atomics) into the row before it and zeroes the buffer of the row before that; one fold, a workgroup per row, into
// res_dev[held + 1][kPathRes]
void launch_path_summary(hipStream_t s, const DeviceState& d, const PathRing& ring, unsigned* cnt_dev, double* ref_dev, double* part_dev,
                         double* res_dev);
// The path estimate by the weights of the current particles (pk_k_path_weighted.hip; DESIGN.md section 4, "The weighted path
// estimate"): three launches whatever the ring holds -- particle 0's lineage into ref_dev[held + 1][3]; ONE launch of path_blocks(P)
// workgroups in which every thread walks its own particles' lineages back through rows held .. 0 (w = exp(logw - shift) as
// launch_pose_moments takes it, into wgt_dev[P]; the lineage indices in idx_dev[P]) and reduces each row about its reference pose
// into part_dev[row][path_blocks(P)][kPathSums]; one fold, a workgroup per row, into res_dev[held + 1][kPathWRes] = mean x, mean y,
// sum w sin h, sum w cos h, var x, cov xy, var y, S1, S2 (row `held`'s).
struct PathWeightedArgs {
  const double *x, *y, *h, *logw;  // the live generation
  const double* pose;              // the ring
  const int32_t* anc;
  const double *gmax, *ref;
  int32_t* idx;
  double *wgt, *part;
  int64_t P;
  int cap, first, held, domain;
};
constexpr int kPathWRes = 9;
void launch_path_weighted(hipStream_t s, const DeviceState& d, const PathRing& ring, const double* gmax_dev, int domain,
                          int32_t* idx_dev, double* wgt_dev, double* ref_dev, double* part_dev, double* res_dev);
// The trunk (pk_k_path_settle.hip; DESIGN.md section 4, "The trunk"): what is left of the rows the ring has given up, one record
// of kPathTrunkRes doubles per step, oldest first -- mean x, mean y, sum w sin h, sum w cos h, var x, cov xy, var y, S1 by the
// weights of the particles that were current when the row was settled (k_path_weighted_fold's first eight words for that row), the
// lowest and the highest lineage index of the row over ALL of those particles (equal: the row is final), and the pose of the
// lowest one as recorded.
struct PathTrunk {
  double* rows = nullptr;  // [cap][kPathTrunkRes]
  int64_t cap = 0;         // rows allocated
  int64_t length = 0;      // rows settled
  int64_t first_step = 0;  // global step index of row 0
  int batch = 0;           // rows path_record settles when it has filled the ring (0: the trunk is off)
  bool scratch_mine = false;  // pk_path_trunk_enable made the settle scratch (host bookkeeping: switching off gives it back)
};
constexpr int kPathTrunkRes = 13;
// Settles held rows 0 .. settle - 1 (1 <= settle <= ring.held; nothing for settle <= 0) into out_dev[settle][kPathTrunkRes].
// Four launches whatever the ring holds: particle 0's lineage into ref_dev[held + 1][3]; a lane per particle -- its weight
// (weighting: 0 / 1 as launch_path_weighted's domain, 2: every weight 1.0) into wgt_dev[P] and its lineage index in row `settle`,
// walked by index alone, into idx_dev[P]; k_path_weighted's reduction of rows settle - 1 .. 0 with each workgroup's lowest and
// highest lineage index into part_dev[row][path_blocks(P)][kPathSums]; one fold, a workgroup per row.  The ring is read only.
void launch_path_settle(hipStream_t s, const DeviceState& d, const PathRing& ring, int settle, const double* gmax_dev, int weighting,
                        int32_t* idx_dev, double* wgt_dev, double* ref_dev, double* part_dev, double* out_dev);
// The particle with the largest log-weight, the lowest index among equals, NaN never: part_dev[path_blocks(P)][2], then one fold
// in workgroup order into out_dev[2] = the log-weight, the index as a double (-1: every log-weight is NaN)
void launch_best_particle(hipStream_t s, const DeviceState& d, double* part_dev, double* out_dev);
// Adaptive resampling (pk_k_adaptive.hip; DESIGN.md section 4, "Adaptive resampling"): the effective sample size of the weights
// k_scan_local has just scanned, and the resample that declines when it is large enough -- decided on the device.
// What a gated call leaves for the host to read when it asks (pk_resample_stats); one thread writes it.
struct GateOutcome {
  double n_eff, s1, s2, shift;          // of the call: S1 / S2 * S1, sum w, sum w^2, what k_scan_local subtracted
  unsigned long long resampled;         // 1: it resampled, 0: it kept
  unsigned long long calls, resamples;  // since pk_create
};
constexpr int kGatePlan = 4;  // S1, S2, n_eff, keep (1.0 / 0.0)
// sum w^2 per scan block (w as k_scan_local takes it: the same shift), s2tot_dev[nb]; block 0 leaves the shift in shift_dev[0]
void launch_weight_sq(hipStream_t s, const DeviceState& d, const double* gmax_dev, int domain, const unsigned long long* gmax_key_dev,
                      double* s2tot_dev, double* shift_dev);
// one workgroup: the exclusive scan of the block totals (offsets_dev[nb], or NULL: not wanted) with k_scan_blocks' additions, then
// plan_dev[kGatePlan] -- S1 (the sum k_scan_blocks leaves), S2 over the blocks in order, n_eff, keep = n_eff >= threshold * P
void launch_gate_plan(hipStream_t s, const double* totals_dev, const double* s2tot_dev, int64_t nb, double* offsets_dev,
                      double* plan_dev, double threshold, int64_t P);
// launch_ancestors with the gather, behind the gate.  offsets_dev == plan_dev == NULL (nb <= kAncestorsScanMaxBlocks): every
// workgroup derives offsets, S1, S2 and the verdict from the block totals itself.  Resampled: pk_resample's ancestors and gather,
// log-weights 0; kept: anc[k] = k, the poses and sources copied, logw - shift.  The pose buffers flip either way.
void launch_ancestors_gated(hipStream_t s, const double* clocal_dev, const double* totals_dev, const double* s2tot_dev,
                            const double* offsets_dev, const double* plan_dev, int64_t nb, double u, double threshold,
                            const double* shift_dev, int32_t* anc_dev, DeviceState& d, GateOutcome* outcome_dev);
// The weighted pose summary: w = exp(logw - shift) (shift = gmax_dev[0] in the log domain, 0 where that is not finite or in the
// linear one), moments of (x, y) - particle 0's as k_path_row takes them, sum w sin h, sum w cos h, sum w^2.
// part_dev[path_blocks(P)][kPathSums]; res_dev[kPoseRes] = mean x, mean y, sum w sin h, sum w cos h, var x, cov xy, var y, S1, S2
constexpr int kPoseRes = 9;
void launch_pose_moments(hipStream_t s, const DeviceState& d, const double* gmax_dev, int domain, double* part_dev, double* res_dev);
// map maintenance
void launch_materialise(hipStream_t s, DeviceState& d);
void launch_broadcast_slot(hipStream_t s, DeviceState& d, const unsigned char* slot_dev);
void launch_probe(hipStream_t s, const double* in_dev, double* out_dev);
// the general dense path (pk_k_dense.hip): 30-row slots, full 5x5 covariances, any 4x4 Qt; one kernel does the (brute-force)
// maximum-likelihood association -- or takes supplied ids --, the EKF updates in scan order and the log-weight.
// update = false: association only (ids_out_dev), no state is touched.
size_t dense_lds_bytes(int Lp, int B);
// scan: B, blobs and dir alone.  ids_in_dev: [B] supplied ids shared by all particles, or NULL; ids_out_dev: [P][B] or NULL
void launch_observe_dense(hipStream_t s, DeviceState& d, const ScanTables& scan, const int32_t* ids_in_dev, int32_t* ids_out_dev,
                          const double Qt[16], bool update, const ObserveExtras& ex);
void launch_probe_dense(hipStream_t s, const double* in_dev, double* out_dev);
// sharded resample
// record header in front of the map slot: x, y, h, logw, slot_lo, slot_hi (the last two int64:
// the global output slots this copy fills at its destination; 0, 0 when the caller plans on the host)
// balanced placement: + klo (int64, the logical index of the child in slot_lo) + one spare word -- 64 bytes
constexpr size_t kPoseRecordBytes = 8 * sizeof(double);
// device tables of the balanced plan (all sized for the WHOLE filter: every rank derives the whole plan by itself)
struct BalancedBuffers {
  double* glogw = nullptr;    // [Pg] log-weights in logical order
  double* clocal = nullptr;   // [Pg] block-local weight scans, [nbg] totals, [nbg + 1] offsets: the 1-GPU scan's tables
  double* totals = nullptr;
  double* offsets = nullptr;
  double* sum = nullptr;
  int64_t* H = nullptr;       // [Pg + 1] offspring table in logical order
  long long* cloc = nullptr;  // [Pg] packed (children << 32 | has children) block-local scans in PHYSICAL order
  long long* ctot = nullptr;  // [nbg], [nbg + 1]
  long long* coff = nullptr;
  int64_t* rel = nullptr;     // [P + 1] this rank's child positions
  int64_t* Hl = nullptr;      // [P]
  int32_t* alive = nullptr;   // [P]
  int* bad = nullptr;         // consistency failures seen by the kernels (must stay 0)
  int64_t cap = 0;            // Pg the tables were sized for
};
void launch_iota64(hipStream_t s, int64_t* p, int64_t n, int64_t off);
void launch_bal_state(hipStream_t s, const DeviceState& d, double* out_dev);
void launch_bal_plan(hipStream_t s, const DeviceState& d, const double* gstate_dev, int64_t Pg, int world, int rank,
                     const double* gmax_dev, int domain, double u, BalancedBuffers& b, int64_t* table_dev);
void launch_bal_pack(hipStream_t s, DeviceState& d, const BalancedBuffers& b, int64_t a0, int64_t n, int64_t ebase_s,
                     int64_t dbase_d, int64_t dd_d, int64_t m_d, unsigned char* buf_dev, size_t stride, const GrowState* g,
                     int64_t keep = -1);
void launch_bal_adopt(hipStream_t s, DeviceState& d, const BalancedBuffers& b, int64_t m, const unsigned char* buf_dev,
                      int64_t n_recv, int64_t* rh_dev, int mode, size_t stride, int32_t* anc_dev);
void launch_offspring(hipStream_t s, const double* clocal_dev, const double* offsets_dev, const double* sum_dev,
                      int64_t first_block, int64_t P_local, int64_t P_global, double u, int last_shard,
                      int64_t* hi_dev);
void launch_offspring_plan(hipStream_t s, const double* clocal_dev, const double* global_totals_dev,
                           int64_t n_global_blocks, int64_t first_block, int64_t P_local, int64_t P_global, double u,
                           int last_shard, int64_t* hi_dev, int world, int64_t* ranges_dev, unsigned* ticket_dev);
void launch_offspring_global(hipStream_t s, const double* clocal_global_dev, const double* offsets_dev, const double* sum_dev,
                             int64_t goff, int64_t P_local, int64_t P_global, double u, int last_shard, int64_t* hi_dev);
void launch_scan_local_of(hipStream_t s, const double* logw_dev, int64_t n, const double* gmax_dev, int domain,
                          double* clocal_dev, double* totals_dev);
void launch_pack(hipStream_t s, DeviceState& d, const int64_t* idx_dev, int64_t n, unsigned char* buf_dev);
void launch_adopt(hipStream_t s, DeviceState& d, const int64_t* src_dev, const unsigned char* buf_dev);
// device-resident variant of the exchange (no per-particle host metadata)
void launch_shard_ranges(hipStream_t s, const int64_t* hi_dev, int64_t P_local, int world, int64_t* ranges_dev);
void launch_pack_range(hipStream_t s, DeviceState& d, const int64_t* hi_dev, int64_t j0, int64_t n, int64_t slot_start,
                       int64_t slot_end, unsigned char* buf_dev);
// mode 0: the whole new generation; 1: only the slots this shard's own particles fill (the generation becomes current);
// 2: only the slots filled by received records (into the generation mode 1 made current)
void launch_adopt_dev(hipStream_t s, DeviceState& d, const int64_t* hi_dev, int64_t slot_start,
                      const unsigned char* buf_dev, int64_t n_recv, int64_t* rlohi_dev, int mode = 0, int64_t span_lo = INT64_MIN, int64_t span_hi = INT64_MAX);
void launch_iota(hipStream_t s, int32_t* p, int64_t n);
// unm_dev != NULL: the unmatched blobs of particle p come from its bit row there (the one-pass kernels leave it) unless pflag_dev[p] != 0
// (the fall-back kernels took the particle and left its ids in ids_dev's row)
// init.mode picks the kernel's instance; q00 = Qt[0][0] of this scan (the triangulated covariance's bearing variance)
// rng_dev != NULL (pk_grow_ranges, a scan in which some blob has a range): the scan's range rows ([B][2] range, variance, scan
// order) -- the ranged instance of the rule init.mode picks; NULL: today's kernels
void launch_new_landmarks(hipStream_t s, DeviceState& d, GrowState& g, const GrowInit& init, double q00, const int32_t* ids_dev,
                          const double* blobs_dev, int B, const unsigned* unm_dev = nullptr, int unm_words = 0,
                          const unsigned char* pflag_dev = nullptr, const double* rng_dev = nullptr);
// anc >= 0: a particle of this filter; anc < 0: record -anc - 1 of buf (stride bytes apart, its bookkeeping tail_off bytes in)
void launch_grow_gather(hipStream_t s, GrowState& g, const int32_t* anc_dev, int64_t P, const unsigned char* buf_dev = nullptr,
                        size_t stride = 0, size_t tail_off = 0);
// behind launch_new_landmarks while retirement is on (r.t already counts this scan): every particle's slot is its own
// (v.on: k_grow_retire_view at the live poses d.x / d.y / d.h [d.cur], its counters in v.stats; otherwise k_grow_retire as ever)
void launch_grow_retire(hipStream_t s, DeviceState& d, const GrowState& g, const RetireState& r, const RetireView& v);
// the clocks by the same ancestors, into the buffers launch_grow_gather makes current: BEFORE it (it flips g.cur)
void launch_retire_gather(hipStream_t s, const GrowState& g, const RetireState& r, const int32_t* anc_dev, int64_t P);
// scan block: pinned (device-mapped) host memory -> HBM by a kernel, in stream order
void launch_upload(hipStream_t s, void* dst_dev, const void* src_host_mapped, size_t bytes);

}  // namespace pk

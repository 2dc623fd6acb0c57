/*
 * parakeet_slam.h -- C ABI of the MI355X-native FastSLAM-1.0 particle update.
 *
 * This is the drop-in boundary for the hot path of buckbaskin/parakeet_slam:
 * the per-timestep particle update in src/prkt_core_v2.py (+ src/matrix.py).
 * The reference has no FFI of its own -- its boundary is the Python class
 * surface FastSLAM / FilterParticle / Feature -- so each entry point below
 * names the reference method (file:line) whose arithmetic it replaces; the
 * Python facade in parakeet_slam_amd/core.py keeps the class surface and calls
 * these through ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 (PK_OK) or a negative pk_status; the message of
 *     the most recent failure on the calling thread is pk_last_error().
 *   - the caller owns every host buffer; the library owns every device buffer.
 *   - one caller thread per handle (the facade serialises with a mutex; the
 *     reference itself races here, prkt_ros.py:113-121 vs prkt_core_v2.py:162).
 *   - all host-side numbers are float64, the reference's arithmetic type.
 *   - kernels are enqueued on the handle's HIP stream; entry points that return
 *     data to the host synchronise that stream, the others do not.
 *   - landmark ids are the reference's: 1..L in preset order, 0 = "no match"
 *     (prkt_core_v2.py:294-299, :369-381).
 *
 * State layout in HBM: see DESIGN.md section 3.
 */
#ifndef PARAKEET_SLAM_H_
#define PARAKEET_SLAM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */
#endif

#define PK_ABI_VERSION 1

typedef enum pk_status {
  PK_OK = 0,
  PK_ERR_INVALID = -1,     /* bad argument (null pointer, size, non-finite input) */
  PK_ERR_HIP = -2,         /* a HIP runtime call failed; pk_last_error() has the text */
  PK_ERR_STATE = -3,       /* call order violated (e.g. observe before a map upload) */
  PK_ERR_UNSUPPORTED = -4, /* valid request the device path does not implement */
  PK_ERR_NOMEM = -5        /* host or device allocation failed */
} pk_status;

/* weight_domain of pk_resample */
/* Flag in a landmark's count word (pk_upload_landmarks / pk_download_landmarks): a POTENTIAL feature -- the reference's
 * negative ids, prkt_core_v2.py:109-118: matched and updated like any landmark, but a match multiplies the particle's
 * weight by 0.1 instead of the importance factor; the kernels clear the flag when the update count passes 5 (:113-117). */
#define PK_LANDMARK_POTENTIAL 0x40000000
#define PK_WEIGHTS_LINEAR 0 /* w = exp(logw): the reference's quantity, underflows like it */
#define PK_WEIGHTS_LOG 1    /* w = exp(logw - max logw): same ancestors unless the former underflows */

/* kernel slots of pk_timings */
enum {
  PK_T_MOTION = 0,
  PK_T_ASSOC = 1,
  PK_T_OBSERVE = 2,
  PK_T_WEIGHTS = 3,
  PK_T_RESAMPLE = 4,
  PK_T_SUMMARY = 5,
  PK_T_MATERIALISE = 6,
  PK_T_PROPOSE = 7, /* k_propose (pk_propose, pk_propose_odom) */
  PK_T_COUNT = 8    /* was 7 before PK_T_PROPOSE was appended: pk_timings writes PK_T_COUNT entries into both of its arrays, so a
                     * caller compiled against the shorter enum must be rebuilt (or pass arrays of at least 8) */
};

typedef struct pk_filter pk_filter; /* opaque */

int pk_abi_version(void);
const char* pk_status_string(int status);
const char* pk_last_error(void);

/* Number of HIP devices visible to this process (0 when there is none). */
int pk_device_count(void);

/* ---- life cycle -------------------------------------------------------------
 * FastSLAM.__init__ (prkt_core_v2.py:38-57) + FilterParticle.__init__ (:279-292):
 * P particles at pose (0,0,0), weight 1, Qt = 0.1*I4, empty map of capacity L.
 * The reference hard-codes P = 50 (:41); here it is a parameter. */
int pk_create(int64_t num_particles, int32_t num_landmarks, int32_t device, pk_filter** out);
int pk_destroy(pk_filter* f);

/* Use a caller-provided hipStream_t (e.g. torch's current stream); NULL restores the
 * handle's own stream. */
int pk_set_stream(pk_filter* f, void* hip_stream);
int pk_synchronize(pk_filter* f);
int64_t pk_num_particles(const pk_filter* f);
int32_t pk_num_landmarks(const pk_filter* f);
/* Bytes of HBM the handle holds (maps are double-buffered). */
int64_t pk_device_bytes(const pk_filter* f);

/* Tuning knobs that never change results:
 *   "assoc_kernel" = 0 (colour-grid association kernel, default) or 1 (brute-force reference
 *                    kernel that gate-tests every landmark x blob pair);
 *   "assoc_dup"    = 1 (default: 9x column-duplicated blob index list when it fits in LDS) or 0;
 *   "fast_observe" = 1 (default: contested associations are settled inside the EKF kernel --
 *                    k_observe_fast with the landmark state in registers for L <= 512,
 *                    k_observe_sweep in two sweeps over landmark chunks above that), 0 (general
 *                    path: association kernel writes ids), 2 (k_observe_sweep for every L) or 3 (the same with
 *                    eight hand-off slots per landmark, the default only for scans of >= 3000 blobs);
 *   "timing_stride" = 1 (default) .. n: with pk_enable_timing, bracket only every n-th launch of a
 *                    slot (two event records cost the stream a few microseconds each time);
 *   "upload_kernel" = 1 (default: the per-scan block is read from pinned host memory by a small
 *                    kernel in stream order) or 0 (hipMemcpyAsync);
 *   "fused_step"   = 1 (default: with "fast_observe" = 1, L <= 512 and scan tables that fit LDS twice
 *                    per CU, gates + settling + EKF update of a particle run in ONE kernel,
 *                    k_step_fused, without the hand-off through HBM) or 0;
 *   "regs_step"    = 1 (default: with "fast_observe" = 1, 512 < L <= 2048 and scan tables that fit LDS,
 *                    gates + settling + EKF update of a particle run in ONE pass, k_step_regs, with the
 *                    particle's whole map in registers) or 0 (k_assoc_grid hand-off + k_observe_sweep);
 *   "pub_step"     = 1 (default: the register route settles contested blobs by static publish / subscribe -- k_step_pub,
 *                    the inverse candidate lists lay a per-scan table out in LDS, every landmark publishes its verdicts
 *                    there, one lane per contested blob picks the winner; two landmark pairs per lane, 512 lanes -- while
 *                    the table fits LDS and no candidate list overflows; decided per scan on the device,
 *                    pk_observe_published) or 0 (k_step_regs: per-blob counters, probability queue, bids);
 *   "pub_duo"      = 0 (default), 1 or 2: maps of 2 049 .. 5 120 landmarks: a scan whose publish table fits its share of a CU's LDS is
 *                    worked on by k_step_pub_duo -- the two-pass kernel k_step_pub_big with ONE landmark at a time and one carried
 *                    word per landmark: 1 = 512 lanes, at most 128 VGPRs, TWO workgroups per CU; 2 = 256 lanes with a pair of
 *                    landmarks each, at most 168 VGPRs, THREE workgroups per CU -- so that one workgroup's memory waits are the
 *                    others' arithmetic; decided per scan on the device (pk_observe_pub_stats).  Measured slower than one
 *                    workgroup per CU (twice / three times the particles in flight no longer find their second read of the
 *                    map in the Infinity Cache: DESIGN.md section 4), hence off.  "pub_duo_park_limit" >= 0 (tests) treats its
 *                    overflow area -- where a landmark with several blobs of probability > 0 parks its slots between the
 *                    passes -- as that many places;
 *   "far_prune"    = 1 (default) or 0: once per scan, the look-alikes whose match probability is certainly 0 for every particle
 *                    (a key beyond the float64 underflow edge by the reference particle's bound with margins) leave the candidate
 *                    lists of the publish / subscribe kernels; a landmark whose own bound is weaker re-checks them itself
 *                    (prkt_core_v2.py:369: probability 0 never matches).  0: every particle tests and judges them (round 4).
 *   "pub_lean"     = 1 (default) or 0: k_step_pub's two-pair instance (1 025 .. 2 048 landmarks) lets the (wave, pair) groups whose
 *                    landmarks all have at most one candidate blob that nobody else lists skip the publish / subscribe machinery
 *                    (pk_observe_lean_stats); the results are the same bits either way.  0: every group takes the usual body;
 *   "pub_small"    = -1 (default), 0 or 1: maps of at most 512 landmarks through k_step_pub's 256-lane instance (three workgroups per
 *                    CU, candidate lists made once per scan) instead of k_step_fused.  Its kernel is 11-18 % faster, its per-scan
 *                    kernels cost 27 us whatever the number of particles: -1 takes it where the whole step was measured no slower --
 *                    filters of at least 5e6 particle.landmarks and 128 landmarks (BASELINE configs[1], 10 000 x 500, is the tie;
 *                    DESIGN.md section 10.3) --, 1 always, 0 never;
 *   "pub_entry_limit" = 0 (default: what LDS holds) or n: treat the publish table as n entries small (tests: scans
 *                    whose table does not fit fall back to k_step_regs);
 *   "cand_lists"   = 1 (default: k_step_regs tests each landmark against the candidate list of a reference particle
 *                    -- k_candidates, once per scan -- instead of walking the colour grid; particles outside the
 *                    list's margins go the general way) or 0 (grid walk);
 *   "split_reserve_cus" = 0..128 (default 16): CUs the first part of a split step (pk_observe_staged_range, first = 1,
 *                    last = 0) leaves without a workgroup -- k_step_regs holds a CU's whole register file for the whole
 *                    launch, and the all-to-all that is to run meanwhile needs CUs of its own;
 *   "regs_retry"   = 1 (default: particles k_step_regs flags -- a landmark passing more than four blobs -- get a second
 *                    chance on the eight-slot hand-off + k_observe_sweep before the general kernels) or 0;
 *   "regs_warm"    = 0..2: how much of the NEXT particle's map slot k_step_regs touches ahead of time
 *                    (0 nothing, 1 the mean rows -- the default --, 2 the whole slot: measured slower) so that it waits in L2;
 *   "observe_landmarks_per_lane" = 0 (default), 1 or 2  (process-wide). */
int pk_set_option(pk_filter* f, const char* name, int64_t value);

/* ---- configuration ----------------------------------------------------------
 * FastSLAM.Qt (prkt_core_v2.py:50-53), row-major 4x4.  Qt = [q00] (+) [3x3 symmetric] runs on the compact layout and
 * the fast kernels; any other finite Qt (bearing-colour coupling, asymmetry) switches the filter to the dense layout and
 * the general dense kernel (PK_ROUTE_DENSE), converting maps that are already loaded. */
int pk_set_measurement_noise(pk_filter* f, const double Qt[16]);

/* The measurement model of the filter's observes ("The bearing model").  It keeps no state of its own and may be
 * changed at any time between scans.
 *   PK_MODEL_REFERENCE (default)  the reference's, quirks included: what a filter that never asks computes, bit for bit.
 *   PK_MODEL_BEARING              the textbook robot-frame bearing.  With wrap(a) = a - 2 pi rint(a / 2 pi), pse = atan2(dy, dx):
 *       gate        |wrap(bearing - (pse - heading))| > 0.5 -> probability 0 (the colour gate is unchanged);
 *       position    the blob's unit ray turned by the heading is the ray's world direction; closest point and 2x2 density as ever,
 *                   without the reference's half-plane test and behind-the-ray branch (neither can fire behind the gate);
 *       update      zhat0 = pse - heading, innovation wrap(bearing - zhat0), H's first row (-dy / q, dx / q); the colour block as ever;
 *       weight      log w = -2 log 2 pi - 1/2 log det Q - 1/2 d' Q^-1 d, det Q = Q00 det(C + Qc); potential features and unmatched
 *                   blobs weigh 0.1 as ever.
 *     Its scans take the general kernels alone: PK_ROUTE_KNOWN_IDS with ids, else PK_ROUTE_ML_GENERAL (the association kernel, or the
 *     brute-force one with "assoc_kernel" = 1, then k_observe); pk_associate runs the same model.  Motion, resampling, summaries, the
 *     path, the map estimates and the new-landmark bookkeeping with its retirement are the same under both models.
 *     PK_ERR_UNSUPPORTED while it is on: the dense layout (covariances or a Qt that couple position, bearing and colour) in
 *     pk_observe* / pk_associate / pk_step*, and pk_observe_staged_range (the ranged and split observes of the sharded step).
 * pk_set_measurement_model: PK_ERR_INVALID for any other value, PK_ERR_STATE inside a split observe; nothing changed either way. */
#define PK_MODEL_REFERENCE 0
#define PK_MODEL_BEARING 1
int pk_set_measurement_model(pk_filter* f, int32_t model);
int pk_measurement_model(const pk_filter* f, int32_t* model);

/* Range-bearing scans ("Range-bearing scans"): an option of PK_MODEL_BEARING on the compact layout.  A scan may
 * carry a range and a range variance per blob -- a depth camera, a stereo pair or a lidar front end beside the colour camera --, for
 * all of its blobs or for some: NaN means "this blob has none", and such a blob is handled exactly as the bearing model handles it.
 * For a blob with a finite range rho and variance q_rho, with u the blob's unit ray turned by the heading, n = (-uy, ux) and q00 = Qt[0][0]:
 *   gates       unchanged (the wrapped bearing difference, the squared colour distance);
 *   position    the 2x2 density at the MEASURED POINT s + rho u instead of the closest point on the ray, under
 *               S = Sigma_xy + q_rho u u' + rho^2 q00 n n'; colour probability, factors, argmax and settling as ever;
 *   update      the position part is the 2-D measurement (bearing, range): H = [[-dy / q, dx / q], [dx / r, dy / r]], r = sqrt(q) (both
 *               rows (0, 0) at q = 0), S2 = H Sigma_xy H' + diag(q00, q_rho), innovation (wrap(bearing - zhat0), rho - r); the colour
 *               block, immutable landmarks, the update count and potential features as ever;
 *   weight      log w = -5/2 log 2 pi - 1/2 log(det S2 det(C + Qc)) - 1/2 (d' S2^-1 d + the colour term).
 * A landmark matched by several blobs takes them in scan order, with ranges and without.
 *
 * pk_scan_ranges names the ranges of the NEXT scan: ranges[num_blobs] (NaN, or finite and > 0) and variances[num_blobs] (finite
 * and > 0 wherever the range is finite; not read elsewhere).  They are consumed, on success or failure, by the next call that takes
 * blobs -- pk_stage_scan, pk_observe, pk_observe_fresh, pk_associate, pk_step, pk_step_adaptive, pk_step_odom -- and a scan that
 * pk_stage_scan staged keeps its ranges until it is observed or discarded.  num_blobs == 0 or ranges == NULL disarms.  Anything else
 * is PK_ERR_INVALID, and nothing is armed.  Ranges are not state: no snapshot holds them.
 * A scan in which no blob has a finite range stages, launches and computes what it would without the call; the first scan with one
 * may grow the per-scan block (pk_device_bytes) by 32 bytes a blob.  Its route is PK_ROUTE_KNOWN_IDS or PK_ROUTE_ML_GENERAL as ever.
 * While ranges are armed (or staged) the consuming call refuses, in this order, changes nothing, and the ranges are gone:
 *   PK_ERR_INVALID      another num_blobs than the ranges were named for;
 *   PK_ERR_UNSUPPORTED  a filter that is not on PK_MODEL_BEARING; the dense layout (the bearing model's own refusal); growing maps
 *                       (pk_grow_enable: a new landmark is still placed from two bearings) unless pk_grow_ranges is on;
 * and pk_propose / pk_propose_odom refuse them with PK_ERR_UNSUPPORTED before anything else (the proposal samples from the bearings)
 * unless pk_proposal_ranges has switched ranges into the proposal.
 * pk_scan_ranges_state: *armed = the num_blobs of the armed ranges (0: none), *staged = that of a staged scan that was given ranges
 * (0: none); either pointer may be NULL. */
int pk_scan_ranges(pk_filter* f, const double* ranges, const double* variances, int32_t num_blobs);
int pk_scan_ranges_state(const pk_filter* f, int32_t* armed, int32_t* staged);

/* FilterParticle.load_feature_list (prkt_core_v2.py:294-299) for every particle:
 * means[L*5] (x,y,r,g,b), covs[L*25] row-major 5x5, immutable[L] = Feature.__immutable__
 * (:883; NULL = all mutable).  update_count starts at 0.  Symmetric, block-diagonal covariances
 * (xy 2x2 (+) rgb 3x3 -- the structure the reference's update preserves) take the compact
 * 14-row layout and the fast kernels; a map in which ANY covariance couples position and colour or is not
 * symmetric takes the dense 30-row layout (the reference's full 5 + 25 state) and the general dense kernel
 * (PK_ROUTE_DENSE: the reference's 4x4 / 5x4 / 5x5 algebra entry by entry, :804-833, :897-930) -- correct, slow. */
int pk_upload_map(pk_filter* f, const double* means, const double* covs, const uint8_t* immutable);

/* Poses as rows (x, y, heading, weight); weight is the linear particle weight
 * (FilterParticle.weight, :288), stored on the device as its natural log. */
int pk_upload_poses(pk_filter* f, const double* xyhw);
int pk_download_poses(pk_filter* f, double* xyhw);
/* One particle's pose and weight -- FastSLAM.particles[i] = p, prkt_core_v2.py:162 -- without touching the other particles'
 * log-weights (which a download / upload of all poses sends through exp and log: every weight that underflows comes back as 0). */
int pk_upload_pose(pk_filter* f, int64_t particle, const double xyhw[4]);
/* The natural logarithms of the particle weights (the quantity the filter keeps: with B >~ 1000
 * blobs per scan the weights themselves underflow float64, prkt_core_v2.py:95,124). */
int pk_download_log_weights(pk_filter* f, double* logw);
/* ... and back, bit for bit (pk_upload_poses takes log(weight), and exp / log do not round-trip): what a snapshot of a filter whose
 * weights carry over between resamples (pk_resample_adaptive) restores.  -inf is a weight of zero; NaN and +inf are refused. */
int pk_upload_log_weights(pk_filter* f, const double* logw);

/* Landmark state of particles [p0, p1): means (n*L*5), covs (n*L*25 dense 5x5),
 * counts (n*L) = Feature.update_count.  Any output/input pointer may be NULL. */
int pk_download_landmarks(pk_filter* f, int64_t p0, int64_t p1, double* means, double* covs,
                          int32_t* counts);
int pk_upload_landmarks(pk_filter* f, int64_t p0, int64_t p1, const double* means,
                        const double* covs, const int32_t* counts);

/* ---- the step ---------------------------------------------------------------
 * particles[i].weight = 1 (prkt_core_v2.py:73). */
int pk_reset_weights(pk_filter* f);

/* FastSLAM.motion_update/motion_model (prkt_core_v2.py:148-208) for every particle.
 * z != NULL: host array P*3 of standard normals in the reference's draw order
 *            (drive, heading-1, heading-2 per particle) -- fixed-seed parity mode;
 * z == NULL: device counter-based generator (Philox4x32-10) keyed by (seed, draw). */
int pk_motion(pk_filter* f, double v, double w, double dt, const double* z, uint64_t seed,
              uint64_t draw);

/* The per-particle body of FastSLAM.cam_cb (prkt_core_v2.py:82-124): data association
 * (match_features_to_scan :317-381, probability_of_match :383-455), then per blob in scan
 * order generate_measurement :859, measurement_jacobian :748, measurement_covariance :804,
 * inverse matrix.py:11, kalman_gain :821, Feature.update_mean :897 / update_covar :916,
 * importance_factor :835 or no_match_weight :851, multiplied into the particle weight.
 *   blobs: B rows (bearing, r, g, b)  (matrix.blob_to_matrix, matrix.py:35-39)
 *   ids:   NULL -> maximum-likelihood association on the device, per particle;
 *          else B landmark ids (0 = unmatched) applied to every particle.
 *   ids_out: NULL or P*B int32 receiving the ids each particle used. */
int pk_observe(pk_filter* f, const double* blobs, int32_t num_blobs, const int32_t* ids,
               int32_t* ids_out);
/* pk_reset_weights + pk_observe in one pass over the particles: every weight restarts from 1
 * (prkt_core_v2.py:73) before the scan is applied -- what cam_cb does, and what pk_step uses. */
int pk_observe_fresh(pk_filter* f, const double* blobs, int32_t num_blobs, const int32_t* ids,
                     int32_t* ids_out);
/* The same in two halves, for callers that have host work to hide: pk_stage_scan does the HOST
 * part of a maximum-likelihood observe (checks, ray directions, association tables, all into a
 * pinned staging slot; no kernel is launched), pk_observe_staged enqueues the upload and the
 * kernels for the scan staged last (fresh != 0: weights restart from 1 first).  Any other
 * observe / associate call in between discards the staged scan. */
int pk_stage_scan(pk_filter* f, const double* blobs, int32_t num_blobs);
int pk_observe_staged(pk_filter* f, int32_t fresh);

/* Data association alone (FilterParticle.match_features_to_scan, prkt_core_v2.py:317-351):
 * ids_out[P*B] receives, per particle, the landmark id each blob matches (0 = none).
 * No state changes. */
int pk_associate(pk_filter* f, const double* blobs, int32_t num_blobs, int32_t* ids_out);

/* ---- new landmarks: FilterParticle.add_hypothesis / find_nearest_reading / ray_intersect /
 * color_distance / add_new_feature / cross_readings / add_orphaned_reading (prkt_core_v2.py:546-746) for every particle on the
 * device.  The filter's landmarks beyond the first `preset_landmarks` are SPARE slots (upload them with a colour no blob can gate
 * against).  From then on every maximum-likelihood observe (pk_observe / pk_observe_fresh / pk_step without ids) ends with one
 * kernel that walks each particle's unmatched blobs in scan order (:92-95): a blob pairs with the particle's nearest stored reading
 * -- rays crossing, colour distance below pair_threshold; the one change to the reference, whose find_nearest_reading (:579) walks
 * potential_features where the readings are in hypothesis_set and so never pairs anything -- and becomes a potential feature at
 * the crossing in the next spare slot (mean colour, identity covariance, count word PK_LANDMARK_POTENTIAL, :656-686); else it is
 * stored as an orphaned reading (:739-746).  Each particle keeps up to reading_capacity readings (the reference's dict grows
 * without bound; what does not fit is counted, see below).  pk_resample carries the bookkeeping along with the particles (:243).
 * Supplied ids and the dense layout are refused while it is on (PK_ERR_STATE). */
int pk_grow_enable(pk_filter* f, int32_t preset_landmarks, int32_t reading_capacity, double pair_threshold);
/* The bookkeeping of particles [p0, p1) (any pointer may be NULL): counters[n][4] = readings stored, spare slots in use, next_id
 * (:298), readings dropped because the ring was full; readings[n][reading_capacity][8] = id, x, y, heading, bearing, r, g, b of each
 * stored reading (the rows beyond `readings stored` are undefined); slot_ids[n][spare] = the feature id of each spare slot in use
 * (potential: the reference's -id, promoted: +id). */
int pk_grow_download(pk_filter* f, int64_t p0, int64_t p1, int32_t* counters, double* readings, int32_t* slot_ids);
int pk_grow_upload(pk_filter* f, int64_t p0, int64_t p1, const int32_t* counters, const double* readings, const int32_t* slot_ids);
int pk_grow_shape(const pk_filter* f, int32_t* preset_landmarks, int32_t* spare_slots, int32_t* reading_capacity);
/* Where, and how surely, the bookkeeping places a new feature ("Parallax-gated pairing").  It holds no
 * per-particle state -- records, pack / adopt, the sharded exchange and pk_device_bytes are what they were -- and may be changed
 * between any two scans; a filter that never calls it computes what it did, bit for bit.
 *   PK_GROW_INIT_REFERENCE (default)  the reference's rule above: any crossing, identity position covariance; min_parallax is ignored.
 *   PK_GROW_INIT_TRIANGULATED         a stored reading is a candidate only if its ray crosses the blob's (as above) AND the angle
 *       between the two rays is min_parallax or more: |den| >= sin(min_parallax), den = ay bx - ax by the determinant ray_intersect
 *       forms (:611-643), the sine formed once here in float64; a NaN fails.  Among the candidates the choice is unchanged (smallest
 *       colour distance, then smallest index; pair_threshold; a free spare slot), and a blob with no candidate is stored as an
 *       orphaned reading, so that a later scan can pair with it across a wider baseline.  The new feature's position covariance is
 *       the triangulation's own, J diag(q00, q00) J' over the two world bearings t1, t3 (q00 = Qt[0][0] of the scan; the pose
 *       uncertainty lives in the particles): with (s, c) their sines and cosines, (ox, oy) the crossing, (x1, y1) the reading's
 *       pose and (px, py) the particle's,
 *           sd = s3 c1 - c3 s1,  a = ((ox - x1) c1 + (oy - y1) s1) / sd,  b = ((ox - px) c3 + (oy - py) s3) / sd,
 *           Pxx = q00 (a^2 c3^2 + b^2 c1^2),  Pxy = q00 (a^2 c3 s3 + b^2 c1 s1),  Pyy = q00 (a^2 s3^2 + b^2 s1^2).
 *       Mean, colour mean, colour block (identity), count word and slot id are the reference rule's.
 * PK_ERR_STATE without pk_grow_enable; PK_ERR_INVALID for another mode, a NaN, or min_parallax outside [0, pi / 2]; nothing changed
 * either way.  pk_grow_init_mode reads both back (either pointer may be NULL; REFERENCE and 0 on a filter that never asked). */
#define PK_GROW_INIT_REFERENCE 0
#define PK_GROW_INIT_TRIANGULATED 1
int pk_grow_init(pk_filter* f, int32_t mode, double min_parallax);
int pk_grow_init_mode(const pk_filter* f, int32_t* mode, double* min_parallax);
/* Ranged scans on a growing map ("Single-sighting initialisation"; off by default).  Off, armed ranges
 * (pk_scan_ranges) are refused on a filter with pk_grow_enable, as ever.  On, that refusal steps aside (the others stay, in their
 * order): pk_observe, pk_observe_fresh, pk_stage_scan + pk_observe_staged (which re-checks), pk_step, pk_step_adaptive and
 * pk_step_odom consume the ranges.  Matched blobs are associated and updated as on a preset map (potential features update, weigh
 * 0.1 and are promoted as ever), and the bookkeeping, per particle and unmatched blob in scan order, becomes: a blob with a finite
 * range rho (variance q_rho), while a spare slot is free, is a potential feature in the next spare slot at once -- no search of the
 * stored readings, nothing stored.  With (px, py, ph) the particle's pose, zb the bearing, (s, c) the sine and cosine of ph + zb and
 * q00 = Qt[0][0] of the scan,
 *     mean = (px + rho c, py + rho s, r, g, b)   (the blob's own colour),     a = rho^2 q00,
 *     Pxx = q_rho c^2 + a s^2,   Pxy = (q_rho - a) c s,   Pyy = q_rho s^2 + a c^2,
 * the colour block is the identity, the count word PK_LANDMARK_POTENTIAL, the slot id next_id (which advances).  Every other
 * unmatched blob -- without a range, or ranged with every spare slot taken -- goes through the rule pk_grow_init selects, unchanged.
 * A scan in which no blob has a finite range launches and computes what it would with the mode off, bit for bit.  The mode holds no
 * per-particle state (pk_device_bytes, records, pack / adopt and the resample are what they were), may be switched between any two
 * scans, and composes with pk_grow_retire unchanged.  pk_propose / pk_propose_odom and the split observe refuse growing maps as ever.
 * PK_ERR_STATE without pk_grow_enable; PK_ERR_INVALID unless on is 0 or 1; nothing changed either way.
 * pk_grow_ranges_state: *on = 1 or 0 (0 on a filter that never asked). */
int pk_grow_ranges(pk_filter* f, int32_t on);
int pk_grow_ranges_state(const pk_filter* f, int32_t* on);
/* Growing maps that also shrink (the reference's hypothesis_set and potential_features only grow; off by default, and a filter
 * that never calls this does and holds what it did without it).  While a threshold is non-zero, one more kernel runs behind the
 * bookkeeping of every non-empty maximum-likelihood scan.  t counts those scans (uint32, wrapping; ages are differences modulo 2^32).
 * Per particle, in this order: (1) every spare slot the last pass knew whose count word changed since -- a match, a promotion --
 * restarts its idle count, the others add one to it (saturating); (2) slots and readings that are new since the last pass, or were
 * written by pk_grow_upload, are stamped: idle 0, scan t; (3) reading_max_age A > 0: the longest PREFIX of the ring whose readings
 * are A scans old or older goes -- the ring is filled in time order; a stale reading behind a fresh one stays -- and the rest moves
 * down to index 0; (4) potential_max_idle M > 0: the slots whose word carries PK_LANDMARK_POTENTIAL and that were idle for M passes
 * go; the survivors move down in their order (rows, count word, slot id, clocks), and every vacated slot returns to the state of a
 * spare slot that never held anything: mean (0, 0, 2^100, 2^100, 2^100), identity covariance, count word 0.  A promoted feature is
 * never retired; next_id is untouched.  A feature made by scan t0 and never matched is gone at the end of scan t0 + M.
 * 0 for a threshold: never.  The first call with a non-zero value allocates the clocks (pk_device_bytes) with nothing covered, so
 * the next pass stamps what is there as new; later calls only change the thresholds, from the next pass on; (0, 0) frees the clocks.
 * PK_ERR_STATE without pk_grow_enable; PK_ERR_INVALID for a negative value or one above 2^30.  While it is on, what moves particles
 * between filters (pk_pack_particles, pk_adopt_particles, pk_shard_pack_* / pk_shard_adopt_*, the balanced ones included, and
 * pk_shard_state_dev) returns PK_ERR_STATE: a record carries no clocks.  pk_resample and pk_resample_adaptive carry them along. */
int pk_grow_retire(pk_filter* f, int32_t reading_max_age, int32_t potential_max_idle);
/* The clocks of particles [p0, p1) while retirement is on (PK_ERR_STATE otherwise; any pointer may be NULL): counters[n][4] =
 * readings covered by the last pass, spare slots covered, readings retired, features retired; reading_scan[n][reading_capacity] =
 * the scan each stored reading was filed at; slot_seen[n][spare] / slot_idle[n][spare] = the count word of each spare slot in use at
 * the last pass and the passes it has not changed for (rows beyond what is covered are undefined); *scan_now = t.  The upload
 * takes the same (scan_now: the new t, NULL leaves it) and returns PK_ERR_INVALID where a particle's covered readings / slots exceed
 * what it stores / uses.  pk_grow_upload on particles while retirement is on sets their two covered counts to 0: their clocks
 * restart at the next pass, their retired counters stay. */
int pk_grow_clocks_download(pk_filter* f, int64_t p0, int64_t p1, int32_t* counters, uint32_t* reading_scan, int32_t* slot_seen,
                            int32_t* slot_idle, uint32_t* scan_now);
int pk_grow_clocks_upload(pk_filter* f, int64_t p0, int64_t p1, const int32_t* counters, const uint32_t* reading_scan,
                          const int32_t* slot_seen, const int32_t* slot_idle, const uint32_t* scan_now);
/* A field of view for retirement ("A field of view for retirement"; off by default, and with it off every call
 * launches and computes what it did, bit for bit).  As in Probabilistic Robotics, Table 13.1, a feature's evidence falls only when
 * the feature lies inside the sensor's perceptual range and was not observed; a feature out of view is left alone, and a feature
 * whose evidence runs out is discarded whether it was ever confirmed or not.  With a view (half_fov, range_min, range_max) and a
 * bound C = confirmed_max_misses, steps 2, 3 and 5 of pk_grow_retire's pass, its compaction and the state of a vacated slot are
 * unchanged, and steps 1 and 4 become
 *   1'. a spare slot the last pass knew: count word changed -> seen = word, idle = 0, as ever; word unchanged and the slot IN VIEW
 *       -> idle += 1 (saturating); word unchanged and not in view -> idle stays as it is;
 *   4'. a slot goes if M > 0, its seen word carries PK_LANDMARK_POTENTIAL and idle >= M, or if C > 0, its seen word does not carry
 *       the flag (a promoted feature) and idle >= C.  Preset landmarks are never touched; the survivors move down in order.
 * In view: with (px, py, ph) the particle's live pose at the pass -- in pk_step* the pose the scan was applied at, before the
 * resample; in pk_propose* (pk_proposal_grow) the sampled pose -- and (mx, my) the slot's position mean (evaluated only for a slot
 * this scan did not change), in float64 without contraction, in this order:
 *     (sn, ch) = sincos(ph);  dx = mx - px, dy = my - py;  q = dx dx + dy dy;  a = dx ch + dy sn;  c = dy ch - dx sn;
 *     in view  iff  q > 0  and  q >= range_min^2  and  q <= range_max^2  and  |atan2(c, a)| <= half_fov
 * (the squares formed once on the host; range_max = +inf is allowed; a NaN anywhere fails every comparison: not in view; no wrap,
 * no occlusion; the mean only -- a caller who wants a margin for the landmark's uncertainty passes a narrower field).
 * half_fov == 0 switches the view off and sets C to 0 (the other arguments are ignored).  PK_ERR_STATE without pk_grow_enable or
 * while retirement is off; PK_ERR_INVALID for half_fov NaN or outside [0, pi], range_min NaN, negative or infinite, range_max NaN or
 * <= range_min, C < 0 or C > 2^30; nothing changes in either case.  pk_grow_retire(f, 0, 0) frees the clocks and clears the view with
 * them; any other pk_grow_retire call leaves it alone (to retire confirmed features only: M = 2^30).  The view may be changed
 * between any two scans and holds from the next pass on.  It holds no per-particle memory: the clocks, the resample, the clock
 * transfers and what retirement refuses are what they were, and the clocks' "features retired" counts both kinds.  Its
 * PK_GROW_VIEW_STATS_BYTES of counters are counted in pk_device_bytes from the first call that switches a view on and are released
 * with the clocks.
 * pk_grow_view_state: *on, view = (half_fov, range_min, range_max) (zeros while off), *confirmed_max_misses; any pointer may be NULL.
 * pk_grow_view_stats (synchronises; PK_ERR_STATE without a view): out[0] = of the last pass, the slots it knew that did not change,
 * out[1] = of those, the ones in view (the ones that aged), out[2] / out[3] = potential / confirmed features retired since the view
 * was last switched on, all summed over the particles. */
#define PK_GROW_VIEW_STATS_BYTES 32
int pk_grow_view(pk_filter* f, double half_fov, double range_min, double range_max, int32_t confirmed_max_misses);
int pk_grow_view_state(const pk_filter* f, int32_t* on, double view[3], int32_t* confirmed_max_misses);
int pk_grow_view_stats(pk_filter* f, int64_t out[4]);

/* FastSLAM.low_variance_resample (prkt_core_v2.py:210-252) with step = u * sum/P, u in
 * [0,1) standing for random.random() (:226).  ancestors_out: NULL or P int64. */
int pk_resample(pk_filter* f, double u, int32_t weight_domain, int64_t* ancestors_out);

/* FastSLAM.summary (prkt_core_v2.py:254-276): (mean x, mean y, circular mean heading). */
int pk_summary(pk_filter* f, double out[3]);

/* The four sums FastSLAM.summary reduces (prkt_core_v2.py:267-271): sum x, sum y, sum sin h,
 * sum cos h -- what a sharded filter all-reduces before dividing / atan2. */
int pk_pose_sums(pk_filter* f, double out[4]);

/* The map estimate: per-landmark moments of the particles' landmark EKFs, reduced over the particles on the device (the particles
 * are read where they are: nothing is materialised, no filter state changes; the reference has no counterpart -- its summary,
 * prkt_core_v2.py:254-276, stops at the pose).  Landmarks covered: all L, or the preset ones of a growing filter (pk_grow_enable).
 * weighting PK_MAP_UNIFORM: w_p = 1 (pk_summary's convention: behind a resample the population is the estimate);
 * PK_MAP_WEIGHTED: w_p = exp(logw_p - gmax), for use between an observe and a resample. */
#define PK_MAP_UNIFORM 0
#define PK_MAP_WEIGHTED 1
/* One shard's moments (what a sharded filter combines, as pk_pose_sums is to pk_summary).  gmax: the filter-wide maximum
 * log-weight for PK_MAP_WEIGHTED, NaN = this handle's own; ignored for PK_MAP_UNIFORM.  Any output may be NULL.
 * wsum[2] = sum w, sum w^2;  mean[L*5];  m2[L*15] = sum w (mu-mean)(mu-mean)^T, upper triangle row-major, about THIS shard's mean;
 * within[L*9] = sum w Sigma_p (compact field order);  counts[L] = sum w * update_count.  Rows l >= Ls are NaN. */
int pk_map_moments(pk_filter* f, int32_t weighting, double gmax, double wsum[2], double* mean, double* m2, double* within, double* counts);
/* The finished estimate of ONE filter: mean[L*5], cov_within[L*25], cov_between[L*25] (dense row-major 5x5, like pk_download_landmarks),
 * update_count[L], n_eff[1].  Any output may be NULL. */
int pk_map_summary(pk_filter* f, int32_t weighting, double* mean, double* cov_within, double* cov_between, double* update_count, double* n_eff);

/* The DISCOVERED landmarks of a growing filter (pk_grow_enable): the spare slots, which pk_map_summary leaves NaN because slot j of
 * one particle and slot j of another need not hold the same feature (only the children of one ancestor agree slot by slot, and the
 * feature ids are per particle).  The correspondence is geometric.  For every reference feature r = (x, y, r, g, b) and every
 * particle, among the particle's spare slots in use (its counter word 1, at most S), a slot with mean mu is a candidate when
 *   dpos2 = (mu_x - r_x)^2 + (mu_y - r_y)^2 <= radius^2   and   dcol2 = ((mu_r - r_r)^2 + (mu_g - r_g)^2) + (mu_b - r_b)^2 <= colour_radius^2
 * (evaluated exactly so, in double, without fused multiply-adds; a NaN mean fails), and the match is the candidate with the strictly
 * smallest score dpos2 / radius^2 + dcol2 / colour_radius^2 (the reciprocals formed once; 0 for an infinite radius), the lowest
 * slot among equals.  Matches are taken independently per reference feature: they are NOT one-to-one, two reference features
 * closer than the radii can claim one slot -- keep radius below half the smallest separation of the landmarks.  radius and
 * colour_radius must be > 0 (+inf is allowed).  Per reference feature the matched slots are reduced as pk_map_moments reduces a
 * preset landmark, with w_p as there; the sums are shifted by the reference feature, which the radii bound.  No float atomics, every
 * sum in a fixed order: the same state gives the same bits on every call.  Nothing is moved, no filter state changes, and there is
 * no host round trip between the launches; the scratch is allocated by the first call.
 * PK_ERR_STATE: pk_grow_enable was not called, no map, no finite maximum log-weight (weighted), weights that do not sum to a positive
 * finite value; PK_ERR_UNSUPPORTED: the dense layout; PK_ERR_INVALID: the arguments.
 *
 * pk_map_match_moments: the unfinished moments about ANY reference points (0 <= n_ref <= 4096; what shards would combine).  gmax as
 * for pk_map_moments.  wsum[2] = sum w, sum w^2 over ALL particles; support[n_ref*3] = per feature W_j = sum w, sum w^2, sum w over
 * the matches whose count word carries PK_LANDMARK_POTENTIAL; mean[n_ref*5] = r_j + sum w (mu - r_j) / W_j; m2[n_ref*15] = sum w
 * (mu - mean)(mu - mean)^T, upper triangle row-major; within[n_ref*9] = sum w Sigma; counts[n_ref] = sum w update_count;
 * matches[P*n_ref] = the spare slot matched (0 .. S - 1, landmark preset + slot of the particle), -1 = none.  A feature nobody
 * matched: W_j = 0, mean and m2 NaN.  Any output may be NULL. */
int pk_map_match_moments(pk_filter* f, int32_t weighting, double gmax, const double* ref_means, int32_t n_ref, double radius,
                         double colour_radius, double wsum[2], double* support, double* mean, double* m2, double* within, double* counts,
                         int32_t* matches);
/* The finished estimate about ONE particle's own features: the reference features are the spare slots in use of particle
 * reference_particle, -1 = pk_best_particle's choice (taken on the device).  reference_out[1] = that particle, n_out[1] = its
 * features n <= S; per spare slot (S rows): ids = the reference particle's feature ids, ref_counts = its count words, mean[S*5],
 * cov_within[S*25], cov_between[S*25] (dense 5x5 as pk_map_summary), update_count[S], support[S] = W_j / W, the share of the
 * population that holds the feature, potential_fraction[S] = the share of those that still hold it as a potential feature,
 * n_eff[S] = W_j^2 / sum_j w^2, n_eff_all[1] = W^2 / sum w^2.  A feature nobody matched (a reference particle of weight 0 alone
 * holds it): support 0, NaN elsewhere; rows n .. S - 1: ids and ref_counts 0, support 0, NaN elsewhere.  Any output may be NULL. */
int pk_map_discovered(pk_filter* f, int32_t weighting, int64_t reference_particle, double radius, double colour_radius,
                      int64_t* reference_out, int32_t* n_out, int32_t* ids, int32_t* ref_counts, double* mean, double* cov_within,
                      double* cov_between, double* update_count, double* support, double* potential_fraction, double* n_eff,
                      double* n_eff_all);

/* ---- the path estimate: lineages recorded at every resample, traced back ("The path estimate") --------
 * FastSLAM factors the posterior over the robot's PATH; pk_resample overwrites the generation it resamples, so without a record
 * the filter knows the end of the path only (the reference keeps no more either: prkt_core_v2.py:210-252 replaces
 * self.particles).  pk_path_enable(capacity > 0) allocates a ring of the last `capacity` generations -- counted in
 * pk_device_bytes -- and from then on every pk_resample (those of pk_step included) records one ROW behind its own kernels:
 *   poses      x, y, heading of all P particles of the generation that was just resampled (the pose at which the scan was
 *              applied, after every motion update since the last resample), float64;
 *   ancestors  anc[k] = the index IN THAT GENERATION of the parent of particle k of the new generation, int32.
 * A full ring overwrites its oldest row (unless a trunk takes the oldest rows first: pk_path_trunk_enable, below); `recorded`
 * counts the rows ever recorded.  capacity 0 switches recording off and
 * releases the memory; any pk_path_enable starts from an empty ring.  Off is the default: a step then launches what it always did.
 * Row convention everywhere: rows 0 .. held - 1 are the recorded steps, oldest first; row `held` is the CURRENT generation.
 * The lineage of a current particle k: j_held = k, j_t = anc_t[j_{t + 1}]; its path is pose_t[j_t], then its current pose.
 * pk_upload_poses empties the ring (a replaced population has no lineage); pk_upload_pose does not (only the present changes).
 * While recording is on, the sharded protocol (pk_pack_particles, pk_adopt_particles, every pk_shard_* adoption,
 * pk_shard_state_dev) and the split step (pk_observe_staged_range) are refused with PK_ERR_STATE: lineages across ranks are
 * not recorded.  Every call below except pk_path_enable is PK_ERR_STATE while recording is off.
 *   pk_path_shape     capacity, rows held, rows ever recorded since pk_path_enable.  Any output may be NULL.
 *   pk_path_download  rows [t0, t1) of the held ones, n = t1 - t0: poses[n][P][3], ancestors[n][P].  Either may be NULL.
 *   pk_path_upload    replaces the ring by n <= capacity rows (snapshot restore, tests); recorded >= n is the counter to go on
 *                     from.  Any map is taken (ancestors need not be sorted); one outside [0, P) is PK_ERR_INVALID.
 *   pk_path_trace     the paths of the n listed current particles: out[n][held + 1][3].  Pure gathers: bit for bit what was
 *                     recorded.  n == 0 is fine.
 *   pk_path_summary   the smoothed path over the P lineages, every current particle counting once (pk_summary's convention:
 *                     behind a resample the population is the estimate; the weights are not read, so between two resamples of
 *                     an adaptively resampled filter it describes the population, not the posterior: pk_path_summary_weighted does).  Per row: mean[3] = mean x, mean y, circular mean
 *                     heading; spread[4] = var x, cov xy, var y, mean resultant length of the headings; survivors = the
 *                     number of distinct ancestors j_t the population still has in that row (exact).  The position moments
 *                     are taken about particle 0's lineage, so a row with ONE survivor has its recorded pose as mean, bit for
 *                     bit, and exactly zero spread.  Integer atomics and fixed-order sums only: the same bits on every call.
 *                     Any output may be NULL.
 *   pk_path_summary_weighted  the same path by the WEIGHTS of the current particles, w_k = exp(logw_k - shift) as
 *                     pk_summary_weighted takes them (weight_domain, shift: see adaptive resampling below): the estimate
 *                     between an observe and a resample.  mean[held + 1][3] and spread[held + 1][4] carry pk_path_summary's
 *                     figures and row convention; the variances are over S1 = sum w, the mean resultant length is hypot / S1;
 *                     n_eff = (S1 / S2) * S1 is ONE number, that of the current weights.  Row `held` is pk_summary_weighted's
 *                     estimate.  A particle of weight 0 contributes nothing.  Five launches whatever the ring holds (ONE
 *                     walks all rows): every thread walks its own particles' lineages back, so nothing is scattered -- no atomics at all, every sum in a
 *                     fixed order, the same bits on every call; a row all of whose lineages share one ancestor has its recorded
 *                     pose as mean, bit for bit, and exactly zero variances.  PK_ERR_INVALID for a bad domain; weights that sum to
 *                     zero or to a non-finite value: PK_ERR_STATE.  Any output may be NULL.  Changes no filter state; its
 *                     scratch (12 bytes per particle, the rows' partial sums) is allocated by the first call and released with
 *                     the ring.
 * pk_best_particle (needs no ring) hands out the index of the particle with the largest log-weight and that log-weight: the
 * lowest index among equals, a log-weight that is not a number never; PK_ERR_STATE when every one is.  All at -inf: index 0.
 * Deterministic, no atomics; either output may be NULL.  pk_path_trace of that index is the most likely particle's path. */
int pk_path_enable(pk_filter* f, int32_t capacity);
int pk_path_shape(const pk_filter* f, int32_t* capacity, int32_t* held, int64_t* recorded);
int pk_path_download(pk_filter* f, int32_t t0, int32_t t1, double* poses, int32_t* ancestors);
int pk_path_upload(pk_filter* f, int32_t n, int64_t recorded, const double* poses, const int32_t* ancestors);
int pk_path_trace(pk_filter* f, const int64_t* particles, int64_t n, double* out);
int pk_path_summary(pk_filter* f, double* mean, double* spread, int64_t* survivors);
int pk_path_summary_weighted(pk_filter* f, int32_t weight_domain, double* mean, double* spread, double* n_eff);
int pk_best_particle(pk_filter* f, int64_t* index, double* log_weight);

/* ---- the trunk: the whole run's path in bounded memory ("The trunk") ----------------------------------
 * A full ring overwrites its oldest row, and with it the start of the run.  With a trunk, a row's estimate is SETTLED into one
 * record of 13 doubles on the device before the row leaves the ring; the filter's whole path is then the trunk, the ring, the
 * current generation.  Off by default: a filter that does not ask for it holds, launches and returns what it always did.
 *   lo_t, hi_t   the lowest and highest lineage index j_t(k) of row t over ALL current particles, whatever their weight.  The
 *                row is FINAL iff lo_t == hi_t: every current particle descends from that one ancestor, and no later step can
 *                change the row's pose, pose_t[lo_t].  The final rows are a prefix of the ring.
 *   a trunk row  doubles 0-7: mean x, mean y, sum w sin h, sum w cos h, var x, cov xy, var y, S1 -- the row's estimate by the
 *                current particles' weights at the moment it was settled, bit for bit the numbers pk_path_summary_weighted
 *                takes for that row (the same weights, reference pose and order of every sum); 8, 9: lo_t, hi_t (exact);
 *                10-12: x, y, heading of pose_t[lo_t] as recorded.  It stands at global step index first_step + t, first_step =
 *                recorded - held of the ring at that moment.
 *   weighting    PK_WEIGHTS_LINEAR, PK_WEIGHTS_LOG, or PK_PATH_UNIFORM: every current particle counts once, w = 1.0 (the sums
 *                of PK_WEIGHTS_LOG with every log-weight 0).  Weights that sum to nothing leave NaN in doubles 0-7 of the rows
 *                that are not final; lo, hi and the pose are exact regardless.  Settling reads nothing back and refuses nothing
 *                on that account.
 * Settling E rows drops them from the ring (held -= E; `recorded` stays) and writes nothing else of the filter.  While the trunk
 * is on, trunk first_step + length == ring recorded - held at all times.  Five launches whatever the ring holds (the maximum
 * log-weight for PK_WEIGHTS_LOG, particle 0's lineage, the walk by index down to row E, the reduction of rows E - 1 .. 0, the
 * fold), no floating-point atomics, no host round trip.  The trunk's rows start at max(4 batch, 1024) and grow by doubling
 * (allocate, device-to-device copy, free): that is the ONLY synchronisation a settling step can ever meet.  All of it is counted
 * in pk_device_bytes; the scratch is pk_path_summary_weighted's, reserved by pk_path_trunk_enable.
 *   pk_path_trunk_enable    batch in [1, capacity] switches the trunk on: from then on the record that fills the ring (held ==
 *                     capacity behind it) settles the oldest `batch` rows at once, in the PK_T_RESAMPLE span, so that between
 *                     calls the ring holds capacity - batch .. capacity - 1 rows and overwrites nothing.  Behind pk_resample /
 *                     pk_step the weighting is PK_PATH_UNIFORM (behind a resample the population is the estimate); behind
 *                     pk_resample_adaptive / pk_step_adaptive it is that call's weight domain over the NEW generation's
 *                     log-weights (0 after a resample, carried over after a kept step: the verdict stays on the device).  A
 *                     ring that is full already stays full: pk_path_settle makes room, or else the next record first settles
 *                     `batch` rows by the generation it is about to record, every particle once (its lineages include the new
 *                     generation's: what is reported final is final).  batch 0 switches off and releases;
 *                     PK_ERR_STATE without a ring, PK_ERR_INVALID outside [0, capacity].  pk_path_enable (any capacity)
 *                     starts without a trunk; pk_upload_poses empties it and sets its first_step to `recorded`.
 *   pk_path_settle    the explicit form: settles held rows 0 .. rows - 1 by `weighting`.  PK_ERR_INVALID for rows outside
 *                     [0, held] or a bad weighting; rows == 0 is fine and launches nothing.
 *   pk_path_trunk_shape     batch, first_step, length.  Any output may be NULL.
 *   pk_path_trunk_download  the raw rows of global steps [s0, s1): rows[s1 - s0][13] -- what a snapshot carries.
 *   pk_path_trunk_upload    replaces the trunk by n rows from first_step on and sets recorded = first_step + n.  Only while the
 *                     ring holds no rows (PK_ERR_STATE otherwise); lo <= hi, both whole and in [0, P), else PK_ERR_INVALID.
 *   pk_path_trunk_summary   steps [s0, s1), n = s1 - s0, host arithmetic: mean[n][3], spread[n][4] in pk_path_summary_weighted's
 *                     convention, ancestors[n][2] = lo, hi.  A final row: the mean is doubles 10-12 as recorded, the spread
 *                     (0, 0, 0, 1).  Any output may be NULL.
 * With the trunk on, pk_path_upload must continue it: an empty trunk takes first_step = recorded - n, otherwise recorded - n must
 * equal the trunk's end (PK_ERR_INVALID, nothing changed); n == capacity settles `batch` rows at once, uniformly.  Every call here
 * but pk_path_trunk_enable is PK_ERR_STATE while the trunk is off. */
#define PK_PATH_UNIFORM 2
int pk_path_trunk_enable(pk_filter* f, int32_t batch);
int pk_path_settle(pk_filter* f, int32_t rows, int32_t weighting);
int pk_path_trunk_shape(const pk_filter* f, int32_t* batch, int64_t* first_step, int64_t* length);
int pk_path_trunk_download(pk_filter* f, int64_t s0, int64_t s1, double* rows);
int pk_path_trunk_upload(pk_filter* f, int64_t first_step, int64_t n, const double* rows);
int pk_path_trunk_summary(pk_filter* f, int64_t s0, int64_t s1, double* mean, double* spread, int64_t* ancestors);

/* One whole cam_cb without host synchronisation: reset weights, motion, observe,
 * resample.  Arguments as in the calls above. */
int pk_step(pk_filter* f, double v, double w, double dt, const double* z, uint64_t seed,
            uint64_t draw, const double* blobs, int32_t num_blobs, const int32_t* ids, double u,
            int32_t weight_domain);

/* ---- adaptive (selective) resampling: resample only when the weights have degenerated ("Adaptive
 * resampling").  The reference resamples behind every scan (prkt_core_v2.py:137); so do pk_resample and pk_step.  The calls below
 * decide on the device, so nothing crosses to the host in a step:
 *   shift  what the weight scan subtracts: the maximum log-weight in PK_WEIGHTS_LOG, 0 in PK_WEIGHTS_LINEAR, 0 when no weight is finite;
 *   w_p = exp(logw_p - shift),  S1 = sum w_p,  S2 = sum w_p^2,  n_eff = (S1 / S2) * S1  (that one float64 expression).
 *   S1 is the very sum pk_resample divides by P: the totals of the 1 024-particle scan blocks added in block order.  S2: per scan
 *   block four particles of a lane in order (fused multiply-adds), the wave by the xor butterfly, the four waves in order; then the
 *   blocks in block order.  No floating-point atomics: the same state gives the same bits on every call.
 *   KEEP iff n_eff >= threshold * (double)P, in float64.  NaN (every weight zero) fails the comparison: the call resamples, as
 *   pk_resample does.  threshold: finite and >= 0 (else PK_ERR_INVALID); 0 never resamples, anything above 1 always does.
 *   Resampled: ancestors, poses and map sources exactly pk_resample(u, weight_domain)'s from the same state; the new generation's
 *              log-weights are 0 (pk_resample itself carries the old ones along for the next observe to reset; the adaptive caller
 *              observes WITHOUT the reset -- pk_observe, not pk_observe_fresh).
 *   Kept:      poses and map sources carried over bit for bit, ancestor[k] = k, logw'_k = logw_k - shift (one rounded
 *              subtraction: a long run without a resample does not drive the linear weights of pk_download_poses to zero).
 *   Either way the ancestors are in place for the new-landmark bookkeeping (gathered by them) and, while pk_path_enable is on, ONE
 *   ring row is recorded per call -- a kept step records identity ancestors, so a row of the ring is then one call, not one resample.
 *   pk_path_summary still counts every current particle once: between two resamples it describes the population, not the posterior
 *   -- pk_path_summary_weighted is the path estimate by the weights.
 * pk_resample_adaptive  pk_resample's arguments, refusals and ancestors_out, plus the threshold.
 * pk_step_adaptive      pk_step with the weights carried over (no reset) and the gated resample: no host synchronisation.
 * pk_resample_stats     what the last gated call decided: out[4] = n_eff, S1, S2, shift; resampled = 1 / 0; counts[2] = gated calls,
 *                       resamples among them, since pk_create (kept on the device; this call reads them).  Any output may be NULL.
 *                       PK_ERR_STATE before the first gated call.
 * pk_weight_sums        out[2] = S1, S2 of the CURRENT weights, summed as above -- what the shards of a filter would add (as
 *                       pk_pose_sums is to pk_summary).  gmax: the filter-wide maximum log-weight for PK_WEIGHTS_LOG, NaN = this
 *                       handle's own; ignored for PK_WEIGHTS_LINEAR.  Changes no filter state (it scans in the resample's
 *                       workspace: not between pk_shard_block_totals and the pk_shard_offspring that reads that scan).
 * pk_summary_weighted   pk_summary by the weights: mean[3] = weighted mean x, mean y, circular mean heading; spread[4] = var x, cov xy,
 *                       var y (over S1) and the mean resultant length of the headings -- pk_path_summary's figures; n_eff.  The
 *                       position moments are taken about particle 0's pose and merged pairwise in a fixed order: particles that all
 *                       share a pose give it back bit for bit with exactly zero variances.  Weights that sum to zero or to a
 *                       non-finite value: PK_ERR_STATE.  Any output may be NULL.  Changes no filter state. */
int pk_resample_adaptive(pk_filter* f, double u, int32_t weight_domain, double threshold, int64_t* ancestors_out);
int pk_step_adaptive(pk_filter* f, double v, double w, double dt, const double* z, uint64_t seed, uint64_t draw,
                     const double* blobs, int32_t num_blobs, const int32_t* ids, double u, int32_t weight_domain,
                     double threshold);
int pk_resample_stats(pk_filter* f, double out[4], int32_t* resampled, int64_t counts[2]);
int pk_weight_sums(pk_filter* f, int32_t weight_domain, double gmax, double out[2]);
int pk_summary_weighted(pk_filter* f, int32_t weight_domain, double mean[3], double spread[4], double* n_eff);

/* ---- the odometry motion model ("The odometry motion model") -------------------------------------------
 * The reference declares FastSLAM.odom_motion_update (prkt_core_v2.py:140-146) and leaves it empty; pk_motion moves the particles
 * by a commanded twist only.  These calls move them by the CHANGE between two odometry poses instead: the model of Thrun, Burgard,
 * Fox, Probabilistic Robotics, Table 5.6 -- rotate by rot1, translate by trans, rotate by rot2 -- with four noise parameters.
 *   wrap(a) = remainder(a, 2 pi) (IEEE): into [-pi, pi]; the one wrap every angle below goes through.
 *   delta of prev = (x, y, th), now = (x', y', th'):
 *     trans = hypot(x' - x, y' - y);  dth = wrap(th' - th)
 *     rot1  = trans < min_trans ? 0 : wrap(atan2(y' - y, x' - x) - th);  rot2 = wrap(dth - rot1)
 *   min_trans guards the turn in place, where atan2 of a vanishing translation is noise: below it the translation is applied along
 *   the current heading.  The heading stays exact; the position is off by 2 trans sin(phi / 2), phi the angle between the heading
 *   and the direction that was dropped: at most min_trans for a creep within 60 degrees of the heading, never more than
 *   2 trans < 2 min_trans (a creep backwards, applied forwards).  min_trans = 0: no guard.
 *   sigmas of a delta, alpha = (a1, a2, a3, a4); rotations are folded so that driving backwards (rot1 near +-pi) is not taken
 *   for a large turn, r1n = min(|rot1|, pi - |rot1|), r2n likewise:
 *     sigma_rot1 = sqrt(a1 r1n^2 + a2 trans^2);  sigma_trans = sqrt(a3 trans^2 + a4 (r1n^2 + r2n^2));
 *     sigma_rot2 = sqrt(a1 r2n^2 + a2 trans^2)     -- the same for every particle: formed once, on the host.
 *   the sample, per particle with standard normals z0, z1, z2:
 *     r1 = rot1 - sigma_rot1 z0;  t = trans - sigma_trans z1;  r2 = rot2 - sigma_rot2 z2
 *     x += t cos(h + r1);  y += t sin(h + r1);  h = wrapped((h + r1) + r2), to (-pi, pi] as pk_motion leaves it.
 * pk_odom_delta, pk_odom_sigmas   host only, no filter: delta[3] = (rot1, trans, rot2); sigma[3] = (rot1, trans, rot2).
 * pk_motion_odom         pk_motion for a delta: z and (seed, draw) as there -- the Philox counters and keys are pk_motion's, so the
 *                        normals of (particle, seed, draw) are the same in both -- in the PK_T_MOTION span; a staged scan rides
 *                        the launch.
 * pk_motion_odom_range   pk_motion_range for a delta: the particles [p0, p1), device noise.
 * pk_step_odom           pk_step with pk_motion_odom for its motion; threshold NaN: pk_step's reset and resample, else
 *                        pk_step_adaptive's carried weights and gate.
 * PK_ERR_INVALID, nothing changed: NULL arguments, a delta that is not finite or has trans < 0, an alpha or min_trans that is not
 * finite or negative, a bad particle range, a bad threshold. */
int pk_odom_delta(const double prev[3], const double now[3], double min_trans, double delta[3]);
int pk_odom_sigmas(const double delta[3], const double alpha[4], double sigma[3]);
int pk_motion_odom(pk_filter* f, const double delta[3], const double alpha[4], const double* z, uint64_t seed, uint64_t draw);
int pk_motion_odom_range(pk_filter* f, const double delta[3], const double alpha[4], uint64_t seed, uint64_t draw, int64_t p0,
                         int64_t p1);
int pk_step_odom(pk_filter* f, const double delta[3], const double alpha[4], const double* z, uint64_t seed, uint64_t draw,
                 const double* blobs, int32_t num_blobs, const int32_t* ids, double u, int32_t weight_domain, double threshold);

/* ---- the measurement-informed proposal (FastSLAM 2.0 sampling) ----
 * pk_motion + pk_observe draw every pose from the motion model alone and let the scan only weigh it (FastSLAM 1.0).  These calls
 * draw it from the motion model CONDITIONED on the scan, in the space of the three standard normals xi the motion kernels consume
 * (prior N(0, I)); s = the sigmas of the launch (pk_motion's sd, sh, sh; pk_odom_sigmas), g = the motion model as it stands:
 *   1. predicted pose x^ = g(x-, u, 0): the same kernel with normals 0.
 *   2. G = d pose / d (s . xi) at 0, closed form, h1 the heading the translation is made along:
 *        twist     h1 = h^ - w dt / 2, ds = v dt: columns (cos h1, sin h1, 0), (-ds sin h1, ds cos h1, 1), (0, 0, 1)
 *        odometry  h1 = h^ - rot2, t = trans:     columns (t sin h1, -t cos h1, -1), (-cos h1, -sin h1, 0), (0, 0, -1)
 *   3. association at x^ (the bearing model's kernels, or ids); tentative ids are settled there against the untouched landmarks,
 *      a dropped id becomes 0.
 *   4. every settled match b -> j, j not potential, against j's state BEFORE the scan (a landmark matched by several blobs gives
 *      each of them against that same state): dx = fx - x^, dy = fy - y^, q = dx^2 + dy^2, nu = wrap(beta - (atan2(dy, dx) - h^)),
 *      h_x = (dy / q, -dx / q, -1), h_m = (-dy / q, dx / q) (both 0 at q = 0), sigma^2 = h_m' P h_m + Q00, a = s . (G' h_x);
 *      Lambda += a a' / sigma^2, eta += a nu / sigma^2, c += nu^2 / sigma^2, l += log sigma^2,
 *      kappa += log det(C + Qc) + d_c' (C + Qc)^-1 d_c, n += 1.
 *   5. Lambda <- I + Lambda = R R' (Cholesky), m = Lambda^-1 eta; xi = m + R^-T z, z the normals the motion kernel would have drawn
 *      (z[3 p ..], or the Philox draws of (particle, seed, draw)); the weight increment
 *        dlogw = -2 n log 2 pi - (l + log det Lambda) / 2 - (c - eta' m) / 2 - kappa / 2 + (unmatched + potential matches) log 0.1
 *      is the Gaussian marginal of the stacked innovations under the joint linearisation.  No settled match: xi = z bit for bit.
 *   6. the sampled pose is the motion kernel's for x- with normals xi, bit for bit (pk_motion / pk_motion_odom with z = xi).
 *   7. the landmarks are updated at the sampled pose by the bearing model's EKF with the settled ids, in scan order; the log-weight
 *      becomes (fresh ? 0 : old) + dlogw (the updates' own importance factors are not added).
 * pk_propose        one pk_motion(v, w, dt, z, seed, draw) plus one pk_observe(blobs, num_blobs, ids, ids_out) (fresh != 0:
 *                   pk_observe_fresh) under that rule.  No resample: pk_resample, pk_resample_adaptive, the path and the summaries
 *                   follow as ever.  pk_observe_route: PK_ROUTE_KNOWN_IDS with ids, else PK_ROUTE_ML_GENERAL.  k_propose is timed in
 *                   PK_T_PROPOSE, the rest in the spans of the plain calls.
 * pk_propose_odom   the same for an odometry delta: pk_motion_odom(delta, alpha, z, seed, draw).
 * pk_proposal_download  the last call's per-particle results: xi[P][3], dlogw[P], used[P] (the matches of step 4); any may be NULL.
 *                   PK_ERR_STATE before the first call.
 * The first call allocates 84 P bytes of state (pk_device_bytes: ten rows of P doubles, one of P int32).  The scan itself uses the
 * buffers a pk_observe of the same scan uses -- the id table of a maximum-likelihood scan, and the per-scan block, which with supplied
 * ids also carries the id row (4 num_blobs bytes more than pk_observe's, where that makes the block grow).  A filter that never
 * calls them allocates and launches what it did.  The limits of a maximum-likelihood pk_observe (65 535 blobs, the LDS chains of
 * landmarks + 2 x blobs) hold for maximum-likelihood scans here; supplied ids have neither.
 * Refused, nothing changed -- PK_ERR_UNSUPPORTED: a filter not on PK_MODEL_BEARING (the reference model's Jacobian is not one), the
 * dense layout, growing maps or retirement (pk_grow_enable, pk_grow_retire) unless pk_proposal_grow is on, a shard of a sharded
 * filter or a split step in progress;
 * PK_ERR_STATE: a staged scan in flight (pk_stage_scan), no map; PK_ERR_INVALID: the arguments, as pk_motion / pk_motion_odom /
 * pk_observe refuse them. */
int pk_propose(pk_filter* f, double v, double w, double dt, const double* z, uint64_t seed, uint64_t draw, const double* blobs,
               int32_t num_blobs, const int32_t* ids, int32_t fresh, int32_t* ids_out);
int pk_propose_odom(pk_filter* f, const double delta[3], const double alpha[4], const double* z, uint64_t seed, uint64_t draw,
                    const double* blobs, int32_t num_blobs, const int32_t* ids, int32_t fresh, int32_t* ids_out);
int pk_proposal_download(pk_filter* f, double* xi, double* dlogw, int32_t* used);

/* Ranges in the proposal ("Ranges in the proposal"): an opt-in mode of pk_propose / pk_propose_odom.  Off (the
 * default) they refuse armed ranges (pk_scan_ranges) as ever.  On, with nothing armed, they do what they did, bit for bit; with ranges
 * armed they consume them -- pk_scan_ranges' own refusals first (num_blobs, the model, the dense layout, growing maps), then the
 * proposal's; a refused call changes nothing and the ranges are gone -- and the rule above becomes, for a blob with a finite range
 * (rho, q_rho); a blob without one (NaN) is handled exactly as above, blob by blob:
 *   3. association at x^ by the range kernels (the density at the measured point); a tentative id of a ranged blob is settled there too;
 *   4. r^ = sqrt(q), nu = (wrap(beta - (atan2(dy, dx) - h^)), rho - r^), h_x = [[dy / q, -dx / q, -1], [-dx / r^, -dy / r^, 0]],
 *      h_m = [[-dy / q, dx / q], [dx / r^, dy / r^]] (all 0 at q = 0), S2 = h_m P h_m' + diag(Q00, q_rho), A (2 x 3) with rows
 *      s . (G' h_x); Lambda += A' S2^-1 A, eta += A' S2^-1 nu, c += nu' S2^-1 nu, l += log det S2, kappa and n as above, n_rho += 1;
 *   5. dlogw = -(2 n + n_rho / 2) log 2 pi - ... as above: the Gaussian marginal of the stacked innovations, 1 x 1 and 2 x 2 blocks;
 *   7. the update at the sampled pose takes the range-bearing EKF (pk_scan_ranges' update) for a ranged blob.
 * A scan in which some blob has a range takes k_propose_range and k_observe_proposed_range and may grow the per-scan block by 32
 * bytes a blob, as in pk_observe; an armed scan without a finite range stages, launches and computes what the unarmed call does.
 * pk_proposal_ranges_state: *on = 1 or 0. */
int pk_proposal_ranges(pk_filter* f, int32_t on);
int pk_proposal_ranges_state(const pk_filter* f, int32_t* on);

/* The proposal on growing maps ("The proposal on growing maps"): an opt-in mode of pk_propose / pk_propose_odom.
 * Off (the default) they refuse a filter with pk_grow_enable or pk_grow_retire on, as ever.  On (on = 1; anything but 0 or 1 is
 * PK_ERR_INVALID and changes nothing), a filter without either does what it did, bit for bit, and a growing filter runs steps 1-7
 * above unchanged, with two steps behind them:
 *   3. the association sees the untouched state, spare slots included; with ranges it is "Ranges in the proposal"'s;
 *   4. only settled matches to CONFIRMED landmarks condition the draw: a match to a potential feature is updated at the sampled
 *      pose and weighs log 0.1, as does a blob nobody matched;
 *   8. behind the update, pk_observe's new-landmark bookkeeping at the SAMPLED pose on the settled ids (0 = unmatched), by the rule
 *      pk_grow_init selected; with pk_grow_ranges on it takes the scan's ranges -- a ranged unmatched blob becomes a potential
 *      feature at once, at the sampled pose + rho u;
 *   9. then pk_grow_retire's pass, its clock advanced, as behind pk_observe.
 * An empty scan (num_blobs = 0): xi = z, no bookkeeping, and the retirement clock stands still.  The resample, the path, the
 * adaptive gate and the summaries follow unchanged.  The new launches are timed in PK_T_OBSERVE.
 * Refused on a growing filter with the mode on, nothing changed and armed ranges gone, in this order: the ranges' own refusals
 * (armed ranges need pk_proposal_ranges and pk_grow_ranges: without the former the proposal's refusal of ranges answers, without
 * the latter pk_scan_ranges' refusal 4), the proposal's, then supplied ids with num_blobs > 0 -- PK_ERR_STATE, in pk_observe's
 * words: the bookkeeping follows the maximum-likelihood association.
 * The mode holds no device memory (pk_device_bytes is what it was).  pk_proposal_grow_state: *on = 1 or 0. */
int pk_proposal_grow(pk_filter* f, int32_t on);
int pk_proposal_grow_state(const pk_filter* f, int32_t* on);

/* Unique association ("Unique association"; the reference's unwritten "Version 2: match each scan to a unique
 * feature", prkt_core_v2.py:317-351): an opt-in mode in which at most one blob of a scan keeps each landmark of a particle.
 * The rule, per particle: with p(b, l) the association's own match probability (for a blob with a finite range, the measured
 * point's) on the untouched landmark state at the live pose, the pairs with p > 0 are walked by p descending, then blob ascending
 * (scan order), then landmark ascending (preset first, then spare slots), and a pair is taken iff neither its blob nor its landmark
 * has been; ids[b] is the taken landmark's id, or 0.  A particle whose maximum-likelihood ids claim no landmark twice keeps them,
 * element for element.  A blob that ends 0 is an unmatched blob in every respect (log 0.1; on a growing filter the new-landmark
 * bookkeeping takes it), and a landmark is updated at most once per scan.
 * Off (the default): every call launches and computes what it did, bit for bit, and pk_device_bytes is what it was.
 * On (on = 1; anything but 0 or 1 is PK_ERR_INVALID, PK_ERR_STATE inside a split observe; nothing changed either way; 64 bytes
 * of counters from the first time): the maximum-likelihood scans of pk_observe, pk_observe_fresh, pk_observe_staged, pk_step,
 * pk_step_adaptive, pk_step_odom and pk_associate take the general route under both measurement models (PK_ROUTE_ML_GENERAL; either
 * association kernel, finalising), k_assoc_unique settles the ids in place in the PK_T_ASSOC span, and k_observe*, the
 * bookkeeping and retirement follow on the settled ids, which ids_out returns.  Supplied ids are applied as ever.
 * Refused while it is on, PK_ERR_UNSUPPORTED, nothing changed, armed ranges gone: a maximum-likelihood scan on the dense layout;
 * pk_observe_staged_range; pk_propose / pk_propose_odom (k_propose settles its own tentative ids); a scan whose tables
 * (12 bytes per padded landmark + 14 per blob) exceed the workgroup's LDS.  pk_step, pk_step_adaptive and pk_step_odom are refused
 * ahead of their motion: no particle has moved.
 * pk_assoc_unique_stats: of the last scan whose association went through the pass -- particles with a conflict, blobs whose id
 * changed, of those the ones matched to another landmark (the rest ended 0), the most passes any particle took (1: no conflict
 * anywhere) --, zeros when the last observe was not in the mode; synchronises.  The pass is bounded at num_blobs + 1 passes per
 * particle; a particle that reached the bound (a device error: no input does) stops with the ids it has, and the next
 * synchronising call of pk_synchronize, pk_assoc_unique_stats, pk_associate or an observe with ids_out fails with PK_ERR_HIP. */
int pk_assoc_unique(pk_filter* f, int32_t on);
int pk_assoc_unique_state(const pk_filter* f, int32_t* on);
int pk_assoc_unique_stats(pk_filter* f, int64_t out[4]);

/* ---- sharded (multi-GPU) resampling: see DESIGN.md section 6 -------------------
 * Particles are sharded contiguously over one process per GPU; global particle index =
 * global_offset + local index.  The collectives themselves are the caller's
 * (torch.distributed over RCCL); the entry points below only read/write host scalars and
 * arrays, plus one caller-owned device buffer for the particles that migrate.
 * pk_set_shard: index of local particle 0 in the whole filter (keys the Philox counters so
 * the motion noise does not depend on the shard count). */
int pk_set_shard(pk_filter* f, int64_t global_offset);
/* max over the shard of log(weight). */
int pk_shard_max_logw(pk_filter* f, double* max_logw);
/* Number of weight-scan blocks of the shard (1024 particles each) and their totals of
 * exp(logw - gmax) (PK_WEIGHTS_LOG) or exp(logw) (PK_WEIGHTS_LINEAR); also leaves the
 * block-local inclusive scans on the device for pk_shard_offspring. */
int64_t pk_shard_num_blocks(const pk_filter* f);
int pk_shard_block_totals(pk_filter* f, double gmax, int32_t weight_domain, double* totals);
/* Given every shard's block totals concatenated in rank order, this shard's first block and
 * the global particle count: slot_hi[0] = number of output slots filled by all earlier
 * shards, slot_hi[1 + j] = that number after local particle j; i.e. local particle j is the
 * ancestor of the global output slots [slot_hi[j], slot_hi[j + 1]).  Same arithmetic as
 * pk_resample, so G shards reproduce the 1-GPU ancestors when shards are multiples of 1024.
 * last_shard: this is the highest rank (its last particle absorbs the clamped tail). */
int pk_shard_offspring(pk_filter* f, const double* global_totals, int64_t n_global_blocks,
                       int64_t first_block, int64_t global_particles, double u, int32_t last_shard,
                       int64_t* slot_hi);
/* Bytes of one migrating particle record: a 64-byte header (x, y, heading, log weight, slot_lo, slot_hi, the logical index of the
 * child in slot_lo, 0) + its landmark slot + -- while the new-landmark bookkeeping is on (pk_grow_enable) -- the particle's
 * counters, spare-slot ids and stored readings behind the slot. */
int64_t pk_particle_bytes(const pk_filter* f);
/* Pack the listed local particles into dev_buf (device pointer owned by the caller, e.g. a
 * torch tensor), n records of pk_particle_bytes. */
int pk_pack_particles(pk_filter* f, const int64_t* local_idx, int64_t n, void* dev_buf);
/* New generation of the shard: slot k takes local particle src[k] (>= 0) or received record
 * -(src[k]) - 1 of dev_buf.  Poses are gathered now; adopted landmark slots are read in place
 * from dev_buf by the next pk_observe / pk_associate / download, so dev_buf must stay alive
 * and unchanged until one of those has run. */
int pk_adopt_particles(pk_filter* f, const int64_t* src, const void* dev_buf, int64_t n_received);

/* Device-resident variants of the same protocol: every buffer is a DEVICE pointer owned by the
 * caller (torch tensors the collectives run on), nothing is copied to the host and nothing
 * synchronises the stream.  plan: leaves the offspring table on the device and writes
 * dev_ranges[2 d], [2 d + 1] = the contiguous local particles [j0, j1) whose offspring overlap
 * rank d's output slots.  pack: records of those particles for every rank but `rank`, in rank
 * order (`ranges` is the host copy of dev_ranges); each record header carries the destination
 * slots [lo, hi) it fills, so no per-particle metadata travels separately.  adopt: builds the
 * new generation from the local table and the received records (source-rank order). */
int pk_shard_max_logw_dev(pk_filter* f, double* dev_out);
int pk_shard_block_totals_dev(pk_filter* f, const double* dev_gmax, int32_t weight_domain,
                              double* dev_totals);
int pk_shard_plan_dev(pk_filter* f, const double* dev_global_totals, int64_t n_global_blocks,
                      int64_t first_block, int64_t global_particles, double u, int32_t last_shard,
                      int32_t world, int64_t* dev_ranges);
/* Debug / test entry (round 4; nothing in the reference: the exchange belongs to the multi-GPU resample of prkt_core_v2.py:210-252):
 * pack the local particles [j0, j1) of the planned resample as exchange records whose slot ranges are clipped to the GLOBAL slots
 * [slot_lo, slot_hi) -- what pk_shard_pack_dev does per destination rank, for an arbitrary slot interval.  With the options
 * "split_loopback_lo" / "split_loopback_hi" (local slot bounds; pk_set_option) a single rank can send records of its OWN
 * particles through the all-to-all to itself and adopt them with pk_shard_adopt_remote_dev: pack -> all_to_all_single(async) ->
 * wait -> adopt with records that really travelled, on one device (tests/test_gpu_sharded.py). */
int pk_shard_pack_slots_dev(pk_filter* f, int64_t j0, int64_t j1, int64_t slot_lo, int64_t slot_hi, void* dev_buf);
/* The same plan for shards of ANY size (the block-total plan above reproduces the 1-GPU ancestors only when shards are
 * multiples of the 1024-particle scan block): the ranks all-gather their log-weights (pk_shard_logw_dev copies the shard's
 * into a caller buffer), and every rank runs the 1-GPU scan kernels on the whole array -- same blocks, same additions,
 * same bits on every rank and as on one GPU -- then derives its own particles' output slots.  8 B per particle of the
 * whole filter travel per resample (the migrating particles' maps are 10^4 times that).
 * pk_shard_download_offspring: the plan's table slot_hi[P + 1] (as pk_shard_offspring returns it), for tests. */
int pk_shard_logw_dev(pk_filter* f, double* dev_out);
int pk_shard_plan_global_dev(pk_filter* f, const double* dev_global_logw, int64_t global_particles, const double* dev_gmax,
                             int32_t weight_domain, double u, int32_t last_shard, int32_t world, int64_t* dev_ranges);
int pk_shard_download_offspring(pk_filter* f, int64_t* slot_hi);
int pk_shard_pack_dev(pk_filter* f, const int64_t* ranges, int32_t world, int32_t rank, void* dev_buf);
int pk_shard_adopt_dev(pk_filter* f, int32_t rank, const void* dev_recv, int64_t n_received);

/* The split step of the sharded filter: the exchange of the migrating particles (each a whole map) runs while the
 * particles that stay on this rank are already being worked on.  The output slots a shard fills with its OWN particles form
 * one contiguous run (ancestors are monotone in the slot index): pk_shard_local_span_dev copies its two global bounds
 * (slot_hi[0], slot_hi[P] of the plan) into a caller's device buffer; pk_shard_adopt_local_dev makes the new generation
 * current with those slots filled, pk_shard_adopt_remote_dev fills the others from the received records;
 * pk_motion_range / pk_observe_staged_range are pk_motion (device noise) / pk_observe_staged on the particles [p0, p1) only:
 * `first` consumes the staged scan (it must take the register route: pk_staged_takes_regs), `last` runs what the one-pass
 * kernel flagged over ALL particles and closes the step.  The reference has one process (prkt_core_v2.py:59-137). */
int pk_shard_local_span_dev(pk_filter* f, int64_t* dev_out2);
int pk_shard_adopt_local_dev(pk_filter* f, int32_t rank);
int pk_shard_adopt_remote_dev(pk_filter* f, int32_t rank, const void* dev_recv, int64_t n_received);
int pk_motion_range(pk_filter* f, double v, double w, double dt, uint64_t seed, uint64_t draw, int64_t p0, int64_t p1);
int pk_staged_takes_regs(pk_filter* f); /* 1: the staged scan will take k_step_regs, 0: not (or nothing staged) */
int pk_observe_staged_range(pk_filter* f, int32_t fresh, int64_t p0, int64_t p1, int32_t first, int32_t last);

/* ---- balanced placement of the sharded filter: minimum migration (round 5) ----------------------
 * The exchange above gives rank r the output slots [r P, (r + 1) P) of prkt_core_v2.py:233-250's ordered walk, so every rank
 * boundary moves by the cumulative imbalance of the ranks below it, and it packs every particle of a contiguous index
 * range, with or without children.  Here the ORDER of that walk is decoupled from where a particle lives: every physical
 * slot carries the LOGICAL index of its particle -- its index in one filter holding all of them; the Philox counters of
 * pk_motion and the weight scan are keyed by it, so the results stay those of one filter, bit for bit -- a rank keeps its
 * own children (in its slots [0, m)), and only a rank's EXCESS children travel, to whichever rank has free slots; only
 * particles that HAVE children there are packed.
 *   pk_shard_state_dev          this rank's row for the ONE all-gather of a resample: [logw(P) | logical(P) as int64 bits]
 *   pk_shard_plan_balanced_dev  from all ranks' rows (rank-major, 2 P words each): the 1-GPU weight scan in logical order, the
 *                               offspring table, and the whole plan -- every rank derives it by itself.  dev_table: world rows
 *                               of 2 world + 4 int64: per destination the range [a0, a1) of the row's rank's particles WITH
 *                               children that it sends there, then n (children), m = min(n, P), ebase, dbase (running sums of
 *                               the excess n - m and of the free slots P - m).  The caller reads the table on the host (it
 *                               sizes the all-to-all) and hands it back to the two calls below.
 *   pk_shard_pack_balanced_dev  the records for every other rank, destination-major; header = x, y, h, logw, lo, up, klo:
 *                               the copy fills the destination's slots [lo, up), the child in slot k is logical klo + k - lo
 *   pk_shard_adopt_balanced_dev mode 0: the whole new generation; 1: the slots [0, m) from this rank's own particles (the
 *                               generation becomes current); 2: the slots [m, P) from the received records (after mode 1:
 *                               the split step works on [0, m) while the records travel)
 *   pk_shard_download_logical / pk_shard_reset_placement (slot j <- logical pk_set_shard's offset + j) /
 *   pk_shard_download_balanced_offspring (the plan's table H[P_global + 1], tests) / pk_shard_balanced_errors (kernel-side
 *   consistency failures: must stay 0).
 * Once pk_shard_state_dev has run on a filter, pk_resample and the contiguous adoptions refuse it (PK_ERR_STATE). */
int pk_shard_state_dev(pk_filter* f, double* dev_out);
int pk_shard_plan_balanced_dev(pk_filter* f, const double* dev_global_state, int64_t global_particles, const double* dev_gmax,
                               int32_t weight_domain, double u, int32_t world, int32_t rank, int64_t* dev_table);
int pk_shard_pack_balanced_dev(pk_filter* f, const int64_t* table, int32_t world, int32_t rank, void* dev_buf);
int pk_shard_adopt_balanced_dev(pk_filter* f, const int64_t* table, int32_t world, int32_t rank, const void* dev_recv,
                                int64_t n_received, int32_t mode);
/* debug (one-rank tests of the balanced exchange over RCCL): with the option "balanced_loopback_keep" = keep set, the next balanced
 * adoption fills only the slots [0, keep) with the rank's own children; its children from position keep on travel as records -- packed
 * here for the particles alive[a0, a1) with the same 64-byte header (and bookkeeping tail) another rank would get -- through the
 * all-to-all to the rank itself and are adopted into [keep, P) from the receive buffer. */
int pk_shard_pack_balanced_loop_dev(pk_filter* f, int64_t keep, int64_t a0, int64_t a1, void* dev_buf);
int pk_shard_download_logical(pk_filter* f, int64_t* logical);
/* tests of the planner in isolation (tests/test_gpu_sharded.py): the placement set from the host -- slot j holds logical particle
 * logical[j] --, and this rank's tables of the last plan: rel[P + 1] (children of its particles [0, j)), Hl[P] (first output slot of
 * particle j's children), alive[P] (its particles with children, ascending; -1 behind the last) */
int pk_shard_upload_logical(pk_filter* f, const int64_t* logical);
int pk_shard_download_balanced_plan(pk_filter* f, int64_t* rel, int64_t* Hl, int32_t* alive);
int pk_shard_reset_placement(pk_filter* f);
int pk_shard_download_balanced_offspring(pk_filter* f, int64_t global_particles, int64_t* H);
int pk_shard_balanced_errors(pk_filter* f, int64_t* count);

/* ---- single-triple probe ------------------------------------------------------
 * Runs the device functions the kernels are built from on ONE (pose, landmark, blob):
 * the scalar methods of FilterParticle the reference's unit tests call.
 * out[PK_PROBE_LEN]:
 *   [0] probability_of_match :383      [1] prob_position_match :457
 *   [2..3] closest_point :496          [4] prob_color_match :524
 *   [5..8] generate_measurement :859   [9..10] measurement_jacobian H[0][0], H[0][1] :748
 *   [11..26] measurement_covariance Q 4x4 :804
 *   [27..46] kalman_gain K 5x4 :821    [47] importance_factor :835
 *   [48..52] updated mean :897         [53..77] updated covariance 5x5 :916
 *   [78] log importance factor */
#define PK_PROBE_LEN 79
int pk_probe(int32_t device, const double pose[3], const double mean[5], const double cov[25],
             const double blob[4], const double Qt[16], double* out);

/* ---- math probe ---------------------------------------------------------------
 * Runs ONE of the float64 primitives the observe kernels are built from (pk_math.hpp, pk_pub_math.hpp, pk_device.hpp) on n
 * rows of arguments, one element per thread: in[n][arity] -> out[n][outputs], row-major.  Diagnostic: the tests hold each
 * primitive to an exact reference through it.  n == 0 returns PK_OK without a launch.
 *   op                        calls                                    arity -> outputs
 *   PK_MATH_LOG_FEW_ULP       log_few_ulp(x)                           1 -> 1
 *   PK_MATH_PUB_LOG           pub_log(x)                               1 -> 1
 *   PK_MATH_PUB_RECIP         pub_recip(x)                             1 -> 1
 *   PK_MATH_ATAN2             pk_atan2(y, x)                           2 -> 1
 *   PK_MATH_ROUND_DOWN_F32    (double)pub_round_down_to_float(x)       1 -> 1
 *   PK_MATH_KEY               double_to_key(x), key_to_double of it    1 -> 2  (both as 64 raw bits in a double's place)
 *   PK_MATH_FAR_BOUND         pub_far_bound(landmark)                  14 -> 2 (mean x y r g b, pxx pxy pyy, crr crg crb cgg cgb
 *                                                                               cbb -> fk, fi)
 *   PK_MATH_PR_FROM_PARTS     pr_from_parts(det2, det3, num2, num3)    4 -> 1
 *   PK_MATH_EKF_UPDATE        ekf_update(landmark, pose, blob, Qt)     31 -> 17
 *       in:  sx sy | the 14 landmark fields as above | count (an integer-valued double, PK_LANDMARK_POTENTIAL included) |
 *            blob bearing r g b | Qt as q00 rr rg rb gg gb bb | zhat0 | flags | prod_in
 *            flags (an integer-valued double): bit 0 immutable, bit 1 zhat0 is passed as the known expected bearing, bit 2 the
 *            colour block is left as it was (the table mode's call), bit 3 the one-logarithm-per-lane form (the squared
 *            Frobenius norm is multiplied into prod, its logarithm left out of the returned value)
 *       out: the returned log weight | the 14 fields afterwards | the count afterwards | prod afterwards
 *   PK_MATH_MATCH             the match probabilities                  23 -> 5
 *       in:  sx sy heading | the 14 landmark fields | blob bearing r g b | ux uy (the blob's unit ray)
 *       out: probability_of_match | prob_position_match (pse = pk_atan2 of the offset) | prob_color_match | closest_point x y
 * The last two are held to an exact dense reference by tests/test_gpu_ekf_reference.py (record: profiles/r10/ekf_errors.json). */
enum {
  PK_MATH_LOG_FEW_ULP = 0,
  PK_MATH_PUB_LOG = 1,
  PK_MATH_PUB_RECIP = 2,
  PK_MATH_ATAN2 = 3,
  PK_MATH_ROUND_DOWN_F32 = 4,
  PK_MATH_KEY = 5,
  PK_MATH_FAR_BOUND = 6,
  PK_MATH_PR_FROM_PARTS = 7,
  /* 8 is no op and never will be: the call carries no buffer lengths, and callers written while 8 was the first
   * unknown op pass it with buffers of a few doubles to see it refused -- an op there would write 17 doubles a row
   * past the end of theirs */
  PK_MATH_EKF_UPDATE = 9,
  PK_MATH_MATCH = 10,
  PK_MATH_COUNT = 11 /* one past the last op */
};
int pk_probe_math(int32_t device, int32_t op, int64_t n, const double* in, double* out);

/* The same for the bearing model's primitives (PK_MODEL_BEARING), an entry point of their own: in[n][arity] -> out[n][outputs].
 *   what  calls                    arity -> outputs
 *   0     the match probabilities  23 -> 5   PK_MATH_MATCH's row; ux uy is the blob's ROBOT-frame unit ray, which the kernel turns by
 *                                            the heading before it calls closest_point
 *   1     the update               32 -> 17  PK_MATH_EKF_UPDATE's row with the heading behind sx sy:
 *         in:  sx sy heading | the 14 landmark fields | count | blob bearing r g b | Qt as q00 rr rg rb gg gb bb | zhat0 | flags | prod_in
 *              flags: bit 0 immutable, bit 1 zhat0 is passed as the known pk_atan2(dy, dx) (the heading is subtracted inside);
 *              any other bit is PK_ERR_INVALID.  prod_in comes back unchanged.
 * PK_ERR_INVALID for any other `what`. */
int pk_probe_bearing(int32_t device, int32_t what, int64_t n, const double* in, double* out);

/* The same for range-bearing blobs (pk_scan_ranges): pk_probe_bearing's rows with the blob's range and its variance behind them.  A
 * NaN range takes the bearing model's functions, as in the kernels.
 *   what  calls                    arity -> outputs
 *   0     the match probabilities  26 -> 5   in:  pk_probe_bearing's 23 | range | range variance | Qt[0][0]
 *                                            out: probability_of_match | position | colour | the point the position density was
 *                                                 taken at, x y (the measured point; the closest point for a NaN range)
 *   1     the update               33 -> 16  in:  pk_probe_bearing's 31 without prod_in (... | zhat0 | flags) | range | range variance
 *                                            out: log-weight | the 14 landmark fields | count
 * PK_ERR_INVALID for any other `what`, and for flags beyond bits 0 and 1. */
int pk_probe_range(int32_t device, int32_t what, int64_t n, const double* in, double* out);

/* ---- instrumentation ----------------------------------------------------------
 * Kernel launches of the enabled PK_T_* slots are bracketed by hipEvents on the handle's
 * stream: `mask` bit i enables slot i, a negative mask enables all, 0 disables.  pk_timings synchronises, then returns accumulated milliseconds and launch
 * counts per PK_T_* slot since the last pk_reset_timings. */
int pk_enable_timing(pk_filter* f, int32_t mask);
int pk_reset_timings(pk_filter* f);
/* (Both arrays hold PK_T_COUNT entries -- 8 since PK_T_PROPOSE was appended, 7 before: see the enum.) */
int pk_timings(pk_filter* f, double ms[PK_T_COUNT], int64_t launches[PK_T_COUNT]);
/* Algorithmic HBM bytes of one observe launch (14 scalars read + 14 written per
 * particle.landmark) and the bytes the layout actually moves (adds update_count, ids). */
int pk_observe_bytes(const pk_filter* f, int32_t num_blobs, int64_t* algorithmic, int64_t* moved);
/* The colour table (options "colour_table": -1 auto (default), 0 off, 1 as auto; "colour_table_depth": levels, default 1024, read at the
 * first scan in the mode behind a pk_upload_map; "colour_table_margin": levels short of the table's end at which the host leaves the
 * mode, -1 (default) min(16, depth / 2), 0 never -- levels beyond the table are then worked out by the kernels themselves, exact and slow).
 * While every map of the filter descends from one pk_upload_map, the colour covariance of a landmark is a function of (landmark,
 * number of updates); the 512-lane publish / subscribe kernel of the 512 < L <= 2048 route then reads it from a shared table
 * instead of streaming six rows per landmark in and out of every map slot (136 instead of 232 bytes per particle.landmark; `moved`
 * of pk_observe_bytes says which).  The slots' colour rows are written back from the table whenever anything else reads them --
 * every download (of the particles asked for), association and exchange sees what it always saw.  The mode ends (until the next pk_upload_map) with
 * pk_upload_landmarks, pk_set_measurement_noise behind an update, pk_grow_enable, any shard / pack / adopt call, an observe on
 * another route, or a landmark updated nearly as often as the table is deep.
 * out[0] the last observe ran in the mode and nothing has ended it since, [1] the table's depth, [2] scans taken in the mode,
 * [3] whole-buffer write-backs of the colour rows -- both since pk_create. */
int pk_colour_table_stats(pk_filter* f, int64_t out[4]);
/* Which kernels the last pk_observe / pk_step used for association + EKF update (instrumentation):
 * PK_ROUTE_NONE before the first call. */
enum {
  PK_ROUTE_NONE = 0,
  PK_ROUTE_KNOWN_IDS = 1,    /* ids supplied: k_observe */
  PK_ROUTE_ML_GENERAL = 2,   /* association kernel writes ids, k_observe builds chains from them */
  PK_ROUTE_ML_HANDOFF = 3,   /* k_assoc_grid hand-off + k_observe_fast (L <= 512) */
  PK_ROUTE_ML_SWEEP = 4,     /* k_assoc_grid hand-off + k_observe_sweep (L > 512) */
  PK_ROUTE_ML_FUSED = 5,     /* k_step_fused: gates + settling + EKF update in one kernel (L <= 512) */
  PK_ROUTE_ML_REGS = 6,      /* k_step_regs: the same in one pass for 512 < L <= 2048, two landmarks per lane */
  PK_ROUTE_DENSE = 8,        /* k_observe_dense: the general dense path (covariances that couple position and colour, or a
                                coupled Qt): association, 4x4 / 5x5 update and weight in one slow, general kernel */
  PK_ROUTE_ML_PUB_BIG = 9,   /* k_step_pub_big: maps of 2 049 ... 6 144 landmarks -- publish / subscribe settling in two passes over the map
                              * (the second one from L2 / Infinity Cache); what it leaves goes through k_observe_sweep */
  /* (7 was k_step_owner, removed in round 3) */
};
int pk_observe_route(const pk_filter* f);
/* The map indirection of the live generation (instrumentation): src[P], the map slot each particle's
 * landmarks currently live in.  After pk_resample slot k holds src[ancestor(k)] (the lazy copy of
 * prkt_core_v2.py:236,:246: maps are not moved until the next observe rewrites them); the number of
 * DISTINCT values is the number of slots the next observe launch really has to fetch.  Negative
 * values name records of a sharded adoption buffer. */
int pk_download_sources(pk_filter* f, int32_t* src);
/* How the last maximum-likelihood observe went (instrumentation): flagged = particles the one-pass kernels
 * (k_step_fused / k_step_regs) handed to the general kernels (a landmark passing more blobs than it has slots, a
 * full probability queue, a particle outside the margins of the reference particle's candidate lists);
 * cand_overflow = landmarks of the reference particle with more candidate blobs than list slots (non-zero: the
 * scan took the grid walk instead of the lists).  Synchronises the stream. */
int pk_observe_flagged(pk_filter* f, int64_t* flagged, int64_t* cand_overflow);
/* The second chance of flagged particles (eight-slot hand-off + k_observe_sweep) has list rows for P / 16 particles (>= 1 024);
 * a scan that wanted more -- the one-pass kernel stood back from it as a whole -- sends the rest through the general kernels
 * ONCE: the rows grow to what the last scan wanted.  wanted: of the last finished scan; capacity: rows the next scan will find. */
int pk_observe_retry_rows(pk_filter* f, int64_t* wanted, int64_t* capacity);
/* Which instance of the register route (PK_ROUTE_ML_REGS) worked on the last scan (instrumentation; the choice is made
 * on the device, per scan): *published = 1 when k_step_pub did -- contested blobs (prkt_core_v2.py:353-381) settled by
 * static publish / subscribe through LDS, three barriers per particle -- 0 when k_step_regs did (the publish table did
 * not fit LDS, a candidate list overflowed, or "pub_step" is off).  Synchronises the stream. */
int pk_observe_published(pk_filter* f, int32_t* published);
/* What the last scan's publish table came to (instrumentation; written by k_cand_entries on the device, once per scan):
 * stats[0] entries of the table (every (landmark, blob) pair several landmarks contend for, prkt_core_v2.py:353-381),
 * [1] contested blobs, [2] landmarks of the reference particle with two or more blobs inside their own gates (:433, :441),
 * [3] the longest candidate list, [4] entries the LDS table was given, [5] which instance worked on the scan: 0 none of the
 * publish / subscribe kernels (the table did not fit, a list overflowed), 1 the one-workgroup-per-CU instance, 2 / 3 the
 * two- / three-workgroups-per-CU instance of the two-pass kernel (k_step_pub_duo, option "pub_duo" = 1 / 2).  All zero when the
 * last observe took another route.  Synchronises the stream. */
int pk_observe_pub_stats(pk_filter* f, int64_t stats[6]);
/* The lean groups of the last scan (instrumentation; maps of 1 025 .. 2 048 landmarks on the publish / subscribe route, whose kernel
 * deals sixteen-landmark octets to sixteen (wave, pair) groups): out[0] groups in use that k_cand_entries marked lean -- every
 * landmark of theirs has at most one candidate blob, which no other landmark lists --, [1] groups in use, [2] pairs of lean groups
 * that took the usual body after all in the scan's launches (a key near the underflow edge, a mean outside the candidate margins,
 * a far bound that did not hold; 0 with "pub_lean" = 0).  All zero when the last observe took another route.  Synchronises the stream. */
int pk_observe_lean_stats(pk_filter* f, int64_t out[3]);
/* Per particle, how the last one-pass maximum-likelihood observe (k_step_fused / k_step_pub / k_step_pub_big / k_step_regs)
 * dealt with it (instrumentation; what the full-size oracle audits of tests/test_gpu_audit.py pick their samples by):
 * flags[P], 0 = settled by the one-pass kernel itself, 2 = redone by the second-chance route (eight-slot hand-off +
 * k_observe_sweep), 1 = redone by the general kernels.  The particles are match_features_to_scan's, prkt_core_v2.py:317-351,
 * whatever the route.  All zeros when the last observe took another route.  Synchronises the stream. */
int pk_observe_flags(pk_filter* f, uint8_t* flags);

/* ---- host-side reproductions of the reference's RNG streams (no GPU needed) ------
 * numpy.random.seed(s); numpy.random.normal(0,1,n)  (legacy MT19937 + polar method), the
 * stream prkt_core_v2.py:185-193 draws from; and random.seed(s); random.random() (:226). */
typedef struct pk_rng pk_rng;
int pk_rng_create_numpy(uint32_t seed, pk_rng** out);
int pk_rng_create_python(uint32_t seed, pk_rng** out);
int pk_rng_destroy(pk_rng* r);
int pk_rng_standard_normal(pk_rng* r, int64_t n, double* out);
int pk_rng_random(pk_rng* r, int64_t n, double* out);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* PARAKEET_SLAM_H_ */

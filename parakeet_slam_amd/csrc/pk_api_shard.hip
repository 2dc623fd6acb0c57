// The multi-GPU protocol behind the C ABI (pk_filter.hpp), three generations of it: the host-side exchange
// (pk_shard_offspring, pk_pack_particles, pk_adopt_particles), the device-resident one (pk_shard_*_dev) and the balanced placement
// (pk_shard_*_balanced_dev).  Host orchestration only.
#include "pk_filter.hpp"

namespace {

// shard / pack / adopt entry points, ahead of their argument checks (a NULL handle passes: the check that follows refuses it): the
// slots get their rows back, and the colour table's mode is never taken on this filter again
int ct_shard_call(pk_filter* f) {
  if (!f) return PK_OK;
  f->ct_sharded = true;
  if (f->colour_rows_valid) {
    f->ct_eligible = false;
    f->ct_engaged = false;
    return PK_OK;
  }
  int rc;
  if ((rc = use_device(f))) return rc;
  return ct_end(f);
}

// ---- the refusals the entry points share, each text once.  A step returns PK_OK or the refusal; every entry point calls its steps
// in an order of its own, which decides the refusal a caller sees when two apply.
// the contiguous exchange carries no bookkeeping rings (a NULL handle passes: some entry points ask before they check it)
int refuse_grow(const pk_filter* f, const char* who) {
  if (f && f->grow_on)
    return fail(PK_ERR_STATE, "%s: the new-landmark bookkeeping (pk_grow_enable) travels with the balanced placement only (pk_shard_*_balanced_dev)", who);
  return PK_OK;
}
// the offspring plan's slot table: "call pk_shard_plan_dev first", or for the read-outs "no plan yet"
int need_plan(const pk_filter* f, const char* who, bool readout = false) {
  if (!f->hi_dev) return fail(PK_ERR_STATE, "%s: %s", who, readout ? "no plan yet" : "call pk_shard_plan_dev first");
  return PK_OK;
}
// the balanced plan's tables
int need_balanced_plan(const pk_filter* f, const char* who) {
  if (!f->bal.rel || !f->d.logical[0]) return fail(PK_ERR_STATE, "%s: call pk_shard_plan_balanced_dev first", who);
  return PK_OK;
}
// an earlier adoption is still referenced: fold it into the map buffer first
int fold_alt(pk_filter* f) {
  if (!f->d.alt) return PK_OK;
  f->src_identity = false;
  return materialise(f);
}

// ---- buffers of the sharded resample that several entry points share
// every shard's block totals and their scan
int ensure_global_totals(pk_filter* f, int64_t n_global_blocks) {
  return dev_reserve_group(f, &f->gblocks_cap, n_global_blocks, n_global_blocks, want(&f->g_totals, (size_t)n_global_blocks),
                           want(&f->g_offsets, (size_t)n_global_blocks + 1));
}
int ensure_hi(pk_filter* f) { return dev_lazy(f, &f->hi_dev, (size_t)f->d.P + 1); }
// (lo, hi) of the received records: `words` int64 are wanted (two per record, three with the balanced placement).  The capacity
// is kept in words too, rounded down to whole pairs -- the figure it had when it counted pairs, so the buffer grows when it did.
int ensure_rlohi(pk_filter* f, int64_t words) {
  const int64_t slack = words + words / 4;
  return dev_reserve_group(f, &f->rlohi_cap, words, slack / 2 * 2, want(&f->rlohi_dev, (size_t)(slack + 16)));
}

}  // namespace

int refuse_balanced(const pk_filter* f, const char* who) {
  if (f->d.logical[0])
    return fail(PK_ERR_STATE, "%s: the balanced placement is active on this filter (its slots carry logical indices): resample through pk_shard_plan_balanced_dev / pk_shard_adopt_balanced_dev", who);
  return PK_OK;
}

// The path ring (pk_path_enable) records the lineages of ONE filter's pk_resample: what builds a generation any other way -- the
// exchange of the sharded filter, the balanced placement, the split step -- is refused while it is on, ahead of everything else
// the entry point does (a NULL handle passes: the check that follows refuses it).
int refuse_path(const pk_filter* f, const char* who) {
  if (f && f->path.cap)
    return fail(PK_ERR_STATE, "%s: the path is being recorded (pk_path_enable): lineages across ranks and split steps are not; switch it off with pk_path_enable(f, 0) first", who);
  return PK_OK;
}

// The clocks of the retirement rule (pk_grow_retire) do not travel in a record's tail: whatever moves particles between filters is
// refused while it is on, ahead of every other step (a NULL handle passes: the check that follows refuses it).
int refuse_retire(const pk_filter* f, const char* who) {
  if (f && f->retire.on())
    return fail(PK_ERR_STATE, "%s: readings and features are being retired (pk_grow_retire): the record carries no clocks; switch it off with pk_grow_retire(f, 0, 0) first", who);
  return PK_OK;
}

extern "C" {

// ---- sharded resampling ---------------------------------------
int pk_shard_max_logw(pk_filter* f, double* max_logw) {
  if (!f || !max_logw) return fail(PK_ERR_INVALID, "pk_shard_max_logw: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  launch_block_max(f->stream, f->d, f->partial, f->gmax);
  PK_HIP(hipMemcpyAsync(max_logw, f->gmax, sizeof(double), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

int64_t pk_shard_num_blocks(const pk_filter* f) { return f ? f->nblocks : -1; }

int pk_shard_block_totals(pk_filter* f, double gmax, int32_t weight_domain, double* totals) {
  if (!f || !totals) return fail(PK_ERR_INVALID, "pk_shard_block_totals: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipMemcpyAsync(f->gmax, &gmax, sizeof(double), hipMemcpyHostToDevice, f->stream));
  launch_scan_local(f->stream, f->d, f->gmax, weight_domain, f->clocal, f->totals);
  PK_HIP(hipMemcpyAsync(totals, f->totals, (size_t)f->nblocks * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

int pk_set_shard(pk_filter* f, int64_t global_offset) {
  if (int rc = ct_shard_call(f)) return rc;
  if (!f || global_offset < 0) return fail(PK_ERR_INVALID, "pk_set_shard: bad argument");
  f->d.global_offset = global_offset;
  return PK_OK;
}

int pk_shard_offspring(pk_filter* f, const double* global_totals, int64_t n_global_blocks, int64_t first_block,
                       int64_t global_particles, double u, int32_t last_shard, int64_t* slot_hi) {
  if (!f || !global_totals || !slot_hi) return fail(PK_ERR_INVALID, "pk_shard_offspring: NULL argument");
  if (!(u >= 0.0 && u < 1.0)) return fail(PK_ERR_INVALID, "pk_shard_offspring: u = %g outside [0,1)", u);
  if (first_block < 0 || first_block + f->nblocks > n_global_blocks || global_particles < f->d.P)
    return fail(PK_ERR_INVALID, "pk_shard_offspring: shard [%lld, +%lld) does not fit %lld global blocks",
                (long long)first_block, (long long)f->nblocks, (long long)n_global_blocks);
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = ensure_global_totals(f, n_global_blocks))) return rc;
  if ((rc = ensure_hi(f))) return rc;
  PK_HIP(hipMemcpyAsync(f->g_totals, global_totals, (size_t)n_global_blocks * sizeof(double), hipMemcpyHostToDevice,
                        f->stream));
  {
    Span t(f, PK_T_WEIGHTS);
    launch_scan_blocks(f->stream, f->g_totals, n_global_blocks, f->g_offsets, f->sum);
    launch_offspring(f->stream, f->clocal, f->g_offsets, f->sum, first_block, f->d.P, global_particles, u,
                     last_shard ? 1 : 0, f->hi_dev);
  }
  PK_HIP(hipMemcpyAsync(slot_hi, f->hi_dev, ((size_t)f->d.P + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

// one particle in the sharded exchange: header | map slot | the new-landmark bookkeeping when it is on (pk_grow_enable)
static size_t record_stride(const pk_filter* f) { return kPoseRecordBytes + f->d.lay.slot_bytes + (f->grow_on ? grow_tail_bytes(f->grow) : 0); }
int64_t pk_particle_bytes(const pk_filter* f) { return f ? (int64_t)record_stride(f) : -1; }

int pk_pack_particles(pk_filter* f, const int64_t* local_idx, int64_t n, void* dev_buf) {
  if (int rc = refuse_retire(f, "pk_pack_particles")) return rc;
  if (int rc = refuse_path(f, "pk_pack_particles")) return rc;
  if (int rc = ct_shard_call(f)) return rc;
  if (!f || n < 0 || (n > 0 && (!local_idx || !dev_buf))) return fail(PK_ERR_INVALID, "pk_pack_particles: bad argument");
  // (pk_particle_bytes() counts the bookkeeping's tail, k_pack writes records without one -- and pk_adopt_particles
  // would leave readings and id counters on the wrong particles)
  if (int rc = refuse_grow(f, "pk_pack_particles")) return rc;
  if (n > f->d.P) return fail(PK_ERR_INVALID, "pk_pack_particles: %lld records from %lld particles", (long long)n, (long long)f->d.P);
  for (int64_t i = 0; i < n; ++i)
    if (local_idx[i] < 0 || local_idx[i] >= f->d.P) return fail(PK_ERR_INVALID, "pk_pack_particles: index %lld out of range", (long long)local_idx[i]);
  if (n == 0) return PK_OK;
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = dev_lazy(f, &f->idx_dev, (size_t)f->d.P))) return rc;
  PK_HIP(hipMemcpyAsync(f->idx_dev, local_idx, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, f->stream));
  {
    Span t(f, PK_T_RESAMPLE);
    launch_pack(f->stream, f->d, f->idx_dev, n, static_cast<unsigned char*>(dev_buf));
  }
  PK_HIP(hipStreamSynchronize(f->stream));  // the collective that ships dev_buf runs on another stream
  return PK_OK;
}

int pk_adopt_particles(pk_filter* f, const int64_t* src, const void* dev_buf, int64_t n_received) {
  if (int rc = refuse_retire(f, "pk_adopt_particles")) return rc;
  if (int rc = refuse_path(f, "pk_adopt_particles")) return rc;
  if (int rc = ct_shard_call(f)) return rc;
  poses_change(f);
  if (!f || !src || n_received < 0 || (n_received > 0 && !dev_buf)) return fail(PK_ERR_INVALID, "pk_adopt_particles: bad argument");
  if (int rc = refuse_grow(f, "pk_adopt_particles")) return rc;
  const int64_t P = f->d.P;
  for (int64_t k = 0; k < P; ++k)
    if (src[k] >= P || src[k] < -n_received) return fail(PK_ERR_INVALID, "pk_adopt_particles: src[%lld] = %lld out of range", (long long)k, (long long)src[k]);
  if (int rc = refuse_balanced(f, "pk_adopt_particles")) return rc;
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = fold_alt(f))) return rc;
  if ((rc = dev_lazy(f, &f->srcs_dev, (size_t)P))) return rc;
  PK_HIP(hipMemcpyAsync(f->srcs_dev, src, (size_t)P * sizeof(int64_t), hipMemcpyHostToDevice, f->stream));
  {
    Span t(f, PK_T_RESAMPLE);
    launch_adopt(f->stream, f->d, f->srcs_dev, static_cast<const unsigned char*>(dev_buf));
  }
  if (n_received == 0) f->d.alt = nullptr;
  f->src_identity = false;
  f->gmax_fused = false;
  PK_HIP(hipStreamSynchronize(f->stream));  // src was pageable host memory
  return PK_OK;
}

// ---- device-resident variants: every buffer is a device pointer owned by the caller (torch
// tensors), nothing synchronises the stream; see DESIGN.md section 6 --------------------------
int pk_shard_max_logw_dev(pk_filter* f, double* dev_out) {
  if (!f || !dev_out) return fail(PK_ERR_INVALID, "pk_shard_max_logw_dev: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  Span t(f, PK_T_WEIGHTS);
  if (f->gmax_fused)
    launch_keys_max(f->stream, ctl_gmax_key(f), dev_out);  // the observe kernels kept the running max
  else
    launch_block_max(f->stream, f->d, f->partial, dev_out);
  return PK_OK;
}

int pk_shard_block_totals_dev(pk_filter* f, const double* dev_gmax, int32_t weight_domain, double* dev_totals) {
  if (!f || !dev_totals || (weight_domain == PK_WEIGHTS_LOG && !dev_gmax))
    return fail(PK_ERR_INVALID, "pk_shard_block_totals_dev: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  Span t(f, PK_T_WEIGHTS);
  launch_scan_local(f->stream, f->d, dev_gmax ? dev_gmax : f->gmax, weight_domain, f->clocal, dev_totals);
  return PK_OK;
}

int pk_shard_plan_dev(pk_filter* f, const double* dev_global_totals, int64_t n_global_blocks, int64_t first_block,
                      int64_t global_particles, double u, int32_t last_shard, int32_t world, int64_t* dev_ranges) {
  if (!f || !dev_global_totals || !dev_ranges || world < 1) return fail(PK_ERR_INVALID, "pk_shard_plan_dev: bad argument");
  if (!(u >= 0.0 && u < 1.0)) return fail(PK_ERR_INVALID, "pk_shard_plan_dev: u = %g outside [0,1)", u);
  if (first_block < 0 || first_block + f->nblocks > n_global_blocks || global_particles != (int64_t)world * f->d.P)
    return fail(PK_ERR_INVALID, "pk_shard_plan_dev: shard geometry (%lld blocks from %lld of %lld, %lld particles x %d)",
                (long long)f->nblocks, (long long)first_block, (long long)n_global_blocks, (long long)f->d.P, world);
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = ensure_global_totals(f, n_global_blocks))) return rc;
  if ((rc = ensure_hi(f))) return rc;
  if (!f->plan_ticket) {
    if ((rc = dev_alloc(f, &f->plan_ticket, (size_t)1))) return rc;
    PK_HIP(hipMemsetAsync(f->plan_ticket, 0, sizeof(unsigned), f->stream));
  }
  Span t(f, PK_T_WEIGHTS);
  if (n_global_blocks <= kAncestorsScanMaxBlocks) {
    // one launch: every workgroup scans the few global block totals itself, the last one to finish
    // writes the per-destination ranges
    launch_offspring_plan(f->stream, f->clocal, dev_global_totals, n_global_blocks, first_block, f->d.P, global_particles, u,
                          last_shard ? 1 : 0, f->hi_dev, world, dev_ranges, f->plan_ticket);
    return PK_OK;
  }
  launch_scan_blocks(f->stream, dev_global_totals, n_global_blocks, f->g_offsets, f->sum);
  launch_offspring(f->stream, f->clocal, f->g_offsets, f->sum, first_block, f->d.P, global_particles, u,
                   last_shard ? 1 : 0, f->hi_dev);
  launch_shard_ranges(f->stream, f->hi_dev, f->d.P, world, dev_ranges);
  return PK_OK;
}

// ---- the same plan from the scan of the WHOLE filter's weights: any shard size ----------------------------------------
int pk_shard_logw_dev(pk_filter* f, double* dev_out) {
  if (!f || !dev_out) return fail(PK_ERR_INVALID, "pk_shard_logw_dev: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipMemcpyAsync(dev_out, f->d.logw[f->d.cur], (size_t)f->d.P * sizeof(double), hipMemcpyDeviceToDevice, f->stream));
  return PK_OK;
}

int pk_shard_plan_global_dev(pk_filter* f, const double* dev_global_logw, int64_t global_particles, const double* dev_gmax,
                             int32_t weight_domain, double u, int32_t last_shard, int32_t world, int64_t* dev_ranges) {
  if (!f || !dev_global_logw || !dev_ranges || world < 1) return fail(PK_ERR_INVALID, "pk_shard_plan_global_dev: bad argument");
  if (weight_domain == PK_WEIGHTS_LOG && !dev_gmax) return fail(PK_ERR_INVALID, "pk_shard_plan_global_dev: NULL maximum");
  if (!(u >= 0.0 && u < 1.0)) return fail(PK_ERR_INVALID, "pk_shard_plan_global_dev: u = %g outside [0,1)", u);
  const int64_t P = f->d.P, goff = f->d.global_offset;
  if (global_particles != (int64_t)world * P || goff < 0 || goff + P > global_particles)
    return fail(PK_ERR_INVALID, "pk_shard_plan_global_dev: shard [%lld, +%lld) of %lld particles, world %d", (long long)goff,
                (long long)P, (long long)global_particles, world);
  int rc;
  if ((rc = use_device(f))) return rc;
  const int64_t nbg = (global_particles + kScanBlock - 1) / kScanBlock;
  if ((rc = dev_reserve_group(f, &f->gl_cap, global_particles, global_particles, want(&f->gl_clocal, (size_t)global_particles),
                              want(&f->gl_totals, (size_t)nbg), want(&f->gl_offsets, (size_t)nbg + 1))))
    return rc;
  if ((rc = ensure_hi(f))) return rc;
  Span t(f, PK_T_WEIGHTS);
  // exactly the kernels of the 1-GPU resample on the whole filter's log-weights: same blocks, same additions, same bits
  launch_scan_local_of(f->stream, dev_global_logw, global_particles, dev_gmax ? dev_gmax : f->gmax, weight_domain, f->gl_clocal,
                       f->gl_totals);
  launch_scan_blocks(f->stream, f->gl_totals, nbg, f->gl_offsets, f->sum);
  launch_offspring_global(f->stream, f->gl_clocal, f->gl_offsets, f->sum, goff, P, global_particles, u, last_shard ? 1 : 0,
                          f->hi_dev);
  launch_shard_ranges(f->stream, f->hi_dev, P, world, dev_ranges);
  PK_LAUNCH_CHECK("pk_shard_plan_global_dev");
  return PK_OK;
}

int pk_shard_download_offspring(pk_filter* f, int64_t* slot_hi) {
  if (!f || !slot_hi) return fail(PK_ERR_INVALID, "pk_shard_download_offspring: NULL argument");
  if (int rc = need_plan(f, "pk_shard_download_offspring", true)) return rc;
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipMemcpyAsync(slot_hi, f->hi_dev, ((size_t)f->d.P + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

int pk_shard_pack_dev(pk_filter* f, const int64_t* ranges, int32_t world, int32_t rank, void* dev_buf) {
  if (int rc = refuse_retire(f, "pk_shard_pack_dev")) return rc;
  if (int rc = ct_shard_call(f)) return rc;
  if (int rc = refuse_grow(f, "pk_shard_pack_dev")) return rc;
  if (!f || !ranges || world < 1 || rank < 0 || rank >= world) return fail(PK_ERR_INVALID, "pk_shard_pack_dev: bad argument");
  if (int rc = need_plan(f, "pk_shard_pack_dev")) return rc;
  int rc;
  if ((rc = use_device(f))) return rc;
  const int64_t P = f->d.P;
  const size_t stride = kPoseRecordBytes + f->d.lay.slot_bytes;
  int64_t rec = 0;
  Span t(f, PK_T_RESAMPLE);
  for (int d = 0; d < world; ++d) {
    if (d == rank) continue;
    const int64_t j0 = ranges[2 * d], j1 = ranges[2 * d + 1];
    if (j0 < 0 || j1 < j0 || j1 > P) return fail(PK_ERR_INVALID, "pk_shard_pack_dev: range [%lld, %lld) for rank %d", (long long)j0, (long long)j1, d);
    if (j1 > j0 && !dev_buf) return fail(PK_ERR_INVALID, "pk_shard_pack_dev: NULL buffer");
    launch_pack_range(f->stream, f->d, f->hi_dev, j0, j1 - j0, (int64_t)d * P, (int64_t)(d + 1) * P,
                      static_cast<unsigned char*>(dev_buf) + (size_t)rec * stride);
    rec += j1 - j0;
  }
  return PK_OK;
}

int pk_shard_pack_slots_dev(pk_filter* f, int64_t j0, int64_t j1, int64_t slot_lo, int64_t slot_hi, void* dev_buf) {
  if (int rc = refuse_retire(f, "pk_shard_pack_slots_dev")) return rc;
  if (int rc = ct_shard_call(f)) return rc;
  if (int rc = refuse_grow(f, "pk_shard_pack_slots_dev")) return rc;
  if (!f || j0 < 0 || j1 < j0 || j1 > f->d.P || slot_hi < slot_lo) return fail(PK_ERR_INVALID, "pk_shard_pack_slots_dev: bad argument");
  if (int rc = need_plan(f, "pk_shard_pack_slots_dev")) return rc;
  if (j1 > j0 && !dev_buf) return fail(PK_ERR_INVALID, "pk_shard_pack_slots_dev: NULL buffer");
  int rc;
  if ((rc = use_device(f))) return rc;
  Span t(f, PK_T_RESAMPLE);
  launch_pack_range(f->stream, f->d, f->hi_dev, j0, j1 - j0, slot_lo, slot_hi, static_cast<unsigned char*>(dev_buf));
  PK_LAUNCH_CHECK("pk_shard_pack_slots_dev");
  return PK_OK;
}

int pk_shard_adopt_dev(pk_filter* f, int32_t rank, const void* dev_recv, int64_t n_received) {
  if (int rc = refuse_retire(f, "pk_shard_adopt_dev")) return rc;
  if (int rc = refuse_path(f, "pk_shard_adopt_dev")) return rc;
  if (int rc = ct_shard_call(f)) return rc;
  if (int rc = refuse_grow(f, "pk_shard_adopt_dev")) return rc;
  poses_change(f);
  if (!f || rank < 0 || n_received < 0 || (n_received > 0 && !dev_recv)) return fail(PK_ERR_INVALID, "pk_shard_adopt_dev: bad argument");
  if (int rc = need_plan(f, "pk_shard_adopt_dev")) return rc;
  if (int rc = refuse_balanced(f, "pk_shard_adopt_dev")) return rc;
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = fold_alt(f))) return rc;
  if ((rc = ensure_rlohi(f, 2 * n_received))) return rc;
  Span t(f, PK_T_RESAMPLE);
  launch_adopt_dev(f->stream, f->d, f->hi_dev, (int64_t)rank * f->d.P, static_cast<const unsigned char*>(dev_recv),
                   n_received, f->rlohi_dev);
  f->src_identity = false;
  f->gmax_fused = false;
  return PK_OK;
}

int pk_shard_adopt_local_dev(pk_filter* f, int32_t rank) {
  if (int rc = refuse_retire(f, "pk_shard_adopt_local_dev")) return rc;
  if (int rc = refuse_path(f, "pk_shard_adopt_local_dev")) return rc;
  if (int rc = ct_shard_call(f)) return rc;
  if (int rc = refuse_grow(f, "pk_shard_adopt_local_dev")) return rc;
  poses_change(f);
  if (!f || rank < 0) return fail(PK_ERR_INVALID, "pk_shard_adopt_local_dev: bad argument");
  if (int rc = need_plan(f, "pk_shard_adopt_local_dev")) return rc;
  if (int rc = refuse_balanced(f, "pk_shard_adopt_local_dev")) return rc;
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = fold_alt(f))) return rc;
  Span t(f, PK_T_RESAMPLE);
  const int64_t base = (int64_t)rank * f->d.P;
  launch_adopt_dev(f->stream, f->d, f->hi_dev, base, nullptr, 0, nullptr, 1, f->loop_lo == INT64_MIN ? INT64_MIN : base + f->loop_lo,
                   f->loop_hi == INT64_MAX ? INT64_MAX : base + f->loop_hi);
  f->src_identity = false;
  f->gmax_fused = false;
  f->adopt_local_done = true;
  return PK_OK;
}

int pk_shard_adopt_remote_dev(pk_filter* f, int32_t rank, const void* dev_recv, int64_t n_received) {
  if (int rc = refuse_retire(f, "pk_shard_adopt_remote_dev")) return rc;
  if (int rc = refuse_path(f, "pk_shard_adopt_remote_dev")) return rc;
  if (int rc = ct_shard_call(f)) return rc;
  if (int rc = refuse_grow(f, "pk_shard_adopt_remote_dev")) return rc;
  poses_change(f);
  if (!f || rank < 0 || n_received < 0 || (n_received > 0 && !dev_recv)) return fail(PK_ERR_INVALID, "pk_shard_adopt_remote_dev: bad argument");
  if (int rc = need_plan(f, "pk_shard_adopt_remote_dev")) return rc;
  if (!f->adopt_local_done)
    return fail(PK_ERR_STATE, "pk_shard_adopt_remote_dev: pk_shard_adopt_local_dev first (it makes the new generation current)");
  f->adopt_local_done = false;
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = ensure_rlohi(f, 2 * n_received))) return rc;
  Span t(f, PK_T_RESAMPLE);
  const int64_t base = (int64_t)rank * f->d.P;
  launch_adopt_dev(f->stream, f->d, f->hi_dev, base, static_cast<const unsigned char*>(dev_recv), n_received, f->rlohi_dev, 2,
                   f->loop_lo == INT64_MIN ? INT64_MIN : base + f->loop_lo, f->loop_hi == INT64_MAX ? INT64_MAX : base + f->loop_hi);
  f->loop_lo = INT64_MIN;
  f->loop_hi = INT64_MAX;
  return PK_OK;
}

int pk_shard_local_span_dev(pk_filter* f, int64_t* dev_out2) {
  if (!f || !dev_out2) return fail(PK_ERR_INVALID, "pk_shard_local_span_dev: NULL argument");
  if (int rc = need_plan(f, "pk_shard_local_span_dev", true)) return rc;
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipMemcpyAsync(dev_out2, f->hi_dev, sizeof(int64_t), hipMemcpyDeviceToDevice, f->stream));
  PK_HIP(hipMemcpyAsync(dev_out2 + 1, f->hi_dev + f->d.P, sizeof(int64_t), hipMemcpyDeviceToDevice, f->stream));
  return PK_OK;
}

// ---- balanced placement: minimum migration (sharded.py::plan_balanced is the readable reference) ----
static int ensure_logical(pk_filter* f) {
  DeviceState& d = f->d;
  if (d.logical[0]) return PK_OK;
  int rc;
  int64_t *a = nullptr, *b = nullptr;  // (a kernel takes a non-null logical[] for indices: both go in, or neither)
  if ((rc = dev_alloc(f, &a, (size_t)d.P)) || (rc = dev_alloc(f, &b, (size_t)d.P))) {
    dev_free(f, &a);
    return rc;
  }
  launch_iota64(f->stream, a, d.P, d.global_offset);
  launch_iota64(f->stream, b, d.P, d.global_offset);
  d.logical[0] = a;
  d.logical[1] = b;
  return PK_OK;
}

int pk_shard_reset_placement(pk_filter* f) {
  if (!f) return fail(PK_ERR_INVALID, "pk_shard_reset_placement: NULL handle");
  int rc;
  if ((rc = use_device(f))) return rc;
  if (f->d.logical[0]) launch_iota64(f->stream, f->d.logical[f->d.cur], f->d.P, f->d.global_offset);
  return PK_OK;
}

int pk_shard_download_logical(pk_filter* f, int64_t* logical) {
  if (!f || !logical) return fail(PK_ERR_INVALID, "pk_shard_download_logical: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  if (!f->d.logical[0]) {
    for (int64_t j = 0; j < f->d.P; ++j) logical[j] = f->d.global_offset + j;
    return PK_OK;
  }
  PK_HIP(hipMemcpyAsync(logical, f->d.logical[f->d.cur], (size_t)f->d.P * sizeof(int64_t), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

/* The placement set from the host (tests of the planner in isolation; restoring a snapshot taken in physical order): slot j holds
 * logical particle logical[j].  Every index must lie in [0, 2^31). */
int pk_shard_upload_logical(pk_filter* f, const int64_t* logical) {
  if (!f || !logical) return fail(PK_ERR_INVALID, "pk_shard_upload_logical: NULL argument");
  for (int64_t j = 0; j < f->d.P; ++j)
    if (logical[j] < 0 || logical[j] >= ((int64_t)1 << 31)) return fail(PK_ERR_INVALID, "pk_shard_upload_logical: logical[%lld] = %lld", (long long)j, (long long)logical[j]);
  if (f->split.active) return fail(PK_ERR_STATE, "pk_shard_upload_logical: a split observe is in progress");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = ensure_logical(f))) return rc;
  PK_HIP(hipMemcpyAsync(f->d.logical[f->d.cur], logical, (size_t)f->d.P * sizeof(int64_t), hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

/* This rank's tables of the last balanced plan (tests): rel[P + 1] the children of its particles [0, j), Hl[P] the first output slot
 * of every particle's children, alive[P] its particles with children, ascending -- the first rel-derived count of them is valid,
 * the rest is -1. */
int pk_shard_download_balanced_plan(pk_filter* f, int64_t* rel, int64_t* Hl, int32_t* alive) {
  if (!f || !rel || !Hl || !alive) return fail(PK_ERR_INVALID, "pk_shard_download_balanced_plan: NULL argument");
  if (!f->bal.rel || !f->bal.Hl || !f->bal.alive) return fail(PK_ERR_STATE, "pk_shard_download_balanced_plan: no balanced plan yet (pk_shard_plan_balanced_dev)");
  int rc;
  if ((rc = use_device(f))) return rc;
  const int64_t P = f->d.P;
  PK_HIP(hipMemcpyAsync(rel, f->bal.rel, ((size_t)P + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipMemcpyAsync(Hl, f->bal.Hl, (size_t)P * sizeof(int64_t), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipMemcpyAsync(alive, f->bal.alive, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  int64_t n = 0;  // particles with children: what k_bal_own wrote of alive[]
  for (int64_t j = 0; j < P; ++j) n += rel[j + 1] > rel[j] ? 1 : 0;
  for (int64_t j = n; j < P; ++j) alive[j] = -1;
  return PK_OK;
}

int pk_shard_state_dev(pk_filter* f, double* dev_out) {
  if (int rc = refuse_retire(f, "pk_shard_state_dev")) return rc;
  if (int rc = refuse_path(f, "pk_shard_state_dev")) return rc;
  if (!f || !dev_out) return fail(PK_ERR_INVALID, "pk_shard_state_dev: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = ensure_logical(f))) return rc;
  launch_bal_state(f->stream, f->d, dev_out);
  PK_LAUNCH_CHECK("pk_shard_state_dev");
  return PK_OK;
}

int pk_shard_plan_balanced_dev(pk_filter* f, const double* dev_global_state, int64_t global_particles, const double* dev_gmax,
                               int32_t weight_domain, double u, int32_t world, int32_t rank, int64_t* dev_table) {
  if (!f || !dev_global_state || !dev_table || world < 1 || world > 64 || rank < 0 || rank >= world)
    return fail(PK_ERR_INVALID, "pk_shard_plan_balanced_dev: bad argument (world 1 .. 64)");
  if (weight_domain != PK_WEIGHTS_LINEAR && weight_domain != PK_WEIGHTS_LOG)
    return fail(PK_ERR_INVALID, "pk_shard_plan_balanced_dev: weight_domain %d", weight_domain);
  if (weight_domain == PK_WEIGHTS_LOG && !dev_gmax) return fail(PK_ERR_INVALID, "pk_shard_plan_balanced_dev: NULL maximum");
  if (!(u >= 0.0 && u < 1.0)) return fail(PK_ERR_INVALID, "pk_shard_plan_balanced_dev: u = %g outside [0,1)", u);
  const int64_t P = f->d.P, Pg = global_particles;
  if (Pg != (int64_t)world * P || Pg >= ((int64_t)1 << 31))
    return fail(PK_ERR_INVALID, "pk_shard_plan_balanced_dev: %lld particles are not %d shards of %lld (or more than 2^31)", (long long)Pg, world, (long long)P);
  if (f->split.active) return fail(PK_ERR_STATE, "pk_shard_plan_balanced_dev: a split observe is in progress");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = ensure_logical(f))) return rc;
  BalancedBuffers& b = f->bal;
  const int64_t nbg = (Pg + kScanBlock - 1) / kScanBlock;
  if ((rc = dev_reserve_group(f, &b.cap, Pg, Pg, want(&b.glogw, (size_t)Pg), want(&b.clocal, (size_t)Pg), want(&b.totals, (size_t)nbg),
                              want(&b.offsets, (size_t)nbg + 1), want(&b.H, (size_t)Pg + 1), want(&b.cloc, (size_t)Pg),
                              want(&b.ctot, (size_t)nbg), want(&b.coff, (size_t)nbg + 1))))
    return rc;
  if ((rc = dev_lazy(f, &b.sum, (size_t)1))) return rc;
  if ((rc = dev_lazy(f, &b.rel, (size_t)P + 1))) return rc;
  if ((rc = dev_lazy(f, &b.Hl, (size_t)P))) return rc;
  if ((rc = dev_lazy(f, &b.alive, (size_t)P))) return rc;
  if (!b.bad) {
    if ((rc = dev_alloc(f, &b.bad, (size_t)1))) return rc;
    PK_HIP(hipMemsetAsync(b.bad, 0, sizeof(int), f->stream));
  }
  Span t(f, PK_T_WEIGHTS);
  launch_bal_plan(f->stream, f->d, dev_global_state, Pg, world, rank, dev_gmax ? dev_gmax : f->gmax, weight_domain, u, b, dev_table);
  PK_LAUNCH_CHECK("pk_shard_plan_balanced_dev");
  f->bal_m = -1;
  return PK_OK;
}

int pk_shard_download_balanced_offspring(pk_filter* f, int64_t global_particles, int64_t* H) {
  if (!f || !H) return fail(PK_ERR_INVALID, "pk_shard_download_balanced_offspring: NULL argument");
  if (!f->bal.H || global_particles != f->bal.cap) return fail(PK_ERR_STATE, "pk_shard_download_balanced_offspring: no balanced plan of %lld particles yet", (long long)global_particles);
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipMemcpyAsync(H, f->bal.H, ((size_t)global_particles + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

// the plan's table as the host read it: world rows of (a0, a1) x world, n, m, ebase, dbase
static int balanced_row_check(const int64_t* table, int world, int64_t P, const char* who) {
  const int row = 2 * world + 4;
  int64_t e_sum = 0, d_sum = 0;
  for (int r = 0; r < world; ++r) {
    const int64_t n = table[(size_t)r * row + 2 * world], m = table[(size_t)r * row + 2 * world + 1];
    if (n < 0 || m != (n < P ? n : P) || table[(size_t)r * row + 2 * world + 2] != e_sum || table[(size_t)r * row + 2 * world + 3] != d_sum)
      return fail(PK_ERR_INVALID, "%s: the plan table is not one pk_shard_plan_balanced_dev wrote (rank %d)", who, r);
    e_sum += n - m;
    d_sum += P - m;
    for (int d = 0; d < world; ++d) {
      const int64_t a0 = table[(size_t)r * row + 2 * d], a1 = table[(size_t)r * row + 2 * d + 1];
      if (a0 < 0 || a1 < a0 || a1 > P) return fail(PK_ERR_INVALID, "%s: range [%lld, %lld) from rank %d to rank %d", who, (long long)a0, (long long)a1, r, d);
    }
  }
  if (e_sum != d_sum) return fail(PK_ERR_INVALID, "%s: excess %lld and free slots %lld differ", who, (long long)e_sum, (long long)d_sum);
  return PK_OK;
}

int pk_shard_pack_balanced_dev(pk_filter* f, const int64_t* table, int32_t world, int32_t rank, void* dev_buf) {
  if (int rc = refuse_retire(f, "pk_shard_pack_balanced_dev")) return rc;
  if (int rc = ct_shard_call(f)) return rc;
  if (!f || !table || world < 1 || world > 64 || rank < 0 || rank >= world) return fail(PK_ERR_INVALID, "pk_shard_pack_balanced_dev: bad argument");
  if (int rc = need_balanced_plan(f, "pk_shard_pack_balanced_dev")) return rc;
  int rc;
  const int64_t P = f->d.P;
  if ((rc = balanced_row_check(table, world, P, "pk_shard_pack_balanced_dev"))) return rc;
  if ((rc = use_device(f))) return rc;
  const int row = 2 * world + 4;
  const size_t stride = record_stride(f);
  const int64_t ebase_s = table[(size_t)rank * row + 2 * world + 2];
  int64_t rec = 0;
  Span t(f, PK_T_RESAMPLE);
  for (int d = 0; d < world; ++d) {
    if (d == rank) continue;
    const int64_t a0 = table[(size_t)rank * row + 2 * d], a1 = table[(size_t)rank * row + 2 * d + 1];
    if (a1 <= a0) continue;
    if (!dev_buf) return fail(PK_ERR_INVALID, "pk_shard_pack_balanced_dev: NULL buffer");
    const int64_t m_d = table[(size_t)d * row + 2 * world + 1], dbase_d = table[(size_t)d * row + 2 * world + 3];
    launch_bal_pack(f->stream, f->d, f->bal, a0, a1 - a0, ebase_s, dbase_d, P - m_d, m_d,
                    static_cast<unsigned char*>(dev_buf) + (size_t)rec * stride, stride, f->grow_on ? &f->grow : nullptr);
    rec += a1 - a0;
  }
  PK_LAUNCH_CHECK("pk_shard_pack_balanced_dev");
  return PK_OK;
}

/* debug (one-rank tests of the balanced exchange, option "balanced_loopback_keep"): records of this rank's particles alive[a0, a1) for
 * ITSELF -- the children from position `keep` on, destined for its own slots [keep, P): what k_bal_pack writes for another rank whose
 * free slots are [keep, P), with the 64-byte balanced header (and the new-landmark bookkeeping behind the map while that is on). */
int pk_shard_pack_balanced_loop_dev(pk_filter* f, int64_t keep, int64_t a0, int64_t a1, void* dev_buf) {
  if (int rc = refuse_retire(f, "pk_shard_pack_balanced_loop_dev")) return rc;
  if (int rc = ct_shard_call(f)) return rc;
  if (!f || keep < 0 || keep > f->d.P || a0 < 0 || a1 < a0 || a1 > f->d.P || (a1 > a0 && !dev_buf))
    return fail(PK_ERR_INVALID, "pk_shard_pack_balanced_loop_dev: bad argument");
  if (int rc = need_balanced_plan(f, "pk_shard_pack_balanced_loop_dev")) return rc;
  int rc;
  if ((rc = use_device(f))) return rc;
  Span t(f, PK_T_RESAMPLE);
  // (k_bal_pack's "P" is the number of children a rank keeps: here keep; excess positions count from 0, the destination's free slots
  // are [keep, P): ebase = dbase = 0, dd = P - keep, m_d = keep)
  launch_bal_pack(f->stream, f->d, f->bal, a0, a1 - a0, 0, 0, f->d.P - keep, keep, static_cast<unsigned char*>(dev_buf), record_stride(f),
                  f->grow_on ? &f->grow : nullptr, keep);
  PK_LAUNCH_CHECK("pk_shard_pack_balanced_loop_dev");
  return PK_OK;
}

int pk_shard_adopt_balanced_dev(pk_filter* f, const int64_t* table, int32_t world, int32_t rank, const void* dev_recv,
                                int64_t n_received, int32_t mode) {
  if (int rc = refuse_retire(f, "pk_shard_adopt_balanced_dev")) return rc;
  if (int rc = refuse_path(f, "pk_shard_adopt_balanced_dev")) return rc;
  if (int rc = ct_shard_call(f)) return rc;
  poses_change(f);
  if (!f || !table || world < 1 || world > 64 || rank < 0 || rank >= world || n_received < 0 || mode < 0 || mode > 2 ||
      (n_received > 0 && !dev_recv))
    return fail(PK_ERR_INVALID, "pk_shard_adopt_balanced_dev: bad argument");
  if (int rc = need_balanced_plan(f, "pk_shard_adopt_balanced_dev")) return rc;
  if (f->grow_on && mode != 0) return fail(PK_ERR_STATE, "pk_shard_adopt_balanced_dev: the new-landmark bookkeeping (pk_grow_enable) is adopted whole (mode 0)");
  int rc;
  const int64_t P = f->d.P;
  if ((rc = balanced_row_check(table, world, P, "pk_shard_adopt_balanced_dev"))) return rc;
  const int row = 2 * world + 4;
  int64_t m = table[(size_t)rank * row + 2 * world + 1];
  // debug loopback (one rank): the rank's own children fill [0, keep) only, its children from position keep on arrive as records
  const bool loop = f->bal_loop_keep >= 0 && world == 1;
  if (loop) m = f->bal_loop_keep < m ? f->bal_loop_keep : m;
  if (mode == 2) {
    if (!f->adopt_local_done) return fail(PK_ERR_STATE, "pk_shard_adopt_balanced_dev: mode 1 first (it makes the new generation current)");
    f->adopt_local_done = false;
  }
  if (mode != 1) {
    int64_t expect = 0;
    for (int s = 0; s < world; ++s)
      if (s != rank) expect += table[(size_t)s * row + 2 * rank + 1] - table[(size_t)s * row + 2 * rank];
    if (!loop && expect != n_received) return fail(PK_ERR_INVALID, "pk_shard_adopt_balanced_dev: %lld records received, the plan sends %lld", (long long)n_received, (long long)expect);
    if (m < P && n_received == 0) return fail(PK_ERR_INVALID, "pk_shard_adopt_balanced_dev: %lld free slots and no records", (long long)(P - m));
    f->bal_loop_keep = -1;  // (one adoption: cleared behind mode 0 or mode 2)
  }
  if ((rc = use_device(f))) return rc;
  if (mode != 2 && (rc = fold_alt(f))) return rc;
  if ((rc = ensure_rlohi(f, 3 * n_received))) return rc;
  Span t(f, PK_T_RESAMPLE);
  const size_t stride = record_stride(f);
  launch_bal_adopt(f->stream, f->d, f->bal, m, static_cast<const unsigned char*>(dev_recv), n_received, f->rlohi_dev, mode, stride,
                   f->grow_on ? f->anc : nullptr);
  if (f->grow_on)  // the bookkeeping follows: own children from this filter's arrays, adopted ones from their records' tails
    launch_grow_gather(f->stream, f->grow, f->anc, P, static_cast<const unsigned char*>(dev_recv), stride, kPoseRecordBytes + f->d.lay.slot_bytes);
  PK_LAUNCH_CHECK("pk_shard_adopt_balanced_dev");
  f->src_identity = false;
  f->gmax_fused = false;
  if (mode == 1) f->adopt_local_done = true;
  return PK_OK;
}

/* consistency failures the balanced kernels counted since the filter was made (a logical index out of range, received
 * records that do not tile the free slots): 0 unless the plan and the exchange disagree */
int pk_shard_balanced_errors(pk_filter* f, int64_t* count) {
  if (!f || !count) return fail(PK_ERR_INVALID, "pk_shard_balanced_errors: NULL argument");
  *count = 0;
  if (!f->bal.bad) return PK_OK;
  int rc;
  if ((rc = use_device(f))) return rc;
  int v = 0;
  PK_HIP(hipMemcpyAsync(&v, f->bal.bad, sizeof(int), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  *count = v;
  return PK_OK;
}

}  // extern "C"

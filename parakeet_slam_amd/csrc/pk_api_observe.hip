// The observe pipeline behind the C ABI (pk_filter.hpp): which kernels a scan gets (plan_scan; DESIGN.md section 4, "Routing"), the
// association, the dense observe, the one-pass stages, the new-landmark bookkeeping's launch, observe_impl, the proposal's scan and
// the pk_observe* entry points with their read-outs; and the colour table's host side (ct_*).  How the scan got onto the device is
// pk_api_scan.hip's.  Host orchestration only.
#include "pk_filter.hpp"

// a pinned block of 64 bytes whose first word starts at 0 (retry_seen, ct_seen)
static int host_word(pk_filter* f, unsigned** p) {
  if (*p) return PK_OK;
  int rc;
  if ((rc = host_alloc(f, p, 16, hipHostMallocDefault))) return rc;
  **p = 0u;
  return PK_OK;
}

// The bearing model runs on the compact layout's general kernels of one whole filter: everything else says so here, once.
int refuse_bearing(const pk_filter* f, const char* who, const char* what) {
  if (f && f->model == PK_MODEL_BEARING)
    return fail(PK_ERR_UNSUPPORTED, "%s: the bearing measurement model (pk_set_measurement_model) has no kernel for %s; "
                                    "pk_set_measurement_model(f, PK_MODEL_REFERENCE) takes it", who, what);
  return PK_OK;
}

// Behind an observe: every map slot was just rewritten from its source (the receive buffer of the last exchange is free), and ctl
// holds the maximum of the new log-weights
static void observe_done(pk_filter* f) {
  f->src_identity = true;
  f->d.alt = nullptr;
  f->gmax_fused = true;
}

// ---- the colour table's host side
static ColourTable ct_view(const pk_filter* f) { return ColourTable{f->ct_tab, f->ct_depth}; }
// The slots of the live buffer get their colour rows back (no-op while they are valid).  Called at the top of every entry point that
// reads colour rows of slots or hands them out.
static int ensure_colour_rows(pk_filter* f) {
  if (f->colour_rows_valid) return PK_OK;
  {
    Span t(f, PK_T_MATERIALISE);
    launch_colour_rows(f->stream, f->d, ct_view(f), f->ct_qt);
  }
  PK_LAUNCH_CHECK("ensure_colour_rows");
  f->colour_rows_valid = true;
  f->ct_whole += 1;
  return PK_OK;
}
// A download of some particles' maps: only their slots get their rows (behind materialise: slot p is particle p's), and the rest of
// the buffer stays as stale as it was -- a caller that looks at one particle every step does not pay for all of them.
int colour_rows_for_download(pk_filter* f, int64_t p0, int64_t p1) {
  if (f->colour_rows_valid || p0 >= p1) return PK_OK;
  if (p0 == 0 && p1 == f->d.P) return ensure_colour_rows(f);
  {
    Span t(f, PK_T_MATERIALISE);
    ParticleRange range;
    range.p0 = p0;
    range.p1 = p1;
    launch_colour_rows(f->stream, f->d, ct_view(f), f->ct_qt, range);
  }
  PK_LAUNCH_CHECK("colour_rows_for_download");
  return PK_OK;
}
// ... and the mode stays off until the next pk_upload_map
int ct_end(pk_filter* f) {
  f->ct_eligible = false;
  f->ct_engaged = false;
  return ensure_colour_rows(f);
}
// Does the filter's colour-table state let a scan take the table-mode kernel?  (plan_scan asks for the scans that go to k_step_pub's
// 512-lane instances alone, with pruned lists: a scan that kernel stands back from then goes to the general kernels as a whole,
// behind k_colour_rows, and never to k_step_regs.)
static bool ct_state_ok(const pk_filter* f) {
  if (f->opt.colour_table == 0 || !f->ct_eligible || f->ct_sharded || f->grow_on || f->dense || !f->ct_base) return false;
  if (f->d.lay.Lp <= 2 * kPubSmallThreads) return false;
  // beyond the table's end the kernel runs the recurrence itself, lane by lane (exact, slow): the host leaves the mode before the
  // levels it knows of get there (colour_table_margin = 0: never -- the kernel's own handling carries every scan)
  const int margin = f->opt.colour_table_margin >= 0 ? f->opt.colour_table_margin : std::min(16, f->ct_depth > 0 ? f->ct_depth / 2 : 16);
  if (margin > 0 && f->ct_built && f->ct_seen && (int64_t)*reinterpret_cast<volatile unsigned*>(f->ct_seen) + margin >= f->ct_depth) return false;
  return true;
}
// Has no slot of the live buffer a landmark off level 0?  (Every slot: behind an observe each of them was written, by the upload or by
// the kernels; behind a resample some are nobody's any more, which errs on the safe side.)  A full pass over the counts -- P L 4 B read at a stride of slot_bytes, 0.8 GB at 100 000 x 2 000 -- and a
// synchronisation: for pk_set_measurement_noise on an engaged filter only, never for a call of the step.
int ct_maps_untouched(pk_filter* f, bool* untouched) {
  *untouched = false;
  if (!f->ct_max_dev || !f->ct_seen) return PK_OK;
  PK_HIP(hipMemsetAsync(f->ct_max_dev + 1, 0, sizeof(unsigned), f->stream));
  launch_colour_counts_any(f->stream, f->d, f->ct_max_dev + 1);
  PK_LAUNCH_CHECK("colour counts");
  PK_HIP(hipMemcpyAsync(f->ct_seen + 1, f->ct_max_dev + 1, sizeof(unsigned), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  *untouched = f->ct_seen[1] == 0u;
  return PK_OK;
}
// The table is allocated and built when the mode first engages on a map (built again if Qt changed before any update); the depth is
// the option's value at that first scan, and holds until the next pk_upload_map
static int ct_engage(pk_filter* f) {
  int rc;
  const int Lp = f->d.lay.Lp;
  const int depth = f->ct_built ? f->ct_depth : f->opt.colour_table_depth;
  if ((rc = host_word(f, &f->ct_seen))) return rc;
  if ((rc = dev_lazy(f, &f->ct_max_dev, 16))) return rc;
  const bool same_qt = memcmp(&f->ct_qt, &f->qt, sizeof(NoiseD)) == 0;
  if (f->ct_built && same_qt && f->ct_depth == depth) return PK_OK;
  if (!f->ct_tab || f->ct_depth != depth) {
    PK_HIP(hipStreamSynchronize(f->stream));
    dev_free(f, &f->ct_tab);
    if ((rc = dev_alloc(f, &f->ct_tab, (size_t)depth * 6 * Lp))) return rc;
    f->ct_depth = depth;
  }
  f->ct_qt = f->qt;
  launch_colour_table(f->stream, f->ct_base, f->ct_tab, depth, Lp, f->ct_qt);
  PK_HIP(hipMemsetAsync(f->ct_max_dev, 0, 16, f->stream));
  *f->ct_seen = 0u;
  PK_LAUNCH_CHECK("colour table");
  f->ct_built = true;
  return PK_OK;
}

// rows: particles the lists have room for -- all of them (the hand-off routes), or the capped number of second-chance rows
// (ADVICE round 2 / VERDICT round 3: the second chance used to allocate lists for ALL P particles with the route, 6.4 GB at
// 100 000 x 2 000, for the few percent a scan flags at worst)
// (a scan the one-pass kernel stands back from as a WHOLE -- a list overflowed, the publish table does not fit -- flags
// all P particles; the rows grow to what the last scan wanted, so only the first such scan sends particles beyond P / 16 through
// the general kernels)
static int64_t retry_rows(const pk_filter* f) {
  return std::min<int64_t>(f->d.P, std::max<int64_t>(std::max<int64_t>(1024, f->d.P / 16), f->retry_rows_min));
}
static int ensure_handoff(pk_filter* f, int B, int slots, bool lists = true, bool retry_only = false) {
  if (retry_only && f->retry_seen) {
    const int64_t wanted = *reinterpret_cast<volatile unsigned*>(f->retry_seen);  // (the last finished scan's, or the one before)
    if (wanted > retry_rows(f)) f->retry_rows_min = std::min<int64_t>(f->d.P, wanted + wanted / 4);
  }
  const int64_t rows = retry_only ? retry_rows(f) : f->d.P;
  const int64_t need_l = lists ? rows * (int64_t)f->d.lay.Lp * (slots == kSweepSlots ? 2 : 1) : 0;
  const int64_t need_b = lists ? rows * (int64_t)std::max(B, 1) : 0;
  int rc;
  if (retry_only && (rc = dev_lazy(f, &f->fh.row_of, (size_t)f->d.P))) return rc;
  if ((rc = dev_reserve(f, &f->fh.lmpass, &f->fh_cap_l, need_l, need_l))) return rc;
  if ((rc = dev_reserve(f, &f->fh.bcount, &f->fh_cap_b, need_b, need_b))) return rc;
  return dev_lazy(f, &f->fh.pflag, (size_t)f->d.P);
}

// Maps of at most 512 landmarks: the publish / subscribe instance (k_step_pub<1, 256> on candidate lists) or k_step_fused?  The former's
// kernel is the faster one and costs two per-scan kernels whatever the number of particles; measured over P x L (DESIGN.md section 10,
// profiles/r06/pub_small_sweep*.log) the whole step ties at 10 000 x 500 and wins from there on: from 5e6 particle.landmarks on, and
// not below 128 landmarks, where nothing was measured.
constexpr int64_t kPubSmallAutoWork = 5000000;
constexpr int kPubSmallAutoLandmarks = 128;

// Which kernels does this scan get?  The one place that decides (the conditions, kind by kind: DESIGN.md section 4, "Routing").  Reads
// the filter and the scan's facts, touches nothing.  grow: the new-landmark bookkeeping follows the scan -- a kernel of the publish /
// subscribe family (they leave every particle's unmatched blobs as bit rows) or the general association (ids), never another.
// whole: the launches that follow cover every particle.
static ScanPlan plan_scan(const pk_filter* f, int B, bool use_grid, int ncell, int n9, bool want_fast, bool finalize, bool grow, bool whole) {
  ScanPlan p;
  if (!use_grid) return p;
  p.kind = ScanKind::General;
  // the bearing model (pk_set_measurement_model) has the general kernels alone: no hand-off, no one-pass kernel, no stand-by launch
  if (f->model == PK_MODEL_BEARING) return p;
  // unique association (pk_assoc_unique): the settling pass stands between the general association and k_observe, for both models
  if (f->uq.on) return p;
  const int L = f->d.lay.L, Lp = f->d.lay.Lp;
  const bool sweep = L > kFastMaxL || f->opt.fast_observe >= 2;
  auto sweep_fits = [&] { return observe_sweep_plan(f->d, B).grid > 0; };
  auto limited = [&](int ecap) { return f->opt.pub_entry_limit > 0 && ecap > f->opt.pub_entry_limit ? f->opt.pub_entry_limit : ecap; };
  const bool lists_both_ways = f->opt.pub_step && f->opt.cand_lists;
  const bool onepass = want_fast && !finalize && f->opt.fast_observe == 1 && B > 0 && (!grow || (lists_both_ways && B <= 32 * 176));
  if (onepass && f->opt.fused_step && !sweep && n9 > 0 && fused_lds_bytes(ncell, B, n9) <= kFusedMaxLds &&
      (!grow || (step_pub_entry_capacity_small(B) > 0 && B <= 32 * 32))) {
    const bool wanted = grow || (f->opt.pub_small >= 0 ? f->opt.pub_small != 0
                                                   : f->d.P * (int64_t)L >= kPubSmallAutoWork && L >= kPubSmallAutoLandmarks);
    p.kind = wanted && lists_both_ways && step_pub_entry_capacity_small(B) > 0 ? ScanKind::PubSmall : ScanKind::Fused;
    p.route = PK_ROUTE_ML_FUSED;
    if (p.kind == ScanKind::PubSmall) {
      p.cand_slots = kCandSlots;
      p.ecap = limited(step_pub_entry_capacity_small(B));
    }
  } else if (onepass && f->opt.regs_step && L > kFastMaxL && L <= kRegsMaxL && n9 > 0 && regs_lds_bytes(ncell, B, n9) <= kMaxDynLds &&
             (!grow || (step_pub_entry_capacity(B) > 0 && regs_cand_lds_bytes(Lp, B) <= kMaxDynLds && B <= 32 * 96))) {
    // the flags, and -- when the two-sweep kernel can take this scan -- eight-slot hand-off lists for the second chance of the
    // particles k_step_regs flags (growing maps: no second chance -- what the kernel hands on goes to the general kernels, which leave ids)
    p.lists = f->opt.regs_retry && sweep_fits();
    p.retry = p.lists && !grow;
    p.slots = p.lists ? kSweepSlots : kFastSlots;
    p.kind = ScanKind::Regs;
    p.route = PK_ROUTE_ML_REGS;
    if (f->opt.cand_lists && regs_cand_lds_bytes(Lp, B) <= kMaxDynLds) {
      p.cand_slots = kCandSlots;
      p.ecap = f->opt.pub_step ? limited(step_pub_entry_capacity(B)) : 0;
      // pruned lists: k_step_regs' candidate-list instance never takes them (k_cand_entries: skip_cand) and is not even launched
      if (p.ecap > 0) p.kind = f->opt.far_prune || grow ? ScanKind::Pub : ScanKind::PubRegs;
    }
  } else if (onepass && lists_both_ways && L > kRegsMaxL && L <= kPubBigMaxL && step_pub_big_entry_capacity(B) > 0 && sweep_fits()) {
    // what k_step_pub_big flags -- or the whole scan, when a sixteen-entry list overflows or the publish table does not fit LDS --
    // goes through the eight-slot hand-off and k_observe_sweep, then the general kernels
    p.kind = ScanKind::PubBig;
    p.route = PK_ROUTE_ML_PUB_BIG;
    p.lists = true;
    p.retry = !grow;
    p.slots = kSweepSlots;
    p.cand_slots = 2 * kCandSlots;
    p.ecap = limited(step_pub_big_entry_capacity(B));
    if (f->opt.duo_on) {
      step_pub_duo_limits(B, Lp, f->opt.duo_on, &p.duo);
      p.duo.ecap = limited(p.duo.ecap);
      p.duo.park_limit = f->opt.duo_park_limit;
    }
  } else if (want_fast && !grow && !finalize && f->opt.fast_observe && B > 0 && (sweep ? sweep_fits() : observe_fast_lds_bytes(B) <= kMaxDynLds)) {
    // eight hand-off slots per landmark for the large scans (a landmark's colour neighbourhood gets busier with B: at B = 5 000
    // random colours some landmark of every particle passes 5-7 blobs), four (16-byte entries) otherwise; "fast_observe" = 3 forces eight
    p.kind = sweep ? ScanKind::HandoffSweep : ScanKind::HandoffFast;
    p.route = sweep ? PK_ROUTE_ML_SWEEP : PK_ROUTE_ML_HANDOFF;
    p.lists = true;
    p.slots = sweep && (B >= 3000 || f->opt.fast_observe == 3) ? kSweepSlots : kFastSlots;
    // the hand-off instance tests each landmark against the reference particle's candidate list instead of walking the colour grid
    // (sixteen entries per list: with several thousand blobs around the robot eight overflow somewhere in every scan)
    if (f->opt.cand_lists && L < 65535) p.cand_slots = 2 * kCandSlots;
  }
  p.publish = p.ecap > 0;
  p.far = p.publish && f->opt.far_prune;
  // no stand-by kernel behind these: a scan they stand back from goes to the fall-back kernels as a whole
  const bool alone = p.kind == ScanKind::PubSmall || p.kind == ScanKind::Pub || p.kind == ScanKind::PubBig;
  p.flag_fold = alone && whole;
  p.flag_range = alone && !whole;
  p.colour_table = p.kind == ScanKind::Pub && p.far && ct_state_ok(f);
  return p;
}

// Upload one scan for maximum-likelihood association (one block), plan it and enqueue what the plan wants of the association:
// nothing (the one-pass kinds), k_candidates + k_assoc_grid, or k_assoc_brute.  `blobs` may be the staged copy itself (pk_observe_staged).
static int enqueue_association(pk_filter* f, const double* blobs, int B, bool finalize, bool want_fast, AssocLaunch* out, bool grow = false,
                        bool whole = false, const RangeScan* rs = nullptr) {
  int rc;
  pk_filter::Staged& sg = f->staged;
  if (!is_staged_scan(f, blobs, B))
    if ((rc = stage_ml_scan(f, blobs, B, rs))) return rc;
  sg.valid = false;  // consumed
  const MlScanLayout& lay = sg.lay;
  if (!sg.uploaded) {
    if ((rc = upload_scan(f, sg.st, lay.upload_bytes, sg.slot))) return rc;
  }
  sg.uploaded = false;
  f->gmax_fused = false;
  AssocLaunch al;
  al.plan = plan_scan(f, B, sg.use_grid, sg.g.ncell, sg.n9, want_fast, finalize, grow, whole);
  const ScanPlan& plan = al.plan;
  ScanTables& scan = al.scan;
  scan.B = B;
  scan.grid = sg.g;
  scan.n9 = sg.n9;
  scan.blobs = reinterpret_cast<const double*>(f->scan_dev + lay.blobs);
  scan.dir = reinterpret_cast<const double*>(f->scan_dev + lay.dir);
  if (lay.rng) {
    scan.rng = reinterpret_cast<const double*>(f->scan_dev + lay.rng);
    scan.rng_cell = reinterpret_cast<const double*>(f->scan_dev + lay.rng_cell);
  }
  if (sg.use_grid) {
    scan.tables = f->scan_dev + lay.tables;
    scan.exact = reinterpret_cast<const double*>(f->scan_dev + lay.exact);
    scan.order = reinterpret_cast<const unsigned short*>(f->scan_dev + lay.order);
  }
  if (out) {
    *out = al;
    f->route = plan.route;  // (the one place: pk_associate, which passes no `out`, leaves the last observe's)
  }
  // the hand-off's buffers (allocated here, not at the first flagged particle in the middle of a run)
  if (plan.onepass() || plan.lists)
    if ((rc = ensure_handoff(f, B, plan.slots, plan.lists, plan.ranged()))) return rc;
  if (plan.onepass()) return PK_OK;
  if (plan.kind == ScanKind::Brute && assoc_brute_lds_bytes(B) > kMaxDynLds)
    return fail(PK_ERR_UNSUPPORTED,
                "maximum-likelihood association of %d blobs: neither the colour-grid tables nor the brute-force kernel's "
                "%zu bytes of per-blob state fit the workgroup's %zu bytes of LDS", B, assoc_brute_lds_bytes(B), (size_t)kMaxDynLds);
  if ((rc = ct_end(f))) return rc;  // (the general association reads the slots' colour rows)
  Span t(f, PK_T_ASSOC);
  // unique association: final ids from either kernel, then k_assoc_unique on them, in this span
  const bool unique = f->uq.on;
  if (unique) finalize = true;
  if (plan.kind == ScanKind::Brute) {
    launch_assoc_brute(f->stream, f->d, scan, f->ids_dev, f->model, f->qt.q00);
    return unique ? unique_settle(f, scan) : PK_OK;
  }
  if (f->model == PK_MODEL_BEARING) {
    launch_assoc_grid_bearing(f->stream, f->d, scan, f->ids_dev, finalize, f->qt.q00);
    return unique ? unique_settle(f, scan) : PK_OK;
  }
  FastHandoff fh{};
  CandTable cand;
  if (plan.lists) {
    f->fh.slots = plan.slots;
    fh = f->fh;
    fh.n_flagged = ctl_n_flagged(f);
    if (plan.cand_slots) {  // (a list that overflows leaves the scan to the grid walk)
      if ((rc = dev_lazy(f, &f->cand_dev, ((size_t)f->d.lay.Lp + kCandSpare) * 3))) return rc;
      launch_summary_partials(f->stream, f->d, f->partial, f->out4);  // the reference pose: the particles' mean
      CandidatesLaunch cl{};
      cl.rec = f->cand_dev;
      cl.over = ctl_cand_over(f);
      cl.slots = plan.cand_slots;
      cl.pose_sums4 = f->out4;
      launch_candidates(f->stream, f->d, scan, cl);
      cand.rec = f->cand_dev;
      cand.over = ctl_cand_over(f);
      cand.slots = plan.cand_slots;
    }
  }
  launch_assoc_grid(f->stream, f->d, scan, f->ids_dev, finalize, fh, cand);
  return unique ? unique_settle(f, scan) : PK_OK;
}

// The dense path (maps with xy-rgb coupling or a coupled Qt): one general kernel does association (or takes the ids),
// EKF updates and weights.  update = false: association only.
static int dense_observe(pk_filter* f, const double* blobs, int32_t B, const int32_t* ids, int32_t* ids_out, bool reset,
                         bool update) {
  int rc;
  const MapLayout& lay = f->d.lay;
  f->staged.valid = false;
  if (int rb = refuse_bearing(f, "pk_observe", "the dense layout (covariances or a Qt that couple position, bearing and colour)")) return rb;
  if (dense_lds_bytes(lay.Lp, B) > kMaxDynLds)
    return fail(PK_ERR_UNSUPPORTED, "dense observe: %d landmarks and %d blobs need %zu bytes of LDS per particle, the workgroup has %zu",
                lay.Lp, B, dense_lds_bytes(lay.Lp, B), (size_t)kMaxDynLds);
  const DenseScanLayout blk = dense_scan_layout(B);
  unsigned char* st = nullptr;
  int slot = 0;
  if ((rc = take_stage(f, blk.upload_bytes, &st, &slot))) return rc;
  if (ids_out && !ids && (rc = ensure_ids_capacity(f, B))) return rc;
  memset(st, 0, kCtlBytes);
  if (B > 0) {
    memmove(st + blk.blobs, blobs, (size_t)B * 4 * sizeof(double));
    blob_directions(reinterpret_cast<const double*>(st + blk.blobs), B, reinterpret_cast<double*>(st + blk.dir));
    if (ids) memcpy(st + blk.ids, ids, (size_t)B * sizeof(int32_t));
  }
  if ((rc = upload_scan(f, st, blk.upload_bytes, slot))) return rc;
  ObserveExtras ex;
  ex.reset = reset;
  ex.gmax_key = ctl_gmax_key(f);
  {
    Span t(f, update ? PK_T_OBSERVE : PK_T_ASSOC);
    ScanTables scan;
    scan.B = B;
    scan.blobs = reinterpret_cast<const double*>(f->scan_dev + blk.blobs);
    scan.dir = reinterpret_cast<const double*>(f->scan_dev + blk.dir);
    const int32_t* ids_in = ids ? reinterpret_cast<const int32_t*>(f->scan_dev + blk.ids) : nullptr;
    int32_t* ids_to = (ids_out && !ids) ? f->ids_dev : nullptr;
    launch_observe_dense(f->stream, f->d, scan, ids_in, ids_to, f->qt16, update, ex);
  }
  PK_LAUNCH_CHECK("pk_observe (dense)");
  if (update) {
    observe_done(f);
    f->route = PK_ROUTE_DENSE;
  } else {
    f->gmax_fused = false;  // the control words were overwritten by this upload
  }
  return return_ids(f, ids_out, B, ids);
}

// ---- the one-pass kinds (ScanPlan::onepass) in three pieces, so that the sharded filter can run the middle one on a part of the
// particles while the rest are still on the wire (pk_observe_staged_range) ------------------------------------------------
// 1. the reference particle's candidate lists and the publish table's layout, timed with the association; first their buffers
static int ensure_inverse_lists(pk_filter* f, int B, int slots = kCandSlots) {
  int rc;
  B = B * (slots / kCandSlots);  // (capacity in units of eight-entry lists: sixteen-entry lists take two)
  if (B > f->bcand_cap) {
    const int64_t cap = (int64_t)B + B / 4 + 64;
    if ((rc = dev_reserve_group(f, &f->bcand_cap, (int64_t)B, cap, want(&f->bcnt_dev, (size_t)cap), want(&f->brec_dev, (size_t)cap),
                                want(&f->binfo_dev, (size_t)cap), want(&f->glist_dev, 2 * (size_t)cap + 1 + 256 + 16),
                                want(&f->gate4_dev, (size_t)cap))))
      return rc;
    // (empty inverse lists: k_candidates appends to them, k_cand_entries empties them again behind its last read)
    PK_HIP(hipMemsetAsync(f->bcnt_dev, 0, (size_t)cap * sizeof(unsigned), f->stream));
    PK_HIP(hipMemsetAsync(f->brec_dev, 0xFF, (size_t)cap * sizeof(uint4), f->stream));
  }
  return PK_OK;
}
// the per-map buffers of the plan's lists, allocated when a scan first wants them
static int ensure_list_buffers(pk_filter* f, const ScanPlan& plan, int B) {
  int rc;
  const size_t Lpp = (size_t)f->d.lay.Lp + kCandSpare;
  const bool big = plan.kind == ScanKind::PubBig;  // sixteen-entry lists both ways
  if ((rc = dev_lazy(f, &f->cand_dev, Lpp * 3))) return rc;
  if (!plan.publish) return PK_OK;
  if ((rc = big ? dev_lazy(f, &f->erec_dev2, Lpp * 2) : dev_lazy(f, &f->erec_dev, Lpp))) return rc;
  if ((rc = dev_lazy(f, &f->npass_dev, Lpp))) return rc;
  if ((rc = dev_lazy(f, &f->far_dev, Lpp * 3))) return rc;
  if (big && (rc = dev_lazy(f, &f->prim_dev, prim_table_uint4(f->d.lay.Lp)))) return rc;
  return ensure_inverse_lists(f, B, plan.cand_slots);
}
// ref: the particle whose MAP the candidate lists are made from -- particle 0, or in a split step the first particle of the range
// that has been filled already (the slots at either end still hold the old generation then)
static int onepass_prepare(pk_filter* f, const AssocLaunch& al, PubTables* pub, int64_t ref = 0) {
  int rc;
  const ScanPlan& plan = al.plan;
  *pub = PubTables();
  f->pub_ecap = plan.ecap;
  if (!plan.cand_slots) return PK_OK;
  if ((rc = ensure_list_buffers(f, plan, al.scan.B))) return rc;
  Span t(f, PK_T_ASSOC);
  CandidatesLaunch cl{};
  cl.rec = f->cand_dev;
  cl.over = ctl_cand_over(f);
  cl.slots = plan.cand_slots;
  cl.ref_particle = ref;
  // the reference pose: the particles' mean -- from the sums the motion launch left, or (poses touched since) two launches
  cl.pose_sums4 = f->out4;
  if (f->pose_part_ok)
    cl.pose_part = f->pose_part;
  else
    launch_summary_partials(f->stream, f->d, f->partial, f->out4);
  CandTable& cand = pub->cand;
  cand.rec = f->cand_dev;
  cand.over = ctl_cand_over(f);
  cand.slots = plan.cand_slots;
  if (!plan.publish) {
    launch_candidates(f->stream, f->d, al.scan, cl);
    return PK_OK;
  }
  // candidate lists both ways, and the publish table's layout
  const bool big = plan.kind == ScanKind::PubBig;  // the two-pass kernels: sixteen-entry lists
  pub->erec = big ? f->erec_dev2 : f->erec_dev;
  pub->glist = f->glist_dev;
  pub->bcnt = f->bcnt_dev;
  pub->brec = f->brec_dev;
  pub->binfo = f->binfo_dev;
  pub->npass = f->npass_dev;
  pub->stats = ctl_pub_stats(f);
  pub->skip_pub = ctl_skip_pub(f);
  pub->skip_cand = ctl_skip_cand(f);
  pub->ecap = plan.ecap;
  if (big) {  // ... which also get the blobs' float records, the primary-blob table and the choice between their two instances
    pub->gate4 = f->gate4_dev;
    pub->prim = f->prim_dev;
    pub->skip_duo = ctl_skip_duo(f);
    pub->skip_big = ctl_skip_big(f);
  }
  pub->duo = plan.duo;
  cl.bcnt = pub->bcnt;
  cl.brec = pub->brec;
  cl.npass = pub->npass;
  if (plan.far) cl.far = f->far_dev;
  if (plan.colour_table) cl.ct = ct_view(f);
  if (!big) cl.qt = &f->ct_qt;
  launch_candidates(f->stream, f->d, al.scan, cl);
  CandEntriesLaunch ce;
  ce.pub = *pub;
  ce.pruned = plan.far;
  if (plan.flag_fold) {
    ce.flag_all = f->fh.pflag;
    ce.n_flagged = ctl_n_flagged(f);
  }
  launch_cand_entries(f->stream, f->d, al.scan, ce);
  cand.far = cl.far;
  if (!big) cand.skip_cand = ctl_skip_cand(f);
  return PK_OK;
}
// 2. the one-pass kernel on the particles [p0, p1) (k_step_fused: the whole range only)
static int onepass_launch(pk_filter* f, const AssocLaunch& al, const ObserveExtras& ex, const PubTables& pub, const ParticleRange& range) {
  const ScanPlan& plan = al.plan;
  FastHandoff fh = f->fh;
  fh.n_flagged = ctl_n_flagged(f);
  fh.flags_only = true;
  Span t(f, PK_T_OBSERVE);
  ObserveExtras e1 = ex;
  e1.flip = false;
  if (plan.colour_table) {
    e1.ctab = f->ct_tab;
    e1.ctab_depth = f->ct_depth;
    e1.ctab_max = f->ct_max_dev;
  }
  e1.lean = f->opt.pub_lean;
  e1.lean_stats = ctl_pub_stats(f);
  switch (plan.kind) {
    case ScanKind::PubBig:
      // the scan goes to ONE of the two instances (k_cand_entries decided which: the two-workgroups-per-CU instance when its share of
      // LDS holds the scan's publish table); both are launched, one returns at once
      if (plan.duo.tbytes > 0) launch_step_pub_duo(f->stream, f->d, al.scan, fh, f->qt, e1, pub, range);
      launch_step_pub_big(f->stream, f->d, al.scan, fh, f->qt, e1, pub, range);
      break;
    case ScanKind::PubSmall:
    case ScanKind::Pub:
    case ScanKind::PubRegs:
      launch_step_pub(f->stream, f->d, al.scan, fh, f->qt, e1, pub, range);
      if (plan.kind != ScanKind::PubRegs) break;
      [[fallthrough]];  // (the stand-by: returns at once unless k_step_pub stood back)
    case ScanKind::Regs:
      launch_step_regs(f->stream, f->d, al.scan, fh, f->qt, e1, f->opt.regs_warm, pub.cand, range);
      break;
    case ScanKind::Fused:
      launch_step_fused(f->stream, f->d, al.scan, fh, f->qt, e1);
      break;
    default:
      break;
  }
  // a scan the kernel stood back from (a list overflowed, the table did not fit): every particle to the fall-back kernels
  if (plan.flag_range) launch_flag_range_if(f->stream, ctl_skip_pub(f), fh.pflag, fh.n_flagged, range.p0, range.end(f->d.P));
  return PK_OK;
}
// k_observe_sweep's per-workgroup result lists
static int ensure_sweep_results(pk_filter* f, const SweepPlan& plan) {
  const size_t need = (size_t)plan.grid * plan.results_per_wg;
  return dev_reserve(f, &f->sweep_results, &f->sweep_cap, need, need);
}
// 3. what the one-pass kernel flagged, over all particles: second chance, then the general kernels (which swap the map buffers)
static int onepass_finish(pk_filter* f, const AssocLaunch& al, const ObserveExtras& ex, const CandTable& cand) {
  int rc;
  FastHandoff fh = f->fh;
  fh.n_flagged = ctl_n_flagged(f);
  fh.flags_only = true;
  if (al.plan.retry) {
    // second chance for what k_step_regs flagged (some landmark passes more than its four register slots -- 2 us per
    // particle in the general kernels, and up to 9 % of the particles at some poses of the bench's trajectory): the
    // hand-off instance with eight slots and k_observe_sweep, both on the flagged particles only (timed with the other
    // fallbacks in the association slot: the observe slot holds the one-pass kernel alone, one span per launch)
    Span t(f, PK_T_ASSOC);
    const SweepPlan plan = observe_sweep_plan(f->d, al.scan.B);
    if ((rc = ensure_sweep_results(f, plan))) return rc;
    FastHandoff fr = f->fh;
    fr.slots = kSweepSlots;
    fr.retry = true;
    fr.n_flagged = ctl_n_flagged(f);
    fr.row_next = ctl_retry_rows(f);
    fr.row_cap = retry_rows(f);
    // (pruned candidate lists are the publish / subscribe kernels' alone: the hand-off instance walks the colour grid then)
    const CandTable unpruned = cand.far ? CandTable() : cand;
    launch_assoc_grid(f->stream, f->d, al.scan, f->ids_dev, false, fr, unpruned);
    ObserveExtras e3 = ex;
    e3.flip = false;
    e3.sweep_only_value = 2;
    e3.n_flagged = ctl_n_flagged(f);
    launch_observe_sweep(f->stream, f->d, al.scan, fr, f->qt, e3, plan, f->sweep_results);
    (void)host_word(f, &f->retry_seen);  // (without it the rows do not grow: no error)
    if (f->retry_seen) (void)hipMemcpyAsync(f->retry_seen, ctl_retry_rows(f), sizeof(unsigned), hipMemcpyDeviceToHost, f->stream);
    (void)hipGetLastError();
  }
  // the particles still flagged (a landmark passing more blobs than any slot count): general kernels, both timed in the
  // association slot
  Span t(f, PK_T_ASSOC);
  launch_assoc_grid(f->stream, f->d, al.scan, f->ids_dev, false, fh);
  ObserveExtras e2 = ex;
  e2.only_flagged = f->fh.pflag;
  e2.n_flagged = ctl_n_flagged(f);
  launch_observe(f->stream, f->d, al.scan, f->ids_dev, f->qt, e2);
  return PK_OK;
}

// Behind the observe launches of a growing filter's non-empty scan (pk_observe, pk_step; pk_propose / pk_propose_odom with
// pk_proposal_grow): :92-95 for every particle at its live pose, on the ids the association left in HBM -- or, where the last
// observe's one-pass kernel left them (grow_bits), on its bit rows -- (every particle's slot is its own now), then retirement's pass
// with its clock advanced, then the launch check.  The one place: the plain path and the proposal's cannot drift apart.
int grow_bookkeeping(pk_filter* f, const char* who, const ScanTables& scan, int32_t B) {
  {
    Span t(f, PK_T_OBSERVE);
    launch_new_landmarks(f->stream, f->d, f->grow, f->grow_init, f->qt.q00, f->ids_dev, scan.blobs, B, f->grow_bits ? f->unm_dev : nullptr,
                         f->unm_words, f->grow_bits ? f->fh.pflag : nullptr,
                         f->grow_ranges ? scan.rng : nullptr);  // (pk_grow_ranges; NULL too when no blob has a finite range)
    if (f->retire.on()) {  // pk_grow_retire: stale readings and unconfirmed features go, behind this scan's bookkeeping
      f->retire.t += 1u;
      if (f->view.on)  // pk_grow_view: the first two counters are this pass's
        PK_HIP(hipMemsetAsync(f->view.stats, 0, 2 * sizeof(unsigned long long), f->stream));
      launch_grow_retire(f->stream, f->d, f->grow, f->retire, f->view);
    }
  }
  const std::string what = std::string(who) + " (new landmarks)";
  PK_LAUNCH_CHECK(what.c_str());
  return PK_OK;
}

int observe_impl(pk_filter* f, const double* blobs, int32_t B, const int32_t* ids, int32_t* ids_out,
                        bool reset) {
  if (!f) return fail(PK_ERR_INVALID, "pk_observe: NULL handle");
  int rc;
  // the ranges of this scan (pk_scan_ranges): armed ones are consumed here, whatever follows; a staged scan brought its own, and
  // is held to the same refusals once more (the filter may have changed since pk_stage_scan) -- refused, it is discarded
  RangeScan rs;
  if (!is_staged_scan(f, blobs, B)) {
    if ((rc = ranges_take(f, "pk_observe", B, &rs))) return rc;
  } else if (f->staged.with_ranges && (rc = refuse_ranges(f, "pk_observe", B, f->staged.B))) {
    f->staged.valid = false;
    return rc;
  }
  if ((rc = check_scan_shape(f, "pk_observe", blobs, B))) return rc;
  if (f->split.active) return fail(PK_ERR_STATE, "pk_observe: a split observe is in progress (pk_observe_staged_range with last = 1 ends it)");
  if ((rc = use_device(f))) return rc;
  if ((rc = check_scan_values(f, "pk_observe", blobs, B, &ids))) return rc;
  // section 8(f4) on the device: the unmatched blobs of every particle go through the new-landmark bookkeeping behind the observe
  const bool grow = f->grow_on && B > 0;
  if (grow && ids) return refuse_grow_ids("pk_observe");
  if (grow && f->dense)
    return fail(PK_ERR_STATE, "pk_observe: the new-landmark bookkeeping (pk_grow_enable) writes the compact landmark layout; this filter "
                              "is on the dense one (a covariance or Qt that couples position and colour)");
  // unique association (pk_assoc_unique) is the maximum-likelihood scans' alone: supplied ids are applied as ever
  f->uq.last = false;
  if (!ids && B > 0 && (rc = unique_check(f, "pk_observe", B))) {
    f->staged.valid = false;
    f->dense_staged.clear();
    return rc;
  }
  f->ct_updated = true;
  if (f->dense) return dense_observe(f, blobs, B, ids, ids_out, reset, true);
  ObserveExtras ex;
  ex.reset = reset;
  ex.model = f->model;
  if (ids) {
    if ((rc = ct_end(f))) return rc;  // (another route: k_observe streams whole slots)
    f->staged.valid = false;  // a staged ML scan does not survive another observe
    KnownScan ks;
    if ((rc = upload_known_scan(f, blobs, B, ids, false, &ks, &rs))) return rc;
    if (ks.lay.rng) ex.rng = reinterpret_cast<const double*>(f->scan_dev + ks.lay.rng);
    ex.single_sightings = ks.single_sightings;
    ex.gmax_key = ctl_gmax_key(f);
    {
      Span t(f, PK_T_OBSERVE);
      launch_observe(f->stream, f->d, known_scan_tables(f, ks, B), known_chains(f, ks), f->qt, ex);
    }
    PK_LAUNCH_CHECK("pk_observe");
    observe_done(f);
    f->route = PK_ROUTE_KNOWN_IDS;
    return return_ids(f, ids_out, B, ids);
  }
  // maximum-likelihood association on the device
  AssocLaunch al;
  // (ids wanted: the association kernel + k_observe; growing maps: a publish / subscribe kernel, or that)
  if ((rc = enqueue_association(f, blobs, B, false, ids_out == nullptr, &al, grow, true, &rs))) return rc;
  ex.rng = al.scan.rng;
  const ScanPlan& plan = al.plan;
  // the colour table's mode: this scan takes the table-mode kernel, or the mode ends here (the slots get their colour rows first)
  if (plan.colour_table ? (rc = ct_engage(f)) : (rc = ct_end(f))) return rc;
  f->grow_bits = false;
  if (grow && plan.onepass()) {
    // round 6: the one-pass kernel leaves every particle's unmatched blobs as a bit row (scan order)
    const int words = 2 * ((B + 63) / 64);
    if ((rc = dev_reserve(f, &f->unm_dev, &f->unm_cap, (int64_t)f->d.P * words, (int64_t)f->d.P * (words + words / 4 + 2)))) return rc;
    f->unm_words = words;
    ex.unm = f->unm_dev;
    ex.unm_words = words;
    f->grow_bits = true;
  }
  ex.gmax_key = ctl_gmax_key(f);
  if (plan.onepass()) {
    PubTables pub;
    if ((rc = onepass_prepare(f, al, &pub))) return rc;
    if ((rc = onepass_launch(f, al, ex, pub, ParticleRange()))) return rc;
    if (plan.colour_table) {
      // what the kernel handed on (or the whole scan, where it stood back) goes to kernels that read whole slots: the SOURCE slots of
      // those particles get their colour rows from the table first -- a launch that returns in its first wave on the usual scan
      Span t(f, PK_T_ASSOC);
      launch_colour_rows(f->stream, f->d, ct_view(f), f->ct_qt, ParticleRange(), f->fh.pflag, ctl_n_flagged(f));
      (void)hipMemcpyAsync(f->ct_seen, f->ct_max_dev, sizeof(unsigned), hipMemcpyDeviceToHost, f->stream);
      (void)hipGetLastError();
      f->colour_rows_valid = false;
      f->ct_engaged = true;
      f->ct_scans += 1;
    }
    if ((rc = onepass_finish(f, al, ex, pub.cand))) return rc;
  } else {
    Span t(f, PK_T_OBSERVE);
    if (plan.lists) {  // the hand-off was written
      ObserveExtras e1 = ex;
      e1.flip = false;
      if (plan.kind == ScanKind::HandoffSweep) {
        const SweepPlan sweep = observe_sweep_plan(f->d, B);
        if ((rc = ensure_sweep_results(f, sweep))) return rc;
        launch_observe_sweep(f->stream, f->d, al.scan, f->fh, f->qt, e1, sweep, f->sweep_results);
      } else {
        launch_observe_fast(f->stream, f->d, al.scan, f->fh, f->qt, e1);
      }
      ex.only_flagged = f->fh.pflag;
      ex.n_flagged = ctl_n_flagged(f);
    }
    launch_observe(f->stream, f->d, al.scan, f->ids_dev, f->qt, ex);
  }
  PK_LAUNCH_CHECK("pk_observe");
  observe_done(f);
  if (grow && (rc = grow_bookkeeping(f, "pk_observe", al.scan, B))) return rc;
  if ((rc = return_ids(f, ids_out, B, nullptr))) return rc;
  return ids_out && B > 0 ? unique_error(f, "pk_observe") : PK_OK;  // (behind return_ids' synchronisation)
}

// A proposal step's scan (pk_api_propose.hip) on the device, ahead of k_propose: supplied ids as pk_observe uploads them -- the block
// ctl | blobs | first | next, and behind it the id row itself -- or the bearing model's association at the live (predicted) poses,
// which leaves tentative ids in ids_dev and touches no state.  The caller has checked the blobs, the ids and the filter.  rs: the
// ranges the step took (pk_proposal_ranges), staged as pk_observe stages them -- a scan without a finite range stages the bytes
// it always staged.  grow: the new-landmark bookkeeping follows the step (pk_proposal_grow), as plan_scan is told.
int proposal_scan(pk_filter* f, const double* blobs, int32_t B, const int32_t* ids, ProposalScan* out, const RangeScan* rs, bool grow) {
  int rc;
  *out = ProposalScan();
  f->ct_updated = true;
  f->uq.last = false;  // (the proposal is refused while unique association is on: this scan is not in the mode)
  if (ids) {
    if ((rc = ct_end(f))) return rc;
    f->staged.valid = false;
    KnownScan ks;
    if ((rc = upload_known_scan(f, blobs, B, ids, true, &ks, rs))) return rc;
    if (ks.lay.rng) out->rng = reinterpret_cast<const double*>(f->scan_dev + ks.lay.rng);
    f->gmax_fused = false;
    out->scan = known_scan_tables(f, ks, B);
    out->known = known_chains(f, ks);
    out->known.n_unmatched = 0;  // (k_observe_proposed takes the weight from k_propose, unmatched blobs and all)
    out->ids = reinterpret_cast<int32_t*>(f->scan_dev + ks.lay.ids);
    return PK_OK;
  }
  AssocLaunch al;
  if ((rc = enqueue_association(f, blobs, B, false, false, &al, grow, true, rs))) return rc;
  if (al.plan.onepass()) return fail(PK_ERR_UNSUPPORTED, "pk_propose: the scan did not take the general association");
  f->grow_bits = false;  // (the bookkeeping behind this scan reads the ids, never an earlier observe's bit rows)
  if ((rc = ct_end(f))) return rc;
  out->scan = al.scan;
  out->rng = al.scan.rng;
  out->ids = f->ids_dev;
  return PK_OK;
}
// ... and behind its observe launch
void proposal_observed(pk_filter* f, bool known) {
  observe_done(f);
  f->route = known ? PK_ROUTE_KNOWN_IDS : PK_ROUTE_ML_GENERAL;
}

extern "C" {

int pk_observe(pk_filter* f, const double* blobs, int32_t B, const int32_t* ids, int32_t* ids_out) {
  return observe_impl(f, blobs, B, ids, ids_out, false);
}

int pk_observe_fresh(pk_filter* f, const double* blobs, int32_t B, const int32_t* ids, int32_t* ids_out) {
  return observe_impl(f, blobs, B, ids, ids_out, true);
}

int pk_observe_staged(pk_filter* f, int32_t fresh) {
  if (!f) return fail(PK_ERR_INVALID, "pk_observe_staged: NULL handle");
  if (f->dense && !f->dense_staged.empty()) {
    std::vector<double> b;
    b.swap(f->dense_staged);
    return observe_impl(f, b.data(), (int32_t)(b.size() / 4), nullptr, nullptr, fresh != 0);
  }
  if (!f->staged.valid) return fail(PK_ERR_STATE, "pk_observe_staged: no staged scan (pk_stage_scan)");
  return observe_impl(f, staged_blobs(f->staged), f->staged.B, nullptr, nullptr, fresh != 0);
}

int pk_staged_takes_regs(pk_filter* f) {
  if (!f || f->dense || f->grow_on || !f->staged.valid) return 0;  // (growing maps: whole observes only)
  const pk_filter::Staged& sg = f->staged;
  return plan_scan(f, sg.B, sg.use_grid, sg.g.ncell, sg.n9, true, false, false, false).ranged() ? 1 : 0;
}

int pk_observe_staged_range(pk_filter* f, int32_t fresh, int64_t p0, int64_t p1, int32_t first, int32_t last) {
  if (!f) return fail(PK_ERR_INVALID, "pk_observe_staged_range: NULL handle");
  if (int rc = refuse_path(f, "pk_observe_staged_range")) return rc;
  if (int rc = refuse_bearing(f, "pk_observe_staged_range", "the ranged and split observes of the sharded step")) return rc;
  if (int rc = unique_refuse(f, "pk_observe_staged_range", "the ranged and split observes of the sharded step")) return rc;
  if (p0 < 0 || p1 < p0 || p1 > f->d.P) return fail(PK_ERR_INVALID, "pk_observe_staged_range: bad particle range [%lld, %lld)", (long long)p0, (long long)p1);
  if (f->grow_on) return fail(PK_ERR_STATE, "pk_observe_staged_range: the new-landmark bookkeeping (pk_grow_enable) runs behind whole observes (pk_observe / pk_observe_staged)");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = ct_end(f))) return rc;  // (ranged observes: another route)
  f->ct_updated = true;
  pk_filter::Split& sp = f->split;
  if (first) {
    if (sp.active) return fail(PK_ERR_STATE, "pk_observe_staged_range: the previous split observe was not finished (last = 1)");
    if (!pk_staged_takes_regs(f))
      return fail(PK_ERR_STATE, "pk_observe_staged_range: needs a staged scan that takes the register route (pk_staged_takes_regs)");
    sp.reset = fresh != 0;
    sp.al = AssocLaunch();
    if ((rc = enqueue_association(f, staged_blobs(f->staged), f->staged.B, false, true, &sp.al))) return rc;
    if (!sp.al.plan.ranged()) return fail(PK_ERR_STATE, "pk_observe_staged_range: the scan did not take the register route");
    if ((rc = onepass_prepare(f, sp.al, &sp.pub, p1 > p0 ? p0 : 0))) return rc;
    sp.active = true;
  } else if (!sp.active) {
    return fail(PK_ERR_STATE, "pk_observe_staged_range: no split observe in progress (first = 1)");
  }
  ObserveExtras ex;
  ex.reset = sp.reset;
  ex.gmax_key = ctl_gmax_key(f);
  // the first part of a split step runs while the exchange is in flight: it leaves some CUs to the collective's kernels
  ParticleRange range;
  range.p0 = p0;
  range.p1 = p1;
  if (first && !last) range.reserve_cus = f->opt.split_reserve_cus;
  if (p1 > p0 && (rc = onepass_launch(f, sp.al, ex, sp.pub, range))) {
    sp.active = false;  // a failed piece ends the split observe: the filter is not left waiting for a "last" that cannot come
    return rc;
  }
  if (last) {
    sp.active = false;
    if ((rc = onepass_finish(f, sp.al, ex, sp.pub.cand))) return rc;
    PK_LAUNCH_CHECK("pk_observe_staged_range");
    observe_done(f);
  }
  return PK_OK;
}

int pk_associate(pk_filter* f, const double* blobs, int32_t B, int32_t* ids_out) {
  if (!f || !ids_out) return fail(PK_ERR_INVALID, "pk_associate: NULL argument");
  RangeScan rs;
  int rc;
  if ((rc = ranges_take(f, "pk_associate", B, &rs))) return rc;
  if ((rc = check_scan_shape(f, "pk_associate", blobs, B))) return rc;
  if (B == 0) return PK_OK;
  if ((rc = use_device(f))) return rc;
  if ((rc = check_scan_values(f, "pk_associate", blobs, B))) return rc;
  f->uq.last = false;
  if ((rc = unique_check(f, "pk_associate", B))) return rc;
  if (f->dense) return dense_observe(f, blobs, B, nullptr, ids_out, false, false);
  if ((rc = ensure_colour_rows(f))) return rc;  // (the colour table's mode goes on: nothing is updated)
  {
    const bool keep = f->ct_eligible, engaged = f->ct_engaged;  // (enqueue_association ends the mode where it launches the general association)
    rc = enqueue_association(f, blobs, B, true, false, nullptr, false, false, &rs);
    f->ct_eligible = keep;
    f->ct_engaged = engaged;
  }
  if (rc) return rc;
  PK_LAUNCH_CHECK("pk_associate");
  if ((rc = return_ids(f, ids_out, B, nullptr))) return rc;
  return unique_error(f, "pk_associate");
}

int pk_set_measurement_model(pk_filter* f, int32_t model) {
  if (!f) return fail(PK_ERR_INVALID, "pk_set_measurement_model: NULL handle");
  if (model != PK_MODEL_REFERENCE && model != PK_MODEL_BEARING)
    return fail(PK_ERR_INVALID, "pk_set_measurement_model: %d is neither PK_MODEL_REFERENCE (0) nor PK_MODEL_BEARING (1)", (int)model);
  if (f->split.active) return fail(PK_ERR_STATE, "pk_set_measurement_model: a split observe is in progress");
  f->model = model;  // (a staged scan stays: its tables serve both models)
  return PK_OK;
}
int pk_measurement_model(const pk_filter* f, int32_t* model) {
  if (!f || !model) return fail(PK_ERR_INVALID, "pk_measurement_model: NULL argument");
  *model = f->model;
  return PK_OK;
}

int pk_observe_route(const pk_filter* f) { return f ? f->route : PK_ROUTE_NONE; }
int pk_observe_flagged(pk_filter* f, int64_t* flagged, int64_t* cand_overflow) {
  if (!f) return fail(PK_ERR_INVALID, "pk_observe_flagged: NULL handle");
  int rc;
  if ((rc = use_device(f))) return rc;
  unsigned w[2] = {0u, 0u};
  if (f->scan_dev && f->route != PK_ROUTE_NONE && f->route != PK_ROUTE_KNOWN_IDS) {
    PK_HIP(hipMemcpyAsync(w, ctl_n_flagged(f), sizeof(w), hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
  }
  if (flagged) *flagged = w[0];
  if (cand_overflow) *cand_overflow = w[1];
  return PK_OK;
}
/* second-chance rows: how many the last scan wanted (particles the one-pass kernel flagged) and how many there are */
int pk_observe_retry_rows(pk_filter* f, int64_t* wanted, int64_t* capacity) {
  if (!f) return fail(PK_ERR_INVALID, "pk_observe_retry_rows: NULL handle");
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipStreamSynchronize(f->stream));
  if (wanted) *wanted = f->retry_seen ? (int64_t)*f->retry_seen : 0;
  if (capacity) *capacity = retry_rows(f);
  return PK_OK;
}
int pk_observe_flags(pk_filter* f, uint8_t* flags) {
  if (!f || !flags) return fail(PK_ERR_INVALID, "pk_observe_flags: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  const bool onepass = f->route == PK_ROUTE_ML_REGS || f->route == PK_ROUTE_ML_FUSED || f->route == PK_ROUTE_ML_PUB_BIG;
  if (onepass && f->fh.pflag) {
    PK_HIP(hipMemcpyAsync(flags, f->fh.pflag, (size_t)f->d.P, hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
  } else {
    memset(flags, 0, (size_t)f->d.P);
  }
  return PK_OK;
}
int pk_observe_published(pk_filter* f, int32_t* published) {
  if (!f || !published) return fail(PK_ERR_INVALID, "pk_observe_published: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  *published = 0;
  if (f->scan_dev && (f->route == PK_ROUTE_ML_REGS || f->route == PK_ROUTE_ML_FUSED || f->route == PK_ROUTE_ML_PUB_BIG) && f->pub_ecap > 0) {
    unsigned w = 1u;
    PK_HIP(hipMemcpyAsync(&w, ctl_skip_pub(f), sizeof(w), hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    *published = w == 0u ? 1 : 0;
  }
  return PK_OK;
}
int pk_observe_pub_stats(pk_filter* f, int64_t stats[6]) {
  if (!f || !stats) return fail(PK_ERR_INVALID, "pk_observe_pub_stats: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  for (int i = 0; i < 6; ++i) stats[i] = 0;
  if (f->scan_dev && (f->route == PK_ROUTE_ML_REGS || f->route == PK_ROUTE_ML_FUSED || f->route == PK_ROUTE_ML_PUB_BIG) && f->pub_ecap > 0) {
    unsigned w[4] = {0u, 0u, 0u, 0u}, sk[2] = {1u, 1u};
    PK_HIP(hipMemcpyAsync(w, ctl_pub_stats(f), sizeof(w), hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipMemcpyAsync(&sk[0], ctl_skip_pub(f), sizeof(unsigned), hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipMemcpyAsync(&sk[1], ctl_skip_duo(f), sizeof(unsigned), hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    for (int i = 0; i < 4; ++i) stats[i] = w[i];
    stats[4] = f->pub_ecap;
    // which instance worked on the scan: 0 none of the publish / subscribe kernels, 1 the one-workgroup-per-CU instance, 2 k_step_pub_duo
    stats[5] = sk[0] != 0u ? 0 : (f->route == PK_ROUTE_ML_PUB_BIG && f->opt.duo_on && sk[1] == 0u) ? 1 + f->opt.duo_on : 1;
  }
  return PK_OK;
}
int pk_observe_lean_stats(pk_filter* f, int64_t out[3]) {
  if (!f || !out) return fail(PK_ERR_INVALID, "pk_observe_lean_stats: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  for (int i = 0; i < 3; ++i) out[i] = 0;
  // (only the two-pair instance deals octets to groups: maps of 1 025 .. 2 048 padded landmarks on the publish / subscribe route)
  if (f->scan_dev && f->route == PK_ROUTE_ML_REGS && f->pub_ecap > 0 && f->d.lay.Lp > 2 * kPubThreads && f->d.lay.Lp <= 4 * kPubThreads) {
    unsigned w[3] = {0u, 0u, 0u}, sk = 1u;
    PK_HIP(hipMemcpyAsync(w, ctl_pub_stats(f) + 4, sizeof(w), hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipMemcpyAsync(&sk, ctl_skip_pub(f), sizeof(unsigned), hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    if (sk == 0u)
      for (int i = 0; i < 3; ++i) out[i] = w[i];
  }
  return PK_OK;
}
int pk_observe_bytes(const pk_filter* f, int32_t B, int64_t* algorithmic, int64_t* moved) {
  if (!f) return fail(PK_ERR_INVALID, "pk_observe_bytes: NULL handle");
  const int64_t P = f->d.P, L = f->d.lay.L;
  if (algorithmic) *algorithmic = P * L * 28 * (int64_t)sizeof(double);  // 14 read + 14 written
  // (the colour table's mode: eight rows and the count each way, 136 B per particle.landmark instead of 232)
  const int64_t rows = f->ct_engaged ? 16 : 28;
  if (moved) *moved = P * (L * (rows * (int64_t)sizeof(double) + 8) + (int64_t)B * 32);
  return PK_OK;
}

int pk_colour_table_stats(pk_filter* f, int64_t out[4]) {
  if (!f || !out) return fail(PK_ERR_INVALID, "pk_colour_table_stats: NULL argument");
  out[0] = f->ct_engaged ? 1 : 0;
  out[1] = f->ct_built ? f->ct_depth : f->opt.colour_table_depth;
  out[2] = f->ct_scans;
  out[3] = f->ct_whole;
  return PK_OK;
}

}  // extern "C"

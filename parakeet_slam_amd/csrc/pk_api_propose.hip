// The measurement-informed proposal behind the C ABI (include/parakeet_slam.h; DESIGN.md section 4, "The measurement-informed
// proposal"): one move plus one observe in which every particle's pose is drawn from the motion model CONDITIONED on the scan
// (FastSLAM 2.0).  Host orchestration only: the kernels are the motion kernels as they stand (twice: with zero normals for the
// predicted pose, with k_propose's normals for the sampled one), the bearing model's association, k_propose (pk_k_propose.hip)
// and k_observe_proposed (pk_k_observe.hip) -- for a scan with ranged blobs (pk_proposal_ranges) the range association,
// k_propose_range and k_observe_proposed_range.  On a growing filter (pk_proposal_grow) pk_observe's own tail follows:
// k_new_landmarks* at the sampled poses on the ids k_propose settled, then k_grow_retire.
#include "pk_filter.hpp"

namespace {

// What the proposal has no kernels for, each said once; nothing has changed when one of them answers.
int refuse_proposal(const pk_filter* f, const char* who) {
  if (f->model != PK_MODEL_BEARING)
    return fail(PK_ERR_UNSUPPORTED, "%s: the measurement-informed proposal needs a measurement with a pose Jacobian: the bearing model "
                                    "(pk_set_measurement_model(f, PK_MODEL_BEARING)); the reference model's is not one", who);
  if (f->dense || f->qt_dense)
    return fail(PK_ERR_UNSUPPORTED, "%s: the measurement-informed proposal has no kernel for the dense layout (covariances or a Qt that "
                                    "couple position, bearing and colour)", who);
  if ((f->grow_on || f->retire.on()) && !f->prop.grow)
    return fail(PK_ERR_UNSUPPORTED, "%s: the measurement-informed proposal has no kernel for growing maps (pk_grow_enable, "
                                    "pk_grow_retire): new landmarks are found by the plain step, or behind the proposal's own once "
                                    "pk_proposal_grow(f, 1) switches that in", who);
  if (f->split.active || f->ct_sharded || f->d.global_offset != 0 || f->d.logical[0] || f->d.alt)
    return fail(PK_ERR_UNSUPPORTED, "%s: the measurement-informed proposal runs on one whole filter: this one is a shard of a sharded "
                                    "filter or inside a split step", who);
  if (f->staged.valid || !f->dense_staged.empty())
    return fail(PK_ERR_STATE, "%s: a staged scan is in flight (pk_stage_scan); pk_observe_staged takes it first", who);
  return PK_OK;
}

// the state of pk_filter::Proposal, from the one owner of device memory, at the first call
int ensure_state(pk_filter* f) {
  pk_filter::Proposal& q = f->prop;
  if (q.used) return PK_OK;
  const size_t P = (size_t)f->d.P;
  int rc;
  if ((rc = dev_lazy(f, &q.pose, 3 * P)) || (rc = dev_lazy(f, &q.zero, 3 * P)) || (rc = dev_lazy(f, &q.xi, 3 * P)) ||
      (rc = dev_lazy(f, &q.dlogw, P)))
    return rc;
  PK_HIP(hipMemsetAsync(q.zero, 0, 3 * P * sizeof(double), f->stream));
  return dev_lazy(f, &q.used, P);
}

int copy_poses(pk_filter* f, bool save) {
  const size_t P = (size_t)f->d.P, n = P * sizeof(double);
  if (P == 0) return PK_OK;
  double* live[3] = {f->d.x[f->d.cur], f->d.y[f->d.cur], f->d.h[f->d.cur]};
  for (int k = 0; k < 3; ++k) {
    double* kept = f->prop.pose + (size_t)k * P;
    PK_HIP(hipMemcpyAsync(save ? kept : live[k], save ? live[k] : kept, n, hipMemcpyDeviceToDevice, f->stream));
  }
  return PK_OK;
}

int propose_impl(pk_filter* f, const char* who, const StepMotion& m, const double* z, uint64_t seed, uint64_t draw,
                 const double* blobs, int32_t B, const int32_t* ids, bool fresh, int32_t* ids_out) {
  int rc;
  // armed ranges (pk_scan_ranges): refused and gone -- or, with pk_proposal_ranges on, consumed here whatever follows, with the
  // range scans' own refusals ahead of the proposal's
  RangeScan rs;
  if (!f->prop.ranges) {
    if ((rc = refuse_ranges_proposal(f, who))) return rc;
  } else if ((rc = ranges_take(f, who, B, &rs))) {
    return rc;
  }
  if ((rc = refuse_proposal(f, who))) return rc;
  if ((rc = unique_refuse(f, who, "the measurement-informed proposal, which settles its own tentative ids inside k_propose"))) return rc;
  // pk_proposal_grow: the new-landmark bookkeeping follows the step -- at the sampled poses, on the ids k_propose settles
  const bool grow = f->grow_on && B > 0;
  if (grow && ids) return refuse_grow_ids(who);
  if ((rc = check_scan_shape(f, who, blobs, B))) return rc;
  if ((rc = check_scan_values(f, who, blobs, B, &ids))) return rc;
  if (!ids && B > 65535) return fail(PK_ERR_UNSUPPORTED, "%s: at most 65535 blobs per scan (got %d)", who, B);
  if (!ids && observe_general_lds_bytes(f->d.lay.Lp, B) > kMaxDynLds)  // (supplied ids: shared chains, no LDS tables)
    return fail(PK_ERR_UNSUPPORTED, "%s: %d landmarks + 2 x %d blobs need %zu bytes of LDS chains per particle, the workgroup has %zu", who,
                f->d.lay.Lp, B, observe_general_lds_bytes(f->d.lay.Lp, B), (size_t)kMaxDynLds);
  if ((rc = use_device(f))) return rc;
  if ((rc = ensure_state(f))) return rc;
  pk_filter::Proposal& q = f->prop;
  q.valid = false;
  poses_change(f);

  double u[3] = {m.v, m.w, m.dt}, sigma[3];
  if (m.odom) {
    memcpy(u, m.delta, sizeof(u));
    memcpy(sigma, m.sigma, sizeof(sigma));
  } else {  // launch_motion's own
    motion_sigmas(m.v, m.w, &sigma[0], &sigma[1]);
    sigma[2] = sigma[1];
  }
  auto move = [&](const double* zd, double* pose_part) {
    if (m.odom)
      launch_motion_odom(f->stream, f->d, m.delta, m.sigma, zd, seed, draw, nullptr, nullptr, 0, pose_part);
    else
      launch_motion(f->stream, f->d, m.v, m.w, m.dt, zd, seed, draw, 0, nullptr, nullptr, 0, pose_part);
  };
  const double* zd = nullptr;
  if (z) {  // the caller's (pageable) buffer is consumed before we return, as pk_motion does
    PK_HIP(hipMemcpyAsync(f->z_dev, z, (size_t)f->d.P * 3 * sizeof(double), hipMemcpyHostToDevice, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    zd = f->z_dev;
  }
  {  // the predicted pose: the same kernel, normals 0
    Span t(f, PK_T_MOTION);
    if ((rc = copy_poses(f, true))) return rc;
    move(q.zero, nullptr);
  }
  ProposalScan sc;
  rc = proposal_scan(f, blobs, B, ids, &sc, &rs, grow);  // (the association, in its own span)
  if (!rc) {
    Span t(f, PK_T_PROPOSE);
    ProposeLaunch pl;
    pl.blobs_dev = sc.scan.blobs;
    pl.blobdir_dev = sc.scan.dir;
    pl.rng_dev = sc.rng;
    pl.B = B;
    pl.ids_dev = sc.ids;
    pl.ids_shared = ids != nullptr;
    pl.z_dev = zd;
    pl.seed = seed;
    pl.draw = draw;
    pl.odom = m.odom;
    memcpy(pl.u, u, sizeof(u));
    memcpy(pl.sigma, sigma, sizeof(sigma));
    pl.qt = f->qt;
    pl.xi_dev = q.xi;
    pl.dlogw_dev = q.dlogw;
    pl.used_dev = q.used;
    launch_propose(f->stream, f->d, pl);
  }
  {  // the sampled pose: the poses before the move, moved with k_propose's normals (the scan failed: with the caller's, the plain move)
    Span t(f, PK_T_MOTION);
    int rc2 = copy_poses(f, false);
    if (rc2) return rc2;
    if (rc) return rc;  // the poses are what they were
    move(q.xi, f->pose_part);
    f->pose_part_ok = true;
  }
  {
    Span t(f, PK_T_OBSERVE);
    ObserveExtras ex;
    ex.reset = fresh;
    ex.model = PK_MODEL_BEARING;
    ex.gmax_key = ctl_gmax_key(f);
    ex.dlogw = q.dlogw;
    ex.rng = sc.rng;
    if (ids)
      launch_observe(f->stream, f->d, sc.scan, sc.known, f->qt, ex);
    else
      launch_observe(f->stream, f->d, sc.scan, sc.ids, f->qt, ex);
  }
  PK_LAUNCH_CHECK(who);
  proposal_observed(f, ids != nullptr);
  q.valid = true;
  // a growing filter (pk_proposal_grow): pk_observe's own tail, at the sampled poses on the settled ids (0 = unmatched; no bit rows)
  if (grow && (rc = grow_bookkeeping(f, who, sc.scan, B))) return rc;
  return return_ids(f, ids_out, B, ids);
}

}  // namespace

extern "C" {

int pk_propose(pk_filter* f, double v, double w, double dt, const double* z, uint64_t seed, uint64_t draw, const double* blobs,
               int32_t num_blobs, const int32_t* ids, int32_t fresh, int32_t* ids_out) {
  if (!f) return fail(PK_ERR_INVALID, "pk_propose: NULL handle");
  const StepMotion m = StepMotion::twist(v, w, dt);
  if (!m.finite()) return fail(PK_ERR_INVALID, "pk_propose: non-finite control");
  return propose_impl(f, "pk_propose", m, z, seed, draw, blobs, num_blobs, ids, fresh != 0, ids_out);
}

int pk_propose_odom(pk_filter* f, const double delta[3], const double alpha[4], const double* z, uint64_t seed, uint64_t draw,
                    const double* blobs, int32_t num_blobs, const int32_t* ids, int32_t fresh, int32_t* ids_out) {
  if (!f) return fail(PK_ERR_INVALID, "pk_propose_odom: NULL handle");
  StepMotion m;
  m.odom = true;
  if (int rc = pk_odom_sigmas(delta, alpha, m.sigma)) return rc;  // before anything moves
  memcpy(m.delta, delta, sizeof(m.delta));
  return propose_impl(f, "pk_propose_odom", m, z, seed, draw, blobs, num_blobs, ids, fresh != 0, ids_out);
}

int pk_proposal_ranges(pk_filter* f, int32_t on) {
  if (!f) return fail(PK_ERR_INVALID, "pk_proposal_ranges: NULL handle");
  f->prop.ranges = on != 0;
  return PK_OK;
}

int pk_proposal_ranges_state(const pk_filter* f, int32_t* on) {
  if (!f) return fail(PK_ERR_INVALID, "pk_proposal_ranges_state: NULL handle");
  if (on) *on = f->prop.ranges ? 1 : 0;
  return PK_OK;
}

// pk_proposal_grow: the step on a growing filter -- refuse_proposal's growing-map clause steps aside, and pk_observe's bookkeeping
// and retirement run behind the step (grow_bookkeeping, pk_api_observe.hip).  No device state: kernels the library has, reordered.
int pk_proposal_grow(pk_filter* f, int32_t on) {
  if (!f) return fail(PK_ERR_INVALID, "pk_proposal_grow: NULL handle");
  if (on != 0 && on != 1) return fail(PK_ERR_INVALID, "pk_proposal_grow: on = %d is neither 0 nor 1", (int)on);
  f->prop.grow = on == 1;
  return PK_OK;
}

int pk_proposal_grow_state(const pk_filter* f, int32_t* on) {
  if (!f) return fail(PK_ERR_INVALID, "pk_proposal_grow_state: NULL handle");
  if (on) *on = f->prop.grow ? 1 : 0;
  return PK_OK;
}

int pk_proposal_download(pk_filter* f, double* xi, double* dlogw, int32_t* used) {
  if (!f) return fail(PK_ERR_INVALID, "pk_proposal_download: NULL handle");
  if (!f->prop.valid) return fail(PK_ERR_STATE, "pk_proposal_download: no proposal step has run (pk_propose, pk_propose_odom)");
  int rc;
  if ((rc = use_device(f))) return rc;
  const size_t P = (size_t)f->d.P;
  if (xi) PK_HIP(hipMemcpyAsync(xi, f->prop.xi, 3 * P * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  if (dlogw) PK_HIP(hipMemcpyAsync(dlogw, f->prop.dlogw, P * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  if (used) PK_HIP(hipMemcpyAsync(used, f->prop.used, P * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

}  // extern "C"

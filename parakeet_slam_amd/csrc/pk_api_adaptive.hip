// Adaptive resampling behind the C ABI (pk_filter.hpp; DESIGN.md section 4, "Adaptive resampling"): the resample and the step that
// decide on the device whether to resample, what they decided, the weight sums a sharded gate would all-reduce, and the weighted
// pose summary.  Host orchestration only; the kernels are pk_k_adaptive.hip.  pk_step_adaptive runs step_impl (pk_api.hip), the body
// it shares with pk_step.
#include "pk_filter.hpp"

namespace {

// f->ad_words: the scan's shift | the gate's plan (beyond kAncestorsScanMaxBlocks scan blocks, and pk_weight_sums') | a maximum
// log-weight for the calls that take their own | the pose summary
constexpr int kAdShift = 0, kAdPlan = 1, kAdGmax = kAdPlan + kGatePlan, kAdPose = kAdGmax + 1, kAdWords = kAdPose + kPoseRes;

// the buffers of everything here, made when one of the entry points is first called: a filter that never does holds none
int adaptive_ready(pk_filter* f) {
  int rc;
  if ((rc = dev_lazy(f, &f->ad_s2, (size_t)f->nblocks)) || (rc = dev_lazy(f, &f->ad_words, (size_t)kAdWords)) ||
      (rc = dev_lazy(f, &f->ad_part, (size_t)path_blocks(f->d.P) * kPathSums)))
    return rc;
  if (!f->ad_out) {
    if ((rc = dev_alloc(f, &f->ad_out, 1))) return rc;
    PK_HIP(hipMemsetAsync(f->ad_out, 0, sizeof(GateOutcome), f->stream));  // the counters start at zero, in stream order
  }
  return PK_OK;
}

int bad_domain(const char* who, int32_t weight_domain) {
  if (weight_domain == PK_WEIGHTS_LINEAR || weight_domain == PK_WEIGHTS_LOG) return PK_OK;
  return fail(PK_ERR_INVALID, "%s: weight_domain %d", who, weight_domain);
}

// the maximum log-weight a call takes by itself or is given, into ad_words[kAdGmax] (the linear domain reads none)
int own_gmax(pk_filter* f, int32_t weight_domain, double gmax) {
  if (weight_domain != PK_WEIGHTS_LOG) return PK_OK;
  if (std::isnan(gmax)) {
    launch_block_max(f->stream, f->d, f->partial, f->ad_words + kAdGmax);
    return PK_OK;
  }
  PK_HIP(hipMemcpyAsync(f->ad_words + kAdGmax, &gmax, sizeof(double), hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));  // (gmax is the caller's stack)
  return PK_OK;
}

}  // namespace

int bad_threshold(const char* who, double threshold) {
  if (std::isfinite(threshold) && threshold >= 0.0) return PK_OK;
  return fail(PK_ERR_INVALID, "%s: threshold = %g is not a finite share of P >= 0", who, threshold);
}

extern "C" {

int pk_resample_adaptive(pk_filter* f, double u, int32_t weight_domain, double threshold, int64_t* ancestors_out) {
  poses_change(f);
  if (!f) return fail(PK_ERR_INVALID, "pk_resample_adaptive: NULL handle");
  if (!(u >= 0.0 && u < 1.0)) return fail(PK_ERR_INVALID, "pk_resample_adaptive: u = %g outside [0,1)", u);
  int rc;
  if ((rc = bad_domain("pk_resample_adaptive", weight_domain)) || (rc = bad_threshold("pk_resample_adaptive", threshold))) return rc;
  if (f->split.active) return fail(PK_ERR_STATE, "pk_resample_adaptive: a split observe is in progress (half the particles observed)");
  if (int refused = refuse_balanced(f, "pk_resample_adaptive")) return refused;
  if ((rc = use_device(f)) || (rc = adaptive_ready(f))) return rc;
  DeviceState& d = f->d;
  double* const words = f->ad_words;
  const bool few = f->nblocks <= kAncestorsScanMaxBlocks;
  {
    Span t(f, PK_T_WEIGHTS);  // pk_resample's weight kernels, and the squares beside the scan
    const unsigned long long* key = nullptr;
    if (weight_domain == PK_WEIGHTS_LOG) {
      if (f->gmax_fused)
        key = ctl_gmax_key(f);  // the observe kernels kept the max of the weights they wrote
      else
        launch_block_max(f->stream, d, f->partial, f->gmax);
    }
    launch_scan_local(f->stream, d, f->gmax, weight_domain, f->clocal, f->totals, key);
    launch_weight_sq(f->stream, d, f->gmax, weight_domain, key, f->ad_s2, words + kAdShift);
    if (!few) launch_gate_plan(f->stream, f->totals, f->ad_s2, f->nblocks, f->offsets, words + kAdPlan, threshold, d.P);
  }
  {
    Span t(f, PK_T_RESAMPLE);
    launch_ancestors_gated(f->stream, f->clocal, f->totals, f->ad_s2, few ? nullptr : f->offsets, few ? nullptr : words + kAdPlan,
                           f->nblocks, u, threshold, words + kAdShift, f->anc, d, f->ad_out);
  }
  ++f->ad_calls;
  if (f->retire.on()) launch_retire_gather(f->stream, f->grow, f->retire, f->anc, d.P);  // (pk_grow_retire: the clocks too)
  if (f->grow_on) launch_grow_gather(f->stream, f->grow, f->anc, d.P);  // by the ancestors: the identity when the call kept
  if (f->path.cap && (rc = path_record(f, weight_domain))) return rc;    // one ring row per call, kept or not; a trunk settles by
                                                                         // the new generation's weights
  PK_LAUNCH_CHECK("pk_resample_adaptive");
  f->src_identity = false;  // (the host does not know the verdict: as behind a resample)
  f->gmax_fused = false;
  if (ancestors_out) {
    std::vector<int32_t> a((size_t)d.P);
    PK_HIP(hipMemcpyAsync(a.data(), f->anc, (size_t)d.P * 4, hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    for (int64_t i = 0; i < d.P; ++i) ancestors_out[i] = a[i];
  }
  return PK_OK;
}

int pk_step_adaptive(pk_filter* f, double v, double w, double dt, const double* z, uint64_t seed, uint64_t draw, const double* blobs,
                     int32_t B, const int32_t* ids, double u, int32_t weight_domain, double threshold) {
  if (int rc = bad_threshold("pk_step_adaptive", threshold)) return rc;  // before anything moves
  return step_impl(f, StepMotion::twist(v, w, dt), z, seed, draw, blobs, B, ids, u, weight_domain, &threshold);
}

int pk_resample_stats(pk_filter* f, double out[4], int32_t* resampled, int64_t counts[2]) {
  if (!f) return fail(PK_ERR_INVALID, "pk_resample_stats: NULL handle");
  if (f->ad_calls == 0) return fail(PK_ERR_STATE, "pk_resample_stats: no pk_resample_adaptive / pk_step_adaptive call has been made on this filter");
  int rc;
  if ((rc = use_device(f))) return rc;
  GateOutcome o;
  PK_HIP(hipMemcpyAsync(&o, f->ad_out, sizeof(o), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  if (out) {
    out[0] = o.n_eff;
    out[1] = o.s1;
    out[2] = o.s2;
    out[3] = o.shift;
  }
  if (resampled) *resampled = (int32_t)o.resampled;
  if (counts) {
    counts[0] = (int64_t)o.calls;
    counts[1] = (int64_t)o.resamples;
  }
  return PK_OK;
}

int pk_weight_sums(pk_filter* f, int32_t weight_domain, double gmax, double out[2]) {
  if (!f || !out) return fail(PK_ERR_INVALID, "pk_weight_sums: NULL argument");
  int rc;
  if ((rc = bad_domain("pk_weight_sums", weight_domain))) return rc;
  if ((rc = use_device(f)) || (rc = adaptive_ready(f))) return rc;
  double* const words = f->ad_words;
  {
    Span t(f, PK_T_WEIGHTS);
    if ((rc = own_gmax(f, weight_domain, gmax))) return rc;
    // the resample's own scan (its workspace, no filter state), so that S1 is the resample's sum
    launch_scan_local(f->stream, f->d, words + kAdGmax, weight_domain, f->clocal, f->totals, nullptr);
    launch_weight_sq(f->stream, f->d, words + kAdGmax, weight_domain, nullptr, f->ad_s2, words + kAdShift);
    launch_gate_plan(f->stream, f->totals, f->ad_s2, f->nblocks, nullptr, words + kAdPlan, 0.0, f->d.P);
  }
  PK_LAUNCH_CHECK("pk_weight_sums");
  PK_HIP(hipMemcpyAsync(out, words + kAdPlan, 2 * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

int pk_summary_weighted(pk_filter* f, int32_t weight_domain, double mean[3], double spread[4], double* n_eff) {
  if (!f) return fail(PK_ERR_INVALID, "pk_summary_weighted: NULL handle");
  int rc;
  if ((rc = bad_domain("pk_summary_weighted", weight_domain))) return rc;
  if ((rc = use_device(f)) || (rc = adaptive_ready(f))) return rc;
  double* const words = f->ad_words;
  {
    Span t(f, PK_T_SUMMARY);
    if ((rc = own_gmax(f, weight_domain, std::nan("")))) return rc;
    launch_pose_moments(f->stream, f->d, words + kAdGmax, weight_domain, f->ad_part, words + kAdPose);
  }
  PK_LAUNCH_CHECK("pk_summary_weighted");
  double s[kPoseRes];
  PK_HIP(hipMemcpyAsync(s, words + kAdPose, sizeof(s), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  const double S1 = s[7], S2 = s[8];
  if (!(S1 > 0.0) || !std::isfinite(S1) || !std::isfinite(S2))
    return fail(PK_ERR_STATE, "pk_summary_weighted: the weights sum to %g: not positive and finite", S1);
  if (mean) {
    mean[0] = s[0];
    mean[1] = s[1];
    mean[2] = std::atan2(s[2], s[3]);  // as pk_summary: prkt_core_v2.py:275
  }
  if (spread) {
    spread[0] = s[4];
    spread[1] = s[5];
    spread[2] = s[6];
    spread[3] = std::hypot(s[2], s[3]) / S1;
  }
  if (n_eff) *n_eff = S1 / S2 * S1;
  return PK_OK;
}

}  // extern "C"

// The path estimate behind the C ABI (pk_filter.hpp; DESIGN.md section 4, "The path estimate"): the ring of resampled generations,
// its transfers, the trace, the summary, the summary by the weights and the most likely particle.  Host orchestration only; the
// kernels are pk_k_path.hip and pk_k_path_weighted.hip.  pk_resample (pk_api.hip)
// records through path_record; what refuses a recording filter says so through refuse_path (pk_api_shard.hip).
#include "pk_filter.hpp"

namespace {

// every entry point but pk_path_enable: a handle whose ring is on
int need_ring(const pk_filter* f, const char* who) {
  if (!f) return fail(PK_ERR_INVALID, "%s: NULL handle", who);
  if (f->path.cap == 0) return fail(PK_ERR_STATE, "%s: the path is not being recorded (pk_path_enable)", who);
  return PK_OK;
}

// the ring and the scratch of trace and summary go back to the registry (the stream is idle)
void path_release(pk_filter* f) {
  dev_free(f, &f->path.pose);
  dev_free(f, &f->path.anc);
  dev_free(f, &f->pt_idx);
  dev_free(f, &f->pt_out);
  dev_free(f, &f->ps_cnt);
  dev_free(f, &f->ps_ref);
  dev_free(f, &f->ps_part);
  dev_free(f, &f->ps_res);
  dev_free(f, &f->pw_idx);
  dev_free(f, &f->pw_wgt);
  dev_free(f, &f->pw_ref);
  dev_free(f, &f->pw_part);
  dev_free(f, &f->pw_res);
  f->pt_cap = f->pt_out_cap = f->ps_rows = f->pw_rows = 0;
  f->path = PathRing();
}

}  // namespace

int path_record(pk_filter* f) {
  PathRing& r = f->path;
  const int row = r.held < r.cap ? r.row(r.held) : r.first;  // a full ring gives up its oldest row
  {
    Span t(f, PK_T_RESAMPLE);
    launch_path_record(f->stream, f->d, f->anc, r, row);
  }
  if (r.held < r.cap)
    ++r.held;
  else
    r.first = (r.first + 1) % r.cap;
  ++r.recorded;
  return PK_OK;
}

extern "C" {

int pk_path_enable(pk_filter* f, int32_t capacity) {
  if (!f) return fail(PK_ERR_INVALID, "pk_path_enable: NULL handle");
  if (capacity < 0) return fail(PK_ERR_INVALID, "pk_path_enable: capacity %d", capacity);
  if (capacity > 0) {
    if (int rc = refuse_balanced(f, "pk_path_enable")) return rc;
    if (f->split.active) return fail(PK_ERR_STATE, "pk_path_enable: a split observe is in progress");
  }
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipStreamSynchronize(f->stream));
  path_release(f);
  if (capacity == 0) return PK_OK;
  const size_t P = (size_t)f->d.P;
  if ((rc = dev_alloc(f, &f->path.pose, (size_t)capacity * 3 * P)) || (rc = dev_alloc(f, &f->path.anc, (size_t)capacity * P))) {
    path_release(f);
    return rc;
  }
  f->path.cap = capacity;
  return PK_OK;
}

int pk_path_shape(const pk_filter* f, int32_t* capacity, int32_t* held, int64_t* recorded) {
  if (int rc = need_ring(f, "pk_path_shape")) return rc;
  if (capacity) *capacity = f->path.cap;
  if (held) *held = f->path.held;
  if (recorded) *recorded = f->path.recorded;
  return PK_OK;
}

int pk_path_download(pk_filter* f, int32_t t0, int32_t t1, double* poses, int32_t* ancestors) {
  int rc;
  if ((rc = need_ring(f, "pk_path_download"))) return rc;
  const PathRing& r = f->path;
  if (t0 < 0 || t1 < t0 || t1 > r.held) return fail(PK_ERR_INVALID, "pk_path_download: rows [%d, %d) of the %d held", t0, t1, r.held);
  if ((rc = use_device(f))) return rc;
  const size_t P = (size_t)f->d.P;
  std::vector<double> soa;
  try {
    if (poses) soa.resize(3 * P);
  } catch (const std::bad_alloc&) {
    return fail(PK_ERR_NOMEM, "pk_path_download: no host memory to stage a row of %zu particles", P);
  }
  for (int t = t0; t < t1; ++t) {
    const size_t row = (size_t)r.row(t), o = (size_t)(t - t0);
    if (ancestors) PK_HIP(hipMemcpyAsync(ancestors + o * P, r.anc + row * P, P * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
    if (!poses) continue;
    PK_HIP(hipMemcpyAsync(soa.data(), r.pose + row * 3 * P, 3 * P * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    double* out = poses + o * P * 3;
    for (size_t i = 0; i < P; ++i) {
      out[3 * i] = soa[i];
      out[3 * i + 1] = soa[P + i];
      out[3 * i + 2] = soa[2 * P + i];
    }
  }
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

int pk_path_upload(pk_filter* f, int32_t n, int64_t recorded, const double* poses, const int32_t* ancestors) {
  int rc;
  if ((rc = need_ring(f, "pk_path_upload"))) return rc;
  PathRing& r = f->path;
  if (n < 0 || n > r.cap) return fail(PK_ERR_INVALID, "pk_path_upload: %d rows into a ring of %d", n, r.cap);
  if (recorded < n) return fail(PK_ERR_INVALID, "pk_path_upload: %lld rows recorded cannot leave %d held", (long long)recorded, n);
  if (n > 0 && (!poses || !ancestors)) return fail(PK_ERR_INVALID, "pk_path_upload: NULL poses / ancestors");
  const size_t P = (size_t)f->d.P;
  for (size_t i = 0; i < (size_t)n * P; ++i)
    if (ancestors[i] < 0 || (size_t)ancestors[i] >= P)
      return fail(PK_ERR_INVALID, "pk_path_upload: row %zu: the ancestor %d of particle %zu is outside [0, %zu)", i / P, ancestors[i], i % P, P);
  if ((rc = use_device(f))) return rc;
  std::vector<double> soa;
  try {
    soa.resize(3 * P);
  } catch (const std::bad_alloc&) {
    return fail(PK_ERR_NOMEM, "pk_path_upload: no host memory to stage a row of %zu particles", P);
  }
  r.held = r.first = 0;  // (a failure below leaves an empty ring)
  for (int t = 0; t < n; ++t) {
    const double* in = poses + (size_t)t * P * 3;
    for (size_t i = 0; i < P; ++i) {
      soa[i] = in[3 * i];
      soa[P + i] = in[3 * i + 1];
      soa[2 * P + i] = in[3 * i + 2];
    }
    PK_HIP(hipMemcpyAsync(r.pose + (size_t)t * 3 * P, soa.data(), 3 * P * sizeof(double), hipMemcpyHostToDevice, f->stream));
    PK_HIP(hipMemcpyAsync(r.anc + (size_t)t * P, ancestors + (size_t)t * P, P * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));  // the staging row is refilled; the caller's buffers are pageable
  }
  r.held = n;
  r.recorded = recorded;
  return PK_OK;
}

int pk_path_trace(pk_filter* f, const int64_t* particles, int64_t n, double* out) {
  int rc;
  if ((rc = need_ring(f, "pk_path_trace"))) return rc;
  if (n < 0 || (n > 0 && (!particles || !out))) return fail(PK_ERR_INVALID, "pk_path_trace: bad argument");
  const int64_t P = f->d.P;
  for (int64_t i = 0; i < n; ++i)
    if (particles[i] < 0 || particles[i] >= P) return fail(PK_ERR_INVALID, "pk_path_trace: particle %lld of %lld", (long long)particles[i], (long long)P);
  if (n == 0) return PK_OK;
  if ((rc = use_device(f))) return rc;
  const PathRing& r = f->path;
  // in chunks of particles whose paths fit a staging buffer of 64 MB (a ring of 1 024 rows: 2 730 particles at a time)
  const int64_t per = (int64_t)(r.held + 1) * 3;
  int64_t chunk = std::max<int64_t>(1, (int64_t)(8u << 20) / per);
  if (chunk > n) chunk = n;
  if ((rc = dev_reserve(f, &f->pt_idx, &f->pt_cap, chunk, chunk))) return rc;
  if ((rc = dev_reserve(f, &f->pt_out, &f->pt_out_cap, chunk * per, chunk * per))) return rc;
  for (int64_t i0 = 0; i0 < n; i0 += chunk) {
    const int64_t m = std::min(chunk, n - i0);
    PK_HIP(hipMemcpyAsync(f->pt_idx, particles + i0, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, f->stream));
    {
      Span t(f, PK_T_SUMMARY);
      launch_path_trace(f->stream, f->d, r, f->pt_idx, m, f->pt_out);
    }
    PK_LAUNCH_CHECK("pk_path_trace");
    PK_HIP(hipMemcpyAsync(out + (size_t)i0 * per, f->pt_out, (size_t)(m * per) * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
  }
  return PK_OK;
}

int pk_path_summary(pk_filter* f, double* mean, double* spread, int64_t* survivors) {
  int rc;
  if ((rc = need_ring(f, "pk_path_summary"))) return rc;
  if ((rc = use_device(f))) return rc;
  const PathRing& r = f->path;
  const int64_t P = f->d.P, rows = (int64_t)r.held + 1;
  const size_t nb = (size_t)path_blocks(P);
  // (sized for the whole ring at once: a filling ring does not reallocate at every step)
  const int64_t rows_cap = (int64_t)r.cap + 1;
  if ((rc = dev_reserve_group(f, &f->ps_rows, rows, rows_cap, want(&f->ps_cnt, (size_t)3 * P), want(&f->ps_ref, (size_t)rows_cap * 3),
                              want(&f->ps_part, (size_t)rows_cap * nb * kPathSums), want(&f->ps_res, (size_t)rows_cap * kPathRes))))
    return rc;
  std::vector<double> h;
  try {
    h.resize((size_t)rows * kPathRes);
  } catch (const std::bad_alloc&) {
    return fail(PK_ERR_NOMEM, "pk_path_summary: no host memory for %lld rows", (long long)rows);
  }
  {
    Span t(f, PK_T_SUMMARY);
    launch_path_summary(f->stream, f->d, r, f->ps_cnt, f->ps_ref, f->ps_part, f->ps_res);
  }
  PK_LAUNCH_CHECK("pk_path_summary");
  PK_HIP(hipMemcpyAsync(h.data(), f->ps_res, h.size() * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  const double n = (double)P;
  for (int64_t t = 0; t < rows; ++t) {
    const double* s = h.data() + (size_t)t * kPathRes;
    if (mean) {
      mean[3 * t] = s[0];
      mean[3 * t + 1] = s[1];
      mean[3 * t + 2] = std::atan2(s[2], s[3]);  // as pk_summary: prkt_core_v2.py:275
    }
    if (spread) {
      spread[4 * t] = s[4];
      spread[4 * t + 1] = s[5];
      spread[4 * t + 2] = s[6];
      spread[4 * t + 3] = std::hypot(s[2], s[3]) / n;
    }
    if (survivors) survivors[t] = (int64_t)s[7];
  }
  return PK_OK;
}

int pk_path_summary_weighted(pk_filter* f, int32_t weight_domain, double* mean, double* spread, double* n_eff) {
  int rc;
  if ((rc = need_ring(f, "pk_path_summary_weighted"))) return rc;
  if (weight_domain != PK_WEIGHTS_LINEAR && weight_domain != PK_WEIGHTS_LOG)
    return fail(PK_ERR_INVALID, "pk_path_summary_weighted: weight_domain %d", weight_domain);
  if ((rc = use_device(f))) return rc;
  const PathRing& r = f->path;
  const int64_t P = f->d.P, rows = (int64_t)r.held + 1;
  const size_t nb = (size_t)path_blocks(P);
  // (sized for the whole ring at once, as pk_path_summary's)
  const int64_t rows_cap = (int64_t)r.cap + 1;
  if ((rc = dev_reserve_group(f, &f->pw_rows, rows, rows_cap, want(&f->pw_idx, (size_t)P), want(&f->pw_wgt, (size_t)P),
                              want(&f->pw_ref, (size_t)rows_cap * 3), want(&f->pw_part, (size_t)rows_cap * nb * kPathSums),
                              want(&f->pw_res, (size_t)rows_cap * kPathWRes + 1))))
    return rc;
  double* const gmax = f->pw_res + (size_t)rows_cap * kPathWRes;
  std::vector<double> h;
  try {
    h.resize((size_t)rows * kPathWRes);
  } catch (const std::bad_alloc&) {
    return fail(PK_ERR_NOMEM, "pk_path_summary_weighted: no host memory for %lld rows", (long long)rows);
  }
  {
    Span t(f, PK_T_SUMMARY);
    if (weight_domain == PK_WEIGHTS_LOG) launch_block_max(f->stream, f->d, f->partial, gmax);  // (f->partial: a workspace, no filter state)
    launch_path_weighted(f->stream, f->d, r, gmax, weight_domain, f->pw_idx, f->pw_wgt, f->pw_ref, f->pw_part,
                         f->pw_res);
  }
  PK_LAUNCH_CHECK("pk_path_summary_weighted");
  PK_HIP(hipMemcpyAsync(h.data(), f->pw_res, h.size() * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  const double* cur = h.data() + (size_t)r.held * kPathWRes;  // the weights are the current particles': one S1, one S2
  const double S1 = cur[7], S2 = cur[8];
  if (!(S1 > 0.0) || !std::isfinite(S1) || !std::isfinite(S2))
    return fail(PK_ERR_STATE, "pk_path_summary_weighted: the weights sum to %g: not positive and finite", S1);
  for (int64_t t = 0; t < rows; ++t) {
    const double* s = h.data() + (size_t)t * kPathWRes;
    if (mean) {
      mean[3 * t] = s[0];
      mean[3 * t + 1] = s[1];
      mean[3 * t + 2] = std::atan2(s[2], s[3]);  // as pk_summary: prkt_core_v2.py:275
    }
    if (spread) {
      spread[4 * t] = s[4];
      spread[4 * t + 1] = s[5];
      spread[4 * t + 2] = s[6];
      spread[4 * t + 3] = std::hypot(s[2], s[3]) / S1;
    }
  }
  if (n_eff) *n_eff = S1 / S2 * S1;
  return PK_OK;
}

int pk_best_particle(pk_filter* f, int64_t* index, double* log_weight) {
  if (!f) return fail(PK_ERR_INVALID, "pk_best_particle: NULL handle");
  int rc;
  if ((rc = use_device(f))) return rc;
  // f->partial (4 096 doubles, a workspace): the workgroups' pairs, then the result
  double* const out = f->partial + 2 * kPathMaxBlocks;
  {
    Span t(f, PK_T_SUMMARY);
    launch_best_particle(f->stream, f->d, f->partial, out);
  }
  PK_LAUNCH_CHECK("pk_best_particle");
  double h[2];
  PK_HIP(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  if (h[1] < 0.0) return fail(PK_ERR_STATE, "pk_best_particle: every log-weight is NaN");
  if (index) *index = (int64_t)h[1];
  if (log_weight) *log_weight = h[0];
  return PK_OK;
}

}  // extern "C"

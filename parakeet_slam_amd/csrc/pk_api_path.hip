// The path estimate behind the C ABI (pk_filter.hpp; DESIGN.md section 4, "The path estimate"): the ring of resampled generations,
// its transfers, the trace, the summary, the summary by the weights, the trunk the ring's oldest rows are settled into, and the
// most likely particle.  Host orchestration only; the kernels are pk_k_path.hip, pk_k_path_weighted.hip and pk_k_path_settle.hip.
// pk_resample (pk_api.hip) records through path_record; what refuses a recording filter says so through refuse_path (pk_api_shard.hip).
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
  dev_free(f, &f->trunk.rows);
  f->pt_cap = f->pt_out_cap = f->ps_rows = f->pw_rows = 0;
  f->path = PathRing();
  f->trunk = PathTrunk();
}

// every pk_path_trunk_* entry point but pk_path_trunk_enable, and pk_path_settle: a handle whose trunk is on
int need_trunk(const pk_filter* f, const char* who) {
  if (int rc = need_ring(f, who)) return rc;
  if (f->trunk.batch == 0) return fail(PK_ERR_STATE, "%s: the path has no trunk (pk_path_trunk_enable)", who);
  return PK_OK;
}

// pk_path_summary_weighted's scratch, which settling shares (both are call-local), sized for the whole ring at once: a filling
// ring does not reallocate at every step
int weighted_scratch(pk_filter* f, int64_t rows) {
  const size_t nb = (size_t)path_blocks(f->d.P), P = (size_t)f->d.P;
  const int64_t rows_cap = (int64_t)f->path.cap + 1;
  return dev_reserve_group(f, &f->pw_rows, rows, rows_cap, want(&f->pw_idx, P), want(&f->pw_wgt, P), want(&f->pw_ref, (size_t)rows_cap * 3),
                           want(&f->pw_part, (size_t)rows_cap * nb * kPathSums), want(&f->pw_res, (size_t)rows_cap * kPathWRes + 1));
}
double* weighted_gmax(pk_filter* f) { return f->pw_res + (size_t)(f->path.cap + 1) * kPathWRes; }

// room for `need` trunk rows: by doubling -- allocate, device-to-device copy, free.  The synchronisation here is the only one a
// settling step can meet.
int trunk_reserve(pk_filter* f, int64_t need) {
  PathTrunk& k = f->trunk;
  if (need <= k.cap) return PK_OK;
  int64_t cap = k.cap > 0 ? k.cap : 1;
  while (cap < need) cap *= 2;
  double* rows = nullptr;
  if (int rc = dev_alloc(f, &rows, (size_t)cap * kPathTrunkRes)) return rc;
  hipError_t e = hipSuccess;
  if (k.length > 0) e = hipMemcpyAsync(rows, k.rows, (size_t)k.length * kPathTrunkRes * sizeof(double), hipMemcpyDeviceToDevice, f->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    dev_free(f, &rows);
    return fail(PK_ERR_HIP, "the trunk could not grow to %lld rows: %s", (long long)cap, hipGetErrorString(e));
  }
  dev_free(f, &k.rows);
  k.rows = rows;
  k.cap = cap;
  return PK_OK;
}

// The oldest `rows` of the ring into the trunk, then out of the ring.  The host knows every count: nothing is read back.
// d: the generation whose lineages are walked (f->d, but for the one case path_record explains).
int settle(pk_filter* f, DeviceState& d, int rows, int weighting, int slot) {
  if (rows <= 0) return PK_OK;
  PathRing& r = f->path;
  PathTrunk& k = f->trunk;
  if (int rc = trunk_reserve(f, k.length + rows)) return rc;
  {
    Span t(f, slot);
    if (weighting == PK_WEIGHTS_LOG) launch_block_max(f->stream, d, f->partial, weighted_gmax(f));  // (f->partial: a workspace)
    launch_path_settle(f->stream, d, r, rows, weighted_gmax(f), weighting, f->pw_idx, f->pw_wgt, f->pw_ref, f->pw_part,
                       k.rows + (size_t)k.length * kPathTrunkRes);
  }
  r.first = (r.first + rows) % r.cap;
  r.held -= rows;
  k.length += rows;
  return PK_OK;
}

}  // namespace

int path_record(pk_filter* f, int weighting) {
  PathRing& r = f->path;
  if (f->trunk.batch && r.held == r.cap) {
    // The trunk was switched on over a full ring and nothing was settled since: this record must not overwrite.  The ring's rows
    // are the lineages of the generation that is about to be recorded (the OLD half of the pose buffers), so `batch` rows are
    // settled by that generation, every particle once.  Its lineages include those of the new generation: a row that is final
    // here is final; one that the resample has just made final is reported not final, which errs on the safe side.
    DeviceState old = f->d;
    old.cur ^= 1;
    if (int rc = settle(f, old, f->trunk.batch, PK_PATH_UNIFORM, PK_T_RESAMPLE)) return rc;
  }
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
  // with a trunk the ring is never full between two calls: the record that fills it settles the oldest `batch` rows at once
  if (f->trunk.batch && r.held == r.cap) return settle(f, f->d, f->trunk.batch, weighting, PK_T_RESAMPLE);
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
  PathTrunk& k = f->trunk;
  if (k.batch && k.length > 0 && recorded - n != k.first_step + k.length)
    return fail(PK_ERR_INVALID, "pk_path_upload: rows from step %lld on do not follow a trunk that ends at step %lld", (long long)(recorded - n),
                (long long)(k.first_step + k.length));
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
  if (k.batch) {
    if (k.length == 0) k.first_step = recorded - n;
    if (n == r.cap) {  // a full ring: the next record needs room
      if ((rc = settle(f, f->d, k.batch, PK_PATH_UNIFORM, PK_T_SUMMARY))) return rc;
      PK_LAUNCH_CHECK("pk_path_upload");
    }
  }
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
  const int64_t rows = (int64_t)r.held + 1;
  if ((rc = weighted_scratch(f, rows))) return rc;
  double* const gmax = weighted_gmax(f);
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

int pk_path_trunk_enable(pk_filter* f, int32_t batch) {
  if (int rc = need_ring(f, "pk_path_trunk_enable")) return rc;
  PathRing& r = f->path;
  PathTrunk& k = f->trunk;
  if (batch < 0 || batch > r.cap) return fail(PK_ERR_INVALID, "pk_path_trunk_enable: batches of %d rows from a ring of %d", batch, r.cap);
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipStreamSynchronize(f->stream));
  if (batch == 0) {
    dev_free(f, &k.rows);
    if (k.scratch_mine) {  // what switching it on reserved, so that off holds what it held before
      dev_free(f, &f->pw_idx);
      dev_free(f, &f->pw_wgt);
      dev_free(f, &f->pw_ref);
      dev_free(f, &f->pw_part);
      dev_free(f, &f->pw_res);
      f->pw_rows = 0;
    }
    k = PathTrunk();
    return PK_OK;
  }
  if (k.batch == 0) {
    const bool had = f->pw_rows > 0;
    if ((rc = weighted_scratch(f, (int64_t)r.cap + 1)) || (rc = trunk_reserve(f, std::max<int64_t>(4 * (int64_t)batch, 1024)))) {
      dev_free(f, &k.rows);
      k = PathTrunk();
      return rc;
    }
    k.scratch_mine = !had;
    k.length = 0;
    k.first_step = r.recorded - r.held;
  }
  k.batch = batch;  // (a ring that is full already stays so: pk_path_settle, or the next record, makes room -- path_record)
  return PK_OK;
}

int pk_path_settle(pk_filter* f, int32_t rows, int32_t weighting) {
  int rc;
  if ((rc = need_trunk(f, "pk_path_settle"))) return rc;
  if (rows < 0 || rows > f->path.held) return fail(PK_ERR_INVALID, "pk_path_settle: %d rows of the %d held", rows, f->path.held);
  if (weighting != PK_WEIGHTS_LINEAR && weighting != PK_WEIGHTS_LOG && weighting != PK_PATH_UNIFORM)
    return fail(PK_ERR_INVALID, "pk_path_settle: weighting %d", weighting);
  if (rows == 0) return PK_OK;
  if ((rc = use_device(f)) || (rc = settle(f, f->d, rows, weighting, PK_T_SUMMARY))) return rc;
  PK_LAUNCH_CHECK("pk_path_settle");
  return PK_OK;
}

int pk_path_trunk_shape(const pk_filter* f, int32_t* batch, int64_t* first_step, int64_t* length) {
  if (int rc = need_trunk(f, "pk_path_trunk_shape")) return rc;
  if (batch) *batch = f->trunk.batch;
  if (first_step) *first_step = f->trunk.first_step;
  if (length) *length = f->trunk.length;
  return PK_OK;
}

int pk_path_trunk_download(pk_filter* f, int64_t s0, int64_t s1, double* rows) {
  int rc;
  if ((rc = need_trunk(f, "pk_path_trunk_download"))) return rc;
  const PathTrunk& k = f->trunk;
  if (s0 < k.first_step || s1 < s0 || s1 > k.first_step + k.length)
    return fail(PK_ERR_INVALID, "pk_path_trunk_download: steps [%lld, %lld) of the trunk's [%lld, %lld)", (long long)s0, (long long)s1,
                (long long)k.first_step, (long long)(k.first_step + k.length));
  if (s1 == s0) return PK_OK;
  if (!rows) return fail(PK_ERR_INVALID, "pk_path_trunk_download: NULL rows");
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipMemcpyAsync(rows, k.rows + (size_t)(s0 - k.first_step) * kPathTrunkRes, (size_t)(s1 - s0) * kPathTrunkRes * sizeof(double),
                        hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

int pk_path_trunk_upload(pk_filter* f, int64_t first_step, int64_t n, const double* rows) {
  int rc;
  if ((rc = need_trunk(f, "pk_path_trunk_upload"))) return rc;
  if (f->path.held != 0) return fail(PK_ERR_STATE, "pk_path_trunk_upload: the ring holds %d rows (the trunk goes in first)", f->path.held);
  if (first_step < 0 || n < 0 || (n > 0 && !rows)) return fail(PK_ERR_INVALID, "pk_path_trunk_upload: bad argument");
  const double P = (double)f->d.P;
  for (int64_t i = 0; i < n; ++i) {
    const double lo = rows[(size_t)i * kPathTrunkRes + 8], hi = rows[(size_t)i * kPathTrunkRes + 9];
    if (!(lo >= 0.0 && lo <= hi && hi < P) || lo != std::floor(lo) || hi != std::floor(hi))
      return fail(PK_ERR_INVALID, "pk_path_trunk_upload: row %lld: lineages %g .. %g of %g particles", (long long)i, lo, hi, P);
  }
  if ((rc = use_device(f))) return rc;
  PathTrunk& k = f->trunk;
  const int64_t kept = k.length;
  k.length = 0;  // (nothing to carry over if the rows must grow)
  if ((rc = trunk_reserve(f, n))) {
    k.length = kept;
    return rc;
  }
  PK_HIP(hipStreamSynchronize(f->stream));
  if (n > 0) PK_HIP(hipMemcpyAsync(k.rows, rows, (size_t)n * kPathTrunkRes * sizeof(double), hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));  // (the caller's buffer is pageable)
  k.length = n;
  k.first_step = first_step;
  f->path.recorded = first_step + n;
  return PK_OK;
}

int pk_path_trunk_summary(pk_filter* f, int64_t s0, int64_t s1, double* mean, double* spread, int64_t* ancestors) {
  int rc;
  if ((rc = need_trunk(f, "pk_path_trunk_summary"))) return rc;
  const PathTrunk& k = f->trunk;
  if (s0 < k.first_step || s1 < s0 || s1 > k.first_step + k.length)
    return fail(PK_ERR_INVALID, "pk_path_trunk_summary: steps [%lld, %lld) of the trunk's [%lld, %lld)", (long long)s0, (long long)s1,
                (long long)k.first_step, (long long)(k.first_step + k.length));
  const int64_t n = s1 - s0;
  if (n == 0) return PK_OK;
  std::vector<double> h;
  try {
    h.resize((size_t)n * kPathTrunkRes);
  } catch (const std::bad_alloc&) {
    return fail(PK_ERR_NOMEM, "pk_path_trunk_summary: no host memory for %lld rows", (long long)n);
  }
  if ((rc = pk_path_trunk_download(f, s0, s1, h.data()))) return rc;
  for (int64_t t = 0; t < n; ++t) {
    const double* s = h.data() + (size_t)t * kPathTrunkRes;
    const bool final = s[8] == s[9];  // one lineage: its pose as recorded, no spread
    if (mean) {
      mean[3 * t] = final ? s[10] : s[0];
      mean[3 * t + 1] = final ? s[11] : s[1];
      mean[3 * t + 2] = final ? s[12] : std::atan2(s[2], s[3]);  // as pk_path_summary_weighted
    }
    if (spread) {
      spread[4 * t] = final ? 0.0 : s[4];
      spread[4 * t + 1] = final ? 0.0 : s[5];
      spread[4 * t + 2] = final ? 0.0 : s[6];
      spread[4 * t + 3] = final ? 1.0 : std::hypot(s[2], s[3]) / s[7];
    }
    if (ancestors) {
      ancestors[2 * t] = (int64_t)s[8];
      ancestors[2 * t + 1] = (int64_t)s[9];
    }
  }
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

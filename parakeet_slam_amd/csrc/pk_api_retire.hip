// Retirement of stale readings and unconfirmed features behind the C ABI (pk_filter.hpp): switching it on and
// off, the transfers of its clocks, the sensor's field of view (pk_grow_view).  Host orchestration only; the kernels are in pk_k_grow_retire.hip, launched behind
// k_new_landmarks (pk_api_observe.hip) and ahead of k_grow_gather (pk_resample, pk_resample_adaptive).  What cannot carry the clocks
// says so through refuse_retire (pk_api_shard.hip).
#include "pk_filter.hpp"

namespace {

void retire_release(pk_filter* f) {
  RetireState& r = f->retire;
  for (int i = 0; i < 2; ++i) {
    dev_free(f, &r.scan[i]);
    dev_free(f, &r.seen[i]);
    dev_free(f, &r.idle[i]);
    dev_free(f, &r.cnt[i]);
  }
  r = RetireState();
  dev_free(f, &f->view.stats);  // (pk_grow_view: the view goes with the clocks)
  f->view = RetireView();
}

// pk_grow_view / _state / _stats: a handle with retirement on
int view_handle(const pk_filter* f, const char* who) {
  if (!f) return fail(PK_ERR_INVALID, "%s: NULL handle", who);
  if (!f->grow_on) return fail(PK_ERR_STATE, "%s: pk_grow_enable was not called on this filter", who);
  if (!f->retire.on()) return fail(PK_ERR_STATE, "%s: nothing is being retired on this filter (pk_grow_retire)", who);
  return PK_OK;
}

// pk_grow_clocks_download / _upload: a handle with retirement on and a range of its particles
int clocks_range(pk_filter* f, const char* who, int64_t p0, int64_t p1) {
  if (!f) return fail(PK_ERR_INVALID, "%s: NULL handle", who);
  if (!f->grow_on) return fail(PK_ERR_STATE, "%s: pk_grow_enable was not called on this filter", who);
  if (!f->retire.on()) return fail(PK_ERR_STATE, "%s: nothing is being retired on this filter (pk_grow_retire)", who);
  if (p0 < 0 || p1 < p0 || p1 > f->d.P) return fail(PK_ERR_INVALID, "%s: particles [%lld, %lld) of %lld", who, (long long)p0, (long long)p1, (long long)f->d.P);
  return use_device(f);
}

}  // namespace

int retire_restart(pk_filter* f, int64_t p0, int64_t p1) {
  if (p1 <= p0) return PK_OK;
  // covered_readings, covered_slots = 0 (the first two of every particle's four words); the retired counters stay
  PK_HIP(hipMemset2DAsync(f->retire.cnt[f->grow.cur] + 4 * p0, 16, 0, 8, (size_t)(p1 - p0), f->stream));
  return PK_OK;
}

extern "C" {

int pk_grow_retire(pk_filter* f, int32_t reading_max_age, int32_t potential_max_idle) {
  if (!f) return fail(PK_ERR_INVALID, "pk_grow_retire: NULL handle");
  if (!f->grow_on) return fail(PK_ERR_STATE, "pk_grow_retire: pk_grow_enable was not called on this filter");
  constexpr int32_t kMax = 1 << 30;
  if (reading_max_age < 0 || reading_max_age > kMax || potential_max_idle < 0 || potential_max_idle > kMax)
    return fail(PK_ERR_INVALID, "pk_grow_retire: reading_max_age %d, potential_max_idle %d outside 0..2^30", reading_max_age, potential_max_idle);
  int rc;
  if ((rc = use_device(f))) return rc;
  RetireState& r = f->retire;
  if (reading_max_age == 0 && potential_max_idle == 0) {
    if (!r.on()) return PK_OK;
    PK_HIP(hipStreamSynchronize(f->stream));
    retire_release(f);
    return PK_OK;
  }
  if (!r.on()) {
    const GrowState& g = f->grow;
    const size_t P = (size_t)f->d.P;
    for (int i = 0; i < 2; ++i) {
      if (!rc) rc = dev_alloc(f, &r.scan[i], P * g.R);
      if (!rc) rc = dev_alloc(f, &r.seen[i], P * g.S);
      if (!rc) rc = dev_alloc(f, &r.idle[i], P * g.S);
      if (!rc) rc = dev_alloc(f, &r.cnt[i], P * 4);
    }
    if (rc) {
      retire_release(f);
      return rc;
    }
    // covered_* = 0: the next pass stamps what is there as new
    PK_HIP(hipMemsetAsync(r.cnt[g.cur], 0, P * 16, f->stream));
    r.t = 0;
  }
  r.A = reading_max_age;
  r.M = potential_max_idle;
  return PK_OK;
}

int pk_grow_view(pk_filter* f, double half_fov, double range_min, double range_max, int32_t confirmed_max_misses) {
  int rc;
  if ((rc = view_handle(f, "pk_grow_view"))) return rc;
  constexpr double kPi = 3.14159265358979323846;
  if (!(half_fov >= 0.0 && half_fov <= kPi)) return fail(PK_ERR_INVALID, "pk_grow_view: half_fov %g outside [0, pi]", half_fov);
  RetireView& v = f->view;
  if (half_fov == 0.0) {  // off: the counters stay allocated until the clocks go, and start again with the next view
    v.on = false;
    v.C = 0;
    return PK_OK;
  }
  if (!(range_min >= 0.0) || std::isinf(range_min)) return fail(PK_ERR_INVALID, "pk_grow_view: range_min %g is not a finite distance >= 0", range_min);
  if (!(range_max > range_min)) return fail(PK_ERR_INVALID, "pk_grow_view: range_max %g is not above range_min %g", range_max, range_min);
  if (confirmed_max_misses < 0 || confirmed_max_misses > (1 << 30))
    return fail(PK_ERR_INVALID, "pk_grow_view: confirmed_max_misses %d outside 0..2^30", (int)confirmed_max_misses);
  if ((rc = use_device(f))) return rc;
  if (!v.stats && (rc = dev_alloc(f, &v.stats, (size_t)kRetireViewWords))) return rc;
  static_assert(PK_GROW_VIEW_STATS_BYTES == kRetireViewWords * sizeof(unsigned long long), "parakeet_slam.h");
  if (!v.on) PK_HIP(hipMemsetAsync(v.stats, 0, kRetireViewWords * sizeof(unsigned long long), f->stream));  // switched on: the counters start
  v.on = true;
  v.C = confirmed_max_misses;
  v.half_fov = half_fov;
  v.r_min = range_min;
  v.r_max = range_max;
  v.rmin2 = range_min * range_min;
  v.rmax2 = range_max * range_max;
  return PK_OK;
}

int pk_grow_view_state(const pk_filter* f, int32_t* on, double view[3], int32_t* confirmed_max_misses) {
  if (!f) return fail(PK_ERR_INVALID, "pk_grow_view_state: NULL handle");
  const RetireView& v = f->view;
  if (on) *on = v.on ? 1 : 0;
  if (view) {
    view[0] = v.on ? v.half_fov : 0.0;
    view[1] = v.on ? v.r_min : 0.0;
    view[2] = v.on ? v.r_max : 0.0;
  }
  if (confirmed_max_misses) *confirmed_max_misses = v.C;
  return PK_OK;
}

int pk_grow_view_stats(pk_filter* f, int64_t out[4]) {
  int rc;
  if ((rc = view_handle(f, "pk_grow_view_stats"))) return rc;
  if (!out) return fail(PK_ERR_INVALID, "pk_grow_view_stats: NULL argument");
  if (!f->view.on) return fail(PK_ERR_STATE, "pk_grow_view_stats: this filter retires without a field of view (pk_grow_view)");
  if ((rc = use_device(f))) return rc;
  unsigned long long w[kRetireViewWords];
  PK_HIP(hipMemcpyAsync(w, f->view.stats, sizeof(w), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  for (int i = 0; i < kRetireViewWords; ++i) out[i] = (int64_t)w[i];
  return PK_OK;
}

int pk_grow_clocks_download(pk_filter* f, int64_t p0, int64_t p1, int32_t* counters, uint32_t* reading_scan, int32_t* slot_seen,
                            int32_t* slot_idle, uint32_t* scan_now) {
  int rc;
  if ((rc = clocks_range(f, "pk_grow_clocks_download", p0, p1))) return rc;
  const GrowState& g = f->grow;
  const RetireState& r = f->retire;
  const size_t n = (size_t)(p1 - p0);
  if (scan_now) *scan_now = r.t;
  if (n == 0) return PK_OK;
  const int c = g.cur;
  if (counters) PK_HIP(hipMemcpyAsync(counters, r.cnt[c] + 4 * p0, n * 16, hipMemcpyDeviceToHost, f->stream));
  if (reading_scan) PK_HIP(hipMemcpyAsync(reading_scan, r.scan[c] + (size_t)p0 * g.R, n * g.R * 4, hipMemcpyDeviceToHost, f->stream));
  if (slot_seen) PK_HIP(hipMemcpyAsync(slot_seen, r.seen[c] + (size_t)p0 * g.S, n * g.S * 4, hipMemcpyDeviceToHost, f->stream));
  if (slot_idle) PK_HIP(hipMemcpyAsync(slot_idle, r.idle[c] + (size_t)p0 * g.S, n * g.S * 4, hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

int pk_grow_clocks_upload(pk_filter* f, int64_t p0, int64_t p1, const int32_t* counters, const uint32_t* reading_scan,
                          const int32_t* slot_seen, const int32_t* slot_idle, const uint32_t* scan_now) {
  int rc;
  if ((rc = clocks_range(f, "pk_grow_clocks_upload", p0, p1))) return rc;
  const GrowState& g = f->grow;
  RetireState& r = f->retire;
  const size_t n = (size_t)(p1 - p0);
  const int c = g.cur;
  if (counters && n > 0) {  // covered_* within what the particle holds
    std::vector<int32_t> have;
    try {
      have.resize(4 * n);
    } catch (const std::bad_alloc&) {
      return fail(PK_ERR_NOMEM, "pk_grow_clocks_upload: no host memory for the counters of %zu particles", n);
    }
    PK_HIP(hipMemcpyAsync(have.data(), g.cnt[c] + 4 * p0, n * 16, hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    for (size_t i = 0; i < n; ++i) {
      const int32_t* k = counters + 4 * i;
      if (k[0] < 0 || k[0] > have[4 * i] || k[1] < 0 || k[1] > have[4 * i + 1] || k[2] < 0 || k[3] < 0)
        return fail(PK_ERR_INVALID, "pk_grow_clocks_upload: particle %lld: %d readings covered of %d stored, %d slots covered of %d in use",
                    (long long)(p0 + (int64_t)i), k[0], have[4 * i], k[1], have[4 * i + 1]);
    }
  }
  if (scan_now) r.t = *scan_now;
  if (n == 0) return PK_OK;
  if (counters) PK_HIP(hipMemcpyAsync(r.cnt[c] + 4 * p0, counters, n * 16, hipMemcpyHostToDevice, f->stream));
  if (reading_scan) PK_HIP(hipMemcpyAsync(r.scan[c] + (size_t)p0 * g.R, reading_scan, n * g.R * 4, hipMemcpyHostToDevice, f->stream));
  if (slot_seen) PK_HIP(hipMemcpyAsync(r.seen[c] + (size_t)p0 * g.S, slot_seen, n * g.S * 4, hipMemcpyHostToDevice, f->stream));
  if (slot_idle) PK_HIP(hipMemcpyAsync(r.idle[c] + (size_t)p0 * g.S, slot_idle, n * g.S * 4, hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

}  // extern "C"

// Range-bearing scans behind the C ABI (pk_filter.hpp): pk_scan_ranges arms the ranges of the next scan, the calls that take blobs
// consume them (ranges_take), and what such a scan has no kernel for is said here, once (refuse_ranges).  Host orchestration only:
// the ranges travel in the scan's own staging block (pk_api_scan.hip, pk_scan_block.hpp), the kernels are the range instances of pk_k_observe.hip
// and pk_k_assoc.hip, and pk_probe_range lives beside its kernels in pk_k_mathprobe.hip.
#include "pk_filter.hpp"

// What a scan with armed (or staged) ranges is refused for, in this order -- the first that applies answers:
//   1. another number of blobs than the ranges were armed for                          PK_ERR_INVALID
//   2. a filter that is not on PK_MODEL_BEARING                                         PK_ERR_UNSUPPORTED
//   3. the dense layout: the bearing model's own refusal, in its own words              PK_ERR_UNSUPPORTED
//   4. growing maps (pk_grow_enable), unless pk_grow_ranges is on                       PK_ERR_UNSUPPORTED
// pk_propose / pk_propose_odom refuse armed ranges before anything else (refuse_ranges_proposal) -- unless pk_proposal_ranges is on:
// then they consume them (ranges_take), these refusals ahead of the proposal's own.  Nothing has changed when one of them answers,
// except that the ranges are gone.
int refuse_ranges(const pk_filter* f, const char* who, int32_t B, int32_t armed_B) {
  if (B != armed_B)
    return fail(PK_ERR_INVALID, "%s: pk_scan_ranges named the ranges of a scan of %d blobs, this one has %d", who, (int)armed_B, (int)B);
  if (f->model != PK_MODEL_BEARING)
    return fail(PK_ERR_UNSUPPORTED, "%s: per-blob ranges (pk_scan_ranges) are an option of the bearing model "
                                    "(pk_set_measurement_model(f, PK_MODEL_BEARING)); the reference model has no range", who);
  if (f->dense) return refuse_bearing(f, who, "the dense layout (covariances or a Qt that couple position, bearing and colour)");
  if (f->grow_on && !f->grow_ranges)
    return fail(PK_ERR_UNSUPPORTED, "%s: per-blob ranges (pk_scan_ranges) have no kernel for growing maps (pk_grow_enable): a new "
                                    "landmark is still placed from two bearings", who);
  return PK_OK;
}

void ranges_disarm(pk_filter* f) {
  if (f) f->rng = pk_filter::Ranges();
}

int ranges_check(pk_filter* f, const char* who, int32_t B) {
  if (!f || !f->rng.armed) return PK_OK;
  const int rc = refuse_ranges(f, who, B, f->rng.B);
  if (rc) ranges_disarm(f);
  return rc;
}

int ranges_take(pk_filter* f, const char* who, int32_t B, RangeScan* out) {
  *out = RangeScan();
  if (!f || !f->rng.armed) return PK_OK;
  pk_filter::Ranges r;
  std::swap(r, f->rng);  // consumed, whatever follows
  if (int rc = refuse_ranges(f, who, B, r.B)) return rc;
  out->armed = true;
  out->any = r.any;
  out->rv.swap(r.rv);
  return PK_OK;
}

int refuse_ranges_proposal(pk_filter* f, const char* who) {
  if (!f || !f->rng.armed) return PK_OK;
  ranges_disarm(f);
  return fail(PK_ERR_UNSUPPORTED, "%s: per-blob ranges (pk_scan_ranges) are not part of the measurement-informed proposal: it samples "
                                  "the pose from the bearings alone unless pk_proposal_ranges(f, 1) switches them in", who);
}

extern "C" {

int pk_scan_ranges(pk_filter* f, const double* ranges, const double* variances, int32_t B) {
  if (!f) return fail(PK_ERR_INVALID, "pk_scan_ranges: NULL handle");
  if (B < 0) return fail(PK_ERR_INVALID, "pk_scan_ranges: %d blobs", (int)B);
  if (B == 0 || !ranges) {
    ranges_disarm(f);
    return PK_OK;
  }
  ranges_disarm(f);  // (a refused call arms nothing, and what was armed before it is gone)
  bool any = false;
  for (int b = 0; b < B; ++b) {
    const double r = ranges[b];
    if (std::isnan(r)) continue;
    if (!(std::isfinite(r) && r > 0.0)) return fail(PK_ERR_INVALID, "pk_scan_ranges: ranges[%d] = %g is neither NaN (no range) nor finite and > 0", b, r);
    if (!variances || !(std::isfinite(variances[b]) && variances[b] > 0.0))
      return fail(PK_ERR_INVALID, "pk_scan_ranges: variances[%d] = %g is not finite and > 0 beside a finite range", b, variances ? variances[b] : NAN);
    any = true;
  }
  pk_filter::Ranges r;
  r.rv.resize(2 * (size_t)B);
  for (int b = 0; b < B; ++b) {
    const bool has = !std::isnan(ranges[b]);
    r.rv[2 * (size_t)b] = ranges[b];
    r.rv[2 * (size_t)b + 1] = has ? variances[b] : 0.0;
  }
  r.armed = true;
  r.any = any;
  r.B = B;
  std::swap(f->rng, r);
  return PK_OK;
}

// pk_grow_ranges: ranged scans on a growing map -- refusal 4 above steps aside, and the bookkeeping kernel places a new feature from
// one ranged sighting (k_new_landmarks_ranged / _tri_ranged, pk_k_grow.hip), from the next scan on (it keeps no per-particle state)
int pk_grow_ranges(pk_filter* f, int32_t on) {
  if (!f) return fail(PK_ERR_INVALID, "pk_grow_ranges: NULL handle");
  if (!f->grow_on) return fail(PK_ERR_STATE, "pk_grow_ranges: pk_grow_enable was not called on this filter");
  if (on != 0 && on != 1) return fail(PK_ERR_INVALID, "pk_grow_ranges: on = %d is neither 0 nor 1", (int)on);
  f->grow_ranges = on == 1;
  return PK_OK;
}

int pk_grow_ranges_state(const pk_filter* f, int32_t* on) {
  if (!f) return fail(PK_ERR_INVALID, "pk_grow_ranges_state: NULL handle");
  if (on) *on = f->grow_ranges ? 1 : 0;
  return PK_OK;
}

int pk_scan_ranges_state(const pk_filter* f, int32_t* armed, int32_t* staged) {
  if (!f) return fail(PK_ERR_INVALID, "pk_scan_ranges_state: NULL handle");
  if (armed) *armed = f->rng.armed ? f->rng.B : 0;
  if (staged) *staged = (f->staged.valid && f->staged.with_ranges) ? f->staged.B : 0;
  return PK_OK;
}

}  // extern "C"

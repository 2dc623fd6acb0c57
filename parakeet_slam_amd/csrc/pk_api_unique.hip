// Unique association behind the C ABI (include/parakeet_slam.h; DESIGN.md section 4, "Unique association"): pk_assoc_unique and its
// read-outs, the pass that follows the maximum-likelihood association while the mode is on (k_assoc_unique, pk_k_assoc_unique.hip),
// what the mode refuses.  Host orchestration only.  The mode is configuration: no snapshot holds it.
#include "pk_filter.hpp"

int unique_refuse(const pk_filter* f, const char* who, const char* what) {
  if (f && f->uq.on)
    return fail(PK_ERR_UNSUPPORTED, "%s: unique association (pk_assoc_unique) settles the ids of the general association route and "
                                    "has no kernel for %s; pk_assoc_unique(f, 0) takes it", who, what);
  return PK_OK;
}

int unique_fits(const pk_filter* f, const char* who, int32_t B) {
  const int Lp = f->d.lay.Lp;
  if (assoc_unique_lds_bytes(Lp, B) > kMaxDynLds)
    return fail(PK_ERR_UNSUPPORTED, "%s: unique association (pk_assoc_unique) keeps 12 bytes per padded landmark and 14 per blob in LDS: "
                                    "12 x %d + 14 x %d = %zu bytes, the workgroup has %zu", who, Lp, (int)B, assoc_unique_lds_bytes(Lp, B),
                (size_t)kMaxDynLds);
  return PK_OK;
}

int unique_check(const pk_filter* f, const char* who, int32_t B) {
  if (!f->uq.on) return PK_OK;
  if (f->dense) return unique_refuse(f, who, "the dense layout (covariances or a Qt that couple position, bearing and colour)");
  return unique_fits(f, who, B);
}

int unique_settle(pk_filter* f, const ScanTables& scan) {
  pk_filter::Unique& u = f->uq;
  PK_HIP(hipMemsetAsync(u.stats, 0, 4 * sizeof(unsigned long long), f->stream));  // (word 4 stays up until unique_error reports it)
  AssocUniqueLaunch q;
  q.ids_dev = f->ids_dev;
  q.stats_dev = u.stats;
  q.model = f->model;
  q.q00 = f->qt.q00;
  launch_assoc_unique(f->stream, f->d, scan, q);
  PK_HIP(hipMemcpyAsync(u.seen, u.stats, kAssocUniqueWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
  u.last = true;
  return PK_OK;
}

int unique_error(pk_filter* f, const char* who) {
  pk_filter::Unique& u = f->uq;
  if (!u.seen || u.seen[4] == 0ull) return PK_OK;
  u.seen[4] = 0ull;
  PK_HIP(hipMemsetAsync(u.stats + 4, 0, sizeof(unsigned long long), f->stream));
  return fail(PK_ERR_HIP, "%s: k_assoc_unique stopped a particle at its bound of B + 1 passes and left the ids it had (a device error: "
                          "the bound holds for every input)", who);
}

extern "C" {

int pk_assoc_unique(pk_filter* f, int32_t on) {
  if (!f) return fail(PK_ERR_INVALID, "pk_assoc_unique: NULL handle");
  if (on != 0 && on != 1) return fail(PK_ERR_INVALID, "pk_assoc_unique: on = %d is neither 0 nor 1", (int)on);
  if (f->split.active) return fail(PK_ERR_STATE, "pk_assoc_unique: a split observe is in progress");
  if (on && (!f->uq.seen || !f->uq.stats)) {  // (each block on its own: a failure between the two leaves nothing to allocate twice)
    int rc;
    if ((rc = use_device(f))) return rc;
    if (!f->uq.seen) {
      if ((rc = host_alloc(f, &f->uq.seen, kAssocUniqueWords, hipHostMallocDefault))) return rc;
      memset(f->uq.seen, 0, kAssocUniqueWords * sizeof(unsigned long long));
    }
    if (!f->uq.stats) {
      if ((rc = dev_alloc(f, &f->uq.stats, kAssocUniqueWords))) return rc;
      PK_HIP(hipMemsetAsync(f->uq.stats, 0, kAssocUniqueWords * sizeof(unsigned long long), f->stream));
    }
  }
  f->uq.on = on == 1;
  return PK_OK;
}

int pk_assoc_unique_state(const pk_filter* f, int32_t* on) {
  if (!f) return fail(PK_ERR_INVALID, "pk_assoc_unique_state: NULL handle");
  if (on) *on = f->uq.on ? 1 : 0;
  return PK_OK;
}

int pk_assoc_unique_stats(pk_filter* f, int64_t out[4]) {
  if (!f || !out) return fail(PK_ERR_INVALID, "pk_assoc_unique_stats: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  for (int i = 0; i < 4; ++i) out[i] = 0;
  PK_HIP(hipStreamSynchronize(f->stream));
  if ((rc = unique_error(f, "pk_assoc_unique_stats"))) return rc;
  if (f->uq.last && f->uq.seen)
    for (int i = 0; i < 4; ++i) out[i] = (int64_t)f->uq.seen[i];
  if (f->uq.last && out[3] == 0) out[3] = 1;  // (the kernel counts the passes of the particles with a conflict: the others took one)
  return PK_OK;
}

}  // extern "C"

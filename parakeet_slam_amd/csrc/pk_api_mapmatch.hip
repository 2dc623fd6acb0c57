// The discovered landmarks behind the C ABI (pk_filter.hpp; DESIGN.md section 4, "The discovered landmarks"): the moments of the
// particles' spare slots matched against a list of reference features, and the finished estimate about the most likely particle's
// own features.  Host orchestration only; the kernels are pk_k_mapmatch.hip.  Reads the particles where they are (src[], the
// adoption buffer): no materialise, no filter state changes, no synchronisation between the launches.
#include "pk_filter.hpp"

namespace {

constexpr size_t kMmHead = 2 + 2 * (size_t)kMatchMaxGroups;  // f->mm_res: a maximum log-weight (2 words) | the groups' weight sums | the result

struct MatchCall {
  const char* who;
  int32_t weighting;
  double gmax;     // pk_map_match_moments': NaN = this handle's own
  double radius, colour_radius;
  int rows;        // rows of the result
};

// what both entry points refuse, in the order of map_moments_host; then the colour rows and the scratch for `rows` features
int match_ready(pk_filter* f, const MatchCall& c) {
  if (!f) return fail(PK_ERR_INVALID, "%s: NULL handle", c.who);
  if (c.weighting != PK_MAP_UNIFORM && c.weighting != PK_MAP_WEIGHTED) return fail(PK_ERR_INVALID, "%s: weighting %d", c.who, c.weighting);
  if (!(c.radius > 0.0)) return fail(PK_ERR_INVALID, "%s: radius %g is not > 0", c.who, c.radius);
  if (!(c.colour_radius > 0.0)) return fail(PK_ERR_INVALID, "%s: colour_radius %g is not > 0", c.who, c.colour_radius);
  if (!f->map_loaded) return fail(PK_ERR_STATE, "%s: no map uploaded", c.who);
  if (f->dense) return fail(PK_ERR_UNSUPPORTED, "%s: the map estimate reads the compact layout; this filter is on the dense one", c.who);
  if (!f->grow_on) return fail(PK_ERR_STATE, "%s: pk_grow_enable was not called on this filter", c.who);
  if (c.weighting == PK_MAP_WEIGHTED && !std::isnan(c.gmax) && !std::isfinite(c.gmax))
    return fail(PK_ERR_STATE, "%s: no finite maximum log-weight (%g): every weight is zero, or one is not finite", c.who, c.gmax);
  return PK_OK;
}

// the scratch, at the first call and when a call needs more: the reference block and the result by rows, the partials by doubles
int match_scratch(pk_filter* f, int rows, int groups) {
  int rc;
  const size_t r = (size_t)(rows > 0 ? rows : 1);
  if ((rc = dev_reserve_group(f, &f->mm_rows, r, r, want(&f->mm_ref, r * 5), want(&f->mm_refi, 4 + 2 * r),
                              want(&f->mm_res, kMmHead + map_match_res_doubles((int)r)))))
    return rc;
  const size_t need = map_match_part_doubles(rows, groups);
  return dev_reserve(f, &f->mm_part, &f->mm_part_cap, need, need);
}

MatchJob match_job(pk_filter* f, const MatchCall& c, int groups) {
  MatchJob m;
  m.rows = c.rows;
  m.groups = groups;
  m.weighted = c.weighting == PK_MAP_WEIGHTED;
  m.gmax = c.gmax;
  if (m.weighted && std::isnan(c.gmax)) {  // this handle's own maximum, left on the device
    launch_block_max(f->stream, f->d, f->partial, f->mm_res);
    m.gmax_dev = f->mm_res;
  }
  // (in double, once: the kernels and the tests' reference compare against the same four numbers)
  m.rho2 = c.radius * c.radius;
  m.kap2 = c.colour_radius * c.colour_radius;
  m.irho2 = std::isinf(m.rho2) ? 0.0 : 1.0 / m.rho2;
  m.ikap2 = std::isinf(m.kap2) ? 0.0 : 1.0 / m.kap2;
  m.ref_dev = f->mm_ref;
  m.part_dev = f->mm_part;
  m.wpart_dev = f->mm_res + 2;
  m.res_dev = f->mm_res + kMmHead;
  return m;
}

// the result on the host, and what only the device knew: the maximum log-weight it took, the weights' sum
int match_result(pk_filter* f, const MatchCall& c, std::vector<double>& h) {
  PK_LAUNCH_CHECK(c.who);
  PK_HIP(hipMemcpyAsync(h.data(), f->mm_res + kMmHead, h.size() * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  const double gmax = h[2 + (size_t)kMatchSums * c.rows];
  if (c.weighting == PK_MAP_WEIGHTED && !std::isfinite(gmax))
    return fail(PK_ERR_STATE, "%s: no finite maximum log-weight (%g): every weight is zero, or one is not finite", c.who, gmax);
  if (!(h[0] > 0.0) || !std::isfinite(h[0]) || !std::isfinite(h[1]))
    return fail(PK_ERR_STATE, "%s: the weights sum to %g: not positive and finite", c.who, h[0]);
  return PK_OK;
}

}  // namespace

extern "C" {

int pk_map_match_moments(pk_filter* f, int32_t weighting, double gmax, const double* ref_means, int32_t n_ref, double radius,
                         double colour_radius, double wsum[2], double* support, double* mean, double* m2, double* within, double* counts,
                         int32_t* matches) {
  const MatchCall c{"pk_map_match_moments", weighting, gmax, radius, colour_radius, (int)n_ref};
  if (f && (n_ref < 0 || n_ref > kMatchMaxRef || (n_ref > 0 && !ref_means)))
    return fail(PK_ERR_INVALID, "pk_map_match_moments: %d reference features (0 .. %d, with their means)", n_ref, kMatchMaxRef);
  int rc;
  if ((rc = match_ready(f, c))) return rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = colour_rows_for_download(f, 0, f->d.P))) return rc;
  const DeviceState& d = f->d;
  const int groups = map_match_groups(d.P, n_ref, f->opt.map_match_groups);
  if ((rc = match_scratch(f, n_ref, groups))) return rc;
  const size_t n_match = (size_t)d.P * (size_t)n_ref;
  if (matches && n_match && (rc = dev_reserve(f, &f->mm_match, &f->mm_match_cap, n_match, n_match))) return rc;
  std::vector<double> h;
  try {
    h.resize(map_match_res_doubles(n_ref));
  } catch (const std::bad_alloc&) {
    return fail(PK_ERR_NOMEM, "pk_map_match_moments: no host memory for %d features' moments", n_ref);
  }
  if (n_ref) PK_HIP(hipMemcpyAsync(f->mm_ref, ref_means, (size_t)n_ref * 5 * sizeof(double), hipMemcpyHostToDevice, f->stream));
  {
    Span t(f, PK_T_SUMMARY);
    MatchJob m = match_job(f, c, groups);
    m.nref = n_ref;
    m.matches_dev = matches && n_match ? f->mm_match : nullptr;
    launch_map_match(f->stream, d, f->grow, m);
  }
  if (matches && n_match) PK_HIP(hipMemcpyAsync(matches, f->mm_match, n_match * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
  if ((rc = match_result(f, c, h))) return rc;
  const size_t n = (size_t)n_ref;
  if (wsum) memcpy(wsum, h.data(), 2 * sizeof(double));
  if (support) memcpy(support, h.data() + 2, n * 3 * sizeof(double));
  if (mean) memcpy(mean, h.data() + 2 + n * 3, n * 5 * sizeof(double));
  if (m2) memcpy(m2, h.data() + 2 + n * 8, n * 15 * sizeof(double));
  if (within) memcpy(within, h.data() + 2 + n * 23, n * 9 * sizeof(double));
  if (counts) memcpy(counts, h.data() + 2 + n * 32, n * sizeof(double));
  return PK_OK;
}

int pk_map_discovered(pk_filter* f, int32_t weighting, int64_t reference_particle, double radius, double colour_radius,
                      int64_t* reference_out, int32_t* n_out, int32_t* ids, int32_t* ref_counts, double* mean, double* cov_within,
                      double* cov_between, double* update_count, double* support, double* potential_fraction, double* n_eff,
                      double* n_eff_all) {
  MatchCall c{"pk_map_discovered", weighting, std::nan(""), radius, colour_radius, 0};
  if (f && (reference_particle < -1 || reference_particle >= f->d.P))
    return fail(PK_ERR_INVALID, "pk_map_discovered: reference particle %lld of %lld (-1: the most likely one)", (long long)reference_particle,
                (long long)f->d.P);
  int rc;
  if ((rc = match_ready(f, c))) return rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = colour_rows_for_download(f, 0, f->d.P))) return rc;
  const DeviceState& d = f->d;
  const int S = f->grow.S;
  c.rows = S;
  const int groups = map_match_groups(d.P, S, f->opt.map_match_groups);
  if ((rc = match_scratch(f, S, groups))) return rc;
  std::vector<double> h;
  try {
    h.resize(map_match_res_doubles(S));
  } catch (const std::bad_alloc&) {
    return fail(PK_ERR_NOMEM, "pk_map_discovered: no host memory for %d features' moments", S);
  }
  {
    Span t(f, PK_T_SUMMARY);
    MatchJob m = match_job(f, c, groups);
    const double* best = nullptr;
    if (reference_particle < 0) {  // k_best_particle_fold's result feeds the reference kernel on the device (f->partial: a workspace)
      double* const out = f->partial + 2 * kPathMaxBlocks;
      launch_best_particle(f->stream, d, f->partial, out);
      best = out;
    }
    launch_match_reference(f->stream, d, f->grow, best, reference_particle, f->mm_ref, f->mm_refi);
    m.refi_dev = f->mm_refi;
    launch_map_match(f->stream, d, f->grow, m);
  }
  if ((rc = match_result(f, c, h))) return rc;
  const size_t n = (size_t)S;
  const double* tail = h.data() + 2 + n * kMatchSums;
  if (tail[2] < 0.0) return fail(PK_ERR_STATE, "pk_map_discovered: every log-weight is NaN");
  const int nref = (int)tail[1];
  if (reference_out) *reference_out = (int64_t)tail[2];
  if (n_out) *n_out = nref;
  const double W = h[0];
  for (size_t l = 0; l < n; ++l) {
    const double* sup = h.data() + 2 + l * 3;
    const double* s2 = h.data() + 2 + n * 8 + l * 15;
    const double* wi = h.data() + 2 + n * 23 + l * 9;
    const double Wj = sup[0];  // (0 where nobody matched: every quotient below is NaN then, and the support 0)
    const bool in = (int)l < nref;
    if (ids) ids[l] = in ? (int32_t)tail[3 + n + l] : 0;
    if (ref_counts) ref_counts[l] = in ? (int32_t)tail[3 + l] : 0;
    if (mean) memcpy(mean + l * 5, h.data() + 2 + n * 3 + l * 5, 5 * sizeof(double));
    if (cov_within) {  // the compact fields back into the dense 5x5 of pk_map_summary
      double* cw = cov_within + l * 25;
      const double z = in && Wj > 0.0 ? 0.0 : std::nan("");
      for (int i = 0; i < 25; ++i) cw[i] = z;
      cw[0] = wi[F_PXX - F_PXX] / Wj;
      cw[1] = cw[5] = wi[F_PXY - F_PXX] / Wj;
      cw[6] = wi[F_PYY - F_PXX] / Wj;
      cw[12] = wi[F_CRR - F_PXX] / Wj;
      cw[13] = cw[17] = wi[F_CRG - F_PXX] / Wj;
      cw[14] = cw[22] = wi[F_CRB - F_PXX] / Wj;
      cw[18] = wi[F_CGG - F_PXX] / Wj;
      cw[19] = cw[23] = wi[F_CGB - F_PXX] / Wj;
      cw[24] = wi[F_CBB - F_PXX] / Wj;
    }
    if (cov_between) {
      double* cb = cov_between + l * 25;
      int k = 0;
      for (int i = 0; i < 5; ++i)
        for (int j = i; j < 5; ++j) cb[i * 5 + j] = cb[j * 5 + i] = s2[k++] / Wj;
    }
    if (update_count) update_count[l] = h[2 + n * 32 + l] / Wj;
    if (support) support[l] = in ? Wj / W : 0.0;
    if (potential_fraction) potential_fraction[l] = sup[2] / Wj;
    if (n_eff) n_eff[l] = Wj * Wj / sup[1];
  }
  if (n_eff_all) *n_eff_all = W * W / h[1];
  return PK_OK;
}

}  // extern "C"

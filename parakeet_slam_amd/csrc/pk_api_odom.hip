// The odometry motion model behind the C ABI (include/parakeet_slam.h; DESIGN.md section 4, "The odometry motion model"): the delta
// between two odometry poses and its sigmas on the host -- O(1) per message, the same for every particle, as launch_motion forms
// sd and sh -- and the calls that move the particles by them.  Host orchestration only; the kernel is pk_k_motion_odom.hip, the
// step's body step_impl (pk_api.hip).
#include "pk_filter.hpp"

namespace {

constexpr double kPi = 3.14159265358979323846, kTwoPi = 6.28318530717958647692;

// The one wrap of the model: into [-pi, pi].  IEEE remainder is exact, so wrap(a) == a whenever |a| <= pi.
double wrap(double a) { return std::remainder(a, kTwoPi); }

// (every product and sum below rounds by itself: the delta and the sigmas are what any IEEE host computes from the same formulas)
#pragma clang fp contract(off)
void odom_delta(const double prev[3], const double now[3], double min_trans, double delta[3]) {
  const double dx = now[0] - prev[0], dy = now[1] - prev[1];
  const double trans = std::hypot(dx, dy);
  const double dth = wrap(now[2] - prev[2]);
  const double rot1 = trans < min_trans ? 0.0 : wrap(std::atan2(dy, dx) - prev[2]);
  delta[0] = rot1;
  delta[1] = trans;
  delta[2] = wrap(dth - rot1);
}

void odom_sigmas(const double delta[3], const double alpha[4], double sigma[3]) {
  // folded: driving backwards (rot1 near +-pi) is no large turn
  const double r1n = std::fmin(std::fabs(delta[0]), kPi - std::fabs(delta[0]));
  const double r2n = std::fmin(std::fabs(delta[2]), kPi - std::fabs(delta[2]));
  const double r1q = r1n * r1n, r2q = r2n * r2n, tq = delta[1] * delta[1];
  const double a = alpha[0] * r1q, b = alpha[1] * tq, c = alpha[2] * tq, d = alpha[3] * (r1q + r2q), e = alpha[0] * r2q;
  sigma[0] = std::sqrt(a + b);
  sigma[1] = std::sqrt(c + d);
  sigma[2] = std::sqrt(e + b);
}

int bad_delta(const char* who, const double delta[3]) {
  if (!delta) return fail(PK_ERR_INVALID, "%s: delta is NULL", who);
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(delta[i])) return fail(PK_ERR_INVALID, "%s: delta[%d] is not finite", who, i);
  if (delta[1] < 0.0) return fail(PK_ERR_INVALID, "%s: trans = %g is negative", who, delta[1]);
  return PK_OK;
}
int bad_alpha(const char* who, const double alpha[4]) {
  if (!alpha) return fail(PK_ERR_INVALID, "%s: alpha is NULL", who);
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(alpha[i]) || alpha[i] < 0.0) return fail(PK_ERR_INVALID, "%s: alpha[%d] = %g is not finite and >= 0", who, i, alpha[i]);
  return PK_OK;
}

}  // namespace

int motion_odom_checked(pk_filter* f, const double delta[3], const double sigma[3], const double* z, uint64_t seed, uint64_t draw) {
  return motion_impl(f, "pk_motion_odom", z, [&](const double* zd, void* up_dst, const void* up_src, size_t up_bytes) {
    launch_motion_odom(f->stream, f->d, delta, sigma, zd, seed, draw, up_dst, up_src, up_bytes, f->pose_part);
  });
}

extern "C" {

int pk_odom_delta(const double prev[3], const double now[3], double min_trans, double delta[3]) {
  if (!prev || !now || !delta) return fail(PK_ERR_INVALID, "pk_odom_delta: NULL argument");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(prev[i]) || !std::isfinite(now[i])) return fail(PK_ERR_INVALID, "pk_odom_delta: pose component %d is not finite", i);
  if (!std::isfinite(min_trans) || min_trans < 0.0) return fail(PK_ERR_INVALID, "pk_odom_delta: min_trans = %g is not finite and >= 0", min_trans);
  double d[3];
  odom_delta(prev, now, min_trans, d);
  if (int rc = bad_delta("pk_odom_delta", d)) return rc;  // (poses so far apart that their difference overflows)
  memcpy(delta, d, sizeof(d));
  return PK_OK;
}

int pk_odom_sigmas(const double delta[3], const double alpha[4], double sigma[3]) {
  int rc;
  if ((rc = bad_delta("pk_odom_sigmas", delta)) || (rc = bad_alpha("pk_odom_sigmas", alpha))) return rc;
  if (!sigma) return fail(PK_ERR_INVALID, "pk_odom_sigmas: sigma is NULL");
  double s[3];
  odom_sigmas(delta, alpha, s);
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(s[i])) return fail(PK_ERR_INVALID, "pk_odom_sigmas: sigma[%d] is not finite", i);
  memcpy(sigma, s, sizeof(s));
  return PK_OK;
}

int pk_motion_odom(pk_filter* f, const double delta[3], const double alpha[4], const double* z, uint64_t seed, uint64_t draw) {
  if (!f) return fail(PK_ERR_INVALID, "pk_motion_odom: NULL handle");
  double sigma[3];
  if (int rc = pk_odom_sigmas(delta, alpha, sigma)) return rc;
  return motion_odom_checked(f, delta, sigma, z, seed, draw);
}

int pk_motion_odom_range(pk_filter* f, const double delta[3], const double alpha[4], uint64_t seed, uint64_t draw, int64_t p0, int64_t p1) {
  if (!f) return fail(PK_ERR_INVALID, "pk_motion_odom_range: NULL handle");
  double sigma[3];
  int rc;
  if ((rc = pk_odom_sigmas(delta, alpha, sigma))) return rc;
  if (p0 < 0 || p1 < p0 || p1 > f->d.P) return fail(PK_ERR_INVALID, "pk_motion_odom_range: bad particle range [%lld, %lld)", (long long)p0, (long long)p1);
  poses_change(f);
  if ((rc = use_device(f))) return rc;
  Span t(f, PK_T_MOTION);
  launch_motion_odom_range(f->stream, f->d, delta, sigma, seed, draw, p0, p1);
  PK_LAUNCH_CHECK("pk_motion_odom_range");
  return PK_OK;
}

int pk_step_odom(pk_filter* f, const double delta[3], const double alpha[4], const double* z, uint64_t seed, uint64_t draw,
                 const double* blobs, int32_t B, const int32_t* ids, double u, int32_t weight_domain, double threshold) {
  if (!f) return fail(PK_ERR_INVALID, "pk_step_odom: NULL handle");
  StepMotion m;
  m.odom = true;
  if (int rc = pk_odom_sigmas(delta, alpha, m.sigma)) return rc;  // before anything moves
  memcpy(m.delta, delta, sizeof(m.delta));
  const bool gated = !std::isnan(threshold);  // (NaN: no gate)
  if (gated)
    if (int rc = bad_threshold("pk_step_odom", threshold)) return rc;
  return step_impl(f, m, z, seed, draw, blobs, B, ids, u, weight_domain, gated ? &threshold : nullptr);
}

}  // extern "C"

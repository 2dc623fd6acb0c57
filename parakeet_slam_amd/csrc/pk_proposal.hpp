// The measurement-informed proposal (FastSLAM 2.0 sampling; DESIGN.md section 4, "The measurement-informed proposal"): the device
// math of k_propose (pk_k_propose.hip), register resident like pk_math.hpp and compiled with the same contraction rules.
//
// Everything works in the space of the three standard normals xi the motion kernels consume (prior N(0, I)): the pose is
// g(x-, u, s (.) xi), s the sigmas of the launch.  Around the predicted pose g(x-, u, 0) every settled match b -> j gives one scalar
// innovation nu with variance sigma^2 and the row a = s (.) (G' h_x): nu(xi) ~ nu - a' xi.  The sums below are all a particle needs:
//   Lambda = I + sum a a' / sigma^2,  eta = sum a nu / sigma^2,  c = sum nu^2 / sigma^2,  ell = sum log sigma^2,
//   kappa = sum log det(C + Qc) + d_c' (C + Qc)^-1 d_c,  n = matches,  low = blobs that weigh log 0.1
//
// A match of a blob that carries a range (pk_proposal_ranges; DESIGN.md section 4, "Ranges in the proposal") gives the 2-vector
// nu = (bearing, range) with the 2 x 2 variance S2 and the 2 x 3 block A, rows s (.) (G' h_x): Lambda += A' S2^-1 A, eta += A' S2^-1 nu,
// c += nu' S2^-1 nu, ell += log det S2, and a fifteenth sum n_rho counts them (the density's constant).
#pragma once
#include "pk_math.hpp"

namespace pk {

constexpr int kProposeSums = 14;       // the members of ProposalSums: what k_propose reduces per particle
constexpr int kProposeSumsRange = 15;  // ... and k_propose_range: n_rho, the matches that carried a range, beside them

// G = d pose / d (s (.) xi) at xi = 0, by columns, from the predicted heading and the control alone.
//   twist (motion_model):    h1 = h^ - w dt / 2, ds = v dt:  (cos h1, sin h1, 0), (-ds sin h1, ds cos h1, 1), (0, 0, 1)
//   odometry (odom_motion_model, which SUBTRACTS its noises): h1 = h^ - rot2, t = trans:
//                            (t sin h1, -t cos h1, -1), (-cos h1, -sin h1, 0), (0, 0, -1)
struct NoiseJacobian {
  double g[3][3];  // g[k] = column k
};
// u = (v, w, dt) or (rot1, trans, rot2)
__device__ __forceinline__ NoiseJacobian noise_jacobian(bool odom, double hhat, double u0, double u1, double u2) {
  NoiseJacobian G;
  double s, c;
  if (odom) {
    sincos(hhat - u2, &s, &c);
    const double t = u1;
    G.g[0][0] = t * s;
    G.g[0][1] = -(t * c);
    G.g[0][2] = -1.0;
    G.g[1][0] = -c;
    G.g[1][1] = -s;
    G.g[1][2] = 0.0;
    G.g[2][0] = 0.0;
    G.g[2][1] = 0.0;
    G.g[2][2] = -1.0;
  } else {
    sincos(hhat - u1 * u2 / 2.0, &s, &c);
    const double ds = u0 * u2;
    G.g[0][0] = c;
    G.g[0][1] = s;
    G.g[0][2] = 0.0;
    G.g[1][0] = -(ds * s);
    G.g[1][1] = ds * c;
    G.g[1][2] = 1.0;
    G.g[2][0] = 0.0;
    G.g[2][1] = 0.0;
    G.g[2][2] = 1.0;
  }
  return G;
}

struct ProposalSums {
  double l00, l01, l02, l11, l12, l22;  // sum a a' / sigma^2
  double e0, e1, e2;                    // sum a nu / sigma^2
  double c, ell, kappa, n, low;
};
__device__ __forceinline__ ProposalSums proposal_zero() { return ProposalSums{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

// One settled match against the landmark's state BEFORE the scan, seen from the predicted pose (sx, sy, sh).
// q = 0 (the landmark under the robot): h_x = 0 and h_m = 0 as ekf_update has them -- the colour term, log sigma^2 and nu^2 / sigma^2 stay.
__device__ __forceinline__ void proposal_match(ProposalSums& S, const Landmark<double>& f, double sx, double sy, double sh,
                                               const BlobT<double>& z, const Noise<double>& qt, const NoiseJacobian& G, double s0,
                                               double s1, double s2) {
  const double dx = f.mx - sx, dy = f.my - sy;
  const double q = dx * dx + dy * dy;
  const double nu = wrap_angle(z.bearing - (pk_atan2(dy, dx) - sh));
  double hx0 = 0.0, hx1 = 0.0, hx2 = 0.0;
  if (q != 0.0) {
    const double iq = 1.0 / q;
    hx0 = dy * iq;
    hx1 = -(dx * iq);
    hx2 = -1.0;
  }
  const double m0 = -hx0, m1 = -hx1;  // h_m
  const double p0 = f.pxx * m0 + f.pxy * m1;
  const double p1 = f.pxy * m0 + f.pyy * m1;
  const double sig2 = m0 * p0 + m1 * p1 + qt.q00;
  const double is2 = 1.0 / sig2;
  const double a0 = s0 * (G.g[0][0] * hx0 + G.g[0][1] * hx1 + G.g[0][2] * hx2);
  const double a1 = s1 * (G.g[1][0] * hx0 + G.g[1][1] * hx1 + G.g[1][2] * hx2);
  const double a2 = s2 * (G.g[2][0] * hx0 + G.g[2][1] * hx1 + G.g[2][2] * hx2);
  const double b0 = a0 * is2, b1 = a1 * is2, b2 = a2 * is2;
  S.l00 += a0 * b0;
  S.l01 += a0 * b1;
  S.l02 += a0 * b2;
  S.l11 += a1 * b1;
  S.l12 += a1 * b2;
  S.l22 += a2 * b2;
  S.e0 += b0 * nu;
  S.e1 += b1 * nu;
  S.e2 += b2 * nu;
  S.c += nu * nu * is2;
  S.ell += log_few_ulp(sig2);
  double detc;
  const Sym3<double> qci =
      sym3_inverse(Sym3<double>{f.crr + qt.rr, f.crg + qt.rg, f.crb + qt.rb, f.cgg + qt.gg, f.cgb + qt.gb, f.cbb + qt.bb}, detc);
  S.kappa += log_few_ulp(detc) + sym3_quad(qci, z.r - f.mr, z.g - f.mg, z.b - f.mb);
  S.n += 1.0;
}

// The same for a blob with the range rho of variance qr: the 2-D measurement (bearing, range) of ekf_update_range.
//   h_x = [[dy / q, -dx / q, -1], [-dx / r, -dy / r, 0]],  h_m = [[-dy / q, dx / q], [dx / r, dy / r]],  r = sqrt(q); all zero at q = 0
//   S2 = h_m Sigma_xy h_m' + diag(q00, qr), inverted in closed form
__device__ __forceinline__ void proposal_match_range(ProposalSums& S, double& nrho, const Landmark<double>& f, double sx, double sy, double sh,
                                                     const BlobT<double>& z, double rho, double qr, const Noise<double>& qt,
                                                     const NoiseJacobian& G, double s0, double s1, double s2) {
  const double dx = f.mx - sx, dy = f.my - sy;
  const double q = dx * dx + dy * dy;
  const double rhat = sqrt(q);
  const double nb = wrap_angle(z.bearing - (pk_atan2(dy, dx) - sh));
  const double nr = rho - rhat;
  double hb0 = 0.0, hb1 = 0.0, hb2 = 0.0, hr0 = 0.0, hr1 = 0.0;  // h_x: the bearing's row, the range's (its third entry is 0)
  if (q != 0.0) {
    const double iq = 1.0 / q, ir = 1.0 / rhat;
    hb0 = dy * iq;
    hb1 = -(dx * iq);
    hb2 = -1.0;
    hr0 = -(dx * ir);
    hr1 = -(dy * ir);
  }
  const double mb0 = -hb0, mb1 = -hb1, mr0 = -hr0, mr1 = -hr1;  // h_m
  const double pb0 = f.pxx * mb0 + f.pxy * mb1, pb1 = f.pxy * mb0 + f.pyy * mb1;
  const double pr0 = f.pxx * mr0 + f.pxy * mr1, pr1 = f.pxy * mr0 + f.pyy * mr1;
  const double s00 = mb0 * pb0 + mb1 * pb1 + qt.q00;
  const double s01 = mb0 * pr0 + mb1 * pr1;
  const double s11 = mr0 * pr0 + mr1 * pr1 + qr;
  const double dets = s00 * s11 - s01 * s01;
  const double idet = 1.0 / dets;
  const double i00 = s11 * idet, i01 = -(s01 * idet), i11 = s00 * idet;  // S2^-1
  // A: the bearing's row ab, the range's row ar
  const double ab0 = s0 * (G.g[0][0] * hb0 + G.g[0][1] * hb1 + G.g[0][2] * hb2);
  const double ab1 = s1 * (G.g[1][0] * hb0 + G.g[1][1] * hb1 + G.g[1][2] * hb2);
  const double ab2 = s2 * (G.g[2][0] * hb0 + G.g[2][1] * hb1 + G.g[2][2] * hb2);
  const double ar0 = s0 * (G.g[0][0] * hr0 + G.g[0][1] * hr1);
  const double ar1 = s1 * (G.g[1][0] * hr0 + G.g[1][1] * hr1);
  const double ar2 = s2 * (G.g[2][0] * hr0 + G.g[2][1] * hr1);
  // S2^-1 A by rows: cb, cr
  const double cb0 = i00 * ab0 + i01 * ar0, cb1 = i00 * ab1 + i01 * ar1, cb2 = i00 * ab2 + i01 * ar2;
  const double cr0 = i01 * ab0 + i11 * ar0, cr1 = i01 * ab1 + i11 * ar1, cr2 = i01 * ab2 + i11 * ar2;
  S.l00 += ab0 * cb0 + ar0 * cr0;
  S.l01 += ab0 * cb1 + ar0 * cr1;
  S.l02 += ab0 * cb2 + ar0 * cr2;
  S.l11 += ab1 * cb1 + ar1 * cr1;
  S.l12 += ab1 * cb2 + ar1 * cr2;
  S.l22 += ab2 * cb2 + ar2 * cr2;
  S.e0 += cb0 * nb + cr0 * nr;
  S.e1 += cb1 * nb + cr1 * nr;
  S.e2 += cb2 * nb + cr2 * nr;
  S.c += (i00 * nb * nb + 2.0 * i01 * nb * nr) + i11 * nr * nr;
  S.ell += log_few_ulp(dets);
  double detc;
  const Sym3<double> qci =
      sym3_inverse(Sym3<double>{f.crr + qt.rr, f.crg + qt.rg, f.crb + qt.rb, f.cgg + qt.gg, f.cgb + qt.gb, f.cbb + qt.bb}, detc);
  S.kappa += log_few_ulp(detc) + sym3_quad(qci, z.r - f.mr, z.g - f.mg, z.b - f.mb);
  S.n += 1.0;
  nrho += 1.0;
}

// The particle's normals xi = m + R^-T z and its weight increment from the reduced sums: Lambda = I + sum = R R' (Cholesky, R lower),
// m = Lambda^-1 eta.  delta = -2 n log 2 pi - (ell + log det Lambda) / 2 - (c - eta' m) / 2 - kappa / 2 + low log 0.1: the Gaussian
// marginal of the stacked innovations (Woodbury, the determinant lemma).  No settled match: xi = z, bit for bit.
// RANGE: every ranged match stacks one more innovation -- the constant is -(2 n + n_rho / 2) log 2 pi.
template <bool RANGE = false>
__device__ __forceinline__ double proposal_finish(const ProposalSums& S, double z0, double z1, double z2, double& x0, double& x1,
                                                  double& x2, double nrho = 0.0) {
  const double low = S.low * Consts<double>::log_no_match;
  if (S.n == 0.0) {
    x0 = z0;
    x1 = z1;
    x2 = z2;
    return low;
  }
  const double r00 = sqrt(1.0 + S.l00);
  const double r10 = S.l01 / r00, r20 = S.l02 / r00;
  const double r11 = sqrt((1.0 + S.l11) - r10 * r10);
  const double r21 = (S.l12 - r20 * r10) / r11;
  const double r22 = sqrt(((1.0 + S.l22) - r20 * r20) - r21 * r21);
  // R y = eta;  R' m = y;  R' t = z
  const double y0 = S.e0 / r00;
  const double y1 = (S.e1 - r10 * y0) / r11;
  const double y2 = ((S.e2 - r20 * y0) - r21 * y1) / r22;
  const double m2 = y2 / r22;
  const double m1 = (y1 - r21 * m2) / r11;
  const double m0 = ((y0 - r10 * m1) - r20 * m2) / r00;
  const double t2 = z2 / r22;
  const double t1 = (z1 - r21 * t2) / r11;
  const double t0 = ((z0 - r10 * t1) - r20 * t2) / r00;
  x0 = m0 + t0;
  x1 = m1 + t1;
  x2 = m2 + t2;
  const double logdet = 2.0 * log_few_ulp(r00 * r11 * r22);
  const double etam = y0 * y0 + y1 * y1 + y2 * y2;  // eta' Lambda^-1 eta
  if constexpr (RANGE)
    return -(2.0 * S.n + 0.5 * nrho) * Consts<double>::log_two_pi - 0.5 * (S.ell + logdet) - 0.5 * (S.c - etam) - 0.5 * S.kappa + low;
  return -2.0 * S.n * Consts<double>::log_two_pi - 0.5 * (S.ell + logdet) - 0.5 * (S.c - etam) - 0.5 * S.kappa + low;
}

}  // namespace pk

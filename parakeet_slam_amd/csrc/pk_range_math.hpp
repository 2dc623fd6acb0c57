// Range-bearing blobs under the bearing model (pk_scan_ranges; DESIGN.md section 4, "Range-bearing scans"): the measurement model
// of a blob that carries a range rho with variance q_rho beside its bearing.  Register-resident __device__ inlines on scalars,
// next to pk_math.hpp, which they build on: the gates, the colour probability, the colour block's update, count_update and the
// potential-feature rule are that header's own functions, called from here.
//
//   position probability   the 2x2 density at the MEASURED POINT m = s + rho u (u: the blob's unit ray turned by the heading), not at
//                          the closest point on the ray, under S = Sigma_xy + q_rho u u' + rho^2 q00 n n', n = (-uy, ux): the
//                          measurement's own covariance is in it, so that association survives a Sigma_xy below the sensor's noise
//   update                 the position part is the 2-D measurement (bearing, range): H = [[-dy / q, dx / q], [dx / r, dy / r]],
//                          r = sqrt(q), both rows (0, 0) at q = 0; S2 = H Sigma_xy H' + diag(q00, q_rho), its inverse in closed form
//   weight                 log w = -5/2 log 2 pi - 1/2 log(det S2 det(C + Qc)) - 1/2 (d' S2^-1 d + the colour term)
//
// A blob without a range (NaN) never comes here: the callers take pk_math.hpp's kModelBearing path for it, blob by blob.
#pragma once
#include "pk_math.hpp"

namespace pk {

// The range and its variance of blob b of a scan's range rows ([B][2]: range, variance; NaN range = none), one 16-byte load.
struct BlobRange {
  double rho, qr;
  __device__ __forceinline__ bool has() const { return rho == rho; }
};
__device__ __forceinline__ BlobRange load_range(const double* rng, int b) {
  const double2 v = *reinterpret_cast<const double2*>(rng + 2 * (size_t)b);
  return BlobRange{v.x, v.y};
}

// S = Sigma_xy + q_rho u u' + rho^2 q00 n n' and e = m - mu for landmark f seen from (sx, sy) along the world-frame ray (ux, uy)
template <typename T>
__device__ __forceinline__ void range_point_parts(const Landmark<T>& f, T sx, T sy, T ux, T uy, T rho, T qr, T q00, T& sxx, T& sxy,
                                                  T& syy, T& ex, T& ey) {
  const T t = rho * rho * q00;
  sxx = f.pxx + qr * ux * ux + t * uy * uy;
  sxy = f.pxy + (qr - t) * ux * uy;
  syy = f.pyy + qr * uy * uy + t * ux * ux;
  ex = (sx + rho * ux) - f.mx;
  ey = (sy + rho * uy) - f.my;
}

// prob_position_match for a ranged blob: the density of the measured point.  meas_xy (probe): the point itself.
template <typename T>
__device__ __forceinline__ T prob_position_match_range(const Landmark<T>& f, T sx, T sy, T ux, T uy, T rho, T qr, T q00,
                                                       T* meas_xy = nullptr) {
  T sxx, sxy, syy, ex, ey;
  range_point_parts(f, sx, sy, ux, uy, rho, qr, q00, sxx, sxy, syy, ex, ey);
  if (meas_xy) {
    meas_xy[0] = sx + rho * ux;
    meas_xy[1] = sy + rho * uy;
  }
  const T det = sxx * syy - sxy * sxy;
  const T maha = (syy * ex * ex - T(2) * sxy * ex * ey + sxx * ey * ey) / det;
  return exp(T(-0.5) * (T(2) * Consts<T>::log_two_pi + log(det) + maha));
}

// The value behind both gates (the association kernels test the gates themselves): 500 bp 500 cp / 250 000 as ever
template <typename T>
__device__ __forceinline__ T match_value_range(const Landmark<T>& f, T sx, T sy, const BlobT<T>& z, T ux, T uy, T rho, T qr, T q00) {
  const T bp = T(500) * prob_position_match_range(f, sx, sy, ux, uy, rho, qr, q00);
  const T cp = T(500) * prob_color_match(f, z.r, z.g, z.b);
  return bp * cp / T(250000);
}

// probability_of_match for a ranged blob: the bearing model's gates (wrapped difference, colour distance), then the value above.
template <typename T>
__device__ __forceinline__ T probability_of_match_range(const Landmark<T>& f, T sx, T sy, T heading, const BlobT<T>& z, T ux, T uy,
                                                        T rho, T qr, T q00) {
  const T pse = pk_atan2(f.my - sy, f.mx - sx);
  const T delb = wrap_angle(z.bearing - (pse - heading));
  if (fabs(delb) > T(0.5)) return T(0);
  if (fabs(color_distance2(f.mr, f.mg, f.mb, z.r, z.g, z.b)) > T(300)) return T(0);
  return match_value_range(f, sx, sy, z, ux, uy, rho, qr, q00);
}

// match_is_positive (pk_device.hpp) for a ranged blob that passed both gates: is its probability > 0?  The same shortcut: far from
// the underflow edge the answer needs no exp / log.
__device__ __forceinline__ bool match_is_positive_range(const Landmark<double>& f, double sx, double sy, const BlobT<double>& z,
                                                        double ux, double uy, double rho, double qr, double q00) {
  double sxx, sxy, syy, ex, ey;
  range_point_parts(f, sx, sy, ux, uy, rho, qr, q00, sxx, sxy, syy, ex, ey);
  const double det2 = sxx * syy - sxy * sxy;
  const double maha2 = (syy * ex * ex - 2.0 * sxy * ex * ey + sxx * ey * ey) / det2;
  double det3;
  const Sym3<double> inv = sym3_inverse(Sym3<double>{f.crr, f.crg, f.crb, f.cgg, f.cgb, f.cbb}, det3);
  const double maha3 = sym3_quad(inv, z.r - f.mr, z.g - f.mg, z.b - f.mb);
  if (det2 > 0.0 && det2 < 1e60 && det3 > 0.0 && det3 < 1e60 && maha2 >= 0.0 && maha3 >= 0.0 && maha2 + maha3 < 800.0) return true;
  const double bp = 500.0 * exp(-0.5 * (2.0 * Consts<double>::log_two_pi + log(det2) + maha2));
  const double cp = 500.0 * exp(-0.5 * (3.0 * Consts<double>::log_two_pi + log(det3) + maha3));
  return bp * cp / 250000.0 > 0.0;
}

// ekf_update<T, true, kModelBearing> for a ranged blob: the 5x5 / 5x5 algebra factors into a 2x2 problem (bearing, range against
// x, y) and the colour block's 3x3 one, which is pk_math.hpp's, line for line.  zhat0_known: pk_atan2(dy, dx) of this very state.
// Returns the log-weight; the state is updated in place unless the landmark is immutable.
template <typename T>
__device__ __forceinline__ T ekf_update_range(Landmark<T>& f, T sx, T sy, T heading, const BlobT<T>& z, T rho, T qr, const Noise<T>& qt,
                                              bool immutable, const T* zhat0_known = nullptr) {
  const T dx = f.mx - sx, dy = f.my - sy;
  const T zhat0 = (zhat0_known ? *zhat0_known : pk_atan2(dy, dx)) - heading;
  const T q = dx * dx + dy * dy;
  const T rhat = sqrt(q);
  T hb0, hb1, hr0, hr1;  // H: the bearing's row, the range's row
  if (q == T(0)) {
    hb0 = hb1 = hr0 = hr1 = T(0);
  } else {
    const T iq = T(1) / q, ir = T(1) / rhat;
    hb0 = -dy * iq;
    hb1 = dx * iq;
    hr0 = dx * ir;
    hr1 = dy * ir;
  }
  // A = Sigma_xy H' (columns: bearing, range)
  const T ab0 = f.pxx * hb0 + f.pxy * hb1, ab1 = f.pxy * hb0 + f.pyy * hb1;
  const T ar0 = f.pxx * hr0 + f.pxy * hr1, ar1 = f.pxy * hr0 + f.pyy * hr1;
  const T s00 = hb0 * ab0 + hb1 * ab1 + qt.q00;
  const T s01 = hb0 * ar0 + hb1 * ar1;
  const T s11 = hr0 * ar0 + hr1 * ar1 + qr;
  const T dets = s00 * s11 - s01 * s01;
  const T idet = T(1) / dets;
  const T i00 = s11 * idet, i01 = -s01 * idet, i11 = s00 * idet;  // S2^-1
  Sym3<T> qc{f.crr + qt.rr, f.crg + qt.rg, f.crb + qt.rb, f.cgg + qt.gg, f.cgb + qt.gb, f.cbb + qt.bb};
  T detc;
  const Sym3<T> qci = sym3_inverse(qc, detc);

  const T d0 = wrap_angle(z.bearing - zhat0);
  const T dr = rho - rhat;
  const T d1 = z.r - f.mr, d2 = z.g - f.mg, d3 = z.b - f.mb;
  const T v0 = qci.a * d1 + qci.b * d2 + qci.c * d3;
  const T v1 = qci.b * d1 + qci.d * d2 + qci.e * d3;
  const T v2 = qci.c * d1 + qci.e * d2 + qci.f * d3;
  const T maha = (i00 * d0 * d0 + T(2) * i01 * d0 * dr + i11 * dr * dr) + (d1 * v0 + d2 * v1 + d3 * v2);
  T logw = T(-2.5) * Consts<T>::log_two_pi - T(0.5) * log_few_ulp(dets * detc) - T(0.5) * maha;
  if (f.count & kPotentialBit) logw = (T)Consts<double>::log_no_match;

  if (!immutable) {
    // K = A S2^-1 (rows x, y; columns bearing, range)
    const T kb0 = ab0 * i00 + ar0 * i01, kr0 = ab0 * i01 + ar0 * i11;
    const T kb1 = ab1 * i00 + ar1 * i01, kr1 = ab1 * i01 + ar1 * i11;
    f.mx += kb0 * d0 + kr0 * dr;
    f.my += kb1 * d0 + kr1 * dr;
    const T nr = f.mr + (f.crr * v0 + f.crg * v1 + f.crb * v2);
    const T ng = f.mg + (f.crg * v0 + f.cgg * v1 + f.cgb * v2);
    const T nb = f.mb + (f.crb * v0 + f.cgb * v1 + f.cbb * v2);
    // Sigma' = Sigma - K A', its off-diagonal the mean of the two it comes to (as ekf_update keeps pxy)
    const T nxx = f.pxx - (kb0 * ab0 + kr0 * ar0);
    const T nxy = f.pxy - T(0.5) * ((kb0 * ab1 + kr0 * ar1) + (kb1 * ab0 + kr1 * ar0));
    const T nyy = f.pyy - (kb1 * ab1 + kr1 * ar1);
    const Sym3<T> nc = colour_block_update(Sym3<T>{f.crr, f.crg, f.crb, f.cgg, f.cgb, f.cbb}, qci, qt);
    f.mr = nr;
    f.mg = ng;
    f.mb = nb;
    f.pxx = nxx;
    f.pxy = nxy;
    f.pyy = nyy;
    f.crr = nc.a;
    f.crg = nc.b;
    f.crb = nc.c;
    f.cgg = nc.d;
    f.cgb = nc.e;
    f.cbb = nc.f;
    count_update(f.count);
  }
  return logw;
}

}  // namespace pk

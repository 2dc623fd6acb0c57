// Register-resident measurement model of the FastSLAM landmark EKF (gfx950).
//
// Everything here is a __device__ inline on scalars: the linear algebra of the
// path is 2x2 (landmark xy) and 3x3 (landmark rgb), far too small for MFMA, so
// it lives in VGPRs and is written out by hand.  Each function cites the lines
// of /root/reference/src/prkt_core_v2.py it stands for, including the quirks a
// textbook EKF would not have.
#pragma once
#include <hip/hip_runtime.h>

namespace pk {

template <typename T>
struct Consts;
template <>
struct Consts<double> {
  static constexpr double two_pi = 6.283185307179586476925286766559;
  static constexpr double half_pi = 1.5707963267948966192313216916398;
  static constexpr double log_two_pi = 1.8378770664093454835606594728112;
  static constexpr double log_no_match = -2.3025850929940456840179914546844;  // log(0.1), :857
};

// One landmark EKF in the compact layout: mean (x, y, r, g, b), the symmetric
// 2x2 position block and the symmetric 3x3 colour block of its covariance, and
// Feature.update_count (prkt_core_v2.py:881-895).
template <typename T>
struct Landmark {
  T mx, my, mr, mg, mb;
  T pxx, pxy, pyy;
  T crr, crg, crb, cgg, cgb, cbb;
  int count;  // update_count | kPotentialBit
};

// A POTENTIAL feature (the reference's negative ids, prkt_core_v2.py:109-118): matched and updated like any landmark, but
// the particle's weight takes the unmatched-blob factor instead of the importance factor, until its update count passes
// 5 and it joins the full feature set (:113-117).  The flag rides in the count word (PK_LANDMARK_POTENTIAL in the header):
// every kernel only ever adds 2 to that word, so it travels through all of them unchanged.
constexpr int kPotentialBit = 0x40000000;
__device__ __forceinline__ void count_update(int& count) {
  count += 2;  // :914 and :930
  if ((count & kPotentialBit) && (count & ~kPotentialBit) > 5) count &= ~kPotentialBit;  // :113-117 promotion
}

// Measurement noise Qt (prkt_core_v2.py:50-53) in the same block structure.
template <typename T>
struct Noise {
  T q00;
  T rr, rg, rb, gg, gb, bb;
  int diag;  // colour block diagonal (rg = rb = gb = 0, the reference's Qt = 0.1 I, :50-53): short forms below
};
template <typename T>
__host__ __device__ inline Noise<T> make_noise(T q00, T rr, T rg, T rb, T gg, T gb, T bb) {
  return Noise<T>{q00, rr, rg, rb, gg, gb, bb, (rg == T(0) && rb == T(0) && gb == T(0)) ? 1 : 0};
}

// One observed blob (matrix.blob_to_matrix, matrix.py:35-39).
template <typename T>
struct BlobT {
  T bearing, r, g, b;
};

// Inverse (6 unique entries) and determinant of a symmetric 3x3.
template <typename T>
struct Sym3 {
  T a, b, c, d, e, f;  // [[a,b,c],[b,d,e],[c,e,f]]
};

// Adjugate (the symmetric cofactor matrix) and determinant of a symmetric 3x3: inverse = adj / det.
template <typename T>
__device__ __forceinline__ Sym3<T> sym3_adjugate(const Sym3<T>& m, T& det) {
  T c00 = m.d * m.f - m.e * m.e;
  T c01 = m.c * m.e - m.b * m.f;
  T c02 = m.b * m.e - m.c * m.d;
  T c11 = m.a * m.f - m.c * m.c;
  T c12 = m.b * m.c - m.a * m.e;
  T c22 = m.a * m.d - m.b * m.b;
  det = m.a * c00 + m.b * c01 + m.c * c02;
  return Sym3<T>{c00, c01, c02, c11, c12, c22};
}

template <typename T>
__device__ __forceinline__ Sym3<T> sym3_inverse(const Sym3<T>& m, T& det) {
  const Sym3<T> c = sym3_adjugate(m, det);
  T inv = T(1) / det;
  return Sym3<T>{c.a * inv, c.b * inv, c.c * inv, c.d * inv, c.e * inv, c.f * inv};
}

template <typename T>
__device__ __forceinline__ T sym3_quad(const Sym3<T>& m, T x, T y, T z) {
  return m.a * x * x + m.d * y * y + m.f * z * z + T(2) * (m.b * x * y + m.c * x * z + m.e * y * z);
}

// Heading after heading_to_quaternion -> quaternion_to_heading (utils.py:8-35):
// wrapped to (-pi, pi].
template <typename T>
__device__ __forceinline__ T wrap_heading(T h) {
  T s, c;
  sincos(h, &s, &c);
  return atan2(s, c);
}

// a * b + K, one rounding, with the CONSTANT K in a scalar register pair (VOP3 v_fma_f64 takes one scalar operand).  Left to
// itself the compiler writes a Horner step `p = p * z + K` as v_fmac_f64 (VOP2: the addend is the destination), which wants
// K in vector registers first: two v_mov_b32 of 32-bit literals and the multiply-add -- three VALU issue slots (twelve
// cycles of a wave64 SIMD) where one does, in kernels whose gates / keys phases are float64-issue-bound.
// The two s_mov_b32 that load K issue on the scalar unit, beside the other wave's vector instructions.  Same value as the
// contracted expression (one fused multiply-add either way).
__device__ __forceinline__ double fma_k(double a, double b, double k) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(PK_NO_SCALAR_FMA)
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(k));
  return r;
#else
  return __builtin_fma(a, b, k);
#endif
}

// atan2 for the EXPECTED BEARING of a landmark (prkt_core_v2.py:408, :473, :871: math.atan2(fy - sy, fx - sx)), within
// 2.3 ulp (measured on the device against mpmath over 1.1e6 points: 2.2974 just above the tan(pi / 8) switch, where
// pi / 4 is added to a small negative atan; tests/test_gpu_math_probe.py asserts 1.5 times that), in ~47 float64
// instructions against the library's ~100 + 40 constant moves (every particle x landmark pays one, in the issue-bound gates phase of the one-pass kernels).  ONE division for both range reductions:
//   t = min(|x|, |y|) / max(|x|, |y|) in [0, 1];  beyond tan(pi / 8):  atan t = pi / 4 + atan((t - 1) / (t + 1)), and
//   (t - 1) / (t + 1) = (mn - mx) / (mn + mx) -- the same quotient with another numerator and denominator --
// so r = num / den lies in [-tan(pi / 8), tan(pi / 8)] and atan r = r + r s Q(s), s = r^2, Q of degree 10 (coefficients:
// scripts/fit_atan_poly.py, polynomial error 9e-18 relative, 0.64 ulp evaluated in float64).  The quotient by v_rcp_f64, two
// Newton steps and one residual correction (< 1 ulp).  Then the octant: pi / 2 - a where |y| > |x|, pi - a where x < 0
// (hi + lo constants), the sign of y.  atan2(0, 0) = 0 like the library's for +0; NaN in gives NaN out (v_max / v_min drop
// NaNs: restored by hand -- the kernels rely on a NaN state failing every comparison).  Infinite arguments are not handled (a
// state is finite or NaN).  EVERY observe kernel takes its expected bearings here, so the routes stay bit-identical to each
// other; the motion model's heading wrap and summary keep the library's atan2 (O(P) work, utils.py:8-35).
__device__ __forceinline__ double pk_atan2(double y, double x) {
#if defined(PK_LIBM_ATAN2)  // diagnostic build: the library's
  return atan2(y, x);
#else
  const double ax = fabs(x), ay = fabs(y);
  const double mx = fmax(ax, ay), mn = fmin(ax, ay);
  const bool upper = mn > 0.41421356237309503 * mx;  // tan(pi / 8)
  const double num = upper ? mn - mx : mn;
  double den = upper ? mn + mx : mx;
  den = mx == 0.0 ? 1.0 : den;  // atan2(0, 0) = 0
  double rc = __builtin_amdgcn_rcp(den);
  rc = __builtin_fma(__builtin_fma(-den, rc, 1.0), rc, rc);
  rc = __builtin_fma(__builtin_fma(-den, rc, 1.0), rc, rc);
  double r = num * rc;
  r = __builtin_fma(__builtin_fma(-den, r, num), rc, r);
  const double s = r * r;
  double q = -0x1.3a25edd998780p-6;
  q = fma_k(q, s, 0x1.415d4935ee1ffp-5);
  q = fma_k(q, s, -0x1.a09769c825878p-5);
  q = fma_k(q, s, 0x1.dfe5c951ef847p-5);
  q = fma_k(q, s, -0x1.10fa6e9b77db9p-4);
  q = fma_k(q, s, 0x1.3b126231f5ee5p-4);
  q = fma_k(q, s, -0x1.745d0b1c2ae99p-4);
  q = fma_k(q, s, 0x1.c71c7184c78c8p-4);
  q = fma_k(q, s, -0x1.2492492434d72p-3);
  q = fma_k(q, s, 0x1.9999999999310p-3);
  q = fma_k(q, s, -0x1.5555555555555p-2);
  double a = __builtin_fma(r * s, q, r);  // atan r
  a = upper ? 0x1.921fb54442d18p-1 + (a + 0x1.1a62633145c07p-55) : a;        // + pi / 4
  a = ay > ax ? (0x1.921fb54442d18p+0 - a) + 0x1.1a62633145c07p-54 : a;      // pi / 2 - a
  a = x < 0.0 ? (0x1.921fb54442d18p+1 - a) + 0x1.1a62633145c07p-53 : a;      // pi - a
  a += 0.0 * (x + y);  // NaN in, NaN out
  return __builtin_copysign(a, y);
#endif
}

// The measurement model a filter runs (pk_set_measurement_model; DESIGN.md section 4, "The bearing model").  kModelReference is the
// reference's, quirks and all, and what every function below computes unless told otherwise; kModelBearing is the textbook
// robot-frame bearing: the gate and the innovation take the WRAPPED difference to atan2(dy, dx) - heading, the blob's ray is turned
// into the world frame before the closest point is taken, the Jacobian is (-dy / q, dx / q) and the weight is the Gaussian density
// with det Q.  The model is a template parameter resolved with `if constexpr`: the reference model's code is what it was.
constexpr int kModelReference = 0;
constexpr int kModelBearing = 1;

// a - 2 pi rint(a / 2 pi), each operation rounded by itself (no contraction: the host reference forms it the same way).  Returns a
// unchanged, exactly, whenever |a| < pi (rint gives 0).
__device__ __forceinline__ double wrap_angle(double a) {
  const double k = rint(a / Consts<double>::two_pi);
  return __dsub_rn(a, __dmul_rn(Consts<double>::two_pi, k));
}

// The blob's robot-frame unit ray (ux, uy) turned by the heading (ch, sh) = (cos h, sin h): the ray's direction in the world frame.
__device__ __forceinline__ void rotate_ray(double ux, double uy, double ch, double sh, double& wx, double& wy) {
  wx = ux * ch - uy * sh;
  wy = ux * sh + uy * ch;
}

// closest_point, prkt_core_v2.py:496-522.  (ux, uy) = unit((cos b, sin b, 0)),
// utils.py:68-76, precomputed per blob.
// MODEL = kModelBearing: (ux, uy) is the ray in the world frame and the behind-the-ray branch is gone (behind the bearing gate the
// ray and the landmark are at most 0.5 rad apart).
template <typename T, int MODEL = kModelReference>
__device__ __forceinline__ void closest_point(T fx, T fy, T sx, T sy, T ux, T uy, T& nx, T& ny) {
  T ox = fx - sx, oy = fy - sy;
  T mag = ox * ux + oy * uy;  // dot_product, utils.py:37-43
  if constexpr (MODEL == kModelBearing) {
    nx = sx + ux * mag;
    ny = sy + uy * mag;
  } else if (mag < T(0)) {    // :515-516 behind the ray: the robot position itself
    nx = sx;
    ny = sy;
  } else {
    nx = sx + ux * mag;
    ny = sy + uy * mag;
  }
}

// prob_position_match, prkt_core_v2.py:457-494 (scipy multivariate_normal.pdf, k = 2,
// in closed form).  pse = atan2(fy - sy, fx - sx).  MODEL = kModelBearing: (ux, uy) in the world frame, no half-plane test.
template <typename T, int MODEL = kModelReference>
__device__ __forceinline__ T prob_position_match(const Landmark<T>& f, T sx, T sy, T pse, T bearing,
                                                 T ux, T uy, T* near_xy = nullptr) {
  T nx, ny;
  closest_point<T, MODEL>(f.mx, f.my, sx, sy, ux, uy, nx, ny);
  if (near_xy) {
    near_xy[0] = nx;
    near_xy[1] = ny;
  }
  if constexpr (MODEL == kModelReference)
    if (fabs(pse - bearing) > Consts<T>::half_pi) return T(0);  // :473-475, frames mixed as in the reference
  T ex = nx - f.mx, ey = ny - f.my;
  T det = f.pxx * f.pyy - f.pxy * f.pxy;
  T maha = (f.pyy * ex * ex - T(2) * f.pxy * ex * ey + f.pxx * ey * ey) / det;
  return exp(T(-0.5) * (T(2) * Consts<T>::log_two_pi + log(det) + maha));
}

// prob_color_match, prkt_core_v2.py:524-544 (scipy pdf, k = 3).
template <typename T>
__device__ __forceinline__ T prob_color_match(const Landmark<T>& f, T r, T g, T b) {
  T det;
  Sym3<T> inv = sym3_inverse(Sym3<T>{f.crr, f.crg, f.crb, f.cgg, f.cgb, f.cbb}, det);
  T maha = sym3_quad(inv, r - f.mr, g - f.mg, b - f.mb);
  return exp(T(-0.5) * (T(3) * Consts<T>::log_two_pi + log(det) + maha));
}

// The two gates of probability_of_match (prkt_core_v2.py:433, :441) need only the mean.
template <typename T>
__device__ __forceinline__ T color_distance2(T mr, T mg, T mb, T r, T g, T b) {
  T dr = r - mr, dg = g - mg, db = b - mb;
  return dr * dr + dg * dg + db * db;  // :425-427
}

// probability_of_match, prkt_core_v2.py:383-455.  MODEL = kModelBearing: the difference is wrapped, (ux, uy) is the world-frame ray.
template <typename T, int MODEL = kModelReference>
__device__ __forceinline__ T probability_of_match(const Landmark<T>& f, T sx, T sy, T heading,
                                                  const BlobT<T>& z, T ux, T uy) {
  T pse = pk_atan2(f.my - sy, f.mx - sx);
  T delb = z.bearing - (pse - heading);  // :408-415, never wrapped (:416-423 commented out)
  if constexpr (MODEL == kModelBearing) delb = wrap_angle(delb);
  if (fabs(delb) > T(0.5)) return T(0);  // :433
  T cd = color_distance2(f.mr, f.mg, f.mb, z.r, z.g, z.b);
  if (fabs(cd) > T(300)) return T(0);  // :441
  T bp = T(500) * prob_position_match<T, MODEL>(f, sx, sy, pse, z.bearing, ux, uy);  // :439
  T cp = T(500) * prob_color_match(f, z.r, z.g, z.b);                     // :446
  return bp * cp / T(250000);                                            // :455
}

// Natural logarithm accurate to 2 ulp (checked on the host against logl over 2e7 arguments from
// 1e-304 to 1e304 and around 1; on the device, with fma_k's inline v_fma_f64, against mpmath / longdouble over 7.7e5
// arguments that aim at 1, at the mantissa switch and at the powers of two: worst 1.9956,
// tests/test_gpu_math_probe.py): log(x) = e ln 2 + 2 atanh(s), s = (m - 1) / (m + 1), with x = m 2^e
// and m in [sqrt(1/2), sqrt(2)) so that s^2 <= 0.0295 and eleven terms of the atanh series leave
// < 1e-18.  About 45 float64 instructions against ~95 for the library log.  Used for the importance
// factor (:844-849) and for the probabilities of contested pairs (:439, :446) -- quantities whose
// tolerance is 1e-5 relative (north star) and which the parity tests hold to 1e-9; a tie between
// identical landmarks stays a tie (same function, same inputs).  Anything that is not a positive
// normal number takes the library path.
__device__ __forceinline__ double log_few_ulp(double x) {
  if (!(x > 2.3e-308 && x < 1.7e308)) return log(x);
  int e = 0;
  double m = frexp(x, &e);  // m in [0.5, 1)
  if (m < 0.70710678118654752440) {
    m *= 2.0;
    e -= 1;
  }
  const double s = (m - 1.0) / (m + 1.0);
  const double z = s * s;
  double p = 1.0 / 21.0;
  p = fma_k(p, z, 1.0 / 19.0);
  p = fma_k(p, z, 1.0 / 17.0);
  p = fma_k(p, z, 1.0 / 15.0);
  p = fma_k(p, z, 1.0 / 13.0);
  p = fma_k(p, z, 1.0 / 11.0);
  p = fma_k(p, z, 1.0 / 9.0);
  p = fma_k(p, z, 1.0 / 7.0);
  p = fma_k(p, z, 1.0 / 5.0);
  p = fma_k(p, z, 1.0 / 3.0);
  const double lm = 2.0 * s + 2.0 * s * (z * p);  // 2 atanh(s)
  const double ed = (double)e;
  return ed * 0.69314718055994528623 + (ed * 2.3190468138462995584e-17 + lm);  // ln 2 = hi + lo
}

// probability_of_match (:439-455) from the determinants and the Mahalanobis terms' numerators
// (maha = num / det: e' adj(P) e and d' adj(C) d -- the divisions are made here, for the few pairs
// whose probability VALUE is needed, not in the code every lane runs)
__device__ __forceinline__ double pr_from_parts(double det2, double det3, double num2, double num3) {
  const double maha2 = num2 / det2, maha3 = num3 / det3;
  const double bp = 500.0 * exp(-0.5 * (2.0 * Consts<double>::log_two_pi + log_few_ulp(det2) + maha2));  // :439
  const double cp = 500.0 * exp(-0.5 * (3.0 * Consts<double>::log_two_pi + log_few_ulp(det3) + maha3));  // :446
  return bp * cp / 250000.0;                                                                              // :455
}

// Intermediate quantities of one EKF update, for the probe entry point.
template <typename T>
struct EkfAux {
  T zhat0, h0, h1;
  T q00;
  Sym3<T> qc;     // Q[1:,1:]
  T k0, k1;       // K[0:2, 0]
  T kc[9];        // K[2:5, 1:4] row-major
};

// One blob applied to one landmark: generate_measurement :859-877,
// measurement_jacobian :748-802, measurement_covariance :804-819, inverse matrix.py:11,
// kalman_gain :821-833, Feature.update_mean :897-914, Feature.update_covar :916-930,
// importance_factor :835-849.  Returns log(importance factor); the state is updated in
// place unless the landmark is immutable (:909, :926).
//
// With Sigma = Pxy (+) C and Qt = q00 (+) Qc the 4x4 / 5x4 algebra of the reference
// factors exactly into a scalar and a 3x3 problem:
//   Q   = [h' Pxy h + q00] (+) [C + Qc]
//   K   = [Pxy h / Q00]    (+) [C (C + Qc)^-1]
//   Sigma' = [Pxy - (Pxy h)(Pxy h)'/Q00] (+) [C - C (C + Qc)^-1 C]
// With a diagonal Qc the colour block is written C' = Qc (C + Qc)^-1 C (the same matrix:
// I - C (C + Qc)^-1 = Qc (C + Qc)^-1), six products instead of eighteen and without the
// subtraction; the Mahalanobis term is d'v with v = (C + Qc)^-1 d in both forms.
//
// DOMAIN.  Held to an exact dense reference (mpmath; tests/test_gpu_ekf_reference.py through PK_MATH_EKF_UPDATE, figures in
// profiles/r10/ekf_errors.json), every output stays within (32 + kappa^2 / 8) 2^-53 of the sum of the absolute values of its
// terms, kappa = cond_2(C + Qc): 1e-10 of its terms while kappa <~ 2.7e3.  (C + Qc)^-1 is adjugate / determinant, which loses
// kappa^2 in the colour mean and the weight where the reference's LAPACK inverse loses kappa: at kappa up to 1e3 the worst
// measured is 9.9e3 units (log weight; the float64 reference 1.5e2), at kappa up to 1e5 2.5e7 units (colour mean, 2.8e-9 of its
// terms; the reference 6.8e3).  A colour block whose brightness variance is far above its chroma variance on a landmark's first
// update is such a block.  Elsewhere (ranges 1e-6 .. 1e4, P 1e-16 .. 1e12, C 1e-6 .. 1e6, q == 0, a full Qc) the worst is 14 units.
//
// The colour block's step depends on C and Qt alone -- not on the pose, not on the blob: colour_block_update, one function for
// every caller (ekf_update; the colour table of pk_k_colour.hip), so that -ffp-contract=on rounds it the same way everywhere.
// qci = (C + Qc)^-1 as sym3_inverse gives it.
template <typename T>
__device__ __forceinline__ Sym3<T> colour_block_update(const Sym3<T>& C, const Sym3<T>& qci, const Noise<T>& qt) {
  const T crr = C.a, crg = C.b, crb = C.c, cgg = C.d, cgb = C.e, cbb = C.f;
  T nrr, nrg, nrb, ngg, ngb, nbb;
  // M = Qci C (rows r, g, b)
  T m00 = qci.a * crr + qci.b * crg + qci.c * crb;
  T m01 = qci.a * crg + qci.b * cgg + qci.c * cgb;
  T m02 = qci.a * crb + qci.b * cgb + qci.c * cbb;
  T m11 = qci.b * crg + qci.d * cgg + qci.e * cgb;
  T m12 = qci.b * crb + qci.d * cgb + qci.e * cbb;
  T m22 = qci.c * crb + qci.e * cgb + qci.f * cbb;
  if (qt.diag) {  // uniform.  C' = Qc M: the upper triangle of M is all it takes
    nrr = qt.rr * m00;
    nrg = qt.rr * m01;
    nrb = qt.rr * m02;
    ngg = qt.gg * m11;
    ngb = qt.gg * m12;
    nbb = qt.bb * m22;
  } else {  // C' = C - C M (symmetric)
    T m10 = qci.b * crr + qci.d * crg + qci.e * crb;
    T m20 = qci.c * crr + qci.e * crg + qci.f * crb;
    T m21 = qci.c * crg + qci.e * cgg + qci.f * cgb;
    nrr = crr - (crr * m00 + crg * m10 + crb * m20);
    nrg = crg - (crr * m01 + crg * m11 + crb * m21);
    nrb = crb - (crr * m02 + crg * m12 + crb * m22);
    ngg = cgg - (crg * m01 + cgg * m11 + cgb * m21);
    ngb = cgb - (crg * m02 + cgg * m12 + cgb * m22);
    nbb = cbb - (crb * m02 + cgb * m12 + cbb * m22);
  }
  return Sym3<T>{nrr, nrg, nrb, ngg, ngb, nbb};
}
// ... from C and Qt: one level of the colour table (the sum and the inverse as ekf_update forms them)
template <typename T>
__device__ __forceinline__ Sym3<T> colour_block_step(const Sym3<T>& C, const Noise<T>& qt) {
  Sym3<T> qc{C.a + qt.rr, C.b + qt.rg, C.c + qt.rb, C.d + qt.gg, C.e + qt.gb, C.f + qt.bb};
  T detc;
  Sym3<T> qci = sym3_inverse(qc, detc);
  return colour_block_update(C, qci, qt);
}
// COLOUR = false (k_step_pub in table mode, a landmark's only update of the scan): the colour block is left as it was -- the caller
// neither stores it nor reads it again; everything else as ever.
// MODEL = kModelBearing (no fro_prod): zhat0 = atan2(dy, dx) - heading (zhat0_known still holds the atan2), the innovation is
// wrapped, H's first row is (-dy / q, dx / q), and the weight is the density: -2 log 2 pi - 1/2 log(Q00 det(C + Qc)) - 1/2 d' Q^-1 d.
template <typename T, bool COLOUR = true, int MODEL = kModelReference>
__device__ __forceinline__ T ekf_update(Landmark<T>& f, T sx, T sy, const BlobT<T>& z,
                                        const Noise<T>& qt, bool immutable,
                                        EkfAux<T>* aux = nullptr, const T* zhat0_known = nullptr, T* fro_prod = nullptr,
                                        T heading = T(0)) {
  T dx = f.mx - sx, dy = f.my - sy;
  // :871 world frame: the heading is NOT subtracted here.  A caller that already holds
  // atan2(dy, dx) for this very state passes it in (one float64 atan2 saved).
  T zhat0 = zhat0_known ? *zhat0_known : pk_atan2(dy, dx);
  if constexpr (MODEL == kModelBearing) zhat0 = zhat0 - heading;
  T q = dx * dx + dy * dy;  // :785
  T h0, h1;                 // :789/:795 -- (dy/q, dx/q): the reference's signs, not the textbook's
  if (q == T(0)) {          // ZeroDivisionError branch :790,:796
    h0 = T(0);
    h1 = T(0);
  } else {
    T iq = T(1) / q;
    h0 = dy * iq;
    h1 = dx * iq;
    if constexpr (MODEL == kModelBearing) h0 = -h0;
  }
  T a0 = f.pxx * h0 + f.pxy * h1;  // Pxy h
  T a1 = f.pxy * h0 + f.pyy * h1;
  T q00 = h0 * a0 + h1 * a1 + qt.q00;  // :817-818
  Sym3<T> qc{f.crr + qt.rr, f.crg + qt.rg, f.crb + qt.rb, f.cgg + qt.gg, f.cgb + qt.gb, f.cbb + qt.bb};
  T detc;
  Sym3<T> qci = sym3_inverse(qc, detc);  // matrix.py:11-12 on the 3x3 block
  T iq00 = T(1) / q00;

  T d0 = z.bearing - zhat0;  // :846/:911 innovation, not wrapped
  if constexpr (MODEL == kModelBearing) d0 = wrap_angle(d0);
  T d1 = z.r - f.mr, d2 = z.g - f.mg, d3 = z.b - f.mb;

  // importance_factor :844-849: (2 pi ||Q||_F)^-1/2 exp(-1/2 d' Q^-1 d) with the
  // Frobenius norm of Q (matrix.py:31-33), not its determinant.
  T fro2 = q00 * q00 + qc.a * qc.a + qc.d * qc.d + qc.f * qc.f +
           T(2) * (qc.b * qc.b + qc.c * qc.c + qc.e * qc.e);
  // v = (C + Qc)^-1 d_c ;  M = (C + Qc)^-1 C  (3x3, rows r,g,b)
  T v0 = qci.a * d1 + qci.b * d2 + qci.c * d3;
  T v1 = qci.b * d1 + qci.d * d2 + qci.e * d3;
  T v2 = qci.c * d1 + qci.e * d2 + qci.f * d3;
  T maha = d0 * d0 * iq00 + (d1 * v0 + d2 * v1 + d3 * v2);
  // fro_prod (the one-pass kernels): the caller takes ONE logarithm, of the product of the norms of all the updates of its lane,
  // -1/4 log(prod) -- the logarithm is 45 of an update's 300 instructions; here the factor is multiplied in and the term left out
  T logw;
  if constexpr (MODEL == kModelBearing) {
    logw = T(-2) * Consts<T>::log_two_pi - T(0.5) * log_few_ulp(q00 * detc) - T(0.5) * maha;
    if (f.count & kPotentialBit) logw = (T)Consts<double>::log_no_match;
  } else if (fro_prod) {
    logw = T(-0.5) * Consts<T>::log_two_pi - T(0.5) * maha;
    // The product is looked at after EVERY multiplication and is a positive normal number behind each: the caller takes its
    // logarithm once, behind the lane's last update, and Qt is any finite matrix (1e20 I to make the filter ignore colour:
    // fro2 = 3e40, the eight factors of a landmark pair 6.6e323; 1e-20 I: 1.6e-39, eight of them below the subnormals).  Where
    // the product has left the normal numbers (infinite, zero or subnormal: one v_cmp_class and a branch out of line, hardly ever
    // taken; the cost: DESIGN.md section 4) both its factors are split, x = m 2^e with m in [1/2, 1): the exponents go into the
    // log-weight here, e ln 2 / 4 (one rounding, of a part of the terms -1/4 log(fro2) it stands for), and the product of the
    // two m, in [1/4, 1), is the new product -- so it never is anything but a positive normal number, for any number of factors
    // of any size.  An infinite, NaN or zero fro2 has m = fro2 (v_frexp_mant): the product becomes what it is, and the caller's
    // logarithm gives what a logarithm per update gives, -inf, NaN, +inf.  (float64 only: a float product's subnormals would
    // pass the test.)
    static_assert(sizeof(T) == 8, "fro_prod: the test of the product is one of a double");
    const bool potential = (f.count & kPotentialBit) != 0;
    const T old = *fro_prod;
    const T raw = old * fro2;
    T p = potential ? old : raw;
    if (potential) logw = (T)Consts<double>::log_no_match;  // :111-112 "update as if the feature not seen"
    constexpr int kNotPositiveNormal = 0x3FF & ~0x100;     // (v_cmp_class: every class but +normal)
    if (__builtin_expect(!potential && __builtin_amdgcn_class((double)raw, kNotPositiveNormal), 0)) {
      const int e = __builtin_amdgcn_frexp_exp((double)old) + __builtin_amdgcn_frexp_exp((double)fro2);
      p = (T)(__builtin_amdgcn_frexp_mant((double)old) * __builtin_amdgcn_frexp_mant((double)fro2));
      logw -= T(0.25 * 0.69314718055994530941723212145818) * T(e);
    }
    *fro_prod = p;
  } else {
    logw = T(-0.5) * (Consts<T>::log_two_pi + T(0.5) * log_few_ulp(fro2)) - T(0.5) * maha;
    if (f.count & kPotentialBit) logw = (T)Consts<double>::log_no_match;  // :111-112 "update as if the feature not seen"
  }
  T k0 = a0 * iq00, k1 = a1 * iq00;

  if (aux) {
    aux->zhat0 = zhat0;
    aux->h0 = h0;
    aux->h1 = h1;
    aux->q00 = q00;
    aux->qc = qc;
    aux->k0 = k0;
    aux->k1 = k1;
    // Kc = C Qci
    const T C[3][3] = {{f.crr, f.crg, f.crb}, {f.crg, f.cgg, f.cgb}, {f.crb, f.cgb, f.cbb}};
    const T I[3][3] = {{qci.a, qci.b, qci.c}, {qci.b, qci.d, qci.e}, {qci.c, qci.e, qci.f}};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) aux->kc[i * 3 + j] = C[i][0] * I[0][j] + C[i][1] * I[1][j] + C[i][2] * I[2][j];
  }

  if (!immutable) {
    // update_mean :912-913: mu += K d
    f.mx += k0 * d0;
    f.my += k1 * d0;
    T nr = f.mr + (f.crr * v0 + f.crg * v1 + f.crb * v2);
    T ng = f.mg + (f.crg * v0 + f.cgg * v1 + f.cgb * v2);
    T nb = f.mb + (f.crb * v0 + f.cgb * v1 + f.cbb * v2);
    // update_covar :928-929: Sigma' = (I - K H) Sigma
    T nxx = f.pxx - k0 * a0;
    T nxy = f.pxy - T(0.5) * (k0 * a1 + k1 * a0);
    T nyy = f.pyy - k1 * a1;
    Sym3<T> nc{f.crr, f.crg, f.crb, f.cgg, f.cgb, f.cbb};
    if constexpr (COLOUR) nc = colour_block_update(nc, qci, qt);
    f.mr = nr;
    f.mg = ng;
    f.mb = nb;
    f.pxx = nxx;
    f.pxy = nxy;
    f.pyy = nyy;
    if constexpr (COLOUR) {
      f.crr = nc.a;
      f.crg = nc.b;
      f.crb = nc.c;
      f.cgg = nc.d;
      f.cgb = nc.e;
      f.cbb = nc.f;
    }
    count_update(f.count);
  }
  return logw;
}

// motion_model, prkt_core_v2.py:168-208, on one pose.  n0..n2 are the three draws
// normal(0, sigma, 1) already scaled (:185, :190, :193).
template <typename T>
__device__ __forceinline__ void motion_model(T& x, T& y, T& h, T v, T w, T dt, T n0, T n1, T n2) {
  T dheading = w * dt;         // :183
  T ds = v * dt + n0;          // :186
  T h1 = h + dheading / T(2) + n1;   // :191
  T h2 = h1 + dheading / T(2) + n2;  // :194
  T s, c;
  sincos(h1, &s, &c);
  x += ds * c;  // :198,:203
  y += ds * s;  // :199,:204
  h = wrap_heading(h2);  // :206 quaternion round trip
}

// The odometry motion model (Thrun, Burgard, Fox, Probabilistic Robotics, Table 5.6) on one pose: rotate by rot1, translate by
// trans along the new heading, rotate by rot2.  n0..n2 are the three draws already scaled by the sigmas of the delta
// (sigma_rot1 z0, sigma_trans z1, sigma_rot2 z2; the sigmas are the same for every particle and formed on the host), and are
// SUBTRACTED, as the table samples them.  Ends, as motion_model does, with the heading wrapped to (-pi, pi].
template <typename T>
__device__ __forceinline__ void odom_motion_model(T& x, T& y, T& h, T rot1, T trans, T rot2, T n0, T n1, T n2) {
  T r1 = rot1 - n0;
  T t = trans - n1;
  T r2 = rot2 - n2;
  T h1 = h + r1;
  T s, c;
  sincos(h1, &s, &c);
  x += t * c;
  y += t * s;
  h = wrap_heading(h1 + r2);
}

}  // namespace pk

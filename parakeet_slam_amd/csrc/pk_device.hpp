// Device-side helpers shared by the kernel translation units (gfx950, wave64).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstring>
#include <type_traits>

#include "pk_kernels.hpp"
#include "pk_math.hpp"

namespace pk {

constexpr int kWave = 64;
constexpr int kObsThreads = 256;
constexpr int kRedBlocks = 1024;

// Workgroup barrier that orders LDS traffic only: global loads that are still in flight stay in
// flight (__syncthreads() carries a workgroup-scope fence and waits for them, vmcnt(0)).  Only for
// phases that exchange data through LDS alone.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Diagnostic build only (-DPK_STAMPS, never shipped): shader-clock stamps for per-phase cycle sums.
#ifdef PK_STAMPS
#define PK_STAMP(var) \
  unsigned long long var; \
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");
#else
#define PK_STAMP(var)
#endif

// ------------------------------------------------------------------ reductions
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;  // identical in every lane; butterfly order is fixed => deterministic
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
  return v;
}

// Sum over a workgroup of NW waves; result valid in every thread.  Fixed order.
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* lds /* >= NW doubles */) {
  v = wave_sum(v);
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  __syncthreads();
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  double t = lds[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) t += lds[i];
  return t;
}
// The same sum with barriers that order LDS only: the workgroup's stores stay in flight (a
// __syncthreads() waits for vmcnt(0), i.e. until every store of the wave has been acknowledged).
template <int NW>
__device__ __forceinline__ double block_sum_lds_only(double v, double* lds /* >= NW doubles, not in use */, int tid) {
  v = wave_sum(v);
  const int wave = tid / kWave, lane = tid % kWave;
  if (lane == 0) lds[wave] = v;
  lds_barrier();
  double t = lds[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) t += lds[i];
  return t;
}
template <int NW>
__device__ __forceinline__ double block_max(double v, double* lds) {
  v = wave_max(v);
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  __syncthreads();
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  double t = lds[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) t = fmax(t, lds[i]);
  return t;
}

// Order-preserving map double -> uint64 (max of keys == max of doubles), for the running max
// of the log-weights that the observe kernels keep with one atomicMax per particle.
__host__ __device__ inline unsigned long long double_to_key(double x) {
  unsigned long long b;
  memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double key_to_double(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  memcpy(&x, &b, 8);
  return x;
}

// ------------------------------------------------------------------ systematic resampling
// Ancestor of output slot `slot`: first particle j whose inclusive cumulative weight C_j is
// >= u*r + slot*r, r = sum/P  (equivalent to the walk at prkt_core_v2.py:233-250, '<=' at :239).
// C_j = offsets[block of j] + clocal[j]; every operation is a named rounding, so each kernel that
// calls this (k_ancestors, k_ancestors_gated) picks the same ancestor from the same scan.
__device__ __forceinline__ int64_t comb_ancestor(const double* __restrict__ clocal, const double* __restrict__ totals,
                                                 const double* offsets, double sum, int64_t nb, int64_t Pg, int64_t Pscan,
                                                 double u, int64_t slot) {
  const double r = __ddiv_rn(sum, (double)Pg);                                  // range_ :225
  const double t = __dadd_rn(__dmul_rn(u, r), __dmul_rn((double)slot, r));  // step :226 + k*range_
  // block: first b with offsets[b] + totals[b] >= t
  int64_t lo = 0, hi = nb - 1;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (__dadd_rn(offsets[mid], totals[mid]) >= t)
      hi = mid;
    else
      lo = mid + 1;
  }
  const int64_t b = lo;
  const double off = offsets[b];
  int64_t j0 = b * kScanBlock, j1 = j0 + kScanBlock - 1;
  if (j1 > Pscan - 1) j1 = Pscan - 1;
  while (j0 < j1) {
    int64_t mid = (j0 + j1) >> 1;
    if (__dadd_rn(off, clocal[mid]) >= t)
      j1 = mid;
    else
      j0 = mid + 1;
  }
  return j0;
}

// ------------------------------------------------------------------ weighted moments
// Weighted position moments about a reference pose, kept as (n, mean, centred second moments) and merged pairwise (Chan et
// al.): every term of a merge is a square or a product of the same sign as the result, so nothing cancels however far the
// reference lies from the mean -- the shifted raw moments sum c d d - (sum c d)^2 / n lose a factor n once the reference
// sits where few others do.  Elements that all sit ON the reference merge zeros: the sums stay exactly zero.
struct PathMoments {
  double n, mx, my, xx, xy, yy;
};
__device__ __forceinline__ PathMoments path_merge(const PathMoments& a, const PathMoments& b) {
  const double n = a.n + b.n;
  if (!(b.n > 0.0)) return a;
  if (!(a.n > 0.0)) return b;
  const double f = b.n / n, g = a.n * f;
  const double dx = b.mx - a.mx, dy = b.my - a.my;
  PathMoments m;
  m.n = n;
  m.mx = a.mx + dx * f;
  m.my = a.my + dy * f;
  m.xx = a.xx + b.xx + dx * dx * g;
  m.xy = a.xy + b.xy + dx * dy * g;
  m.yy = a.yy + b.yy + dy * dy * g;
  return m;
}
__device__ __forceinline__ PathMoments path_shfl_down(const PathMoments& m, int off) {
  PathMoments o;
  o.n = __shfl_down(m.n, off, kWave);
  o.mx = __shfl_down(m.mx, off, kWave);
  o.my = __shfl_down(m.my, off, kWave);
  o.xx = __shfl_down(m.xx, off, kWave);
  o.xy = __shfl_down(m.xy, off, kWave);
  o.yy = __shfl_down(m.yy, off, kWave);
  return o;
}

// ------------------------------------------------------------------ landmark slot access
__device__ __forceinline__ Landmark<double> load_landmark(const double* f, const int* cnt, int Lp, int l) {
  Landmark<double> m;
  m.mx = f[F_MX * Lp + l];
  m.my = f[F_MY * Lp + l];
  m.mr = f[F_MR * Lp + l];
  m.mg = f[F_MG * Lp + l];
  m.mb = f[F_MB * Lp + l];
  m.pxx = f[F_PXX * Lp + l];
  m.pxy = f[F_PXY * Lp + l];
  m.pyy = f[F_PYY * Lp + l];
  m.crr = f[F_CRR * Lp + l];
  m.crg = f[F_CRG * Lp + l];
  m.crb = f[F_CRB * Lp + l];
  m.cgg = f[F_CGG * Lp + l];
  m.cgb = f[F_CGB * Lp + l];
  m.cbb = f[F_CBB * Lp + l];
  m.count = cnt[l];
  return m;
}

// The same with the five mean rows requested FIRST (vmcnt retires in order: a kernel whose first phase
// needs only the means then waits for five loads, not for wherever the scheduler put them).
__device__ __forceinline__ Landmark<double> load_landmark_means_first(const double* f, const int* cnt, int Lp, int l) {
  Landmark<double> m;
  m.mx = f[F_MX * Lp + l];
  m.my = f[F_MY * Lp + l];
  m.mr = f[F_MR * Lp + l];
  m.mg = f[F_MG * Lp + l];
  m.mb = f[F_MB * Lp + l];
  asm volatile("" ::: "memory");
  m.pxx = f[F_PXX * Lp + l];
  m.pxy = f[F_PXY * Lp + l];
  m.pyy = f[F_PYY * Lp + l];
  m.crr = f[F_CRR * Lp + l];
  m.crg = f[F_CRG * Lp + l];
  m.crb = f[F_CRB * Lp + l];
  m.cgg = f[F_CGG * Lp + l];
  m.cgb = f[F_CGB * Lp + l];
  m.cbb = f[F_CBB * Lp + l];
  m.count = cnt[l];
  return m;
}

__device__ __forceinline__ Landmark<double> load_landmark_nocount(const double* f, int Lp, int l) {
  Landmark<double> m;
  m.mx = f[F_MX * Lp + l];
  m.my = f[F_MY * Lp + l];
  m.mr = f[F_MR * Lp + l];
  m.mg = f[F_MG * Lp + l];
  m.mb = f[F_MB * Lp + l];
  m.pxx = f[F_PXX * Lp + l];
  m.pxy = f[F_PXY * Lp + l];
  m.pyy = f[F_PYY * Lp + l];
  m.crr = f[F_CRR * Lp + l];
  m.crg = f[F_CRG * Lp + l];
  m.crb = f[F_CRB * Lp + l];
  m.cgg = f[F_CGG * Lp + l];
  m.cgb = f[F_CGB * Lp + l];
  m.cbb = f[F_CBB * Lp + l];
  m.count = 0;
  return m;
}

// ------------------------------------------------------------------ settling a tentative match
// Is probability_of_match(...) > 0 for a pair that already passed both gates (:433, :441)?
// The association kernel leaves this to us for blobs with a single gate-passing landmark,
// because the landmark's covariance is in registers here.  pr = (500 exp(a1)) (500 exp(a2))
// / 250000 with a1, a2 the two log-pdfs; whenever a1 + a2 is far from the float64 underflow
// edge the answer is known without evaluating a single exp/log; otherwise evaluate it
// exactly as the reference does.  pse = atan2(f.my - sy, f.mx - sx).  MODEL = kModelBearing: (ux, uy) is the world-frame ray and
// there is no half-plane test.
template <int MODEL = kModelReference>
__device__ __forceinline__ bool match_is_positive(const Landmark<double>& f, double sx, double sy, double pse,
                                                  const BlobT<double>& z, double ux, double uy) {
  if constexpr (MODEL == kModelReference)
    if (fabs(pse - z.bearing) > Consts<double>::half_pi) return false;  // :473-475 -> bp = 0
  double nx, ny;
  closest_point<double, MODEL>(f.mx, f.my, sx, sy, ux, uy, nx, ny);
  const double ex = nx - f.mx, ey = ny - f.my;
  const double det2 = f.pxx * f.pyy - f.pxy * f.pxy;
  const double maha2 = (f.pyy * ex * ex - 2.0 * f.pxy * ex * ey + f.pxx * ey * ey) / det2;
  double det3;
  const Sym3<double> inv = sym3_inverse(Sym3<double>{f.crr, f.crg, f.crb, f.cgg, f.cgb, f.cbb}, det3);
  const double maha3 = sym3_quad(inv, z.r - f.mr, z.g - f.mg, z.b - f.mb);
  // log det <= 138.2 for det <= 1e60, so a1 + a2 >= -0.5 (9.2 + 276.4 + 800) > -543: no underflow
  if (det2 > 0.0 && det2 < 1e60 && det3 > 0.0 && det3 < 1e60 && maha2 >= 0.0 && maha3 >= 0.0 &&
      maha2 + maha3 < 800.0)
    return true;
  const double bp = 500.0 * exp(-0.5 * (2.0 * Consts<double>::log_two_pi + log(det2) + maha2));
  const double cp = 500.0 * exp(-0.5 * (3.0 * Consts<double>::log_two_pi + log(det3) + maha3));
  return bp * cp / 250000.0 > 0.0;
}

__device__ __forceinline__ BlobT<double> load_blob(const double* blobs, int b) {
  const double2 z01 = *reinterpret_cast<const double2*>(blobs + 4 * (size_t)b);
  const double2 z23 = *reinterpret_cast<const double2*>(blobs + 4 * (size_t)b + 2);
  return BlobT<double>{z01.x, z01.y, z23.x, z23.y};
}

}  // namespace pk

// The path estimate by the weights of the current particles (pk_path_summary_weighted) and the most likely particle
// (pk_best_particle).
//
// Plain gfx950 (wave64) HIP.  pk_path_summary needs one launch per row because it scatters descendant counts from row t into row
// t - 1; a weighted summary needs no counts.  The lineage index of current particle k, j_t(k) = anc_t[j_{t+1}(k)], depends on k
// alone: every thread walks ITS particles back through every row, gathers pose_t[j_t(k)] and weights it by w_k.  ONE launch
// covers the whole ring -- no atomics, no grid barrier, no quantised weights.  Every sum runs over k in a fixed order -- lane, wave,
// the waves in order, then the workgroups one by one -- so the same ring and weights give the same bits twice.  DESIGN.md section
// 4, "The weighted path estimate".
#include "pk_path_rows.hpp"  // walk_rows, rows_reduce, the fold of a row: shared with pk_k_path_settle.hip

namespace pk {

// part[row][block][kPathSums]: S1, mean dx, mean dy, xx, xy, yy (centred, weighted; d = pose - the row's reference pose), sum w
// sin h, sum w cos h, sum w^2 (row `held`; 0 elsewhere), 0.  wgt[P] and idx[P] are the launch's own scratch: a thread reads and
// writes the elements of its own particles only.  A thread takes kPwRows rows at a time (walk_rows); what is left at the old end of
// the ring goes one by one.  Every row's sums are taken in the same order either way.
__global__ void __launch_bounds__(kPathLanes) k_path_weighted(PathWeightedArgs a) {
  __shared__ PwLds lds[2];
  const int64_t P = a.P, step = (int64_t)gridDim.x * kPathLanes, i0 = (int64_t)blockIdx.x * kPathLanes + threadIdx.x;
  const int held = a.held;
  double shift = a.domain == 1 ? a.gmax[0] : 0.0;
  if (!(shift > -INFINITY)) shift = 0.0;  // all weights zero: keep exp(-inf) = 0, not NaN (pk_k_adaptive.hip: weight_shift)
  int turn = 0;
  {  // row `held`: the live generation, j = k
    double* __restrict__ const wgt = a.wgt;
    int32_t* __restrict__ const idx = a.idx;
    const double rx = a.ref[3 * held], ry = a.ref[3 * held + 1];
    PathMoments m[1] = {PathMoments{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    double ss[1] = {0.0}, sc[1] = {0.0}, s2 = 0.0;
    for (int64_t i = i0; i < P; i += step) {
      const double w = exp(a.logw[i] - shift);
      wgt[i] = w;
      idx[i] = (int32_t)i;
      s2 = __fma_rn(w, w, s2);  // (a weight that is not a number shows here: path_merge passes it over)
      m[0] = path_merge(m[0], PathMoments{w, a.x[i] - rx, a.y[i] - ry, 0.0, 0.0, 0.0});
      double s, co;
      sincos(a.h[i], &s, &co);
      ss[0] = __fma_rn(w, s, ss[0]);
      sc[0] = __fma_rn(w, co, sc[0]);
    }
    rows_reduce<1>(m, ss, sc, s2, lds[turn], a.part + ((size_t)held * gridDim.x + blockIdx.x) * kPathSums, 0);
    turn ^= 1;
  }
  int t = held - 1;
  int r = held > 0 ? (int)(((int64_t)a.first + held - 1) % a.cap) : 0;  // ring row of held row t
  for (; t >= kPwRows - 1; t -= kPwRows) {
    r = walk_rows<kPwRows>(a, t, r, lds[turn]);
    turn ^= 1;
  }
  for (; t >= 0; --t) {
    r = walk_rows<1>(a, t, r, lds[turn]);
    turn ^= 1;
  }
}

// One workgroup per row: the row's partials merged in workgroup order.  res[row][kPathWRes] = mean x, mean y, sum w sin h, sum w
// cos h, var x, cov xy, var y (over S1), S1, S2 (row `held`: the weights are the same in every row)
__global__ void __launch_bounds__(kWave) k_path_weighted_fold(const double* __restrict__ part, const double* __restrict__ ref, int nb,
                                                              double* __restrict__ res) {
  if (threadIdx.x != 0) return;
  const int t = blockIdx.x;
  path_weighted_fold_row(part + (size_t)t * nb * kPathSums, ref[3 * t + 0], ref[3 * t + 1], nb, res + (size_t)t * kPathWRes);
}

void launch_path_weighted(hipStream_t s, const DeviceState& d, const PathRing& ring, const double* gmax_dev, int domain,
                          int32_t* idx_dev, double* wgt_dev, double* ref_dev, double* part_dev, double* res_dev) {
  const int c = d.cur, nb = path_blocks(d.P);
  launch_path_trace(s, d, ring, nullptr, 1, ref_dev);  // particle 0's lineage: the rows' reference poses
  PathWeightedArgs a;
  a.x = d.x[c];
  a.y = d.y[c];
  a.h = d.h[c];
  a.logw = d.logw[c];
  a.pose = ring.pose;
  a.anc = ring.anc;
  a.gmax = gmax_dev;
  a.ref = ref_dev;
  a.idx = idx_dev;
  a.wgt = wgt_dev;
  a.part = part_dev;
  a.P = d.P;
  a.cap = ring.cap;
  a.first = ring.first;
  a.held = ring.held;
  a.domain = domain;
  hipLaunchKernelGGL(k_path_weighted, dim3((unsigned)nb), dim3(kPathLanes), 0, s, a);
  hipLaunchKernelGGL(k_path_weighted_fold, dim3((unsigned)(ring.held + 1)), dim3(kWave), 0, s, part_dev, ref_dev, nb, res_dev);
}

// ------------------------------------------------------------------ the most likely particle
// (value, index) pairs under one total order -- the larger log-weight, among equals the lower index; a log-weight that is not a
// number never stands, index -1 = nobody yet -- so the result does not depend on how the particles are dealt out.
__device__ __forceinline__ void best_take(double& v, long long& i, double ov, long long oi) {
  const bool take = oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i));
  v = take ? ov : v;
  i = take ? oi : i;
}

// part[block][2] = the workgroup's largest log-weight, its index (as a double: exact below 2^53)
__global__ void __launch_bounds__(kPathLanes) k_best_particle(const double* __restrict__ logw, int64_t P, double* __restrict__ part) {
  __shared__ double wv[kPathLanes / kWave];
  __shared__ long long wi[kPathLanes / kWave];
  double v = -INFINITY;
  long long b = -1;
  for (int64_t i = (int64_t)blockIdx.x * kPathLanes + threadIdx.x; i < P; i += (int64_t)gridDim.x * kPathLanes) {
    const double x = logw[i];
    if (x == x) best_take(v, b, x, (long long)i);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_down(v, off, kWave);
    const long long oi = __shfl_down(b, off, kWave);
    best_take(v, b, ov, oi);
  }
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) {
    wv[wave] = v;
    wi[wave] = b;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int w = 1; w < kPathLanes / kWave; ++w) best_take(v, b, wv[w], wi[w]);  // (thread 0 holds wave 0's)
  part[2 * blockIdx.x] = v;
  part[2 * blockIdx.x + 1] = (double)b;
}
// the workgroups' pairs in workgroup order, by one thread: out[2] = the log-weight, the index (-1: every log-weight is NaN)
__global__ void __launch_bounds__(kWave) k_best_particle_fold(const double* __restrict__ part, int nb, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double v = part[0];
  long long b = (long long)part[1];
  for (int k = 1; k < nb; ++k) best_take(v, b, part[2 * k], (long long)part[2 * k + 1]);
  out[0] = v;
  out[1] = (double)b;
}
void launch_best_particle(hipStream_t s, const DeviceState& d, double* part_dev, double* out_dev) {
  const int nb = path_blocks(d.P);
  hipLaunchKernelGGL(k_best_particle, dim3((unsigned)nb), dim3(kPathLanes), 0, s, d.logw[d.cur], d.P, part_dev);
  hipLaunchKernelGGL(k_best_particle_fold, dim3(1), dim3(kWave), 0, s, part_dev, nb, out_dev);
}

}  // namespace pk

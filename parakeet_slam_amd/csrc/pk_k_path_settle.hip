// Settling the oldest rows of the path ring into the trunk (pk_path_settle, and path_record once the ring is full).
//
// Plain gfx950 (wave64) HIP.  Settling E of the `held` rows is k_path_weighted's walk in which only rows E - 1 .. 0 are reduced:
//   k_path_settle_walk   a lane per particle: its weight, and its lineage index taken down rows held - 1 .. E by index alone --
//                        4-byte dependent gathers, no pose, no sincos, no sum, no barrier.  Latency bound, so every chain gets a
//                        lane of its own: 100 000 particles are 1 563 waves, one or two to a SIMD, and all chains are in flight
//                        at once (a thread of the 256 x 256 grid would take its two chains one behind the other).
//   k_path_settle_rows   walk_rows / rows_reduce of pk_path_rows.hpp on k_path_weighted's grid (the same thread holds the same
//                        particles, every sum runs in the same order), which also carry the lowest and highest lineage index.
//   k_path_settle_fold   a workgroup per settled row: the partials in workgroup order, pose_t[lo_t], 13 doubles into the trunk.
// idx[P] and wgt[P] pass from the first launch to the second through memory.  No floating-point atomics, no scratch, no grid
// barrier, nothing read back.  DESIGN.md section 4, "The trunk".
#include "pk_path_rows.hpp"

namespace pk {

__global__ void __launch_bounds__(kPathLanes) k_path_settle_walk(PathWeightedArgs a, int settle) {
  const int64_t P = a.P, i = (int64_t)blockIdx.x * kPathLanes + threadIdx.x;
  if (i >= P) return;
  double w = 1.0;  // PK_PATH_UNIFORM
  if (a.domain != 2) {
    double shift = a.domain == 1 ? a.gmax[0] : 0.0;
    if (!(shift > -INFINITY)) shift = 0.0;  // as k_path_weighted
    w = exp(a.logw[i] - shift);
  }
  a.wgt[i] = w;
  const int32_t* __restrict__ const anc = a.anc;
  int32_t j = (int32_t)i;
  int r = a.held > 0 ? (int)(((int64_t)a.first + a.held - 1) % a.cap) : 0;  // ring row of held row held - 1
  for (int t = a.held - 1; t >= settle; --t) {
    j = anc[(size_t)r * P + j];
    r = r == 0 ? a.cap - 1 : r - 1;
  }
  a.idx[i] = j;
}

// part[row][block][kPathSums] of rows settle - 1 .. 0: k_path_weighted's first eight words, then the workgroup's lowest and
// highest lineage index.  The rows go in turns of kPwRows from row settle - 1 down, then one by one.
__global__ void __launch_bounds__(kPathLanes) k_path_settle_rows(PathWeightedArgs a, int settle) {
  __shared__ PwSpanLds lds[2];
  int turn = 0;
  int t = settle - 1;
  int r = (int)(((int64_t)a.first + settle - 1) % a.cap);  // ring row of held row t (settle >= 1)
  for (; t >= kPwRows - 1; t -= kPwRows) {
    r = walk_rows<kPwRows, true>(a, t, r, lds[turn]);
    turn ^= 1;
  }
  for (; t >= 0; --t) {
    r = walk_rows<1, true>(a, t, r, lds[turn]);
    turn ^= 1;
  }
}

// One workgroup per settled row: k_path_weighted_fold's row, the workgroups' lo / hi, the pose of the lowest lineage.
// out[row][kPathTrunkRes] (the trunk's rows, at their device address)
__global__ void __launch_bounds__(kWave) k_path_settle_fold(const double* __restrict__ part, const double* __restrict__ ref, int nb,
                                                            const double* __restrict__ pose, int64_t P, int cap, int first,
                                                            double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const int t = blockIdx.x;
  const double* p = part + (size_t)t * nb * kPathSums;
  double s[kPathWRes];
  path_weighted_fold_row(p, ref[3 * t + 0], ref[3 * t + 1], nb, s);
  double lo = p[8], hi = p[9];
  for (int b = 1; b < nb; ++b) {
    lo = fmin(lo, p[(size_t)b * kPathSums + 8]);
    hi = fmax(hi, p[(size_t)b * kPathSums + 9]);
  }
  const double* pr = pose + (size_t)(((int64_t)first + t) % cap) * 3 * P;
  const int64_t j = (int64_t)lo;
  double* o = out + (size_t)t * kPathTrunkRes;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = s[k];
  o[8] = lo;
  o[9] = hi;
  o[10] = pr[j];
  o[11] = pr[P + j];
  o[12] = pr[2 * P + j];
}

void launch_path_settle(hipStream_t s, const DeviceState& d, const PathRing& ring, int settle, const double* gmax_dev, int weighting,
                        int32_t* idx_dev, double* wgt_dev, double* ref_dev, double* part_dev, double* out_dev) {
  if (settle <= 0) return;
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
  a.domain = weighting;
  hipLaunchKernelGGL(k_path_settle_walk, dim3((unsigned)((d.P + kPathLanes - 1) / kPathLanes)), dim3(kPathLanes), 0, s, a, settle);
  hipLaunchKernelGGL(k_path_settle_rows, dim3((unsigned)nb), dim3(kPathLanes), 0, s, a, settle);
  hipLaunchKernelGGL(k_path_settle_fold, dim3((unsigned)settle), dim3(kWave), 0, s, part_dev, ref_dev, nb, ring.pose, d.P, ring.cap,
                     ring.first, out_dev);
}

}  // namespace pk

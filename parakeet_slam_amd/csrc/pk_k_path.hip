// The path estimate (pk_path_*): a ring of the last resampled generations, the lineages traced back through it, and their moments.
//
// Plain gfx950 (wave64) HIP, HBM bound and small: a row of the ring is 28 bytes per particle.  Every row read is coalesced; the
// gathers through the ancestors are the only scattered accesses.  The descendant counts are integer atomics (exact, order-free);
// every floating-point sum is taken in a fixed order -- lane, wave, workgroup, then the workgroups one by one -- so the same ring
// gives the same bits twice.  DESIGN.md section 4, "The path estimate".
#include "pk_device.hpp"

namespace pk {

// One launch behind k_ancestors: the generation it resampled (the OLD half of the pose buffers) and its ancestors into a ring row.
__global__ void __launch_bounds__(kPathLanes) k_path_record(const double* __restrict__ x, const double* __restrict__ y,
                                                            const double* __restrict__ h, const int32_t* __restrict__ anc, int64_t P,
                                                            double* __restrict__ row_pose, int32_t* __restrict__ row_anc) {
  const int64_t i = (int64_t)blockIdx.x * kPathLanes + threadIdx.x;
  if (i >= P) return;
  row_pose[i] = x[i];
  row_pose[P + i] = y[i];
  row_pose[2 * P + i] = h[i];
  row_anc[i] = anc[i];
}

void launch_path_record(hipStream_t s, const DeviceState& d, const int32_t* anc_dev, const PathRing& ring, int row) {
  const int old = d.cur ^ 1;
  hipLaunchKernelGGL(k_path_record, dim3((unsigned)((d.P + kPathLanes - 1) / kPathLanes)), dim3(kPathLanes), 0, s, d.x[old], d.y[old],
                     d.h[old], anc_dev, d.P, ring.pose + (size_t)row * 3 * d.P, ring.anc + (size_t)row * d.P);
}

// One thread per requested particle: j_held = k, j_t = anc_t[j_{t+1}], out[i][t] = pose_t[j_t]; row `held` is the current pose.
__global__ void __launch_bounds__(kPathLanes) k_path_trace(const double* __restrict__ x, const double* __restrict__ y,
                                                           const double* __restrict__ h, const double* __restrict__ pose,
                                                           const int32_t* __restrict__ anc, int64_t P, int cap, int first, int held,
                                                           const int64_t* __restrict__ particles, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kPathLanes + threadIdx.x;
  if (i >= n) return;
  int64_t j = particles ? particles[i] : i;
  double* o = out + (size_t)i * (held + 1) * 3;
  o[(size_t)held * 3 + 0] = x[j];
  o[(size_t)held * 3 + 1] = y[j];
  o[(size_t)held * 3 + 2] = h[j];
  int r = held > 0 ? (int)(((int64_t)first + held - 1) % cap) : 0;
  for (int t = held - 1; t >= 0; --t) {
    j = anc[(size_t)r * P + j];
    const double* pr = pose + (size_t)r * 3 * P;
    o[(size_t)t * 3 + 0] = pr[j];
    o[(size_t)t * 3 + 1] = pr[P + j];
    o[(size_t)t * 3 + 2] = pr[2 * P + j];
    r = r == 0 ? cap - 1 : r - 1;
  }
}

void launch_path_trace(hipStream_t s, const DeviceState& d, const PathRing& ring, const int64_t* particles_dev, int64_t n, double* out_dev) {
  if (n <= 0) return;
  const int c = d.cur;
  hipLaunchKernelGGL(k_path_trace, dim3((unsigned)((n + kPathLanes - 1) / kPathLanes)), dim3(kPathLanes), 0, s, d.x[c], d.y[c], d.h[c],
                     ring.pose, ring.anc, d.P, ring.cap, ring.first, ring.held, particles_dev, n, out_dev);
}

// The position moments of a row about its reference pose are PathMoments triples merged with path_merge (pk_device.hpp): the
// reference is particle 0's lineage, which few others may share.
//
// part[block][kPathSums]: n, mean dx, mean dy, xx, xy, yy (centred, weighted), sum c sin h, sum c cos h, lineages alive, 0
//
// The launch of row t (t = held: the current generation, every count 1 -- cnt == NULL):
//   reduces the row, whose counts are finished, about ref = particle 0's lineage in that row;
//   scatters cnt_{t-1}[anc_{t-1}[k]] += cnt_t[k]          (anc_prev == NULL for t == 0);
//   zeroes the buffer row t - 2 will count in             (it held row t + 1's counts, which the launch before this one read).
__global__ void __launch_bounds__(kPathLanes) k_path_row(const double* __restrict__ px, const double* __restrict__ py,
                                                         const double* __restrict__ ph, const unsigned* __restrict__ cnt,
                                                         const int32_t* __restrict__ anc_prev, unsigned* __restrict__ cnt_prev,
                                                         unsigned* __restrict__ cnt_zero, const double* __restrict__ ref, int64_t P,
                                                         double* __restrict__ part) {
  __shared__ double red[4];
  __shared__ PathMoments wm[kPathLanes / kWave];
  const double rx = ref[0], ry = ref[1];
  PathMoments m{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double ss = 0.0, sc = 0.0, alive = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kPathLanes + threadIdx.x; i < P; i += (int64_t)gridDim.x * kPathLanes) {
    const unsigned c = cnt ? cnt[i] : 1u;
    if (cnt_zero) cnt_zero[i] = 0u;
    if (c == 0u) continue;
    if (anc_prev) atomicAdd(&cnt_prev[anc_prev[i]], c);
    const double w = (double)c;
    const PathMoments e{w, px[i] - rx, py[i] - ry, 0.0, 0.0, 0.0};
    m = path_merge(m, e);
    double s, co;
    sincos(ph[i], &s, &co);
    ss += w * s;
    sc += w * co;
    alive += 1.0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = path_merge(m, path_shfl_down(m, off));  // lane 0 holds the wave's
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) wm[wave] = m;
  ss = block_sum<4>(ss, red);
  sc = block_sum<4>(sc, red);
  alive = block_sum<4>(alive, red);  // (small integers: exact; and the barriers that make wm visible)
  if (threadIdx.x == 0) {
    m = wm[0];
#pragma unroll
    for (int w = 1; w < kPathLanes / kWave; ++w) m = path_merge(m, wm[w]);
    double* o = part + (size_t)blockIdx.x * kPathSums;
    o[0] = m.n;
    o[1] = m.mx;
    o[2] = m.my;
    o[3] = m.xx;
    o[4] = m.xy;
    o[5] = m.yy;
    o[6] = ss;
    o[7] = sc;
    o[8] = alive;
    o[9] = 0.0;
  }
}

// One workgroup per row: the row's partials merged in block order.  res[row][8] = mean x, mean y, sum sin h, sum cos h (over the
// P lineages), var x, cov xy, var y, survivors.
__global__ void __launch_bounds__(kWave) k_path_fold(const double* __restrict__ part, const double* __restrict__ ref, int nb,
                                                     double* __restrict__ res) {
  if (threadIdx.x != 0) return;
  const int t = blockIdx.x;
  const double* p = part + (size_t)t * nb * kPathSums;
  PathMoments m{p[0], p[1], p[2], p[3], p[4], p[5]};
  double ss = p[6], sc = p[7], alive = p[8];
  for (int b = 1; b < nb; ++b) {
    const double* q = p + (size_t)b * kPathSums;
    m = path_merge(m, PathMoments{q[0], q[1], q[2], q[3], q[4], q[5]});
    ss += q[6];
    sc += q[7];
    alive += q[8];
  }
  double* o = res + (size_t)t * kPathRes;
  o[0] = ref[3 * t + 0] + m.mx;
  o[1] = ref[3 * t + 1] + m.my;
  o[2] = ss;
  o[3] = sc;
  o[4] = m.xx / m.n;
  o[5] = m.xy / m.n;
  o[6] = m.yy / m.n;
  o[7] = alive;
}

void launch_path_summary(hipStream_t s, const DeviceState& d, const PathRing& ring, unsigned* cnt_dev, double* ref_dev, double* part_dev,
                         double* res_dev) {
  const int64_t P = d.P;
  const int held = ring.held, nb = path_blocks(P);
  const int c = d.cur;
  launch_path_trace(s, d, ring, nullptr, 1, ref_dev);
  // the first scatter (row held -> held - 1) needs its buffer clear; every later one finds what the launch two before it zeroed
  if (held > 0) (void)hipMemsetAsync(cnt_dev + (size_t)((held - 1) % 3) * P, 0, (size_t)P * sizeof(unsigned), s);
  for (int t = held; t >= 0; --t) {
    const bool current = t == held;
    const double* pose = current ? nullptr : ring.pose + (size_t)ring.row(t) * 3 * P;
    hipLaunchKernelGGL(k_path_row, dim3((unsigned)nb), dim3(kPathLanes), 0, s, current ? d.x[c] : pose, current ? d.y[c] : pose + P,
                       current ? d.h[c] : pose + 2 * P, current ? (const unsigned*)nullptr : cnt_dev + (size_t)(t % 3) * P,
                       t > 0 ? ring.anc + (size_t)ring.row(t - 1) * P : (const int32_t*)nullptr,
                       t > 0 ? cnt_dev + (size_t)((t - 1) % 3) * P : (unsigned*)nullptr,
                       t > 1 ? cnt_dev + (size_t)((t - 2) % 3) * P : (unsigned*)nullptr, ref_dev + (size_t)3 * t, P,
                       part_dev + (size_t)t * nb * kPathSums);
  }
  hipLaunchKernelGGL(k_path_fold, dim3((unsigned)(held + 1)), dim3(kWave), 0, s, part_dev, ref_dev, nb, res_dev);
}

}  // namespace pk

// Adaptive (selective) resampling: the effective sample size on the device, the resample that can decline, and the weighted
// pose summary a filter needs once its weights carry over (pk_resample_adaptive, pk_step_adaptive, pk_weight_sums,
// pk_summary_weighted).
//
// Plain gfx950 (wave64) HIP, O(P) and HBM bound.  The verdict never reaches the host: every workgroup of the gated kernel derives
// it from the block sums (a few hundred doubles, read through LDS) and takes the same branch.  No floating-point atomics: every sum
// is taken lane, wave, workgroup, then the workgroups in order, so the same state gives the same bits.  DESIGN.md section 4,
// "Adaptive resampling".
#include "pk_device.hpp"

namespace pk {

constexpr int kGateMaxBlocks = (int)kAncestorsScanMaxBlocks;

// what k_scan_local subtracts from the log-weights (the same rule, so the same value)
__device__ __forceinline__ double weight_shift(const double* __restrict__ gmax, int domain,
                                               const unsigned long long* __restrict__ gmax_key, double* lds4) {
  double shift = 0.0;
  if (domain == 1) {
    if (gmax_key) {  // max over the sharded running-max keys (kGmaxKeys == blockDim.x)
      shift = block_max<4>(key_to_double(gmax_key[threadIdx.x]), lds4);
      __syncthreads();
    } else {
      shift = gmax[0];
    }
    if (!(shift > -INFINITY)) shift = 0.0;  // all weights zero: keep exp(-inf) = 0, not NaN
  }
  return shift;
}

// n_eff = S1 / S2 * S1, the one expression every kernel here uses; keep iff n_eff >= threshold * P (false for NaN: all weights zero)
__device__ __forceinline__ double gate_n_eff(double s1, double s2) { return __dmul_rn(__ddiv_rn(s1, s2), s1); }
__device__ __forceinline__ bool gate_keep(double n_eff, double threshold, int64_t P) { return n_eff >= __dmul_rn(threshold, (double)P); }

// Sum of w^2 over one scan block of kScanBlock particles, w = exp(logw - shift) as k_scan_local takes it: a lane's four
// particles in order (fused multiply-adds), the wave by the xor butterfly, the four waves in order.
__global__ void __launch_bounds__(256) k_weight_sq(const double* __restrict__ logw, int64_t P, const double* __restrict__ gmax,
                                                   int domain, const unsigned long long* __restrict__ gmax_key,
                                                   double* __restrict__ s2tot, double* __restrict__ shift_out) {
  __shared__ double red[4];
  const double shift = weight_shift(gmax, domain, gmax_key, red);
  const int64_t base = (int64_t)blockIdx.x * kScanBlock + 4 * threadIdx.x;
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double w = (base + i < P) ? exp(logw[base + i] - shift) : 0.0;
    q = __fma_rn(w, w, q);
  }
  q = block_sum<4>(q, red);
  if (threadIdx.x == 0) {
    s2tot[blockIdx.x] = q;
    if (blockIdx.x == 0) shift_out[0] = shift;
  }
}
void launch_weight_sq(hipStream_t s, const DeviceState& d, const double* gmax_dev, int domain, const unsigned long long* gmax_key_dev,
                      double* s2tot_dev, double* shift_dev) {
  const int nb = (int)((d.P + kScanBlock - 1) / kScanBlock);
  hipLaunchKernelGGL(k_weight_sq, dim3(nb), dim3(256), 0, s, d.logw[d.cur], d.P, gmax_dev, domain, gmax_key_dev, s2tot_dev, shift_dev);
}

// Beyond kGateMaxBlocks scan blocks: k_scan_blocks' exclusive scan of the block totals (the same additions in the same order),
// the sum of the blocks' w^2 in block order, and the verdict, by ONE thread.
__global__ void __launch_bounds__(256) k_gate_plan(const double* __restrict__ totals, const double* __restrict__ s2tot, int64_t nb,
                                                   double* __restrict__ offsets, double* __restrict__ plan, double threshold,
                                                   int64_t P) {
  __shared__ double t[2048], q[2048];
  double run = 0.0, s2 = 0.0;
  for (int64_t c0 = 0; c0 < nb; c0 += 2048) {
    const int n = (int)((nb - c0 < 2048) ? (nb - c0) : 2048);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      t[i] = totals[c0 + i];
      q[i] = s2tot[c0 + i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < n; ++i) {
        const double v = t[i];
        t[i] = run;
        run += v;
        s2 += q[i];
      }
    }
    __syncthreads();
    if (offsets)
      for (int i = threadIdx.x; i < n; i += blockDim.x) offsets[c0 + i] = t[i];
  }
  if (threadIdx.x == 0) {
    const double n_eff = gate_n_eff(run, s2);
    plan[0] = run;
    plan[1] = s2;
    plan[2] = n_eff;
    plan[3] = gate_keep(n_eff, threshold, P) ? 1.0 : 0.0;
  }
}
void launch_gate_plan(hipStream_t s, const double* totals_dev, const double* s2tot_dev, int64_t nb, double* offsets_dev,
                      double* plan_dev, double threshold, int64_t P) {
  hipLaunchKernelGGL(k_gate_plan, dim3(1), dim3(256), 0, s, totals_dev, s2tot_dev, nb, offsets_dev, plan_dev, threshold, P);
}

// k_ancestors with its fused gather, behind the gate.  plan == NULL (few blocks): every workgroup fetches the block totals and
// the blocks' w^2 into LDS and one thread sums them in block order -- the additions of k_ancestors' own scan, so S1 is the sum it
// divides by P, bit for bit.  The verdict is a function of those sums alone: the same in every workgroup.
__global__ void __launch_bounds__(256) k_ancestors_gated(const double* __restrict__ clocal, const double* __restrict__ totals,
                                                         const double* __restrict__ s2tot, const double* offsets,
                                                         const double* plan, int64_t nb, int64_t P, double u,
                                                         double threshold, const double* __restrict__ shift_in,
                                                         int32_t* __restrict__ anc, const double* __restrict__ gx,
                                                         const double* __restrict__ gy, const double* __restrict__ gh,
                                                         const double* __restrict__ glw, const int32_t* __restrict__ gsrc,
                                                         double* __restrict__ gx2, double* __restrict__ gy2,
                                                         double* __restrict__ gh2, double* __restrict__ glw2,
                                                         int32_t* __restrict__ gsrc2, GateOutcome* __restrict__ outcome) {
  __shared__ double s_off[kGateMaxBlocks + 1], s_q[kGateMaxBlocks];
  __shared__ double s_gate[kGatePlan];
  if (plan == nullptr) {
    for (int b = threadIdx.x; b < nb; b += blockDim.x) {
      s_off[b] = totals[b];
      s_q[b] = s2tot[b];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double run = 0.0, s2 = 0.0;
      for (int64_t b = 0; b < nb; ++b) {
        const double v = s_off[b];
        s_off[b] = run;
        run += v;
        s2 += s_q[b];
      }
      s_off[nb] = run;
      const double n_eff = gate_n_eff(run, s2);
      s_gate[0] = run;
      s_gate[1] = s2;
      s_gate[2] = n_eff;
      s_gate[3] = gate_keep(n_eff, threshold, P) ? 1.0 : 0.0;
    }
    __syncthreads();
    offsets = s_off;
    plan = s_gate;
  }
  const double s1 = plan[0];
  const bool keep = plan[3] != 0.0;
  const double shift = shift_in[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    outcome->n_eff = plan[2];
    outcome->s1 = s1;
    outcome->s2 = plan[1];
    outcome->shift = shift;
    outcome->resampled = keep ? 0ull : 1ull;
    outcome->calls += 1ull;  // (calls are stream ordered and one thread writes: no atomics)
    if (!keep) outcome->resamples += 1ull;
  }
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= P) return;
  if (keep) {  // the identity gather; the weights renormalised by the shift the scan took (one rounded subtraction)
    anc[k] = (int32_t)k;
    gx2[k] = gx[k];
    gy2[k] = gy[k];
    gh2[k] = gh[k];
    glw2[k] = __dsub_rn(glw[k], shift);
    gsrc2[k] = gsrc[k];
    return;
  }
  const int32_t a = (int32_t)comb_ancestor(clocal, totals, offsets, s1, nb, P, P, u, k);
  anc[k] = a;
  gx2[k] = gx[a];
  gy2[k] = gy[a];
  gh2[k] = gh[a];
  glw2[k] = 0.0;  // the new generation has unit weights: the caller's next observe does not reset them
  gsrc2[k] = gsrc[a];
}
void launch_ancestors_gated(hipStream_t s, const double* clocal_dev, const double* totals_dev, const double* s2tot_dev,
                            const double* offsets_dev, const double* plan_dev, int64_t nb, double u, double threshold,
                            const double* shift_dev, int32_t* anc_dev, DeviceState& d, GateOutcome* outcome_dev) {
  const int c = d.cur, m = c ^ 1;
  hipLaunchKernelGGL(k_ancestors_gated, dim3((unsigned)((d.P + 255) / 256)), dim3(256), 0, s, clocal_dev, totals_dev, s2tot_dev,
                     offsets_dev, plan_dev, nb, d.P, u, threshold, shift_dev, anc_dev, d.x[c], d.y[c], d.h[c], d.logw[c], d.src[c],
                     d.x[m], d.y[m], d.h[m], d.logw[m], d.src[m], outcome_dev);
  d.cur = m;
}

// ------------------------------------------------------------------ the weighted pose summary
// part[block][kPathSums]: S1, mean dx, mean dy, xx, xy, yy (centred, weighted; d = pose - particle 0's), sum w sin h,
// sum w cos h, sum w^2, 0 -- k_path_row's reduction with the particles' weights in place of descendant counts.
__global__ void __launch_bounds__(kPathLanes) k_pose_moments(const double* __restrict__ px, const double* __restrict__ py,
                                                             const double* __restrict__ ph, const double* __restrict__ logw,
                                                             int64_t P, const double* __restrict__ gmax, int domain,
                                                             double* __restrict__ part) {
  __shared__ double red[4];
  __shared__ PathMoments wm[kPathLanes / kWave];
  const double shift = weight_shift(gmax, domain, nullptr, red);
  const double rx = px[0], ry = py[0];
  PathMoments m{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double ss = 0.0, sc = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kPathLanes + threadIdx.x; i < P; i += (int64_t)gridDim.x * kPathLanes) {
    const double w = exp(logw[i] - shift);
    s2 = __fma_rn(w, w, s2);  // (a weight that is not a number shows here: path_merge passes it over)
    const PathMoments e{w, px[i] - rx, py[i] - ry, 0.0, 0.0, 0.0};
    m = path_merge(m, e);
    double s, co;
    sincos(ph[i], &s, &co);
    ss = __fma_rn(w, s, ss);
    sc = __fma_rn(w, co, sc);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = path_merge(m, path_shfl_down(m, off));  // lane 0 holds the wave's
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) wm[wave] = m;
  ss = block_sum<4>(ss, red);
  sc = block_sum<4>(sc, red);
  s2 = block_sum<4>(s2, red);  // (and the barriers that make wm visible)
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
    o[8] = s2;
    o[9] = 0.0;
  }
}
// The workgroups' partials merged in block order by one thread.
__global__ void __launch_bounds__(kWave) k_pose_fold(const double* __restrict__ part, int nb, const double* __restrict__ px,
                                                     const double* __restrict__ py, double* __restrict__ res) {
  if (threadIdx.x != 0) return;
  PathMoments m{part[0], part[1], part[2], part[3], part[4], part[5]};
  double ss = part[6], sc = part[7], s2 = part[8];
  for (int b = 1; b < nb; ++b) {
    const double* q = part + (size_t)b * kPathSums;
    m = path_merge(m, PathMoments{q[0], q[1], q[2], q[3], q[4], q[5]});
    ss += q[6];
    sc += q[7];
    s2 += q[8];
  }
  res[0] = px[0] + m.mx;
  res[1] = py[0] + m.my;
  res[2] = ss;
  res[3] = sc;
  res[4] = m.xx / m.n;
  res[5] = m.xy / m.n;
  res[6] = m.yy / m.n;
  res[7] = m.n;
  res[8] = s2;
}
void launch_pose_moments(hipStream_t s, const DeviceState& d, const double* gmax_dev, int domain, double* part_dev, double* res_dev) {
  const int c = d.cur, nb = path_blocks(d.P);
  hipLaunchKernelGGL(k_pose_moments, dim3((unsigned)nb), dim3(kPathLanes), 0, s, d.x[c], d.y[c], d.h[c], d.logw[c], d.P, gmax_dev,
                     domain, part_dev);
  hipLaunchKernelGGL(k_pose_fold, dim3(1), dim3(kWave), 0, s, part_dev, nb, d.x[c], d.y[c], res_dev);
}

}  // namespace pk

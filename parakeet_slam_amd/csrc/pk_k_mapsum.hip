// The map estimate (pk_map_moments / pk_map_summary): per-landmark moments of the particles' EKFs, reduced over the particles.
//
// Plain gfx950 (wave64) HIP, HBM bound: every distinct slot is read once, 14 coalesced rows and the counts.  No MFMA (the
// algebra is 5-vectors per lane), no float atomics: k_map_partials leaves one partial per (particle group, sum, landmark),
// k_map_fold adds them in group order and k_map_finish un-shifts, so the same filter state gives the same bits twice.  DESIGN.md section 4.
#include "pk_device.hpp"

namespace pk {

constexpr unsigned kCountMask = ~0x40000000u;  // PK_LANDMARK_POTENTIAL (include/parakeet_slam.h) rides in the count word

int map_sum_groups(int64_t P, int Ls, int forced) {
  if (forced > 0) return forced;
  const int64_t tiles = map_sum_tiles(Ls);
  int64_t g = (1024 + tiles - 1) / tiles;  // tiles x groups fills the chip's 256 CUs (four 256-lane workgroups each) about once over ...
  const int64_t by_p = (P + 15) / 16;      // ... while a group still has sixteen particles to walk
  if (g > by_p) g = by_p;
  if (g > kMapSumMaxGroups) g = kMapSumMaxGroups;
  return g < 1 ? 1 : (int)g;
}

// particle p's weight: 1 (PK_MAP_UNIFORM) or exp(logw - gmax)
__device__ __forceinline__ double map_weight(const double* __restrict__ logw, int64_t p, double gmax) {
  return logw ? exp(logw[p] - gmax) : 1.0;
}

// grid (tiles, groups), 256 lanes: lane = landmark of the tile.  The workgroup walks the particles [g chunk, (g + 1) chunk) in order
// with the 30 running sums of its landmark in registers -- shifted by the mean rows of the first local particle's slot (ref), the
// same in every group: raw second moments cancel once a landmark sits far from the origin.  Consecutive particles in one slot (the
// copies of one ancestor behind a resample: k_ancestors is monotone) are read once with their summed weight; that test is
// workgroup-uniform.  part[group][kMapSums][Lq], wpart[group][2] = the group's sum w, sum w^2 (tile 0 writes it).
__global__ void __launch_bounds__(kMapSumLanes) k_map_partials(SlotSource ss, const int32_t* __restrict__ src, const double* __restrict__ logw,
                                                               double gmax, int64_t P, int64_t chunk, int Lp, int Ls, size_t count_off,
                                                               int Lq, double* __restrict__ part, double* __restrict__ wpart) {
  const int l = (int)blockIdx.x * kMapSumLanes + (int)threadIdx.x;
  const int g = blockIdx.y;
  const int lr = l < Ls ? l : (Ls > 0 ? Ls - 1 : 0);  // lanes beyond the map read its last landmark: no branch around the loads; nobody reads their partials
  int64_t p0 = (int64_t)g * chunk, p1 = p0 + chunk;
  if (p0 > P) p0 = P;
  if (p1 > P) p1 = P;
  double ref[5];
  {
    const double* r = reinterpret_cast<const double*>(ss.at(src[0]));
#pragma unroll
    for (int i = 0; i < 5; ++i) ref[i] = r[(size_t)i * Lp + lr];
  }
  double s1[5] = {0, 0, 0, 0, 0};
  double s2[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double wi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double cn = 0.0, ws = 0.0, wq = 0.0;
  // The slot's rows are requested first and the run of equal src[] behind it is walked while they are in flight: src[] and the
  // log-weights come through scalar loads, which the vector memory counter does not wait for.
  int64_t p = p0;
  int32_t slot = p < p1 ? __builtin_amdgcn_readfirstlane(src[p]) : 0;
  while (p < p1) {
    const unsigned char* base = ss.at(slot);
    const double* f = reinterpret_cast<const double*>(base);
    double v[F_COUNT_FIELDS];
#pragma unroll
    for (int i = 0; i < F_COUNT_FIELDS; ++i) v[i] = f[(size_t)i * Lp + lr];
    const unsigned c = reinterpret_cast<const unsigned*>(base + count_off)[lr];
    double w = 0.0;
    int32_t next = slot;
    do {
      const double wn = map_weight(logw, p, gmax);
      ws += wn;
      wq += wn * wn;
      w += wn;
      ++p;
      if (p < p1) next = __builtin_amdgcn_readfirstlane(src[p]);
    } while (p < p1 && next == slot);
    slot = next;
    double d[5], wd[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      d[i] = v[i] - ref[i];
      wd[i] = w * d[i];
      s1[i] += wd[i];
    }
    int k = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int j = i; j < 5; ++j) {
        s2[k] = fma(wd[i], d[j], s2[k]);
        ++k;
      }
#pragma unroll
    for (int i = 0; i < 9; ++i) wi[i] = fma(w, v[5 + i], wi[i]);
    cn = fma(w, (double)(c & kCountMask), cn);
  }
  double* out = part + (size_t)g * kMapSums * Lq + l;  // (l < Lq in every lane: Lq = tiles x lanes)
#pragma unroll
  for (int i = 0; i < 5; ++i) out[(size_t)i * Lq] = s1[i];
#pragma unroll
  for (int i = 0; i < 15; ++i) out[(size_t)(5 + i) * Lq] = s2[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) out[(size_t)(20 + i) * Lq] = wi[i];
  out[(size_t)29 * Lq] = cn;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    wpart[2 * g] = ws;
    wpart[2 * g + 1] = wq;
  }
}

// The groups' partials added in group order, one lane per (sum, landmark): part[0][k][l] += part[g][k][l], g = 1 ..., in place (a lane
// reads and writes its own column only).  With one lane per landmark and the 30 sums in a row the reduction was a serial chain of
// `groups` dependent rounds on a handful of waves (4.7 ms at 10 000 x 500 against 0.15 ms for k_map_partials).  The last workgroup
// adds the groups' weight sums instead, into wpart[0], wpart[1] -- in a fixed order, like everything here.
__global__ void __launch_bounds__(kMapSumLanes) k_map_fold(int groups, size_t n, double* __restrict__ part, double* __restrict__ wpart) {
  if (blockIdx.x + 1 == gridDim.x) {
    __shared__ double red[4];
    double w = 0.0, w2 = 0.0;
    for (int g = threadIdx.x; g < groups; g += kMapSumLanes) {
      w += wpart[2 * g];
      w2 += wpart[2 * g + 1];
    }
    w = block_sum<4>(w, red);
    w2 = block_sum<4>(w2, red);
    if (threadIdx.x == 0) {
      wpart[0] = w;
      wpart[1] = w2;
    }
    return;
  }
  const size_t t = (size_t)blockIdx.x * kMapSumLanes + threadIdx.x;
  if (t >= n) return;
  double s = 0.0;
#pragma unroll 8
  for (int g = 0; g < groups; ++g) s += part[(size_t)g * n + t];
  part[t] = s;
}

// One lane per landmark: the folded sums un-shifted.  res: wsum[2] | mean[L][5] | m2[L][15] | within[L][9] | counts[L] (what
// pk_map_moments hands out); rows Ls <= l < L are NaN.
__global__ void __launch_bounds__(kMapSumLanes) k_map_finish(SlotSource ss, const int32_t* __restrict__ src, int Lp, int L, int Ls, int Lq,
                                                             const double* __restrict__ part, const double* __restrict__ wpart,
                                                             double* __restrict__ res) {
  const int l = (int)blockIdx.x * kMapSumLanes + (int)threadIdx.x;
  const double W = wpart[0], W2 = wpart[1];
  if (l == 0) {
    res[0] = W;
    res[1] = W2;
  }
  if (l >= L) return;
  double* mean = res + 2 + (size_t)l * 5;
  double* m2 = res + 2 + (size_t)L * 5 + (size_t)l * 15;
  double* within = res + 2 + (size_t)L * 20 + (size_t)l * 9;
  double* counts = res + 2 + (size_t)L * 29 + l;
  if (l >= Ls) {  // spare slots of a growing map: different features in different particles
    const double nan = __builtin_nan("");
    for (int i = 0; i < 5; ++i) mean[i] = nan;
    for (int i = 0; i < 15; ++i) m2[i] = nan;
    for (int i = 0; i < 9; ++i) within[i] = nan;
    counts[0] = nan;
    return;
  }
  double s[kMapSums];
#pragma unroll
  for (int k = 0; k < kMapSums; ++k) s[k] = part[(size_t)k * Lq + l];
  const double* r = reinterpret_cast<const double*>(ss.at(src[0]));
#pragma unroll
  for (int i = 0; i < 5; ++i) mean[i] = r[(size_t)i * Lp + l] + s[i] / W;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = i; j < 5; ++j) {
      m2[k] = s[5 + k] - s[i] * s[j] / W;
      ++k;
    }
#pragma unroll
  for (int i = 0; i < 9; ++i) within[i] = s[20 + i];
  counts[0] = s[29];
}

// n: doubles of one group's partials
void launch_map_fold(hipStream_t s, int groups, size_t n, double* part_dev, double* wpart_dev) {
  hipLaunchKernelGGL(k_map_fold, dim3((unsigned)((n + kMapSumLanes - 1) / kMapSumLanes) + 1), dim3(kMapSumLanes), 0, s, groups, n, part_dev,
                     wpart_dev);
}

void launch_map_moments(hipStream_t s, const DeviceState& d, int Ls, int weighted, double gmax, int groups, double* part_dev,
                        double* wpart_dev, double* res_dev) {
  const int tiles = map_sum_tiles(Ls);
  const int Lq = tiles * kMapSumLanes;
  const int64_t chunk = (d.P + groups - 1) / groups;
  const SlotSource ss = slot_source(d);
  hipLaunchKernelGGL(k_map_partials, dim3((unsigned)tiles, (unsigned)groups), dim3(kMapSumLanes), 0, s, ss, d.src[d.cur],
                     weighted ? d.logw[d.cur] : nullptr, gmax, d.P, chunk, d.lay.Lp, Ls, d.lay.count_off, Lq, part_dev, wpart_dev);
  launch_map_fold(s, groups, (size_t)kMapSums * Lq, part_dev, wpart_dev);
  const int L = d.lay.L;
  hipLaunchKernelGGL(k_map_finish, dim3((unsigned)map_sum_tiles(L)), dim3(kMapSumLanes), 0, s, ss, d.src[d.cur],
                     d.lay.Lp, L, Ls, Lq, part_dev, wpart_dev, res_dev);
}

}  // namespace pk

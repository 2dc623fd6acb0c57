// The map estimate of the DISCOVERED landmarks (pk_map_match_moments / pk_map_discovered): for a list of reference features, the
// spare slot of every particle that holds the same feature -- a geometric match, spare slot j of one particle and of another need
// not hold the same thing -- and, per reference feature, the moments pk_k_mapsum.hip takes per preset landmark, over the particles
// that matched.  DESIGN.md section 4, "The discovered landmarks".
//
// Plain gfx950 (wave64) HIP, latency bound: per particle one coalesced read of its candidates' mean rows, then every lane's gather
// of its winner's 14 rows and count word.  No float atomics: k_match_partials leaves one partial per (particle group, sum,
// feature), k_map_fold (pk_k_mapsum.hip) adds them in group order, k_match_finish un-shifts with each feature's own divisor -- the
// same filter state gives the same bits twice.  Nothing of the filter is written.
#include "pk_device.hpp"

namespace pk {

constexpr unsigned kMatchPotential = 0x40000000u;  // PK_LANDMARK_POTENTIAL (include/parakeet_slam.h) rides in the count word

int map_match_groups(int64_t P, int cap, int forced) {
  if (forced > 0) return forced;
  const int64_t tiles = map_match_tiles(cap);
  int64_t g = (2048 + tiles - 1) / tiles;  // one wave per workgroup: tiles x groups gives each of the chip's 1 024 SIMDs about two ...
  const int64_t by_p = (P + 15) / 16;      // ... while a group still has sixteen particles to walk
  if (g > by_p) g = by_p;
  if (g > kMatchMaxGroups) g = kMatchMaxGroups;
  return g < 1 ? 1 : (int)g;
}

__device__ __forceinline__ double match_weight(const double* __restrict__ logw, int64_t p, double gmax) {
  return logw ? exp(logw[p] - gmax) : 1.0;
}

// lane i's v in every lane (i wave-uniform)
__device__ __forceinline__ double lane_value(double v, int i) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), i);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
  return __hiloint2double(hi, lo);
}

// The reference particle's spare slots in use into the reference block: ref[S][5] their means (NaN beyond the u_r in use),
// refi = u_r, the particle, 0, 0 | count words [S] | feature ids [S].  best != NULL: the particle is k_best_particle_fold's
// (best[1], -1: every log-weight is NaN -> no reference feature), else `particle`.
__global__ void __launch_bounds__(kMatchLanes) k_match_ref(SlotSource ss, const int32_t* __restrict__ src, const int32_t* __restrict__ cnt,
                                                           const int32_t* __restrict__ slot_id, const double* __restrict__ best,
                                                           int64_t particle, int64_t P, int Lp, int L0, int S, size_t count_off,
                                                           double* __restrict__ ref, int32_t* __restrict__ refi) {
  int64_t r = best ? (int64_t)best[1] : particle;
  if (r >= P) r = -1;
  int u = 0;
  if (r >= 0) {
    u = cnt[4 * r + 1];
    u = u < 0 ? 0 : (u > S ? S : u);
  }
  const unsigned char* base = r >= 0 ? ss.at(src[r]) : nullptr;
  for (int i = threadIdx.x; i < S; i += kMatchLanes) {
    const bool in = i < u;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      ref[(size_t)i * 5 + k] = in ? reinterpret_cast<const double*>(base)[(size_t)k * Lp + L0 + i] : __builtin_nan("");
    refi[4 + i] = in ? reinterpret_cast<const int32_t*>(base + count_off)[L0 + i] : 0;
    refi[4 + S + i] = in ? slot_id[(size_t)r * S + i] : 0;
  }
  if (threadIdx.x == 0) {
    refi[0] = u;
    refi[1] = (int32_t)r;
    refi[2] = refi[3] = 0;
  }
}

struct MatchGates {
  double rho2, kap2, irho2, ikap2;  // the squared radii and their reciprocals (0 for an infinite radius), formed once on the host
};

// The score is evaluated as the NumPy reference of the tests does, operation for operation: no contraction from here ...
#pragma clang fp contract(off)
// candidate (mx .. mb) against the lane's reference feature r: true and `score` when it passes both gates (a NaN mean fails them)
__device__ __forceinline__ bool match_score(const double r[5], double mx, double my, double mr, double mg, double mb, const MatchGates& q,
                                            double& score) {
  const double dx = mx - r[0], dy = my - r[1];
  const double dpos2 = dx * dx + dy * dy;
  const double dr = mr - r[2], dg = mg - r[3], db = mb - r[4];
  const double dcol2 = (dr * dr + dg * dg) + db * db;
  score = dpos2 * q.irho2 + dcol2 * q.ikap2;
  return dpos2 <= q.rho2 && dcol2 <= q.kap2;
}
#pragma clang fp contract(on)
// ... to here: the sums below are held to a tolerance, not to bits, and use fma like k_map_partials'.

// grid (tiles of 64 reference features, particle groups), ONE wave: lane = reference feature.  The wave walks the particles
// [g chunk, (g + 1) chunk) in order with the 33 running sums of its feature in registers, shifted by the reference feature itself
// (the gates bound the shift).  Per particle: src, the number of spare slots in use and the weight are wave-uniform; the candidates'
// five mean rows are read once, candidate c in lane c (64 at a time), and handed round by v_readlane while every lane scores its own
// feature -- the strictly smallest score among the candidates inside both gates, the lowest slot among equals --; then each lane
// gathers the 14 rows and the count word of its winner.  Two dependent round trips per particle.
// part[group][kMatchSums][Lq]: sum w, sum w^2, sum w[potential] | 5 first | 15 second moments of mu - r | 9 within | count;
// wpart[group][2] = the group's sum w, sum w^2 over ALL its particles (tile 0 writes it); matches[P][stride] (or NULL): the spare
// slot matched, -1 = none.
__global__ void __launch_bounds__(kMatchLanes) k_match_partials(SlotSource ss, const int32_t* __restrict__ src, const int32_t* __restrict__ cnt,
                                                                const double* __restrict__ logw, const double* __restrict__ gmax_dev,
                                                                double gmax, int64_t P, int64_t chunk, int Lp, int L0, int S, size_t count_off,
                                                                const double* __restrict__ ref, const int32_t* __restrict__ nref_dev, int nref,
                                                                MatchGates q, int Lq, double* __restrict__ part, double* __restrict__ wpart,
                                                                int32_t* __restrict__ matches, int stride) {
  const int lane = threadIdx.x;
  const int j = (int)blockIdx.x * kMatchLanes + lane;
  const int g = blockIdx.y;
  if (nref_dev) nref = __builtin_amdgcn_readfirstlane(nref_dev[0]);
  if (gmax_dev) gmax = gmax_dev[0];
  const bool active = j < nref;
  int64_t p0 = (int64_t)g * chunk, p1 = p0 + chunk;
  if (p0 > P) p0 = P;
  if (p1 > P) p1 = P;
  double r[5] = {0, 0, 0, 0, 0};
  if (active) {
#pragma unroll
    for (int i = 0; i < 5; ++i) r[i] = ref[(size_t)j * 5 + i];
  }
  double s1[5] = {0, 0, 0, 0, 0};
  double s2[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double wi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double cn = 0.0, sw = 0.0, sq = 0.0, sp = 0.0, ws = 0.0, wq = 0.0;
  for (int64_t p = p0; p < p1; ++p) {
    const int32_t slot = __builtin_amdgcn_readfirstlane(src[p]);
    int u = __builtin_amdgcn_readfirstlane(cnt[4 * p + 1]);
    u = u < 0 ? 0 : (u > S ? S : u);
    const double w = match_weight(logw, p, gmax);
    ws += w;
    wq += w * w;
    const unsigned char* base = ss.at(slot);
    const double* f = reinterpret_cast<const double*>(base);
    int best = -1;
    double bs = INFINITY;
    for (int c0 = 0; c0 < u; c0 += kMatchLanes) {
      const int n = u - c0 < kMatchLanes ? u - c0 : kMatchLanes;
      const int li = L0 + c0 + (lane < n ? lane : n - 1);  // (the lanes beyond the candidates read the last one again: no branch around the loads)
      double m[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) m[k] = f[(size_t)k * Lp + li];
      for (int i = 0; i < n; ++i) {
        double sc;
        const bool pass = match_score(r, lane_value(m[0], i), lane_value(m[1], i), lane_value(m[2], i), lane_value(m[3], i),
                                      lane_value(m[4], i), q, sc);
        if (pass && active && sc < bs) {
          bs = sc;
          best = c0 + i;
        }
      }
    }
    if (matches && active) matches[(size_t)p * stride + j] = best;
    if (best >= 0) {
      double v[F_COUNT_FIELDS];
#pragma unroll
      for (int i = 0; i < F_COUNT_FIELDS; ++i) v[i] = f[(size_t)i * Lp + L0 + best];
      const unsigned c = reinterpret_cast<const unsigned*>(base + count_off)[L0 + best];
      sw += w;
      sq += w * w;
      if (c & kMatchPotential) sp += w;
      double d[5], wd[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        d[i] = v[i] - r[i];
        wd[i] = w * d[i];
        s1[i] += wd[i];
      }
      int k = 0;
#pragma unroll
      for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int jj = i; jj < 5; ++jj) {
          s2[k] = fma(wd[i], d[jj], s2[k]);
          ++k;
        }
#pragma unroll
      for (int i = 0; i < 9; ++i) wi[i] = fma(w, v[5 + i], wi[i]);
      cn = fma(w, (double)(c & ~kMatchPotential), cn);
    }
  }
  double* out = part + (size_t)g * kMatchSums * Lq + j;  // (j < Lq in every lane: Lq = tiles x lanes)
  out[0] = sw;
  out[(size_t)Lq] = sq;
  out[(size_t)2 * Lq] = sp;
#pragma unroll
  for (int i = 0; i < 5; ++i) out[(size_t)(3 + i) * Lq] = s1[i];
#pragma unroll
  for (int i = 0; i < 15; ++i) out[(size_t)(8 + i) * Lq] = s2[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) out[(size_t)(23 + i) * Lq] = wi[i];
  out[(size_t)32 * Lq] = cn;
  if (blockIdx.x == 0 && lane == 0) {
    wpart[2 * g] = ws;
    wpart[2 * g + 1] = wq;
  }
}

// One lane per row: the folded sums un-shifted, each feature by its own matched weight W_j.
// res: wsum[2] | support[rows][3] = W_j, sum w^2, sum w[potential] | mean[rows][5] = r + S1 / W_j | m2[rows][15] = S2 - S1 S1^T / W_j |
// within[rows][9] | counts[rows] | tail: the maximum log-weight taken, the number of reference features, the reference particle,
// then (refi != NULL) the reference's count words [rows] and feature ids [rows] as doubles.  A feature nobody matched: support 0,
// mean and m2 NaN (0 / 0), within and counts 0; rows beyond the reference features: support 0, NaN elsewhere.
__global__ void __launch_bounds__(kMapSumLanes) k_match_finish(const double* __restrict__ part, const double* __restrict__ wpart,
                                                               const double* __restrict__ ref, const int32_t* __restrict__ refi,
                                                               const int32_t* __restrict__ nref_dev, int nref, const double* __restrict__ gmax_dev,
                                                               double gmax, int rows, int Lq, double* __restrict__ res) {
  const int l = (int)blockIdx.x * kMapSumLanes + (int)threadIdx.x;
  if (nref_dev) nref = nref_dev[0];
  double* tail = res + 2 + (size_t)kMatchSums * rows;
  if (l == 0) {
    res[0] = wpart[0];
    res[1] = wpart[1];
    tail[0] = gmax_dev ? gmax_dev[0] : gmax;
    tail[1] = (double)nref;
    tail[2] = refi ? (double)refi[1] : -1.0;
  }
  if (l >= rows) return;
  if (refi) {
    tail[3 + l] = (double)refi[4 + l];
    tail[3 + rows + l] = (double)refi[4 + rows + l];
  }
  double* support = res + 2 + (size_t)l * 3;
  double* mean = res + 2 + (size_t)rows * 3 + (size_t)l * 5;
  double* m2 = res + 2 + (size_t)rows * 8 + (size_t)l * 15;
  double* within = res + 2 + (size_t)rows * 23 + (size_t)l * 9;
  double* counts = res + 2 + (size_t)rows * 32 + l;
  if (l >= nref) {
    const double nan = __builtin_nan("");
    support[0] = support[1] = support[2] = 0.0;
    for (int i = 0; i < 5; ++i) mean[i] = nan;
    for (int i = 0; i < 15; ++i) m2[i] = nan;
    for (int i = 0; i < 9; ++i) within[i] = nan;
    counts[0] = nan;
    return;
  }
  double s[kMatchSums];
#pragma unroll
  for (int k = 0; k < kMatchSums; ++k) s[k] = part[(size_t)k * Lq + l];
  const double Wj = s[0];
  support[0] = Wj;
  support[1] = s[1];
  support[2] = s[2];
#pragma unroll
  for (int i = 0; i < 5; ++i) mean[i] = ref[(size_t)l * 5 + i] + s[3 + i] / Wj;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int jj = i; jj < 5; ++jj) {
      m2[k] = s[8 + k] - s[3 + i] * s[3 + jj] / Wj;
      ++k;
    }
#pragma unroll
  for (int i = 0; i < 9; ++i) within[i] = s[23 + i];
  counts[0] = s[32];
}

void launch_match_reference(hipStream_t s, const DeviceState& d, const GrowState& g, const double* best_dev, int64_t particle,
                            double* ref_dev, int32_t* refi_dev) {
  hipLaunchKernelGGL(k_match_ref, dim3(1), dim3(kMatchLanes), 0, s, slot_source(d), d.src[d.cur], g.cnt[g.cur], g.slot_id[g.cur], best_dev,
                     particle, d.P, d.lay.Lp, g.L0, g.S, d.lay.count_off, ref_dev, refi_dev);
}

void launch_map_match(hipStream_t s, const DeviceState& d, const GrowState& g, const MatchJob& m) {
  const int tiles = map_match_tiles(m.rows);
  const int Lq = tiles * kMatchLanes;
  const int64_t chunk = (d.P + m.groups - 1) / m.groups;
  const int32_t* nref_dev = m.refi_dev;  // (word 0 of the reference block's integers)
  const MatchGates q{m.rho2, m.kap2, m.irho2, m.ikap2};
  hipLaunchKernelGGL(k_match_partials, dim3((unsigned)tiles, (unsigned)m.groups), dim3(kMatchLanes), 0, s, slot_source(d), d.src[d.cur],
                     g.cnt[g.cur], m.weighted ? d.logw[d.cur] : nullptr, m.gmax_dev, m.gmax, d.P, chunk, d.lay.Lp, g.L0, g.S, d.lay.count_off,
                     m.ref_dev, nref_dev, m.nref, q, Lq, m.part_dev, m.wpart_dev, m.matches_dev, m.nref);
  launch_map_fold(s, m.groups, (size_t)kMatchSums * Lq, m.part_dev, m.wpart_dev);
  hipLaunchKernelGGL(k_match_finish, dim3((unsigned)map_sum_tiles(m.rows)), dim3(kMapSumLanes), 0, s, m.part_dev, m.wpart_dev, m.ref_dev,
                     m.refi_dev, nref_dev, m.nref, m.gmax_dev, m.gmax, m.rows, Lq, m.res_dev);
}

}  // namespace pk

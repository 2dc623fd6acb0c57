// The rows of the weighted path estimate, for the two kernels that reduce them: k_path_weighted (pk_k_path_weighted.hip), which
// takes every row of the ring, and k_path_settle_rows (pk_k_path_settle.hip), which takes the oldest ones on their way into the
// trunk.  One definition: a settled row then carries the bits pk_path_summary_weighted would have given for it, by
// construction.  Device code only; DESIGN.md section 4, "The weighted path estimate" and "The trunk".
#pragma once
#include "pk_device.hpp"

namespace pk {

constexpr int kPwWaves = kPathLanes / kWave;
constexpr int kPwRows = 8;  // rows a thread takes at a time (1, 4 and 8 measured: profiles/r12)

// What one workgroup keeps in LDS per turn (a turn: up to kPwRows rows reduced behind ONE barrier).  Two of them, taken in turn:
// turn n + 1 writes the other one, and the one turn n wrote is written again only behind turn n + 1's barrier, which thread 0
// reaches after it has read.
struct PwLds {
  PathMoments wm[kPwRows][kPwWaves];
  double ss[kPwRows][kPwWaves], sc[kPwRows][kPwWaves], s2[kPwWaves];
};
// ... with the waves' lowest and highest lineage index of every row (kSpan: the settling kernel's rows)
struct PwSpanLds : PwLds {
  int32_t lo[kPwRows][kPwWaves], hi[kPwRows][kPwWaves];
};
template <bool kSpan>
struct PwLdsOf { using type = PwLds; };
template <>
struct PwLdsOf<true> { using type = PwSpanLds; };

// k_pose_moments' reduction of a workgroup, for R rows side by side (R independent chains: their latencies overlap): the wave by
// path_shfl_down (sums: the xor butterfly), the waves in order.  o: the workgroup's partial of row q = 0; row q's lies q *
// row_doubles before it (the rows are taken newest first).  kSpan: lo / hi [R], the thread's lowest and highest lineage index of
// each row, go along -- the wave by integer shuffles, the waves behind the same barrier -- into the partial's last two words (as
// doubles: exact); integer min / max are order-free, and no sum changes.
template <int R, bool kSpan = false>
__device__ __forceinline__ void rows_reduce(PathMoments (&m)[R], double (&ss)[R], double (&sc)[R], double s2,
                                            typename PwLdsOf<kSpan>::type& l, double* __restrict__ o, size_t row_doubles,
                                            int32_t* lo = nullptr, int32_t* hi = nullptr) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int q = 0; q < R; ++q) m[q] = path_merge(m[q], path_shfl_down(m[q], off));  // lane 0 holds the wave's
  }
#pragma unroll
  for (int q = 0; q < R; ++q) {
    ss[q] = wave_sum(ss[q]);
    sc[q] = wave_sum(sc[q]);
  }
  s2 = wave_sum(s2);
  if constexpr (kSpan) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int q = 0; q < R; ++q) {
        lo[q] = min(lo[q], __shfl_down(lo[q], off, kWave));
        hi[q] = max(hi[q], __shfl_down(hi[q], off, kWave));
      }
    }
  }
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < R; ++q) {
      l.wm[q][wave] = m[q];
      l.ss[q][wave] = ss[q];
      l.sc[q][wave] = sc[q];
      if constexpr (kSpan) {
        l.lo[q][wave] = lo[q];
        l.hi[q][wave] = hi[q];
      }
    }
    l.s2[wave] = s2;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  s2 = l.s2[0];
#pragma unroll
  for (int w = 1; w < kPwWaves; ++w) s2 += l.s2[w];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    PathMoments t = l.wm[q][0];
    double s = l.ss[q][0], c = l.sc[q][0];
#pragma unroll
    for (int w = 1; w < kPwWaves; ++w) {
      t = path_merge(t, l.wm[q][w]);
      s += l.ss[q][w];
      c += l.sc[q][w];
    }
    double* __restrict__ const oq = o - (size_t)q * row_doubles;
    oq[0] = t.n;
    oq[1] = t.mx;
    oq[2] = t.my;
    oq[3] = t.xx;
    oq[4] = t.xy;
    oq[5] = t.yy;
    oq[6] = s;
    oq[7] = c;
    if constexpr (kSpan) {
      int32_t a = l.lo[q][0], b = l.hi[q][0];
#pragma unroll
      for (int w = 1; w < kPwWaves; ++w) {
        a = min(a, l.lo[q][w]);
        b = max(b, l.hi[q][w]);
      }
      oq[8] = (double)a;
      oq[9] = (double)b;
    } else {
      oq[8] = q == 0 ? s2 : 0.0;
      oq[9] = 0.0;
    }
  }
}

// Held rows t, t - 1 .. t - R + 1 (r: the ring row of t; returns that of t - R).  Per particle: R steps down the index chain
// j = anc_row[j], the only loads that depend on one another; then the R rows' gathers, which do not, all in flight together.
// kSpan: the lowest and highest j of every row are kept beside the sums (a workgroup always holds at least one particle: P >=
// path_blocks(P) * kPathLanes - kPathLanes + 1; a thread that holds none leaves the neutral pair).
template <int R, bool kSpan = false>
__device__ __forceinline__ int walk_rows(const PathWeightedArgs& a, int t, int r, typename PwLdsOf<kSpan>::type& l) {
  const int64_t P = a.P, step = (int64_t)gridDim.x * kPathLanes, i0 = (int64_t)blockIdx.x * kPathLanes + threadIdx.x;
  const double* __restrict__ const wgt = a.wgt;
  int32_t* __restrict__ const idx = a.idx;
  const int32_t* __restrict__ anc[R];
  const double* __restrict__ px[R];
  double rx[R], ry[R], ss[R], sc[R];
  PathMoments m[R];
  int32_t lo[R], hi[R];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    anc[q] = a.anc + (size_t)r * P;
    px[q] = a.pose + (size_t)r * 3 * P;
    rx[q] = a.ref[3 * (t - q)];
    ry[q] = a.ref[3 * (t - q) + 1];
    ss[q] = sc[q] = 0.0;
    m[q] = PathMoments{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    lo[q] = INT32_MAX;
    hi[q] = -1;
    r = r == 0 ? a.cap - 1 : r - 1;
  }
  for (int64_t i = i0; i < P; i += step) {
    const double w = wgt[i];
    int32_t j = idx[i], jj[R];
#pragma unroll
    for (int q = 0; q < R; ++q) jj[q] = j = anc[q][j];
    idx[i] = j;
    double gx[R], gy[R], gh[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {  // (a loop of their own: sincos branches, and no load is moved across a branch)
      const int32_t k = jj[q];
      gx[q] = px[q][k];
      gy[q] = px[q][P + k];
      gh[q] = px[q][2 * P + k];
      if constexpr (kSpan) {
        lo[q] = min(lo[q], k);
        hi[q] = max(hi[q], k);
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      m[q] = path_merge(m[q], PathMoments{w, gx[q] - rx[q], gy[q] - ry[q], 0.0, 0.0, 0.0});
      double s, co;
      sincos(gh[q], &s, &co);
      ss[q] = __fma_rn(w, s, ss[q]);
      sc[q] = __fma_rn(w, co, sc[q]);
    }
  }
  rows_reduce<R, kSpan>(m, ss, sc, 0.0, l, a.part + ((size_t)t * gridDim.x + blockIdx.x) * kPathSums, (size_t)gridDim.x * kPathSums,
                        lo, hi);
  return r;
}

// The fold of one row: its workgroups' partials merged in workgroup order by one thread.  o[kPathWRes] = mean x, mean y, sum w
// sin h, sum w cos h, var x, cov xy, var y (over S1), S1, the sum of the partials' ninth words.
__device__ __forceinline__ void path_weighted_fold_row(const double* __restrict__ p, double rx, double ry, int nb, double* o) {
  PathMoments m{p[0], p[1], p[2], p[3], p[4], p[5]};
  double ss = p[6], sc = p[7], s2 = p[8];
  for (int b = 1; b < nb; ++b) {
    const double* q = p + (size_t)b * kPathSums;
    m = path_merge(m, PathMoments{q[0], q[1], q[2], q[3], q[4], q[5]});
    ss += q[6];
    sc += q[7];
    s2 += q[8];
  }
  o[0] = rx + m.mx;
  o[1] = ry + m.my;
  o[2] = ss;
  o[3] = sc;
  o[4] = m.xx / m.n;
  o[5] = m.xy / m.n;
  o[6] = m.yy / m.n;
  o[7] = m.n;
  o[8] = s2;
}

}  // namespace pk

// The per-scan blocks: where everything lies in the ONE block a scan travels in, host -> device, and the host code that fills the
// maximum-likelihood one.  No filter, no HIP call: tests/scan_block_host_main.cpp runs all of it on the CPU under sanitizers.
//
// Every block starts with ctl (kCtlBytes: kGmaxKeys running-max keys (u64), then the flagged-particle count, the route control words
// and the publish table's figures: pk_filter.hpp, ctl_*), which the copy zeroes -- that is how every observe starts with a fresh
// max / count -- and the blobs, [B][4] f64 in scan order.  Behind them ([..]: only when asked for):
//   ML (MlScanLayout):    dir [B][2] f64 | exact [B][6] f64 | tables, padded to 16 B | [rng [B][2] f64 | rng_cell [B][2] f64]
//       tables:           start u16[ncell + 1], padded to 16 B | rec32 float4[B] (r, g, b, bearing) | idx9 u16[n9] | order u16[B]
//       without a grid:   dir | [rng | rng_cell] -- neither the exact records nor the tables are sent
//   known ids (KnownScanLayout): first i32[Lp] | next i32[B] | [ids i32[B]] | [padded to 16 B: rng]
//   dense (DenseScanLayout): dir | ids i32[B], padded to 16 B
// exact, rec32, order and rng_cell are in cell order (row t is blob order[t]'s), the rest in scan order; the range rows (range,
// variance) travel only with a scan in which some blob has a range (pk_scan_ranges).
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "pk_kernels.hpp"

namespace pk {

constexpr size_t kCtlBytes = 8 * kGmaxKeys + 64;
inline size_t pad16(size_t n) { return (n + 15) & ~(size_t)15; }

struct MlScanLayout {
  size_t blobs, dir, exact, tables, start, rec32, idx9, order;  // start .. order: inside the tables (offsets into the block, like the rest)
  size_t rng, rng_cell;                                          // 0: the scan has no range rows
  size_t upload_bytes;                                           // what the device needs of the block
};
inline MlScanLayout ml_scan_layout(int B, bool use_grid, int ncell, int n9, bool ranged) {
  const size_t n = (size_t)B, rows = n * 2 * sizeof(double);
  const size_t dir = kCtlBytes + n * 4 * sizeof(double), exact = dir + n * 2 * sizeof(double), tables = exact + n * 6 * sizeof(double);
  const size_t rec32 = tables + grid_cs_bytes(ncell), idx9 = rec32 + n * 16, order = idx9 + (size_t)n9 * 2;
  const size_t end = use_grid ? pad16(order + n * 2) : exact;  // (without a grid the upload ends behind dir)
  return MlScanLayout{kCtlBytes, dir, exact, tables, tables, rec32, idx9, order, ranged ? end : 0, ranged ? end + rows : 0, ranged ? end + 2 * rows : end};
}
// what a staging slot and the device block hold for ANY scan of B blobs: the largest grid, the longest duplicated lists
inline size_t ml_scan_worst_bytes(int B, bool ranged) {
  return ml_scan_layout(B, true, kGridMax * kGridMax * kGridMax, 9 * B + 16, false).upload_bytes + 16 + (ranged ? (size_t)B * 4 * sizeof(double) : 0);
}

struct KnownScanLayout {
  size_t blobs, first, next, ids, rng /* 0: no range rows */, upload_bytes;
};
inline KnownScanLayout known_scan_layout(int B, int Lp, bool with_ids, bool ranged) {
  const size_t first = kCtlBytes + (size_t)B * 4 * sizeof(double), next = first + (size_t)Lp * sizeof(int32_t);
  const size_t ids = next + (size_t)B * sizeof(int32_t), end = ids + (with_ids ? (size_t)B * sizeof(int32_t) : 0);
  const size_t rng = ranged ? pad16(end) : 0;
  return KnownScanLayout{kCtlBytes, first, next, ids, rng, ranged ? rng + (size_t)B * 2 * sizeof(double) : end};
}
struct DenseScanLayout {
  size_t blobs, dir, ids, upload_bytes;
};
inline DenseScanLayout dense_scan_layout(int B) {
  const size_t dir = kCtlBytes + (size_t)B * 4 * sizeof(double), ids = dir + (size_t)B * 2 * sizeof(double);
  return DenseScanLayout{kCtlBytes, dir, ids, pad16(ids + (size_t)B * sizeof(int32_t))};
}

// unit((cos b, sin b, 0.0)) of closest_point (prkt_core_v2.py:510, utils.py:68-76): the ray
// direction of each blob, scaled by 1/length exactly like utils.scale(vector, 1.0/length).
inline void blob_directions(const double* blobs, int B, double* dir) {
  for (int b = 0; b < B; ++b) {
    double c = std::cos(blobs[4 * b]), s = std::sin(blobs[4 * b]);
    double len = std::sqrt(c * c + s * s + 0.0 * 0.0);
    dir[2 * b] = c * (1.0 / len);
    dir[2 * b + 1] = s * (1.0 / len);
  }
}

// Bucket the blobs of one scan into a 3-D colour grid (cell edge kGridCell > sqrt(300), the colour gate radius of
// prkt_core_v2.py:441) and write what k_assoc_grid reads into the block at `st`: the tables and the exact records (bearing, r, g, b,
// ux, uy).  With dup, idx9 lists for every (r, g) column and b cell the blobs (cell-order index) within one cell in r and g, and
// `start` = offsets into idx9; otherwise `start` = cell offsets into rec32.  Returns n9 (0: no duplicated lists).
inline int build_blob_grid(const double* blobs, const double* dir, int B, bool want_dup, BlobGrid& g, unsigned char* st) {
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, M = 0.0, Mb = 0.0;
  for (int k = 0; k < 3; ++k) {
    lo[k] = hi[k] = B ? blobs[1 + k] : 0.0;
    for (int b = 0; b < B; ++b) {
      double v = blobs[4 * b + 1 + k];
      lo[k] = std::fmin(lo[k], v);
      hi[k] = std::fmax(hi[k], v);
      M = std::fmax(M, std::fabs(v));
    }
  }
  for (int b = 0; b < B; ++b) Mb = std::fmax(Mb, std::fabs(blobs[4 * b]));
  g.inv_h = 1.0 / kGridCell;
  g.ncell = 1;
  for (int k = 0; k < 3; ++k) {
    g.lo[k] = lo[k];
    double span = std::floor((hi[k] - lo[k]) * g.inv_h) + 1.0;
    g.G[k] = span > (double)kGridMax ? kGridMax : (int)span;
    g.ncell *= g.G[k];
  }
  // fp32 pre-filter bounds.  Colour: with d the exact channel difference of a pair inside the
  // gate and d' its fp32 evaluation from fp32-rounded colours, |d' - d| <= eta = 2^-24 (2M + 35);
  // then sum d'^2 <= 300 + 60 eta + 3 eta^2 (+ fp32 summation error).  Bearing: a pair inside
  // the gate has |expected| <= Mb + 0.5, so |d' - d| <= 2^-24 (2 Mb + 1.5).  Both doubled.
  const double eta = 2.0 * std::ldexp(2.0 * M + 35.0, -24);
  const double thr = (300.0 + 60.0 * eta + 3.0 * eta * eta + 1e-3) * (1.0 + 1e-6);
  g.thr32 = thr < 3.0e38 ? (float)thr : INFINITY;
  const double thrb = (0.5 + 2.0 * std::ldexp(2.0 * Mb + 1.5, -24) + 1e-6) * (1.0 + 1e-6);
  g.thrb32 = thrb < 3.0e38 ? (float)thrb : INFINITY;
  // The bearing model's screen: d' = fl(fl(bearing) - fl(e)) with e the expected bearing wrapped into [-pi, pi] in float64, then
  // w' = fma(-k, fl(2 pi), d'), k = rint(d' fl(1 / 2 pi)).  |d' - d| <= 2^-24 2 (Mb + pi + 1); for a pair inside the gate k is the
  // exact wrap's integer, |k| <= (Mb + pi) / 2 pi + 1, |fl(2 pi) - 2 pi| < 2^-22, and the fma rounds a value below 1 once:
  // |w' - w| <= 2^-24 (2 (Mb + pi + 1) + 4 |k| + 1) <= 2^-24 (2.64 (Mb + pi) + 7).  Doubled, like the others.
  const double thrbw = (0.5 + 2.0 * std::ldexp(2.64 * (Mb + 3.1415926535897932) + 7.0, -24) + 1e-6) * (1.0 + 1e-6);
  g.thrb32w = thrbw < 3.0e38 ? (float)thrbw : INFINITY;
  auto cell_of = [&](int b) {
    int c[3];
    for (int k = 0; k < 3; ++k) {
      double q = std::floor((blobs[4 * b + 1 + k] - g.lo[k]) * g.inv_h);
      c[k] = q < 0.0 ? 0 : (q > (double)(g.G[k] - 1) ? g.G[k] - 1 : (int)q);
    }
    return (c[0] * g.G[1] + c[1]) * g.G[2] + c[2];
  };
  std::vector<int> cell((size_t)std::max(B, 1)), cs((size_t)g.ncell + 1, 0), fill;
  for (int b = 0; b < B; ++b) {
    cell[b] = cell_of(b);
    ++cs[cell[b] + 1];
  }
  for (int c = 0; c < g.ncell; ++c) cs[c + 1] += cs[c];
  fill = cs;
  // duplicated column lists: size known before laying out `order`
  int n9 = 0;
  if (want_dup) {
    long total = 0;
    for (int r = 0; r < g.G[0]; ++r)
      for (int gg = 0; gg < g.G[1]; ++gg)
        for (int k = 0; k < g.G[2]; ++k)
          for (int r2 = std::max(r - 1, 0); r2 <= std::min(r + 1, g.G[0] - 1); ++r2)
            for (int g2 = std::max(gg - 1, 0); g2 <= std::min(gg + 1, g.G[1] - 1); ++g2) {
              const int c = (r2 * g.G[1] + g2) * g.G[2] + k;
              total += cs[c + 1] - cs[c];
            }
    if (total + 3 <= 65535) n9 = (int)((total + 3 + 7) & ~7L);  // the walk reads up to three entries past a range
  }
  const MlScanLayout l = ml_scan_layout(B, true, g.ncell, n9, false);
  memset(st + l.start, 0, l.rec32 - l.start);
  uint16_t* start = reinterpret_cast<uint16_t*>(st + l.start);
  float* rec32 = reinterpret_cast<float*>(st + l.rec32);
  uint16_t* idx9 = reinterpret_cast<uint16_t*>(st + l.idx9);
  uint16_t* order = reinterpret_cast<uint16_t*>(st + l.order);
  double* exact = reinterpret_cast<double*>(st + l.exact);
  for (int b = 0; b < B; ++b) {  // ascending b inside a cell
    const int pos = fill[cell[b]]++;
    order[pos] = (uint16_t)b;
    const float r32[4] = {(float)blobs[4 * b + 1], (float)blobs[4 * b + 2], (float)blobs[4 * b + 3], (float)blobs[4 * b]};
    const double rec[6] = {blobs[4 * b], blobs[4 * b + 1], blobs[4 * b + 2], blobs[4 * b + 3], dir[2 * b], dir[2 * b + 1]};
    memcpy(rec32 + 4 * (size_t)pos, r32, sizeof(r32));
    memcpy(exact + 6 * (size_t)pos, rec, sizeof(rec));
  }
  if (n9 > 0) {
    int w = 0;
    for (int r = 0; r < g.G[0]; ++r)
      for (int gg = 0; gg < g.G[1]; ++gg)
        for (int k = 0; k < g.G[2]; ++k) {
          start[(r * g.G[1] + gg) * g.G[2] + k] = (uint16_t)w;
          for (int r2 = std::max(r - 1, 0); r2 <= std::min(r + 1, g.G[0] - 1); ++r2)
            for (int g2 = std::max(gg - 1, 0); g2 <= std::min(gg + 1, g.G[1] - 1); ++g2) {
              const int c = (r2 * g.G[1] + g2) * g.G[2] + k;
              for (int t = cs[c]; t < cs[c + 1]; ++t) idx9[w++] = (uint16_t)t;
            }
        }
    start[g.ncell] = (uint16_t)w;
    for (; w < n9; ++w) idx9[w] = 0;
  } else {
    for (int c = 0; c <= g.ncell; ++c) start[c] = (uint16_t)cs[c];
  }
  return n9;
}

// The host half of a maximum-likelihood scan's upload, in two steps around the caller's decision whether the tables fit LDS.
// 1. ctl zeroed, blobs (`blobs` may be the block's own), directions and -- want_grid -- the exact records, the tables, *g and *n9
inline MlScanLayout ml_scan_fill(unsigned char* st, const double* blobs, int B, bool want_grid, bool want_dup, BlobGrid* g, int* n9) {
  const MlScanLayout l = ml_scan_layout(B, false, 0, 0, false);
  memset(st, 0, kCtlBytes);
  memmove(st + l.blobs, blobs, (size_t)B * 4 * sizeof(double));
  double* dir = reinterpret_cast<double*>(st + l.dir);
  blob_directions(blobs, B, dir);
  *g = BlobGrid{};
  *n9 = want_grid ? build_blob_grid(blobs, dir, B, want_dup, *g, st) : 0;
  return ml_scan_layout(B, want_grid, g->ncell, *n9, false);
}
// 2. use_grid is final: the range rows (`rows` [B][2], or NULL: none) as they are and in cell order (without a grid: as they are again)
inline MlScanLayout ml_scan_ranges(unsigned char* st, int B, bool use_grid, int ncell, int n9, const double* rows) {
  const MlScanLayout l = ml_scan_layout(B, use_grid, ncell, n9, rows != nullptr);
  if (!rows) return l;
  memcpy(st + l.rng, rows, (size_t)B * 2 * sizeof(double));
  double* cell = reinterpret_cast<double*>(st + l.rng_cell);
  if (use_grid) {
    const uint16_t* order = reinterpret_cast<const uint16_t*>(st + l.order);
    for (int t = 0; t < B; ++t) {
      cell[2 * (size_t)t] = rows[2 * (size_t)order[t]];
      cell[2 * (size_t)t + 1] = rows[2 * (size_t)order[t] + 1];
    }
  } else {
    memcpy(cell, rows, (size_t)B * 2 * sizeof(double));
  }
  return l;
}

}  // namespace pk

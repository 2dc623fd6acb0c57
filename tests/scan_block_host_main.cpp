// Stand-alone check of the per-scan blocks (parakeet_slam_amd/csrc/pk_scan_block.hpp): the three layouts against the arithmetic the
// host layer wrote out by hand before there was one header, and the fill of the maximum-likelihood block -- every scan filled into a
// heap buffer of EXACTLY ml_scan_worst_bytes, so that a write past the reservation is an AddressSanitizer report.  No GPU, no HIP
// call.  tests/test_scan_block_host.py builds it with -fsanitize=address,undefined and runs it; it prints "scan_block ok" and exits
// 0, or names the first check that failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../parakeet_slam_amd/csrc/pk_scan_block.hpp"

namespace {

const char* g_scan = "";
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s: %s (line %d)\n", g_scan, #cond, __LINE__);   \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// ---- the arithmetic of the old sites, longhand: stage_ml_scan / enqueue_association (o_*), staged_range_offset /
// staged_upload_bytes (pk_filter.hpp: o_exact as kCtlBytes + 6 B doubles), the order table's address, the worst case
const size_t CTL = 8 * 256 + 64;
struct Old {
  size_t o_blobs, o_dir, o_exact, o_tab, cs_b, rec32, idx9, order, tab_bytes, range_off, upload, worst;
};
Old old_ml(int B, bool use_grid, int ncell, int n9, bool ranged) {
  Old o;
  o.o_blobs = CTL;
  o.o_dir = o.o_blobs + (size_t)B * 4 * sizeof(double);
  o.o_exact = o.o_dir + (size_t)B * 2 * sizeof(double);
  o.o_tab = o.o_exact + (size_t)B * 6 * sizeof(double);
  o.cs_b = ((size_t)(ncell + 1) * 2 + 15) & ~(size_t)15;
  o.rec32 = o.o_tab + o.cs_b;
  o.idx9 = o.o_tab + o.cs_b + (size_t)B * 16;
  o.order = o.o_tab + o.cs_b + (size_t)B * 16 + (size_t)n9 * 2;
  o.tab_bytes = (o.cs_b + (size_t)B * 16 + (size_t)n9 * 2 + (size_t)B * 2 + 15) & ~(size_t)15;
  const size_t filter_o_exact = CTL + (size_t)B * 6 * sizeof(double);
  o.range_off = use_grid ? filter_o_exact + (size_t)B * 6 * sizeof(double) + o.tab_bytes : filter_o_exact;
  o.upload = o.range_off + (ranged ? (size_t)B * 4 * sizeof(double) : 0);
  const size_t cs_max = ((size_t)(16 * 16 * 16 + 1) * 2 + 15) & ~(size_t)15;
  const size_t tab_max = (cs_max + (size_t)B * 16 + (size_t)(9 * B + 16) * 2 + (size_t)B * 2 + 15) & ~(size_t)15;
  o.worst = o.o_tab + tab_max + 16 + (ranged ? (size_t)B * 4 * sizeof(double) : 0);
  return o;
}

void check_layout(const pk::MlScanLayout& l, int B, bool use_grid, int ncell, int n9, bool ranged) {
  const Old o = old_ml(B, use_grid, ncell, n9, ranged);
  CHECK(pk::kCtlBytes == CTL);
  CHECK(l.blobs == o.o_blobs && l.dir == o.o_dir && l.exact == o.o_exact && l.tables == o.o_tab);
  CHECK(l.upload_bytes == o.upload);
  CHECK(pk::ml_scan_worst_bytes(B, ranged) == o.worst);
  CHECK(l.upload_bytes <= pk::ml_scan_worst_bytes(B, ranged));
  CHECK(l.upload_bytes % 16 == 0);
  CHECK(l.blobs < l.dir && l.dir < l.exact);
  if (use_grid) {
    CHECK(l.start == o.o_tab && l.rec32 == o.rec32 && l.idx9 == o.idx9 && l.order == o.order);
    CHECK(l.tables % 16 == 0 && l.rec32 % 16 == 0);
    CHECK(l.exact < l.tables && l.start < l.rec32 && l.rec32 < l.idx9 && l.idx9 <= l.order);
    CHECK(l.order + (size_t)B * 2 <= (ranged ? l.rng : l.upload_bytes));
  }
  if (ranged) {
    CHECK(l.rng == o.range_off && l.rng_cell == o.range_off + (size_t)B * 2 * sizeof(double));
    CHECK(l.rng % 8 == 0 && l.rng >= (use_grid ? l.order + (size_t)B * 2 : l.exact));
    CHECK(l.rng_cell + (size_t)B * 2 * sizeof(double) == l.upload_bytes);
  } else {
    CHECK(l.rng == 0 && l.rng_cell == 0);
  }
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// One scan through the fill, as stage_ml_scan drives it: with and without range rows (every third row has no range: NaN), the
// grid kept or -- fits = false -- given up behind the build, as for tables that do not fit LDS.
void run(const char* name, const std::vector<double>& blobs, bool want_grid, bool want_dup, bool fits, bool with_rows, bool expect_n9,
         bool expect_clamp = false) {
  g_scan = name;
  const int B = (int)(blobs.size() / 4);
  std::vector<double> rows;
  if (with_rows)
    for (int b = 0; b < B; ++b) {
      rows.push_back(b % 3 == 1 ? std::numeric_limits<double>::quiet_NaN() : 1.0 + 0.25 * b);
      rows.push_back(b % 3 == 1 ? 0.0 : 0.01 * (b + 1));
    }
  const size_t worst = pk::ml_scan_worst_bytes(B, with_rows);
  unsigned char* st = static_cast<unsigned char*>(std::malloc(worst));
  std::memset(st, 0xA5, worst);
  pk::BlobGrid g;
  int n9 = -1;
  const pk::MlScanLayout filled = pk::ml_scan_fill(st, blobs.data(), B, want_grid, want_dup, &g, &n9);
  check_layout(filled, B, want_grid, g.ncell, n9, false);
  const bool use_grid = want_grid && fits;
  const pk::MlScanLayout l = pk::ml_scan_ranges(st, B, use_grid, g.ncell, n9, with_rows ? rows.data() : nullptr);
  check_layout(l, B, use_grid, g.ncell, n9, with_rows);
  // a scan without range rows (none named, or none finite: the caller passes NULL) has the size it always had
  CHECK(pk::ml_scan_ranges(st, B, use_grid, g.ncell, n9, nullptr).upload_bytes == old_ml(B, use_grid, g.ncell, n9, false).upload);
  CHECK((n9 > 0) == expect_n9);
  for (size_t i = 0; i < CTL; ++i) CHECK(st[i] == 0);
  CHECK(std::memcmp(st + l.blobs, blobs.data(), (size_t)B * 4 * sizeof(double)) == 0);
  const double* dir = reinterpret_cast<const double*>(st + l.dir);
  for (int b = 0; b < B; ++b) {
    const double c = std::cos(blobs[4 * b]), s = std::sin(blobs[4 * b]), len = std::sqrt(c * c + s * s + 0.0 * 0.0);
    CHECK(same_bits(dir[2 * b], c * (1.0 / len)) && same_bits(dir[2 * b + 1], s * (1.0 / len)));
  }
  const double* rng = reinterpret_cast<const double*>(st + l.rng);
  const double* rng_cell = reinterpret_cast<const double*>(st + l.rng_cell);
  if (with_rows) CHECK(std::memcmp(rng, rows.data(), (size_t)B * 2 * sizeof(double)) == 0);
  if (with_rows && !use_grid) CHECK(std::memcmp(rng_cell, rows.data(), (size_t)B * 2 * sizeof(double)) == 0);
  if (use_grid) {  // (given up: the range rows lie where the exact records were, and none of the tables travels)
    CHECK(g.ncell == g.G[0] * g.G[1] * g.G[2] && g.ncell >= 1 && g.ncell <= 16 * 16 * 16);
    for (int k = 0; k < 3; ++k) CHECK(g.G[k] >= 1 && g.G[k] <= 16 && (!expect_clamp || g.G[k] == 16));
    const uint16_t* start = reinterpret_cast<const uint16_t*>(st + filled.start);
    const float* rec32 = reinterpret_cast<const float*>(st + filled.rec32);
    const uint16_t* idx9 = reinterpret_cast<const uint16_t*>(st + filled.idx9);
    const uint16_t* order = reinterpret_cast<const uint16_t*>(st + filled.order);
    const double* exact = reinterpret_cast<const double*>(st + filled.exact);
    // the cell of every blob, and the length of the duplicated lists, longhand
    std::vector<int> cell((size_t)B), count((size_t)g.ncell, 0);
    for (int b = 0; b < B; ++b) {
      int c[3];
      for (int k = 0; k < 3; ++k) {
        const double q = std::floor((blobs[4 * b + 1 + k] - g.lo[k]) * g.inv_h);
        c[k] = q < 0.0 ? 0 : (q > (double)(g.G[k] - 1) ? g.G[k] - 1 : (int)q);
      }
      cell[b] = (c[0] * g.G[1] + c[1]) * g.G[2] + c[2];
      ++count[cell[b]];
    }
    long total = 0;
    for (int r = 0; r < g.G[0]; ++r)
      for (int gg = 0; gg < g.G[1]; ++gg)
        for (int r2 = r - 1; r2 <= r + 1; ++r2)
          for (int g2 = gg - 1; g2 <= gg + 1; ++g2)
            if (r2 >= 0 && r2 < g.G[0] && g2 >= 0 && g2 < g.G[1])
              for (int k = 0; k < g.G[2]; ++k) total += count[(r2 * g.G[1] + g2) * g.G[2] + k];
    if (want_dup) CHECK((n9 > 0) == (total + 3 <= 65535));
    if (n9 > 0) CHECK(n9 % 8 == 0 && total + 3 <= n9 && n9 <= 9 * B + 16);
    for (int c = 0; c < g.ncell; ++c) CHECK(start[c] <= start[c + 1]);
    CHECK(start[0] == 0 && start[g.ncell] == (n9 > 0 ? total : B));
    for (size_t i = (size_t)(g.ncell + 1) * 2; i < filled.rec32 - filled.start; ++i) CHECK(st[filled.start + i] == 0);  // the padding
    std::vector<int> seen((size_t)B, 0);
    for (int t = 0; t < B; ++t) {
      CHECK(order[t] < B && !seen[order[t]]++);
      if (t > 0) CHECK(cell[order[t - 1]] < cell[order[t]] || (cell[order[t - 1]] == cell[order[t]] && order[t - 1] < order[t]));
      const int b = order[t];
      CHECK(rec32[4 * t] == (float)blobs[4 * b + 1] && rec32[4 * t + 1] == (float)blobs[4 * b + 2] &&
            rec32[4 * t + 2] == (float)blobs[4 * b + 3] && rec32[4 * t + 3] == (float)blobs[4 * b]);
      const double* e = exact + 6 * (size_t)t;
      CHECK(same_bits(e[0], blobs[4 * b]) && same_bits(e[1], blobs[4 * b + 1]) && same_bits(e[2], blobs[4 * b + 2]) &&
            same_bits(e[3], blobs[4 * b + 3]) && same_bits(e[4], dir[2 * b]) && same_bits(e[5], dir[2 * b + 1]));
      if (with_rows && use_grid) CHECK(same_bits(rng_cell[2 * t], rows[2 * (size_t)b]) && same_bits(rng_cell[2 * t + 1], rows[2 * (size_t)b + 1]));
    }
    if (n9 == 0)  // `start` = cell offsets into rec32
      for (int c = 0; c < g.ncell; ++c) CHECK(start[c + 1] - start[c] == count[c]);
    for (int i = 0; i < n9; ++i) CHECK(idx9[i] < B);
  }
  // the staged copy handed back (pk_observe_staged on a scan that was discarded): filling a block from its own blobs leaves the same bytes
  std::vector<unsigned char> first(st, st + l.upload_bytes);
  pk::ml_scan_fill(st, reinterpret_cast<const double*>(st + l.blobs), B, want_grid, want_dup, &g, &n9);
  pk::ml_scan_ranges(st, B, use_grid, g.ncell, n9, with_rows ? rows.data() : nullptr);
  CHECK(std::memcmp(first.data(), st, l.upload_bytes) == 0);
  std::free(st);
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
double uniform() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_rng >> 11) / 9007199254740992.0;
}
void blob(std::vector<double>& v, double bearing, double r, double g, double b) {
  v.push_back(bearing);
  v.push_back(r);
  v.push_back(g);
  v.push_back(b);
}

}  // namespace

int main() {
  std::vector<double> one, cell7, wide, rnd, huge;
  blob(one, 0.3, 120.0, 30.0, 200.0);
  for (int i = 0; i < 7; ++i) blob(cell7, -1.0 + 0.3 * i, 100.0 + i, 50.0 + 0.5 * i, 60.0 - i);  // inside one 17.5-wide cell
  for (int i = 0; i < 64; ++i) blob(wide, 0.05 * i - 1.5, 5.5 * i, 5.5 * (63 - i), 5.5 * ((i * 7) % 64));  // 0 .. 346.5: 20 cells an axis
  for (int i = 0; i < 300; ++i) blob(rnd, 6.0 * uniform() - 3.0, 255.0 * uniform(), 255.0 * uniform(), 255.0 * uniform());
  // 7 400 blobs whose duplicated lists pass 65 535 entries: two adjacent cells in the INTERIOR of a 4 x 3 (r, g) grid, each of their
  // blobs listed by nine columns -- 9 x 7 396 entries and the four corner blobs' (two cells on the edge of the grid would be listed
  // by their own two columns alone, 2 B entries)
  blob(huge, 0.0, 0.0, 0.0, 100.0);
  blob(huge, 0.1, 69.0, 0.0, 100.0);
  blob(huge, 0.2, 0.0, 51.0, 100.0);
  blob(huge, 0.3, 69.0, 51.0, 100.0);
  for (int i = 0; i < 7396; ++i) blob(huge, 3.0 * uniform() - 1.5, (i % 2 ? 18.0 : 36.0) + 16.0 * uniform(), 18.0 + 16.0 * uniform(), 100.0 + 10.0 * uniform());
  for (int with_rows = 0; with_rows < 2; ++with_rows) {
    run("B = 1", one, true, true, true, with_rows, true);
    run("B = 7, one cell", cell7, true, true, true, with_rows, true);
    run("B = 7, one cell, no dup", cell7, true, false, true, with_rows, false);
    run("B = 64, clamped to kGridMax", wide, true, true, true, with_rows, true, true);
    run("B = 300, dup", rnd, true, true, true, with_rows, true);
    run("B = 300, no dup", rnd, true, false, true, with_rows, false);
    run("B = 300, tables given up behind the build", rnd, true, true, false, with_rows, true);
    run("B = 7400, lists beyond 65535", huge, true, true, true, with_rows, false);
    run("B = 1, no grid", one, false, true, true, with_rows, false);
    run("B = 300, no grid", rnd, false, false, true, with_rows, false);
    run("B = 7400, no grid", huge, false, true, true, with_rows, false);
  }
  // ---- the known-ids block (upload_known_scan's offsets) and the dense block (dense_observe's), longhand
  g_scan = "known ids / dense";
  for (int B : {0, 1, 7, 300})
    for (int Lp : {8, 515})
      for (int with_ids = 0; with_ids < 2; ++with_ids)
        for (int ranged = 0; ranged < 2; ++ranged) {
          const pk::KnownScanLayout k = pk::known_scan_layout(B, Lp, with_ids != 0, ranged != 0);
          const size_t o_first = CTL + (size_t)B * 4 * sizeof(double), o_next = o_first + (size_t)Lp * sizeof(int32_t);
          const size_t o_ids = o_next + (size_t)B * sizeof(int32_t);
          size_t total = o_ids + (with_ids ? (size_t)B * sizeof(int32_t) : 0), o_rng = 0;
          if (ranged) {
            o_rng = (total + 15) & ~(size_t)15;
            total = o_rng + (size_t)B * 2 * sizeof(double);
          }
          CHECK(k.blobs == CTL && k.first == o_first && k.next == o_next && k.ids == o_ids && k.rng == o_rng && k.upload_bytes == total);
          CHECK(k.rng % 8 == 0);
          const pk::DenseScanLayout d = pk::dense_scan_layout(B);
          const size_t d_dir = CTL + (size_t)B * 4 * sizeof(double), d_ids = d_dir + (size_t)B * 2 * sizeof(double);
          CHECK(d.blobs == CTL && d.dir == d_dir && d.ids == d_ids && d.upload_bytes == ((d_ids + (size_t)B * sizeof(int32_t) + 15) & ~(size_t)15));
        }
  std::printf("scan_block ok\n");
  return 0;
}

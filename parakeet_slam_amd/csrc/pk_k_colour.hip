// The colour table's two maintenance kernels (pk_colour.hpp): k_colour_table builds it, k_colour_rows writes
// the colour rows of map slots back from it.  Neither is on the per-particle path: the first runs once per uploaded map, the second
// over the handful of particles a scan hands to the general kernels, or over the whole buffer when the host wants the rows.
#include <algorithm>

#include "pk_colour.hpp"
#include "pk_device.hpp"

namespace pk {

// One lane per landmark: level 0 is the uploaded block, level k + 1 = colour_block_step(level k).
__global__ void __launch_bounds__(64) k_colour_table(const double* base, double* tab, int depth, int Lp, Noise<double> qt) {
  const int l = blockIdx.x * 64 + threadIdx.x;
  if (l >= Lp) return;
  Sym3<double> C{base[l], base[(size_t)Lp + l], base[2 * (size_t)Lp + l], base[3 * (size_t)Lp + l], base[4 * (size_t)Lp + l],
                 base[5 * (size_t)Lp + l]};
#pragma unroll 1
  for (int k = 0; k < depth; ++k) {
    double* t = tab + ((size_t)k * 6) * Lp + l;
    t[0] = C.a;
    t[(size_t)Lp] = C.b;
    t[2 * (size_t)Lp] = C.c;
    t[3 * (size_t)Lp] = C.d;
    t[4 * (size_t)Lp] = C.e;
    t[5 * (size_t)Lp] = C.f;
    C = colour_block_step(C, qt);
  }
}

void launch_colour_table(hipStream_t s, const double* base_dev, double* tab_dev, int depth, int Lp, const NoiseD& qt) {
  if (depth <= 0 || Lp <= 0) return;
  hipLaunchKernelGGL(k_colour_table, dim3((unsigned)((Lp + 63) / 64)), dim3(64), 0, s, base_dev, tab_dev, depth, Lp,
                     make_noise(qt.q00, qt.rr, qt.rg, qt.rb, qt.gg, qt.gb, qt.bb));
}

struct ColourRowsArgs {
  unsigned char* map;  // the live buffer
  size_t slot_bytes, count_off;
  const int32_t* src;            // with pflag: particle -> source slot
  const unsigned char* pflag;    // [P], or null: every slot
  const unsigned* n_flagged;
  const double* tab;
  int depth, Lp;
  int64_t P;       // slots of the buffer
  int64_t p0, p1;  // the slots (without pflag) or particles (with it) this launch covers
  Noise<double> qt;
};
// A workgroup per slot and turn.  Several flagged copies of one ancestor write the same values into the same source slot.
__global__ void __launch_bounds__(256) k_colour_rows(ColourRowsArgs a) {
  if (a.pflag && *a.n_flagged == 0u) return;  // the usual scan: nobody was handed on
  for (int64_t p = a.p0 + blockIdx.x; p < a.p1; p += gridDim.x) {
    int64_t sl = p;
    if (a.pflag) {
      if (a.pflag[p] == 0) continue;  // workgroup-uniform
      sl = a.src[p];
      if (sl < 0 || sl >= a.P) continue;  // (a record of another shard's: never in table mode)
    }
    unsigned char* slot = a.map + (size_t)sl * a.slot_bytes;
    double* f = reinterpret_cast<double*>(slot);
    const int* cnt = reinterpret_cast<const int*>(slot + a.count_off);
    for (int l = threadIdx.x; l < a.Lp; l += 256) {
      const Sym3<double> C = colour_block_at(a.tab, a.depth, a.Lp, l, colour_level(cnt[l]), a.qt);
      f[(size_t)F_CRR * a.Lp + l] = C.a;
      f[(size_t)F_CRG * a.Lp + l] = C.b;
      f[(size_t)F_CRB * a.Lp + l] = C.c;
      f[(size_t)F_CGG * a.Lp + l] = C.d;
      f[(size_t)F_CGB * a.Lp + l] = C.e;
      f[(size_t)F_CBB * a.Lp + l] = C.f;
    }
  }
}

void launch_colour_rows(hipStream_t s, DeviceState& d, const ColourTable& ct, const NoiseD& qt, const ParticleRange& range,
                        const unsigned char* pflag_dev, const unsigned* n_flagged_dev) {
  const int64_t p0 = range.p0, p1 = range.end(d.P);
  if (!ct.tab || d.P == 0 || p0 < 0 || p1 > d.P || p0 >= p1) return;
  ColourRowsArgs a;
  a.map = d.map[d.mcur];
  a.slot_bytes = d.lay.slot_bytes;
  a.count_off = d.lay.count_off;
  a.src = d.src[d.cur];
  a.pflag = pflag_dev;
  a.n_flagged = n_flagged_dev;
  a.tab = ct.tab;
  a.depth = ct.depth;
  a.Lp = d.lay.Lp;
  a.P = d.P;
  a.p0 = p0;
  a.p1 = p1;
  a.qt = make_noise(qt.q00, qt.rr, qt.rg, qt.rb, qt.gg, qt.gb, qt.bb);
  const int64_t grid = std::min<int64_t>(p1 - p0, 4 * (int64_t)device_cu_count());
  hipLaunchKernelGGL(k_colour_rows, dim3((unsigned)grid), dim3(256), 0, s, a);
}

// Is any landmark of any slot of the live buffer off level 0?  (pk_set_measurement_noise: a new Qt before any update leaves the mode
// on, the table is built afresh.)  A full pass over the counts of the buffer, P L 4 B: not for a call of the step.  A workgroup per
// slot and turn; *any_dev is set, never cleared here.
__global__ void __launch_bounds__(256) k_colour_counts_any(const unsigned char* map, size_t slot_bytes, size_t count_off, int L, int64_t P,
                                                           unsigned* any_dev) {
  bool any = false;
  for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {
    const int* cnt = reinterpret_cast<const int*>(map + (size_t)p * slot_bytes + count_off);
    for (int l = threadIdx.x; l < L; l += 256) any |= cnt[l] != 0;
  }
  if (any) atomicOr(any_dev, 1u);
}

void launch_colour_counts_any(hipStream_t s, DeviceState& d, unsigned* any_dev) {
  if (d.P <= 0 || d.lay.L <= 0) return;
  const int64_t grid = std::min<int64_t>(d.P, 4 * (int64_t)device_cu_count());
  hipLaunchKernelGGL(k_colour_counts_any, dim3((unsigned)grid), dim3(256), 0, s, d.map[d.mcur], d.lay.slot_bytes, d.lay.count_off, d.lay.L,
                     d.P, any_dev);
}

}  // namespace pk

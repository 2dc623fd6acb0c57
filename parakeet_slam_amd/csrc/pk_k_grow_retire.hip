// Growing maps that also shrink (pk_grow_retire): behind k_new_landmarks of every scan, per particle,
//   1. the spare slots the last pass knew: count word changed -> seen = word, idle = 0; else idle += 1 (saturating)
//   2. slots and readings new since the last pass (or written by pk_grow_upload): seen = word, idle = 0; stamp = t
//   3. A > 0: the longest PREFIX of the ring whose stamps are A scans old or older goes (the ring is filled in time order), the rest
//      moves down to index 0
//   4. M > 0: slots whose seen word carries the potential bit and that were idle for M passes go; the survivors move down in order with
//      their 14 rows, count word, slot id, seen and idle; the vacated slots return to the state of a spare slot that never held anything
//   5. covered_readings = readings stored, covered_slots = slots in use
// (tests/grow_retire_reference.py is the same in plain Python.)  The reference has no counterpart: its hypothesis_set only grows.
//
// Hand-written gfx950 (CDNA4, wave64), one wave per particle and four waves per workgroup as in k_new_landmarks: lane j is spare slot
// j (S beyond 64: turns of 64, ascending).  Nothing in k_grow_retire does float arithmetic.
//
// A field of view (pk_grow_view; DESIGN.md section 9, "A field of view for retirement"): k_grow_retire_view is the same body with
// steps 1 and 4 replaced by
//   1'. ... else idle += 1 (saturating) ONLY where the slot's position mean lies in the sensor's field at the particle's live pose
//   4'. M > 0: potential and idle >= M; C > 0: promoted (no potential bit in the seen word) and idle >= C
// and four int64 counters written with integer atomics, once per wave from ballots.  retire_in_view is its only float arithmetic.
#include "pk_device.hpp"

namespace pk {

// What every move below rests on.  A survivor's destination is never above its source, and a turn's destinations lie below every
// source of the turns after it (turn T writes below 64 (T + 1), turn T + 1 reads from 64 (T + 1) on): a turn can only overwrite
// sources of ITS OWN loads.  Those are held in registers across this point: the wave's lanes run in lockstep, a store's data
// depends on the turn's loads, so the wave has waited for all of them (vmcnt) before it issues the first store.  The call keeps
// the compiler from moving memory operations across it.
__device__ __forceinline__ void retire_loads_before_stores() { __builtin_amdgcn_wave_barrier(); }

// Is the point (mx, my) inside the field v of a sensor at (px, py) heading along (ch, sn)?  Float64, operation by operation (no
// contraction into fused multiply-adds: tests/grow_view_reference.py evaluates the same expressions in the same order; sincos and
// pk_atan2 are within an ulp or two of the host's).  A NaN anywhere fails a comparison: not in view.
#pragma clang fp contract(off)
__device__ __forceinline__ bool retire_in_view(const RetireView& v, double px, double py, double sn, double ch, double mx, double my) {
  const double dx = mx - px, dy = my - py;
  const double q = dx * dx + dy * dy;
  const double a = dx * ch + dy * sn;
  const double c = dy * ch - dx * sn;
  return q > 0.0 && q >= v.rmin2 && q <= v.rmax2 && fabs(pk_atan2(c, a)) <= v.half_fov;
}
#pragma clang fp contract(on)

// step 4 / 4': does a slot with this seen word and idle count go
template <bool kView>
__device__ __forceinline__ bool retire_goes(int32_t sn, int32_t id, int M, int C) {
  if constexpr (kView) {
    return (sn & kPotentialBit) ? (M > 0 && id >= M) : (C > 0 && id >= C);
  } else {
    return M > 0 && (sn & kPotentialBit) && id >= M;
  }
}

template <bool kView>
__device__ __forceinline__ void grow_retire_body(const GrowState& g, const RetireState& r, const RetireView& v, const double* __restrict__ x,
                                                 const double* __restrict__ y, const double* __restrict__ h, unsigned char* map,
                                                 size_t slot_bytes, size_t count_off, int Lp, int64_t P) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t p = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
  if (p >= P) return;  // wave-uniform
  const int c = g.cur;
  int32_t* cnt = g.cnt[c] + 4 * p;
  int32_t* rc = r.cnt[c] + 4 * p;
  double* ring = g.hyp[c] + (size_t)p * g.R * 8;
  uint32_t* scan = r.scan[c] + (size_t)p * g.R;
  int32_t* sid = g.slot_id[c] + (size_t)p * g.S;
  int32_t* seen = r.seen[c] + (size_t)p * g.S;
  int32_t* idle = r.idle[c] + (size_t)p * g.S;
  // spare slot j is landmark L0 + j: column j of these
  double* f = reinterpret_cast<double*>(map + (size_t)p * slot_bytes) + g.L0;
  int32_t* fc = reinterpret_cast<int32_t*>(map + (size_t)p * slot_bytes + count_off) + g.L0;
  int n = cnt[0], used = cnt[1];  // what k_new_landmarks has just written
  n = n < 0 ? 0 : n > g.R ? g.R : n;
  used = used < 0 ? 0 : used > g.S ? g.S : used;
  int cr = rc[0], cs = rc[1];
  cr = cr < 0 ? 0 : cr > n ? n : cr;
  cs = cs < 0 ? 0 : cs > used ? used : cs;
  const uint32_t t = r.t, A = (uint32_t)r.A;
  const int M = r.M, C = kView ? v.C : 0;
  double px = 0.0, py = 0.0, psn = 0.0, pch = 1.0;  // the particle's live pose, read once per wave
  if constexpr (kView) {
    px = x[p];
    py = y[p];
    sincos(h[p], &psn, &pch);
  }

  // 1, 2 (slots): three words per slot in use (1': and the two mean rows of an unchanged slot the pass knew)
  int m = 0;                                     // slots to retire
  int n_same = 0, n_view = 0, n_pot = 0;         // kView: unchanged slots the pass knew, those in view, potential ones among m
  for (int j0 = 0; j0 < used; j0 += kWave) {
    const int j = j0 + lane;
    bool gone = false, same = false, view = false, pot = false;
    if (j < used) {
      const int32_t w = fc[j];
      int32_t sn = seen[j], id = idle[j];
      if (j >= cs || w != sn) {
        sn = w;
        id = 0;
      } else if constexpr (kView) {
        same = true;
        view = retire_in_view(v, px, py, psn, pch, f[(size_t)F_MX * Lp + j], f[(size_t)F_MY * Lp + j]);
        if (view && id != INT_MAX) ++id;
      } else if (id != INT_MAX) {
        ++id;
      }
      seen[j] = sn;
      idle[j] = id;
      gone = retire_goes<kView>(sn, id, M, C);
      pot = gone && (sn & kPotentialBit);
    }
    m += __popcll(__ballot(gone));
    if constexpr (kView) {
      n_same += __popcll(__ballot(same));
      n_view += __popcll(__ballot(view));
      n_pot += __popcll(__ballot(pot));
    }
  }
  if constexpr (kView) {  // (integer atomics, one lane per wave; a zero is not sent)
    if (lane == 0) {
      if (n_same) atomicAdd(v.stats + 0, (unsigned long long)n_same);
      if (n_view) atomicAdd(v.stats + 1, (unsigned long long)n_view);
      if (n_pot) atomicAdd(v.stats + 2, (unsigned long long)n_pot);
      if (m - n_pot) atomicAdd(v.stats + 3, (unsigned long long)(m - n_pot));
    }
  }
  // 3: the stale prefix.  Readings from cr on are this scan's (stamp t, age 0): never stale
  int k = 0;
  if (A > 0 && cr > 0 && t - scan[0] >= A) {  // wave-uniform: the first stamp decides whether anything goes
    for (int q0 = 0; q0 < cr; q0 += kWave) {
      const int q = q0 + lane;
      const unsigned long long fresh = ~__ballot(q < cr && t - scan[q] >= A);  // (the subtraction wraps with t)
      if (fresh != 0ull) {
        k = q0 + __builtin_ctzll(fresh);
        break;
      }
      k = q0 + kWave;
    }
    k = k > cr ? cr : k;
  }
  if (k == 0) {  // 2 (readings)
    for (int q = cr + lane; q < n; q += kWave) scan[q] = t;
  }
  if (k == 0 && m == 0) {  // the usual particle: nothing goes, the 14 rows were not touched
    if (lane == 0) {
      rc[0] = n;
      rc[1] = used;
    }
    return;
  }
  if (k > 0) {
    const int left = n - k;
    for (int q0 = 0; q0 < left; q0 += kWave) {  // the stamps move down (this scan's are written here: t)
      const int q = q0 + lane;
      uint32_t v = t;
      if (q < left && q + k < cr) v = scan[q + k];
      retire_loads_before_stores();
      if (q < left) scan[q] = v;
    }
    const int nd = 8 * left;
    const double* src = ring + 8 * (size_t)k;
    for (int i0 = 0; i0 < nd; i0 += 4 * kWave) {  // the readings: four rows of 64 doubles a turn
      const int i = i0 + lane;
      double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
      if (i < nd) v0 = src[i];
      if (i + kWave < nd) v1 = src[i + kWave];
      if (i + 2 * kWave < nd) v2 = src[i + 2 * kWave];
      if (i + 3 * kWave < nd) v3 = src[i + 3 * kWave];
      retire_loads_before_stores();
      if (i < nd) ring[i] = v0;
      if (i + kWave < nd) ring[i + kWave] = v1;
      if (i + 2 * kWave < nd) ring[i + 2 * kWave] = v2;
      if (i + 3 * kWave < nd) ring[i + 3 * kWave] = v3;
    }
    n = left;
  }
  if (m > 0) {
    int base = 0;  // survivors of the turns before this one
    for (int j0 = 0; j0 < used; j0 += kWave) {
      const int j = j0 + lane;
      int32_t sn = 0, id = 0;
      if (j < used) {  // (this lane wrote them above)
        sn = seen[j];
        id = idle[j];
      }
      const bool keep = j < used && !retire_goes<kView>(sn, id, M, C);
      const unsigned long long vote = __ballot(keep);
      const int dst = base + __popcll(vote & ((1ull << lane) - 1ull));
      const bool move = keep && dst != j;
      double row[F_COUNT_FIELDS];
      int32_t fid = 0;
      if (move) {
#pragma unroll
        for (int q = 0; q < F_COUNT_FIELDS; ++q) row[q] = f[(size_t)q * Lp + j];
        fid = sid[j];
      }
      retire_loads_before_stores();
      if (move) {
#pragma unroll
        for (int q = 0; q < F_COUNT_FIELDS; ++q) f[(size_t)q * Lp + dst] = row[q];
        fc[dst] = sn;  // (the count word: step 1 left it in seen)
        sid[dst] = fid;
        seen[dst] = sn;
        idle[dst] = id;
      }
      base += __popcll(vote);
    }
    retire_loads_before_stores();
    for (int j = base + lane; j < used; j += kWave) {  // the vacated slots: what an empty spare slot is uploaded as
      const double empty = 0x1p100;                   // (a colour no blob can gate against)
      f[(size_t)F_MX * Lp + j] = 0.0;
      f[(size_t)F_MY * Lp + j] = 0.0;
      f[(size_t)F_MR * Lp + j] = empty;
      f[(size_t)F_MG * Lp + j] = empty;
      f[(size_t)F_MB * Lp + j] = empty;
      f[(size_t)F_PXX * Lp + j] = 1.0;
      f[(size_t)F_PXY * Lp + j] = 0.0;
      f[(size_t)F_PYY * Lp + j] = 1.0;
      f[(size_t)F_CRR * Lp + j] = 1.0;
      f[(size_t)F_CRG * Lp + j] = 0.0;
      f[(size_t)F_CRB * Lp + j] = 0.0;
      f[(size_t)F_CGG * Lp + j] = 1.0;
      f[(size_t)F_CGB * Lp + j] = 0.0;
      f[(size_t)F_CBB * Lp + j] = 1.0;
      fc[j] = 0;
    }
    used = base;
  }
  if (lane == 0) {
    cnt[0] = n;
    cnt[1] = used;
    rc[0] = n;  // 5
    rc[1] = used;
    rc[2] += k;
    rc[3] += m;
  }
}

__global__ void __launch_bounds__(256) k_grow_retire(GrowState g, RetireState r, unsigned char* map, size_t slot_bytes, size_t count_off,
                                                     int Lp, int64_t P) {
  grow_retire_body<false>(g, r, RetireView(), nullptr, nullptr, nullptr, map, slot_bytes, count_off, Lp, P);
}
// pk_grow_view: rules 1' and 4' at the particles' live poses
__global__ void __launch_bounds__(256) k_grow_retire_view(GrowState g, RetireState r, RetireView v, const double* __restrict__ x,
                                                          const double* __restrict__ y, const double* __restrict__ h, unsigned char* map,
                                                          size_t slot_bytes, size_t count_off, int Lp, int64_t P) {
  grow_retire_body<true>(g, r, v, x, y, h, map, slot_bytes, count_off, Lp, P);
}

void launch_grow_retire(hipStream_t s, DeviceState& d, const GrowState& g, const RetireState& r, const RetireView& v) {
  if (d.P == 0) return;
  const dim3 grid((unsigned)((d.P + 3) / 4)), block(256);
  if (v.on)
    hipLaunchKernelGGL(k_grow_retire_view, grid, block, 0, s, g, r, v, d.x[d.cur], d.y[d.cur], d.h[d.cur], d.map[d.mcur], d.lay.slot_bytes,
                       d.lay.count_off, d.lay.Lp, d.P);
  else
    hipLaunchKernelGGL(k_grow_retire, grid, block, 0, s, g, r, d.map[d.mcur], d.lay.slot_bytes, d.lay.count_off, d.lay.Lp, d.P);
}

// the clocks follow the particles wherever k_grow_gather takes the bookkeeping (launched before g.cur flips): slot k takes ancestor
// anc[k]'s counters and the rows in use
__global__ void __launch_bounds__(64) k_retire_gather(GrowState g, RetireState r, const int32_t* __restrict__ anc, int64_t P) {
  const int64_t k = blockIdx.x;
  if (k >= P) return;
  const int c = g.cur, nx = c ^ 1;
  const int64_t a = anc[k];
  if (a < 0 || a >= P) {  // (a record of another rank carries no clocks -- refused while retirement is on: never taken)
    if (threadIdx.x < 4) r.cnt[nx][4 * k + threadIdx.x] = 0;
    return;
  }
  int n = g.cnt[c][4 * a], used = g.cnt[c][4 * a + 1];
  n = n < 0 ? 0 : n > g.R ? g.R : n;
  used = used < 0 ? 0 : used > g.S ? g.S : used;
  if (threadIdx.x < 4) r.cnt[nx][4 * k + threadIdx.x] = r.cnt[c][4 * a + threadIdx.x];
  const uint32_t* ss = r.scan[c] + (size_t)a * g.R;
  uint32_t* ds = r.scan[nx] + (size_t)k * g.R;
  for (int i = threadIdx.x; i < n; i += blockDim.x) ds[i] = ss[i];
  const int32_t *se = r.seen[c] + (size_t)a * g.S, *si = r.idle[c] + (size_t)a * g.S;
  int32_t *de = r.seen[nx] + (size_t)k * g.S, *di = r.idle[nx] + (size_t)k * g.S;
  for (int i = threadIdx.x; i < used; i += blockDim.x) {
    de[i] = se[i];
    di[i] = si[i];
  }
}
void launch_retire_gather(hipStream_t s, const GrowState& g, const RetireState& r, const int32_t* anc_dev, int64_t P) {
  if (P == 0) return;
  hipLaunchKernelGGL(k_retire_gather, dim3((unsigned)P), dim3(64), 0, s, g, r, anc_dev, P);
}

}  // namespace pk

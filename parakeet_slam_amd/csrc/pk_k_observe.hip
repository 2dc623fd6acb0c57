// K3 EKF update + log-weight: the general kernel (supplied ids, or per-particle ids from the
// association kernel) and the loop-free single-sighting kernel.  The maximum-likelihood variants
// that settle the association themselves are in pk_k_observe_ml.hip.
//
// Hand-written gfx950 (CDNA4, wave64) kernels of the FastSLAM particle update; see DESIGN.md
// section 4.  No MFMA: the algebra is 2x2 / 3x3 and register resident (pk_math.hpp).
#include "pk_device.hpp"
#include "pk_launch.hpp"
#include "pk_range_math.hpp"

namespace pk {

// The updated map rows are written with non-temporal stores: nothing reads them before the next
// step, and keeping them out of L2 / Infinity Cache leaves the caches to the read stream (the
// duplicates a resample leaves read shared source slots): the supplied-ids kernel went from 0.190
// to 0.171 ms at 10 000 x 500 with nothing else changed.
typedef double d2v __attribute__((ext_vector_type(2)));
typedef int i2v __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ K3 observe (EKF + weight)
struct ObserveArgs {
  SlotSource ss;
  unsigned char* map_dst;
  size_t slot_bytes, count_off;
  int32_t* src;  // in: slot of particle p in map_src; out: identity
  const double *x, *y;
  const double* h;       // the bearing model's kernels alone read the headings
  double* logw;
  const double* blobs;   // B x 4
  const double* blobdir; // ML: B x 2 unit ray directions (closest_point :510)
  const double* rng;     // the range instances alone: B x 2 (range, variance) in scan order, NaN range = none (pk_scan_ranges)
  const int32_t* first;  // KNOWN: [L] first blob matched to landmark l, or -1
  const int32_t* next;   // KNOWN: [B] next blob matched to the same landmark, or -1
  int32_t* ids;          // ML: [P x B]; a tentative id whose probability is 0 is reset to 0
  const unsigned char* immutable;
  int n_unmatched;  // KNOWN: blobs with id 0
  const unsigned char* only_flagged;  // when set: skip particles whose flag is 0 (k_observe_fast did them)
  const unsigned* n_flagged;          // with only_flagged: number of flagged particles (0 -> nothing to do)
  int reset;                          // 1: the weight restarts from 1 (prkt_core_v2.py:73) instead of accumulating
  unsigned long long* gmax_key;       // running max of the new log-weights (double_to_key), or NULL
  int L, Lp, B;
  int64_t P;
  Noise<double> qt;
};

// (match_is_positive and load_blob: pk_device.hpp -- k_propose settles with them too)
// All blobs matched to landmark l, in scan order (prkt_core_v2.py:88).
// ML: the ids are tentative.  Association saw the state BEFORE any update (:84), so first
// settle every blob of the chain against the untouched state (s_ids[b] = 0 drops it), then
// apply the surviving ones sequentially.
// MODEL = kModelBearing: (sh, ch, sn) = the particle's heading with its cosine and sine (one sincos per particle).
// SETTLED (k_observe_proposed): the ids are final -- k_propose settled them at the predicted pose; there is no second settling.
// RANGE (k_observe_range, bearing model): a blob with a finite range is settled and applied as a range-bearing measurement
// (pk_range_math.hpp); one without takes the bearing model's path, decided blob by blob.  Each lane walks its OWN landmark's chain,
// so the choice is per lane: a wave whose lanes hold ranged and unranged blobs at the same chain position runs both paths in turn.
// SETTLED and RANGE together (k_observe_proposed_range): k_propose_range settled the ids; a ranged blob takes ekf_update_range.
template <bool KNOWN, int MODEL = kModelReference, bool SETTLED = false, bool RANGE = false>
__device__ __forceinline__ double apply_blobs(Landmark<double>& lm, int l, double sx, double sy,
                                              const ObserveArgs& a, const int32_t* first,
                                              const int32_t* next, int32_t* s_ids, int32_t* gid, double sh = 0.0,
                                              double ch = 1.0, double sn = 0.0) {
  double acc = 0.0;
  const int b0 = first[l];
  if (b0 < 0) return acc;
  const bool imm = a.immutable[l] != 0;
  const double pse = pk_atan2(lm.my - sy, lm.mx - sx);
  if (!KNOWN && !SETTLED) {
    for (int b = b0; b >= 0; b = next[b]) {
      const BlobT<double> z = load_blob(a.blobs, b);
      double2 dir = *reinterpret_cast<const double2*>(a.blobdir + 2 * (size_t)b);
      if constexpr (MODEL == kModelBearing) rotate_ray(dir.x, dir.y, ch, sn, dir.x, dir.y);
      bool positive;
      if constexpr (RANGE) {
        const BlobRange r = load_range(a.rng, b);
        positive = r.has() ? match_is_positive_range(lm, sx, sy, z, dir.x, dir.y, r.rho, r.qr, a.qt.q00)
                           : match_is_positive<MODEL>(lm, sx, sy, pse, z, dir.x, dir.y);
      } else {
        positive = match_is_positive<MODEL>(lm, sx, sy, pse, z, dir.x, dir.y);
      }
      if (!positive) {
        s_ids[b] = 0;
        gid[b] = 0;
      }
    }
  }
  bool fresh = true;  // lm still equals the state pse was computed from
  for (int b = b0; b >= 0; b = next[b]) {
    if (!KNOWN && s_ids[b] == 0) {
      acc += Consts<double>::log_no_match;  // unseen feature: weight *= 0.1 (:94-95)
      continue;
    }
    const BlobT<double> z = load_blob(a.blobs, b);
    if constexpr (RANGE) {
      const BlobRange r = load_range(a.rng, b);
      if (r.has()) {
        acc += ekf_update_range(lm, sx, sy, sh, z, r.rho, r.qr, a.qt, imm, fresh ? &pse : (const double*)nullptr);
        fresh = imm;
        continue;
      }
    }
    if constexpr (MODEL == kModelBearing)
      acc += ekf_update<double, true, MODEL>(lm, sx, sy, z, a.qt, imm, (EkfAux<double>*)nullptr, fresh ? &pse : (const double*)nullptr,
                                             (double*)nullptr, sh);
    else
      acc += ekf_update(lm, sx, sy, z, a.qt, imm, (EkfAux<double>*)nullptr, fresh ? &pse : (const double*)nullptr);
    fresh = imm;
  }
  return acc;
}

// The body of k_observe and of k_observe_bearing, its instance for the bearing model (a kernel of its own: the reference model's
// kernels keep their names and what they compute).  PROPOSED: k_observe_proposed, behind k_propose -- the ids are final and the
// weight increment is dlogw[p].
template <bool KNOWN, int NV, int MODEL, bool PROPOSED = false, bool RANGE = false>
__device__ __forceinline__ void observe_body(const ObserveArgs& a, const double* dlogw = nullptr) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double red[kObsThreads / kWave];
  if (a.only_flagged && *a.n_flagged == 0u) return;  // workgroup-uniform: nobody was handed on
  // One workgroup per particle -- or, behind a one-pass kernel (only_flagged), a few thousand workgroups that walk the flags: the
  // stand-by launch of every step then costs 2 us instead of the 22 us that 100 000 workgroups returning at once take to dispatch.
  for (int64_t p = blockIdx.x; p < a.P; p += gridDim.x) {
  if (a.only_flagged && a.only_flagged[p] != 1) continue;  // workgroup-uniform
  const int tid = threadIdx.x;
  const int32_t sp = a.src[p];
  const unsigned char* sslot = a.ss.at(sp);
  unsigned char* dslot = a.map_dst + (size_t)p * a.slot_bytes;
  const double* sf = reinterpret_cast<const double*>(sslot);
  double* df = reinterpret_cast<double*>(dslot);
  const int* sc = reinterpret_cast<const int*>(sslot + a.count_off);
  int* dc = reinterpret_cast<int*>(dslot + a.count_off);
  const double sx = a.x[p], sy = a.y[p];
  double sh = 0.0, ch = 1.0, sn = 0.0;
  if constexpr (MODEL == kModelBearing) {
    sh = a.h[p];
    sincos(sh, &sn, &ch);
  }
  const int Lp = a.Lp;

  const int32_t* first = a.first;
  const int32_t* next = a.next;
  int n_unmatched = a.n_unmatched;
  int32_t* gid_mut = KNOWN ? nullptr : a.ids + (size_t)p * a.B;
  int32_t* s_ids_mut = nullptr;
  if (!KNOWN) {
    // Build the per-particle landmark -> blob chains in LDS from this particle's ids.
    // Blobs are applied in scan order (prkt_core_v2.py:88): first[l] is the lowest blob
    // index matched to l, next[b] the following blob matched to the same landmark.
    int32_t* s_first = reinterpret_cast<int32_t*>(smem);
    int32_t* s_next = s_first + Lp;
    int32_t* s_ids = s_next + a.B;
    s_ids_mut = s_ids;
    const int32_t* gid = gid_mut;
    for (int l = tid; l < Lp; l += blockDim.x) s_first[l] = INT_MAX;
    for (int b = tid; b < a.B; b += blockDim.x) {
      s_ids[b] = gid[b];
      s_next[b] = -1;
    }
    __syncthreads();
    int cnt0 = 0;
    for (int b = tid; b < a.B; b += blockDim.x) {
      int id = s_ids[b];
      if (id > 0)
        atomicMin(&s_first[id - 1], b);
      else
        ++cnt0;
    }
    __syncthreads();
    for (int b = tid; b < a.B; b += blockDim.x) {
      int id = s_ids[b];
      if (id > 0 && s_first[id - 1] != b) {  // not the first sighting: link from my predecessor
        int q = b - 1;
        while (s_ids[q] != id) --q;  // terminates: first[id-1] < b has this id
        s_next[q] = b;
      }
    }
    for (int l = tid; l < Lp; l += blockDim.x)
      if (s_first[l] == INT_MAX) s_first[l] = -1;
    // number of unmatched blobs of this particle (weight *= 0.1 each, :94-95)
    double c = block_sum<kObsThreads / kWave>((double)cnt0, red);
    n_unmatched = (int)c;
    __syncthreads();
    first = s_first;
    next = s_next;
  }

  double acc = 0.0;
  if (NV == 2) {
    // two adjacent landmarks per lane: 16-byte loads/stores, 14 rows x 1 KiB per wave instruction
    for (int l0 = 2 * tid; l0 < Lp; l0 += 2 * kObsThreads) {
      double2 v[F_COUNT_FIELDS];
#pragma unroll
      for (int f = 0; f < F_COUNT_FIELDS; ++f) v[f] = *reinterpret_cast<const double2*>(sf + (size_t)f * Lp + l0);
      int2 c = *reinterpret_cast<const int2*>(sc + l0);
      Landmark<double> A{v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x,
                         v[8].x, v[9].x, v[10].x, v[11].x, v[12].x, v[13].x, c.x};
      Landmark<double> Bq{v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y,
                          v[8].y, v[9].y, v[10].y, v[11].y, v[12].y, v[13].y, c.y};
      if (l0 < a.L) acc += apply_blobs<KNOWN, MODEL, PROPOSED, RANGE>(A, l0, sx, sy, a, first, next, s_ids_mut, gid_mut, sh, ch, sn);
      if (l0 + 1 < a.L) acc += apply_blobs<KNOWN, MODEL, PROPOSED, RANGE>(Bq, l0 + 1, sx, sy, a, first, next, s_ids_mut, gid_mut, sh, ch, sn);
      __builtin_nontemporal_store(d2v{A.mx, Bq.mx}, reinterpret_cast<d2v*>(df + (size_t)F_MX * Lp + l0));
      __builtin_nontemporal_store(d2v{A.my, Bq.my}, reinterpret_cast<d2v*>(df + (size_t)F_MY * Lp + l0));
      __builtin_nontemporal_store(d2v{A.mr, Bq.mr}, reinterpret_cast<d2v*>(df + (size_t)F_MR * Lp + l0));
      __builtin_nontemporal_store(d2v{A.mg, Bq.mg}, reinterpret_cast<d2v*>(df + (size_t)F_MG * Lp + l0));
      __builtin_nontemporal_store(d2v{A.mb, Bq.mb}, reinterpret_cast<d2v*>(df + (size_t)F_MB * Lp + l0));
      __builtin_nontemporal_store(d2v{A.pxx, Bq.pxx}, reinterpret_cast<d2v*>(df + (size_t)F_PXX * Lp + l0));
      __builtin_nontemporal_store(d2v{A.pxy, Bq.pxy}, reinterpret_cast<d2v*>(df + (size_t)F_PXY * Lp + l0));
      __builtin_nontemporal_store(d2v{A.pyy, Bq.pyy}, reinterpret_cast<d2v*>(df + (size_t)F_PYY * Lp + l0));
      __builtin_nontemporal_store(d2v{A.crr, Bq.crr}, reinterpret_cast<d2v*>(df + (size_t)F_CRR * Lp + l0));
      __builtin_nontemporal_store(d2v{A.crg, Bq.crg}, reinterpret_cast<d2v*>(df + (size_t)F_CRG * Lp + l0));
      __builtin_nontemporal_store(d2v{A.crb, Bq.crb}, reinterpret_cast<d2v*>(df + (size_t)F_CRB * Lp + l0));
      __builtin_nontemporal_store(d2v{A.cgg, Bq.cgg}, reinterpret_cast<d2v*>(df + (size_t)F_CGG * Lp + l0));
      __builtin_nontemporal_store(d2v{A.cgb, Bq.cgb}, reinterpret_cast<d2v*>(df + (size_t)F_CGB * Lp + l0));
      __builtin_nontemporal_store(d2v{A.cbb, Bq.cbb}, reinterpret_cast<d2v*>(df + (size_t)F_CBB * Lp + l0));
      __builtin_nontemporal_store(i2v{A.count, Bq.count}, reinterpret_cast<i2v*>(dc + l0));
    }
  } else {
    // one landmark per lane: half the registers, twice the waves in flight
    for (int l = tid; l < Lp; l += kObsThreads) {
      Landmark<double> A = load_landmark(sf, sc, Lp, l);
      if (l < a.L) acc += apply_blobs<KNOWN, MODEL, PROPOSED, RANGE>(A, l, sx, sy, a, first, next, s_ids_mut, gid_mut, sh, ch, sn);
      __builtin_nontemporal_store(A.mx, &df[(size_t)F_MX * Lp + l]);
      __builtin_nontemporal_store(A.my, &df[(size_t)F_MY * Lp + l]);
      __builtin_nontemporal_store(A.mr, &df[(size_t)F_MR * Lp + l]);
      __builtin_nontemporal_store(A.mg, &df[(size_t)F_MG * Lp + l]);
      __builtin_nontemporal_store(A.mb, &df[(size_t)F_MB * Lp + l]);
      __builtin_nontemporal_store(A.pxx, &df[(size_t)F_PXX * Lp + l]);
      __builtin_nontemporal_store(A.pxy, &df[(size_t)F_PXY * Lp + l]);
      __builtin_nontemporal_store(A.pyy, &df[(size_t)F_PYY * Lp + l]);
      __builtin_nontemporal_store(A.crr, &df[(size_t)F_CRR * Lp + l]);
      __builtin_nontemporal_store(A.crg, &df[(size_t)F_CRG * Lp + l]);
      __builtin_nontemporal_store(A.crb, &df[(size_t)F_CRB * Lp + l]);
      __builtin_nontemporal_store(A.cgg, &df[(size_t)F_CGG * Lp + l]);
      __builtin_nontemporal_store(A.cgb, &df[(size_t)F_CGB * Lp + l]);
      __builtin_nontemporal_store(A.cbb, &df[(size_t)F_CBB * Lp + l]);
      __builtin_nontemporal_store(A.count, &dc[l]);
    }
  }
  double tot = block_sum<kObsThreads / kWave>(acc, red);
  if (tid == 0) {
    double v;
    if constexpr (PROPOSED)
      v = (a.reset ? 0.0 : a.logw[p]) + dlogw[p];
    else
      v = (a.reset ? 0.0 : a.logw[p]) + tot + (double)n_unmatched * Consts<double>::log_no_match;
    a.logw[p] = v;
    if (a.gmax_key) atomicMax(a.gmax_key + (p & (kGmaxKeys - 1)), double_to_key(v));  // sharded: same-address atomics serialise
    a.src[p] = (int32_t)p;
  }
  __syncthreads();  // (the LDS tables and the reduction's scratch are the next particle's)
  }
}

template <bool KNOWN, int NV>
__global__ void __launch_bounds__(kObsThreads) k_observe(ObserveArgs a) {
  observe_body<KNOWN, NV, kModelReference>(a);
}
template <bool KNOWN, int NV>
__global__ void __launch_bounds__(kObsThreads) k_observe_bearing(ObserveArgs a) {
  observe_body<KNOWN, NV, kModelBearing>(a);
}
// ... and its instances for scans that hold at least one ranged blob (pk_scan_ranges)
template <bool KNOWN, int NV>
__global__ void __launch_bounds__(kObsThreads) k_observe_range(ObserveArgs a) {
  observe_body<KNOWN, NV, kModelBearing, false, true>(a);
}
template <bool KNOWN, int NV>
__global__ void __launch_bounds__(kObsThreads) k_observe_proposed(ObserveArgs a, const double* dlogw) {
  observe_body<KNOWN, NV, kModelBearing, true>(a, dlogw);
}
// ... behind k_propose_range: the settled ids are final, a ranged blob updates its landmark with ekf_update_range
template <bool KNOWN, int NV>
__global__ void __launch_bounds__(kObsThreads) k_observe_proposed_range(ObserveArgs a, const double* dlogw) {
  observe_body<KNOWN, NV, kModelBearing, true, true>(a, dlogw);
}


// ------------------------------------------------------------------ K3 (known ids, one sighting per landmark)
// The common supplied-ids scan on a map of <= 1024 landmarks: no landmark is matched by more than
// one blob.  One landmark per lane and no loop at all: straight-line code that the compiler fits
// in 96 VGPRs (the looped k_observe needs 163-194), so 16-20 waves per CU stream the map instead
// of 8-12.  One workgroup of THREADS >= Lp lanes per particle.
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_observe_single(ObserveArgs a) {
  __shared__ double red[THREADS / kWave];
  const int64_t p = blockIdx.x;
  const int l = threadIdx.x;
  const unsigned char* sslot = a.ss.at(a.src[p]);
  unsigned char* dslot = a.map_dst + (size_t)p * a.slot_bytes;
  const double* sf = reinterpret_cast<const double*>(sslot);
  double* df = reinterpret_cast<double*>(dslot);
  const int* sc = reinterpret_cast<const int*>(sslot + a.count_off);
  int* dc = reinterpret_cast<int*>(dslot + a.count_off);
  const double sx = a.x[p], sy = a.y[p];
  const int Lp = a.Lp;
  double acc = 0.0;
  if (l < Lp) {
    Landmark<double> A = load_landmark(sf, sc, Lp, l);
    if (l < a.L) {
      const int b = a.first[l];
      if (b >= 0) {
        const BlobT<double> z = load_blob(a.blobs, b);
        acc = ekf_update(A, sx, sy, z, a.qt, a.immutable[l] != 0);
      }
    }
    __builtin_nontemporal_store(A.mx, &df[(size_t)F_MX * Lp + l]);
    __builtin_nontemporal_store(A.my, &df[(size_t)F_MY * Lp + l]);
    __builtin_nontemporal_store(A.mr, &df[(size_t)F_MR * Lp + l]);
    __builtin_nontemporal_store(A.mg, &df[(size_t)F_MG * Lp + l]);
    __builtin_nontemporal_store(A.mb, &df[(size_t)F_MB * Lp + l]);
    __builtin_nontemporal_store(A.pxx, &df[(size_t)F_PXX * Lp + l]);
    __builtin_nontemporal_store(A.pxy, &df[(size_t)F_PXY * Lp + l]);
    __builtin_nontemporal_store(A.pyy, &df[(size_t)F_PYY * Lp + l]);
    __builtin_nontemporal_store(A.crr, &df[(size_t)F_CRR * Lp + l]);
    __builtin_nontemporal_store(A.crg, &df[(size_t)F_CRG * Lp + l]);
    __builtin_nontemporal_store(A.crb, &df[(size_t)F_CRB * Lp + l]);
    __builtin_nontemporal_store(A.cgg, &df[(size_t)F_CGG * Lp + l]);
    __builtin_nontemporal_store(A.cgb, &df[(size_t)F_CGB * Lp + l]);
    __builtin_nontemporal_store(A.cbb, &df[(size_t)F_CBB * Lp + l]);
    __builtin_nontemporal_store(A.count, &dc[l]);
  }
  const double tot = block_sum<THREADS / kWave>(acc, red);
  if (l == 0) {
    const double v = (a.reset ? 0.0 : a.logw[p]) + tot + (double)a.n_unmatched * Consts<double>::log_no_match;
    a.logw[p] = v;
    if (a.gmax_key) atomicMax(a.gmax_key + (p & (kGmaxKeys - 1)), double_to_key(v));
    a.src[p] = (int32_t)p;
  }
}

int g_observe_nv = 0;  // tuning: 0 = default per variant, 1 / 2 = landmarks per lane

// known.first != NULL: supplied ids (ids_dev NULL); else ids_dev's [P][B]
static void observe_launch(hipStream_t s, DeviceState& d, const ScanTables& scan, const KnownChains& known, int32_t* ids_dev,
                           const NoiseD& qt, const ObserveExtras& ex) {
  if (d.P == 0) return;
  const int B = scan.B;
  ObserveArgs a{};
  fill_state(a, d);
  a.slot_bytes = d.lay.slot_bytes;
  a.blobs = scan.blobs;
  a.blobdir = scan.dir;
  a.rng = ex.rng;
  a.first = known.first;
  a.next = known.next;
  a.ids = ids_dev;
  a.n_unmatched = known.n_unmatched;
  a.only_flagged = ex.only_flagged;
  a.n_flagged = ex.n_flagged;
  a.reset = ex.reset ? 1 : 0;
  a.gmax_key = ex.gmax_key;
  a.B = B;
  a.P = d.P;
  a.qt = device_noise(qt);
  static bool attr_set[kMaxDevices] = {false};  // the instances that build their chains in LDS
  allow_dynamic_lds(attr_set, kMaxDynLds, k_observe_proposed_range<false, 1>, k_observe_proposed<false, 1>, k_observe_range<false, 1>,
                    k_observe_bearing<false, 1>, k_observe<false, 1>, k_observe<false, 2>);
  // (behind a one-pass kernel few particles, if any, are flagged: 4 096 workgroups walk the flags)
  const unsigned grid = (unsigned)(ex.only_flagged && d.P > 4096 ? 4096 : d.P);
  if (ex.dlogw && ex.rng) {  // behind k_propose_range: a proposal step's scan with ranged blobs
    if (ids_dev == nullptr) {
      hipLaunchKernelGGL((k_observe_proposed_range<true, 2>), dim3(grid), dim3(kObsThreads), 0, s, a, ex.dlogw);
    } else {
      const size_t lds = observe_general_lds_bytes(d.lay.Lp, B);  // <= kMaxDynLds: checked by the caller
      hipLaunchKernelGGL((k_observe_proposed_range<false, 1>), dim3(grid), dim3(kObsThreads), lds, s, a, ex.dlogw);
    }
  } else if (ex.dlogw) {  // behind k_propose (bearing model): the same two shapes
    if (ids_dev == nullptr) {
      hipLaunchKernelGGL((k_observe_proposed<true, 2>), dim3(grid), dim3(kObsThreads), 0, s, a, ex.dlogw);
    } else {
      const size_t lds = observe_general_lds_bytes(d.lay.Lp, B);  // <= kMaxDynLds: checked by the caller
      hipLaunchKernelGGL((k_observe_proposed<false, 1>), dim3(grid), dim3(kObsThreads), lds, s, a, ex.dlogw);
    }
  } else if (ex.model == kModelBearing && ex.rng) {  // a scan with ranged blobs: the bearing model's two shapes again
    if (ids_dev == nullptr) {
      hipLaunchKernelGGL((k_observe_range<true, 2>), dim3(grid), dim3(kObsThreads), 0, s, a);
    } else {
      const size_t lds = observe_general_lds_bytes(d.lay.Lp, B);  // <= kMaxDynLds: checked by the caller
      hipLaunchKernelGGL((k_observe_range<false, 1>), dim3(grid), dim3(kObsThreads), lds, s, a);
    }
  } else if (ex.model == kModelBearing) {  // the bearing model: k_observe's two shapes, no loop-free single-sighting kernel
    if (ids_dev == nullptr) {
      hipLaunchKernelGGL((k_observe_bearing<true, 2>), dim3(grid), dim3(kObsThreads), 0, s, a);
    } else {
      const size_t lds = observe_general_lds_bytes(d.lay.Lp, B);  // <= kMaxDynLds: checked by the caller
      hipLaunchKernelGGL((k_observe_bearing<false, 1>), dim3(grid), dim3(kObsThreads), lds, s, a);
    }
  } else if (ids_dev == nullptr && ex.single_sightings && !ex.only_flagged && d.lay.Lp <= 1024 && g_observe_nv == 0) {
    if (d.lay.Lp <= 256)
      hipLaunchKernelGGL((k_observe_single<256>), dim3((unsigned)d.P), dim3(256), 0, s, a);
    else if (d.lay.Lp <= 512)
      hipLaunchKernelGGL((k_observe_single<512>), dim3((unsigned)d.P), dim3(512), 0, s, a);
    else
      hipLaunchKernelGGL((k_observe_single<1024>), dim3((unsigned)d.P), dim3(1024), 0, s, a);
  } else if (ids_dev == nullptr) {
    if (g_observe_nv == 1)
      hipLaunchKernelGGL((k_observe<true, 1>), dim3(grid), dim3(kObsThreads), 0, s, a);
    else
      hipLaunchKernelGGL((k_observe<true, 2>), dim3(grid), dim3(kObsThreads), 0, s, a);
  } else {
    const size_t lds = observe_general_lds_bytes(d.lay.Lp, B);  // <= kMaxDynLds: checked by the caller
    if (g_observe_nv == 2)
      hipLaunchKernelGGL((k_observe<false, 2>), dim3(grid), dim3(kObsThreads), lds, s, a);
    else
      hipLaunchKernelGGL((k_observe<false, 1>), dim3(grid), dim3(kObsThreads), lds, s, a);
  }
  if (ex.flip) {
    d.mcur ^= 1;
    d.alt = nullptr;  // every slot was rewritten into the particle's own map buffer
  }
}
void launch_observe(hipStream_t s, DeviceState& d, const ScanTables& scan, const KnownChains& known, const NoiseD& qt,
                    const ObserveExtras& ex) {
  observe_launch(s, d, scan, known, nullptr, qt, ex);
}
void launch_observe(hipStream_t s, DeviceState& d, const ScanTables& scan, int32_t* ids_dev, const NoiseD& qt, const ObserveExtras& ex) {
  observe_launch(s, d, scan, KnownChains(), ids_dev, qt, ex);
}

}  // namespace pk

// Unique data association (pk_assoc_unique; DESIGN.md section 4, "Unique association"): behind the maximum-likelihood association,
// at most one blob of a scan keeps each landmark of a particle.
//
// The rule, per particle.  p(b, l) is the association kernels' own match probability (probability_of_match<MODEL>, and
// probability_of_match_range for a blob with a finite range) on the untouched landmark state at the live pose.  The pairs with
// p > 0 are walked in the order p descending, b ascending, l ascending, and a pair is taken iff neither side has been taken.
// Both sides prefer by that one strict order, so the stable matching is unique and is this greedy one; the kernel reaches it by
// deferred acceptance, blobs proposing:
//
//   step 0   the ids alone say whether the particle has a conflict: a count per landmark in LDS.  No landmark claimed twice -- the
//            usual particle --: the workgroup leaves, wave-uniformly, having read B ids: no probability worked out, nothing written.
//   step 1   every blob starts at its maximum-likelihood id (the head of its own list) with p(b, id) worked out again.  (An id whose
//            probability does not come out positive -- the association's own bits say it does -- stands aside: it claims nothing
//            and its entry is left as it is, whatever the other blobs do.)
//   claims   per landmark the largest key among the blobs now standing at it (atomicMax on the probability's bits, a table that only
//            ever rises), then the lowest blob that attains it (atomicMin).  A blob that is not that one has LOST.
//            (The first pass of a particle that came past step 0 always has one.)
//   propose  a loser goes to the next pair of its own list that can still win: the largest p(b, l') strictly behind (cur_p, cur_id)
//            that beats what l' holds (the tables are monotone: what cannot win now never can).  One wave per loser, lanes over
//            landmarks, both gates on the mean rows first; a wave reduction with the tie to the lower landmark.  None left: 0.
//
// The best new proposal of a pass beats its landmark's holder and every other new proposal, and all later ones come from blobs that
// stand behind it in the one order: it is never displaced.  Each pass with a loser thus settles one more blob for good, and B + 1
// passes are the bound; a particle that reaches it stops, writes the ids it has (where every blob stands) and raises stats[4]
// (the host's error word).
//
// Integer atomics alone, ties by index: the same state gives the same ids on every call.  Hand-written gfx950 (wave64).
#include "pk_device.hpp"
#include "pk_launch.hpp"
#include "pk_range_math.hpp"

namespace pk {

struct AssocUniqueArgs {
  SlotSource ss;
  size_t count_off;
  const int32_t* src;
  const double *x, *y, *h;
  const double* blobs;    // B x 4, scan order
  const double* blobdir;  // B x 2
  const double* rng;      // RANGE: B x 2 (range, variance), scan order
  double q00;
  int32_t* ids;           // P x B, settled in place
  unsigned long long* stats;  // kAssocUniqueWords
  int L, Lp, B;
};

constexpr int kUniqueThreads = 256;

// p(b, l): full_match_probability of pk_k_assoc.hip on the blob's scan-order rows (the exact records are copies of them)
template <int MODEL, bool RANGE>
__device__ __forceinline__ double unique_probability(const AssocUniqueArgs& a, const double* f, int l, int b, double sx, double sy,
                                                     double sh, double ch, double sn) {
  const Landmark<double> lm = load_landmark_nocount(f, a.Lp, l);
  const BlobT<double> z = load_blob(a.blobs, b);
  double ux = a.blobdir[2 * (size_t)b], uy = a.blobdir[2 * (size_t)b + 1];
  if constexpr (MODEL == kModelBearing) rotate_ray(ux, uy, ch, sn, ux, uy);
  if constexpr (RANGE) {
    const BlobRange r = load_range(a.rng, b);
    if (r.has()) return probability_of_match_range(lm, sx, sy, sh, z, ux, uy, r.rho, r.qr, a.q00);
  }
  return probability_of_match<double, MODEL>(lm, sx, sy, sh, z, ux, uy);
}

template <int MODEL, bool RANGE>
__device__ __forceinline__ void assoc_unique_body(const AssocUniqueArgs& a) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ int n_lost, n_twice;
  const int B = a.B, L = a.L;
  unsigned long long* best = reinterpret_cast<unsigned long long*>(smem);  // [Lp] the key its holder stands at it with; 0: nobody yet
  unsigned long long* cur_p = best + a.Lp;                                 // [B]
  int* win = reinterpret_cast<int*>(cur_p + B);                            // [Lp] the holder (valid where best != 0)
  int* cur_id = win + a.Lp;                                                // [B] landmark the blob stands at, -1: none, -2: stands aside
  unsigned short* queue = reinterpret_cast<unsigned short*>(cur_id + B);   // [B] this pass's losers
  const int64_t p = blockIdx.x;
  const unsigned char* slot = a.ss.at(a.src[p]);
  const double* f = reinterpret_cast<const double*>(slot);
  const double sx = a.x[p], sy = a.y[p], sh = a.h[p];
  double ch = 1.0, sn = 0.0;
  if constexpr (MODEL == kModelBearing) sincos(sh, &sn, &ch);
  int32_t* ids = a.ids + (size_t)p * B;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;

  // ---- step 0: is any landmark claimed twice?  (win[] as the counts; the claims passes write it before they read it)
  for (int l = threadIdx.x; l < L; l += kUniqueThreads) {
    best[l] = 0ull;
    win[l] = 0;
  }
  if (threadIdx.x == 0) n_lost = n_twice = 0;
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += kUniqueThreads) {
    const int id = ids[b];
    if (id > 0 && id <= L && atomicAdd(&win[id - 1], 1) != 0) n_twice = 1;
  }
  __syncthreads();
  if (n_twice == 0) return;  // workgroup-uniform
  // ---- step 1
  for (int b = threadIdx.x; b < B; b += kUniqueThreads) {
    const int id = ids[b];
    int l = id == 0 ? -1 : -2;
    unsigned long long bits = 0ull;
    if (id > 0 && id <= L) {
      const double pr = unique_probability<MODEL, RANGE>(a, f, id - 1, b, sx, sy, sh, ch, sn);
      if (pr > 0.0) {
        l = id - 1;
        bits = (unsigned long long)__double_as_longlong(pr);
      }
    }
    cur_id[b] = l;
    cur_p[b] = bits;
  }
  __syncthreads();

  int rounds = 0;
  bool over = false;
  for (;;) {
    // ---- claims
    for (int b = threadIdx.x; b < B; b += kUniqueThreads) {
      const int l = cur_id[b];
      if (l >= 0) {
        atomicMax(&best[l], cur_p[b]);
        win[l] = INT_MAX;  // (every blob standing at l writes the same)
      }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += kUniqueThreads) {
      const int l = cur_id[b];
      if (l >= 0 && cur_p[b] == best[l]) atomicMin(&win[l], b);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += kUniqueThreads) {
      const int l = cur_id[b];
      if (l >= 0 && win[l] != b) queue[atomicAdd(&n_lost, 1)] = (unsigned short)b;
    }
    __syncthreads();
    ++rounds;
    const int lost = n_lost;  // workgroup-uniform
    if (lost == 0) break;
    if (rounds > B) {  // the bound: B + 1 passes
      over = true;
      break;
    }
    __syncthreads();
    if (threadIdx.x == 0) n_lost = 0;
    // ---- propose: a wave per loser, lanes over landmarks
    for (int i = wave; i < lost; i += kUniqueThreads / kWave) {
      const int b = queue[i];
      const int at = cur_id[b];
      const unsigned long long at_p = cur_p[b];
      const BlobT<double> z = load_blob(a.blobs, b);
      unsigned long long mk = 0ull;
      int ml = INT_MAX;
      for (int l = lane; l < L; l += kWave) {
        // the gates on the mean rows, as probability_of_match forms them (:441, :433): the covariance rows of what passes alone
        if (fabs(color_distance2(f[F_MR * a.Lp + l], f[F_MG * a.Lp + l], f[F_MB * a.Lp + l], z.r, z.g, z.b)) > 300.0) continue;
        double delb = z.bearing - (pk_atan2(f[F_MY * a.Lp + l] - sy, f[F_MX * a.Lp + l] - sx) - sh);
        if constexpr (MODEL == kModelBearing) delb = wrap_angle(delb);
        if (fabs(delb) > 0.5) continue;
        const double pr = unique_probability<MODEL, RANGE>(a, f, l, b, sx, sy, sh, ch, sn);
        if (!(pr > 0.0)) continue;
        const unsigned long long k = (unsigned long long)__double_as_longlong(pr);
        if (!(k < at_p || (k == at_p && l > at))) continue;  // strictly behind where the blob stood
        const unsigned long long held = best[l];
        if (k < held || (k == held && win[l] < b)) continue;  // cannot win l, now or later
        if (k > mk) {  // (l ascends: the first of equal keys stays)
          mk = k;
          ml = l;
        }
      }
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned long long ok = (unsigned long long)__shfl_xor((long long)mk, off, kWave);
        const int ol = __shfl_xor(ml, off, kWave);
        if (ok > mk || (ok == mk && ol < ml)) {
          mk = ok;
          ml = ol;
        }
      }
      if (lane == 0) {
        cur_id[b] = mk != 0ull ? ml : -1;
        cur_p[b] = mk;
      }
    }
    __syncthreads();
  }
  if (rounds == 1) return;  // (the doubly claimed ids stood aside: nothing to settle)
  // ---- the settled ids, and the scan's figures
  int changed = 0, moved = 0;
  for (int b = threadIdx.x; b < B; b += kUniqueThreads) {
    if (cur_id[b] == -2) continue;  // (stood aside)
    const int id = cur_id[b] + 1;
    if (ids[b] != id) {
      ids[b] = id;
      ++changed;
      moved += id != 0;
    }
  }
  if (changed) atomicAdd(&a.stats[1], (unsigned long long)changed);
  if (moved) atomicAdd(&a.stats[2], (unsigned long long)moved);
  if (threadIdx.x == 0) {
    atomicAdd(&a.stats[0], 1ull);
    atomicMax(&a.stats[3], (unsigned long long)rounds);
    if (over) atomicMax(&a.stats[4], 1ull);
  }
}

__global__ void __launch_bounds__(kUniqueThreads) k_assoc_unique(AssocUniqueArgs a) { assoc_unique_body<kModelReference, false>(a); }
__global__ void __launch_bounds__(kUniqueThreads) k_assoc_unique_bearing(AssocUniqueArgs a) { assoc_unique_body<kModelBearing, false>(a); }
__global__ void __launch_bounds__(kUniqueThreads) k_assoc_unique_range(AssocUniqueArgs a) { assoc_unique_body<kModelBearing, true>(a); }

void launch_assoc_unique(hipStream_t s, DeviceState& d, const ScanTables& scan, const AssocUniqueLaunch& q) {
  if (d.P == 0 || scan.B == 0) return;
  AssocUniqueArgs a{};
  fill_particles(a, d);
  a.blobs = scan.blobs;
  a.blobdir = scan.dir;
  a.rng = scan.rng;
  a.q00 = q.q00;
  a.ids = q.ids_dev;
  a.stats = q.stats_dev;
  a.B = scan.B;
  const size_t lds = assoc_unique_lds_bytes(d.lay.Lp, scan.B);  // <= kMaxDynLds: checked by the caller
  static bool attr_set[kMaxDevices] = {false};
  allow_dynamic_lds(attr_set, kMaxDynLds, k_assoc_unique, k_assoc_unique_bearing, k_assoc_unique_range);
  if (q.model == kModelBearing && scan.rng)
    hipLaunchKernelGGL(k_assoc_unique_range, dim3((unsigned)d.P), dim3(kUniqueThreads), lds, s, a);
  else if (q.model == kModelBearing)
    hipLaunchKernelGGL(k_assoc_unique_bearing, dim3((unsigned)d.P), dim3(kUniqueThreads), lds, s, a);
  else
    hipLaunchKernelGGL(k_assoc_unique, dim3((unsigned)d.P), dim3(kUniqueThreads), lds, s, a);
}

}  // namespace pk

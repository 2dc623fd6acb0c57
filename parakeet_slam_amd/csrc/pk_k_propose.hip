// k_propose: the measurement-informed proposal of one scan (FastSLAM 2.0 sampling; DESIGN.md section 4, "The measurement-informed
// proposal").  For every particle, standing at its PREDICTED pose: settle the tentative ids against the untouched landmark state,
// gather the matched landmarks, reduce the fourteen sums of pk_proposal.hpp and leave the particle's normals xi, its weight
// increment, its settled ids and the number of matches used.  It touches no pose, no map and no weight.
//
// Hand-written gfx950 (CDNA4, wave64).  One workgroup of 256 lanes per particle, the particles walked with a grid stride.  Lanes
// stride the particle's blobs; a matched blob gathers its landmark's 14 rows and count word from the particle's map slot -- B
// scattered 8-byte reads per row where the observe streams the whole slot, which is why it costs a fraction of that.  The sums
// are reduced in a fixed order (each lane's blobs in scan order, the wave butterfly, the four waves' sums as block_sum adds them): no float
// atomics, the same bits every run.  No scratch, 448 bytes of LDS (k_propose_range: fifteen sums, 480 bytes).
#include "pk_launch.hpp"
#include "pk_motion_common.hpp"
#include "pk_proposal.hpp"
#include "pk_range_math.hpp"

namespace pk {

struct ProposeArgs {
  SlotSource ss;
  size_t count_off;
  const int32_t* src;
  const double *x, *y, *h;  // the predicted poses
  const double* blobs;      // B x 4
  const double* blobdir;    // B x 2 unit rays: tentative ids are settled with them; NULL: the ids are final (supplied)
  int32_t* ids;             // [P x B] (ids_stride = B), or one row for every particle (ids_stride = 0, never written)
  int64_t ids_stride;
  const double* z;          // P x 3 standard normals, or NULL: motion_normals' Philox draws
  const int64_t* logical;
  int64_t goff;
  uint64_t seed, draw;
  int odom;                 // 0: motion_model with u = (v, w, dt); 1: odom_motion_model with u = (rot1, trans, rot2)
  double u0, u1, u2;
  double s0, s1, s2;        // the sigmas of the launch
  double* xi;               // out: P x 3
  double* dlogw;            // out: P
  int32_t* used;            // out: P
  int L, Lp, B;
  int64_t P;
  Noise<double> qt;
};

// The body of k_propose and of k_propose_range, its instance for scans in which some blob has a range (pk_proposal_ranges; rng: the
// scan's range rows [B][2], NaN range = none).  RANGE: a blob with a finite range is settled and summed as a range-bearing
// measurement (pk_range_math.hpp, proposal_match_range), one without takes the bearing model's path, blob by blob, and the
// fifteenth sum n_rho is reduced beside the fourteen.  (The arguments come by value: by reference the compiler schedules k_propose's
// scalar loads of them quite differently from the kernel this body was lifted out of; DESIGN.md section 4, "Ranges in the proposal".)
template <bool RANGE>
__device__ __forceinline__ void propose_body(const ProposeArgs a, const double* rng,
                                             double (*red)[kObsThreads / kWave]) {  // red: [15 or 14 sums][the waves] of LDS
  constexpr int NS = RANGE ? kProposeSumsRange : kProposeSums;
  const int tid = threadIdx.x;
  for (int64_t p = blockIdx.x; p < a.P; p += gridDim.x) {
    const unsigned char* sslot = a.ss.at(a.src[p]);
    const double* sf = reinterpret_cast<const double*>(sslot);
    const int* sc = reinterpret_cast<const int*>(sslot + a.count_off);
    const double sx = a.x[p], sy = a.y[p], sh = a.h[p];
    double sn, ch;
    sincos(sh, &sn, &ch);
    const NoiseJacobian G = noise_jacobian(a.odom != 0, sh, a.u0, a.u1, a.u2);
    int32_t* gid = a.ids + (size_t)p * a.ids_stride;
    ProposalSums S = proposal_zero();
    double nrho = 0.0;  // (RANGE) the fifteenth sum
    for (int b = tid; b < a.B; b += kObsThreads) {
      const int id = gid[b];
      if (id <= 0 || id > a.L) {  // unmatched: weight *= 0.1
        S.low += 1.0;
        continue;
      }
      const Landmark<double> lm = load_landmark(sf, sc, a.Lp, id - 1);
      const BlobT<double> z = load_blob(a.blobs, b);
      BlobRange r{0.0, 0.0};
      bool ranged = false;
      if constexpr (RANGE) {
        r = load_range(rng, b);
        ranged = r.has();
      }
      if (a.blobdir) {  // (kernel-uniform)
        double2 dir = *reinterpret_cast<const double2*>(a.blobdir + 2 * (size_t)b);
        rotate_ray(dir.x, dir.y, ch, sn, dir.x, dir.y);
        bool positive;
        if constexpr (RANGE) {
          positive = ranged ? match_is_positive_range(lm, sx, sy, z, dir.x, dir.y, r.rho, r.qr, a.qt.q00)
                            : match_is_positive<kModelBearing>(lm, sx, sy, pk_atan2(lm.my - sy, lm.mx - sx), z, dir.x, dir.y);
        } else {
          const double pse = pk_atan2(lm.my - sy, lm.mx - sx);
          positive = match_is_positive<kModelBearing>(lm, sx, sy, pse, z, dir.x, dir.y);
        }
        if (!positive) {
          gid[b] = 0;
          S.low += 1.0;
          continue;
        }
      }
      if (lm.count & kPotentialBit) {  // a potential feature: updated, weighs as if not seen
        S.low += 1.0;
        continue;
      }
      if (RANGE && ranged)
        proposal_match_range(S, nrho, lm, sx, sy, sh, z, r.rho, r.qr, a.qt, G, a.s0, a.s1, a.s2);
      else
        proposal_match(S, lm, sx, sy, sh, z, a.qt, G, a.s0, a.s1, a.s2);
    }
    // the sums, each in block_sum's order and to its bits -- the wave butterfly, then the waves' sums added in wave order --
    // behind ONE barrier instead of block_sum's two per sum
    constexpr int NW = kObsThreads / kWave;
    double* v[NS] = {&S.l00, &S.l01, &S.l02, &S.l11, &S.l12, &S.l22, &S.e0, &S.e1, &S.e2, &S.c, &S.ell, &S.kappa, &S.n, &S.low};
    if constexpr (RANGE) v[kProposeSums] = &nrho;
    const int wave = tid / kWave, lane = tid % kWave;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const double w = wave_sum(*v[k]);
      if (lane == 0) red[k][wave] = w;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        double t = red[k][0];
#pragma unroll
        for (int i = 1; i < NW; ++i) t += red[k][i];
        *v[k] = t;
      }
    }
    if (tid == 0) {
      double z0, z1, z2, x0, x1, x2;
      motion_normals(a.z, p, a.logical, a.goff, a.seed, a.draw, z0, z1, z2);
      const double d = proposal_finish<RANGE>(S, z0, z1, z2, x0, x1, x2, nrho);
      a.xi[3 * p] = x0;
      a.xi[3 * p + 1] = x1;
      a.xi[3 * p + 2] = x2;
      a.dlogw[p] = d;
      a.used[p] = (int32_t)S.n;
    }
    __syncthreads();  // (red is the next particle's)
  }
}

__global__ void __launch_bounds__(kObsThreads) k_propose(ProposeArgs a) {
  __shared__ double red[kProposeSums][kObsThreads / kWave];
  propose_body<false>(a, nullptr, red);
}
__global__ void __launch_bounds__(kObsThreads) k_propose_range(ProposeArgs a, const double* rng) {
  __shared__ double red[kProposeSumsRange][kObsThreads / kWave];
  propose_body<true>(a, rng, red);
}

void launch_propose(hipStream_t s, DeviceState& d, const ProposeLaunch& q) {
  if (d.P == 0) return;
  ProposeArgs a{};
  fill_particles(a, d);
  a.blobs = q.blobs_dev;
  a.blobdir = q.blobdir_dev;
  a.ids = q.ids_dev;
  a.ids_stride = q.ids_shared ? 0 : q.B;
  a.z = q.z_dev;
  a.logical = d.logical[d.cur];
  a.goff = d.global_offset;
  a.seed = q.seed;
  a.draw = q.draw;
  a.odom = q.odom ? 1 : 0;
  a.u0 = q.u[0];
  a.u1 = q.u[1];
  a.u2 = q.u[2];
  a.s0 = q.sigma[0];
  a.s1 = q.sigma[1];
  a.s2 = q.sigma[2];
  a.xi = q.xi_dev;
  a.dlogw = q.dlogw_dev;
  a.used = q.used_dev;
  a.B = q.B;
  a.P = d.P;
  a.qt = device_noise(q.qt);
  const unsigned grid = (unsigned)(d.P > 16384 ? 16384 : d.P);
  if (q.rng_dev)  // a scan in which some blob has a range
    hipLaunchKernelGGL(k_propose_range, dim3(grid), dim3(kObsThreads), 0, s, a, q.rng_dev);
  else
    hipLaunchKernelGGL(k_propose, dim3(grid), dim3(kObsThreads), 0, s, a);
}

}  // namespace pk

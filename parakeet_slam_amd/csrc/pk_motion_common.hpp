// What the two motion kernels (k_motion: the commanded twist, pk_k_motion.hip; k_motion_odom: an odometry delta,
// pk_k_motion_odom.hip) share: the three standard normals of a particle, the extra workgroups that carry a staged scan's upload,
// and the per-block pose sums k_candidates reads.  One definition each, so that the two kernels draw the same noise for the same
// (particle, seed, draw) and leave pose_part in the same order.
#pragma once
#include "pk_device.hpp"
#include "pk_philox.hpp"

namespace pk {

// The extra workgroups of a combined launch: the per-scan upload (see k_upload).  Blocks [motion_blocks, gridDim.x) copy.
__device__ __forceinline__ void motion_upload_tail(int motion_blocks, uint4* __restrict__ up_dst, const uint4* __restrict__ up_src,
                                                   int64_t up_n16) {
  const int64_t nb = (int64_t)gridDim.x - motion_blocks;
  for (int64_t i = (int64_t)(blockIdx.x - motion_blocks) * blockDim.x + threadIdx.x; i < up_n16; i += nb * blockDim.x)
    up_dst[i] = up_src[i];
}

// Particle i's three standard normals: the caller's z[3 i ..], or Philox4x32-10 + Box-Muller.
// The counter is the particle's index in the WHOLE filter: its slot plus the shard's offset, or -- balanced placement of
// the sharded filter -- the logical index its slot carries.  The key is the seed; `draw` and the high bit of counter word 3 tell the
// two calls apart.
__device__ __forceinline__ void motion_normals(const double* __restrict__ z, int64_t i, const int64_t* __restrict__ logical,
                                               int64_t goff, uint64_t seed, uint64_t draw, double& z0, double& z1, double& z2) {
  if (z) {
    z0 = z[3 * i];
    z1 = z[3 * i + 1];
    z2 = z[3 * i + 2];
  } else {
    uint64_t g = logical ? (uint64_t)logical[i] : (uint64_t)(i + goff);
    Philox4 a = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)draw,
                              (uint32_t)(draw >> 32) & 0x7fffffffu, (uint32_t)seed, (uint32_t)(seed >> 32));
    Philox4 b = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)draw,
                              ((uint32_t)(draw >> 32) & 0x7fffffffu) | 0x80000000u, (uint32_t)seed,
                              (uint32_t)(seed >> 32));
    double u1 = u53(a.v[0], a.v[1]), u2 = u53(a.v[2], a.v[3]);
    double u3 = u53(b.v[0], b.v[1]), u4 = u53(b.v[2], b.v[3]);
    double r1 = sqrt(-2.0 * log(u1)), r2 = sqrt(-2.0 * log(u3));
    double s1, c1, s2, c2;
    sincos(Consts<double>::two_pi * u2, &s1, &c1);
    sincos(Consts<double>::two_pi * u4, &s2, &c2);
    z0 = r1 * c1;
    z1 = r1 * s1;
    z2 = r2 * c2;
    (void)s2;
  }
}

// The block's sums of x, y, sin h, cos h of the MOVED particles (fixed order): k_candidates takes the particles' mean pose from
// them (the reference the candidate lists are made around), which used to cost two launches of its own per scan.
// Every thread of the block calls this (lanes past P with zeros); red: four doubles of LDS.
__device__ __forceinline__ void motion_pose_sums(double px, double py, double ps, double pc, double* red,
                                                 double* __restrict__ pose_part) {
  px = block_sum<4>(px, red);
  py = block_sum<4>(py, red);
  ps = block_sum<4>(ps, red);
  pc = block_sum<4>(pc, red);
  if (threadIdx.x == 0) {
    pose_part[4 * blockIdx.x + 0] = px;
    pose_part[4 * blockIdx.x + 1] = py;
    pose_part[4 * blockIdx.x + 2] = ps;
    pose_part[4 * blockIdx.x + 3] = pc;
  }
}

}  // namespace pk

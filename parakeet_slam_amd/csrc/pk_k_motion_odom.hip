// K1 (odometry): the motion sample from an odometry delta (rot1, trans, rot2) -- the sibling of k_motion (pk_k_motion.hip), with
// which it shares the draws, the upload workgroups and the pose sums (pk_motion_common.hpp); see DESIGN.md section 4.
//
// Hand-written gfx950 (CDNA4, wave64).  A streaming kernel: one lane per particle, 24 B read and 24 B written, the arithmetic
// register resident (pk_math.hpp); no scratch, no LDS beyond block_sum's four words, no atomics.
#include "pk_motion_common.hpp"

namespace pk {

// x, y, h: the first of P particles; s0..s2: sigma_rot1, sigma_trans, sigma_rot2 of this delta (pk_odom_sigmas, on the host).
// Blocks [0, motion_blocks) move particles; the blocks beyond them carry a staged scan's upload.  pose_part != NULL: the launch
// covers the whole filter and leaves the per-block pose sums of the moved particles.
__global__ void __launch_bounds__(256) k_motion_odom(double* __restrict__ x, double* __restrict__ y, double* __restrict__ h,
                                                     int64_t P, double rot1, double trans, double rot2, double s0, double s1,
                                                     double s2, const double* __restrict__ z, uint64_t seed, uint64_t draw,
                                                     int64_t goff, int motion_blocks, uint4* __restrict__ up_dst,
                                                     const uint4* __restrict__ up_src, int64_t up_n16,
                                                     const int64_t* __restrict__ logical, double* __restrict__ pose_part) {
  __shared__ double red[4];
  if ((int)blockIdx.x >= motion_blocks) {
    motion_upload_tail(motion_blocks, up_dst, up_src, up_n16);
    return;
  }
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P && pose_part == nullptr) return;
  double px = 0.0, py = 0.0, ps = 0.0, pc = 0.0;  // this particle's share of the block's pose sums
  if (i < P) {
    double z0, z1, z2;
    motion_normals(z, i, logical, goff, seed, draw, z0, z1, z2);
    double xi = x[i], yi = y[i], hi = h[i];
    odom_motion_model(xi, yi, hi, rot1, trans, rot2, s0 * z0, s1 * z1, s2 * z2);
    x[i] = xi;
    y[i] = yi;
    h[i] = hi;
    if (pose_part) {
      px = xi;
      py = yi;
      sincos(hi, &ps, &pc);
    }
  }
  if (pose_part) motion_pose_sums(px, py, ps, pc, red, pose_part);  // (kernel-uniform)
}

void launch_motion_odom(hipStream_t s, DeviceState& d, const double delta[3], const double sigma[3], const double* z_dev,
                        uint64_t seed, uint64_t draw, void* up_dst_dev, const void* up_src_host_mapped, size_t up_bytes,
                        double* pose_part_dev) {
  const int64_t n16 = up_dst_dev ? (int64_t)((up_bytes + 15) / 16) : 0;
  if (d.P == 0 && n16 == 0) return;
  int blocks = (int)((d.P + 255) / 256);
  int64_t ub = (n16 + 255) / 256;
  if (ub > 256) ub = 256;
  hipLaunchKernelGGL(k_motion_odom, dim3((unsigned)(blocks + ub)), dim3(256), 0, s, d.x[d.cur], d.y[d.cur], d.h[d.cur], d.P,
                     delta[0], delta[1], delta[2], sigma[0], sigma[1], sigma[2], z_dev, seed, draw, d.global_offset, blocks,
                     static_cast<uint4*>(up_dst_dev), static_cast<const uint4*>(up_src_host_mapped), n16,
                     (const int64_t*)d.logical[d.cur], pose_part_dev);
}

// The same for the particles [p0, p1) only (device noise; the Philox counters use the global particle index, so the draws
// are those of the whole-range launch).
void launch_motion_odom_range(hipStream_t s, DeviceState& d, const double delta[3], const double sigma[3], uint64_t seed,
                              uint64_t draw, int64_t p0, int64_t p1) {
  if (p1 <= p0) return;
  const int64_t n = p1 - p0;
  int blocks = (int)((n + 255) / 256);
  hipLaunchKernelGGL(k_motion_odom, dim3((unsigned)blocks), dim3(256), 0, s, d.x[d.cur] + p0, d.y[d.cur] + p0, d.h[d.cur] + p0, n,
                     delta[0], delta[1], delta[2], sigma[0], sigma[1], sigma[2], (const double*)nullptr, seed, draw,
                     d.global_offset + p0, blocks, (uint4*)nullptr, (const uint4*)nullptr, (int64_t)0,
                     d.logical[d.cur] ? (const int64_t*)(d.logical[d.cur] + p0) : (const int64_t*)nullptr, (double*)nullptr);
}

}  // namespace pk

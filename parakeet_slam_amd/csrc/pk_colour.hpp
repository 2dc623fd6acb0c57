// The colour table: a landmark's colour covariance as a function of (landmark, number of updates).
//
// ekf_update's colour block is C' = f(C, Qt) (pk_math.hpp: colour_block_step) -- no pose, no blob in it.  pk_upload_map gives every
// particle the same map with update counts 0, and Qt is one per filter, so the block of landmark l in ANY particle is the level
// count / 2 of one sequence per landmark, bit for bit, until somebody edits a single particle's map.  tab[k][6][Lp] holds the first
// `depth` levels, rows laid out like a slot's (crr crg crb cgg cgb cbb, landmark fastest).
#pragma once
#include "pk_math.hpp"

namespace pk {

__device__ __forceinline__ unsigned colour_level(int count) { return (unsigned)(count & ~kPotentialBit) >> 1; }

// Levels beyond the table are reached by the recurrence, at most this many steps of it (a count that names a level further out is
// no count a table-mode scan has written: nothing loops on it for long).
constexpr unsigned kColourBeyondMax = 4096;

// Landmark l's block at `level`: from the table, or -- beyond it -- by the recurrence from the table's last level (slow and rare).
__device__ inline Sym3<double> colour_block_at(const double* tab, int depth, int Lp, int l, unsigned level, const Noise<double>& qt) {
  if (level > (unsigned)depth + kColourBeyondMax) level = (unsigned)depth + kColourBeyondMax;
  unsigned k = level < (unsigned)depth ? level : (unsigned)depth - 1u;
  const double* t = tab + ((size_t)k * 6) * Lp + l;
  Sym3<double> C{t[0], t[(size_t)Lp], t[2 * (size_t)Lp], t[3 * (size_t)Lp], t[4 * (size_t)Lp], t[5 * (size_t)Lp]};
#pragma unroll 1
  for (; k < level; ++k) C = colour_block_step(C, qt);
  return C;
}

}  // namespace pk

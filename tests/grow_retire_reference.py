"""The retirement rule of growing maps (pk_grow_retire, k_grow_retire) in plain Python on top of
oracle/fastslam_oracle.py::GrowingOracle -- what the device is held to, particle by particle.  Needs no GPU.

Per particle, behind the bookkeeping of every non-empty scan (t counts those scans, modulo 2^32):
  1. spare slots the last pass knew: count word changed -> seen = word, idle = 0; else idle += 1 (saturating)
  2. slots and readings that are new since the last pass: seen = word, idle = 0; stamp = t
  3. A > 0: the longest PREFIX of the ring whose readings are A scans old or older goes, the rest moves down
  4. M > 0: slots whose seen word is potential and that have been idle for M passes go, the survivors move down in order,
     the vacated slots return to the empty state
  5. covered_readings = readings stored, covered_slots = slots in use
"""
import numpy as np

from oracle.fastslam_oracle import EMPTY_COLOUR, GrowingOracle

POTENTIAL = 0x40000000  # PK_LANDMARK_POTENTIAL: the flag rides in the count word
INT32_MAX = 2 ** 31 - 1
MASK32 = 0xFFFFFFFF


class RetiringOracle(GrowingOracle):
    def __init__(self, num_particles, means, covs, spare, pair_threshold, reading_max_age=0, potential_max_idle=0):
        super(RetiringOracle, self).__init__(num_particles, means, covs, spare, pair_threshold)
        P = int(num_particles)
        self.A, self.M = int(reading_max_age), int(potential_max_idle)
        self.t = 0
        self.scan = [[] for _ in range(P)]   # stamp of every stored reading, parallel to hyp
        self.seen = [[] for _ in range(P)]   # count word of every spare slot in use at the last pass
        self.idle = [[] for _ in range(P)]   # consecutive passes it did not change
        self.covered_readings = [0] * P
        self.covered_slots = [0] * P
        self.readings_retired = [0] * P
        self.features_retired = [0] * P
        self.max_ring = 0                    # the longest ring any particle ever held (behind a pass)
        self.promoted_vacated = 0            # promoted features a pass vacated: the rule never does

    def word(self, i, j):
        f = self.f
        return int(f.count[i, self.L0 + j]) | (POTENTIAL if f.potential[i, self.L0 + j] else 0)

    def restart(self, i):
        """What pk_grow_upload does to a particle it wrote: the next pass stamps everything as new."""
        self.covered_readings[i] = self.covered_slots[i] = 0

    def retire_pass(self, i):
        f, L0, t = self.f, self.L0, self.t
        n, used = len(self.hyp[i]), self.used[i]
        scan, seen, idle = self.scan[i], self.seen[i], self.idle[i]
        cs, cr = min(self.covered_slots[i], used), min(self.covered_readings[i], n)
        del scan[cr:], seen[cs:], idle[cs:]
        for j in range(cs):                                  # 1
            w = self.word(i, j)
            if w != seen[j]:
                seen[j], idle[j] = w, 0
            else:
                idle[j] = min(idle[j] + 1, INT32_MAX)
        for j in range(cs, used):                            # 2
            seen.append(self.word(i, j))
            idle.append(0)
        scan.extend([t] * (n - cr))
        if self.A > 0:                                       # 3
            k = 0
            while k < n and ((t - scan[k]) & MASK32) >= self.A:
                k += 1
            del self.hyp[i][:k], scan[:k]
            self.readings_retired[i] += k
        if self.M > 0:                                       # 4
            keep = [j for j in range(used) if not ((seen[j] & POTENTIAL) and idle[j] >= self.M)]
            if len(keep) < used:
                self.promoted_vacated += sum(1 for j in range(used) if j not in keep and not (self.word(i, j) & POTENTIAL))
                ids = dict(self.slot_id[i])
                self.slot_id[i] = {}
                for dst, src in enumerate(keep):
                    f.mean[i, L0 + dst] = f.mean[i, L0 + src]
                    f.cov[i, L0 + dst] = f.cov[i, L0 + src]
                    f.count[i, L0 + dst] = f.count[i, L0 + src]
                    f.potential[i, L0 + dst] = f.potential[i, L0 + src]
                    self.slot_id[i][L0 + dst] = ids[L0 + src]
                for j in range(len(keep), used):
                    f.mean[i, L0 + j] = (0.0, 0.0, EMPTY_COLOUR, EMPTY_COLOUR, EMPTY_COLOUR)
                    f.cov[i, L0 + j] = np.identity(5)
                    f.count[i, L0 + j] = 0
                    f.potential[i, L0 + j] = False
                self.seen[i] = [seen[j] for j in keep]
                self.idle[i] = [idle[j] for j in keep]
                self.features_retired[i] += used - len(keep)
                self.used[i] = len(keep)
        self.covered_readings[i] = len(self.hyp[i])          # 5
        self.covered_slots[i] = self.used[i]
        self.max_ring = max(self.max_ring, len(self.hyp[i]))

    def observe(self, blobs):
        blobs = np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
        ids = super(RetiringOracle, self).observe(blobs)
        if len(blobs):  # an empty scan runs nothing and advances no clock
            self.t = (self.t + 1) & MASK32
            for i in range(self.f.P):
                self.retire_pass(i)
        return ids

    def gather(self, anc):
        super(RetiringOracle, self).gather(anc)
        for name in ("scan", "seen", "idle"):
            old = getattr(self, name)
            setattr(self, name, [list(old[a]) for a in anc])
        for name in ("covered_readings", "covered_slots", "readings_retired", "features_retired"):
            old = getattr(self, name)
            setattr(self, name, [old[a] for a in anc])

    def clock_counters(self):
        return np.array([self.covered_readings, self.covered_slots, self.readings_retired, self.features_retired], dtype=np.int64).T

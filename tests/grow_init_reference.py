"""The triangulated initialisation of growing maps (pk_grow_init(f, PK_GROW_INIT_TRIANGULATED, min_parallax); DESIGN.md section 9,
"Parallax-gated pairing") in plain Python on top of oracle/fastslam_oracle.py::GrowingOracle -- what the device is held to, particle
by particle -- and the scenes the CPU and the GPU tests share.  TEST INFRASTRUCTURE ONLY.  Needs no GPU.

Per particle and unmatched blob everything is GrowingOracle.add_hypothesis, except:
  1. a stored reading is a candidate iff its ray crosses the blob's (ray_intersect) AND |den| >= sin(min_parallax), den the
     determinant ray_intersect forms (minus the sine of the angle between the rays); a NaN fails;
  2. the new feature's position covariance is J diag(q00, q00) J' over the two world bearings, q00 = Qt[0][0].
"""
import math

import numpy as np

from oracle.fastslam_oracle import (EMPTY_COLOUR, GrowingOracle, colour_distance, cross_readings, low_variance_ancestors,
                                    synthetic_scan, synthetic_world, truth_step)

from bearing_model_reference import BearingOracle, gate_margins, under_bearing_model, wrapped_scan
from grow_retire_reference import RetiringOracle


def ray_intersect_den(x1, y1, b1, x3, y3, b3):
    """oracle.ray_intersect, operation by operation, which also hands out the determinant: (rays cross, den)."""
    ax, ay = math.cos(b1), math.sin(b1)
    bx, by = math.cos(b3), math.sin(b3)
    den = ay * bx - ax * by
    if den == 0:
        return False, den
    v = (ax * y3 - ay * x3 + ay * x1 - ax * y1) / den
    if abs(ay) < abs(ax):
        u = (x3 + bx * v - x1) / ax
    else:
        u = (y3 + by * v - y1) / ay
    return (u >= 0 and v >= 0), den


def triangulated_covariance(x1, y1, t1, px, py, t3, ox, oy, q00):
    """(Pxx, Pxy, Pyy) of the crossing (ox, oy) of the lines (x1, y1, t1) and (px, py, t3): J diag(q00, q00) J' with
    dX/dt1 = (u / sd) d3 and dX/dt3 = -(v / sd) d1, d = (cos t, sin t), in the order the kernel evaluates it."""
    s1, c1 = math.sin(t1), math.cos(t1)
    s3, c3 = math.sin(t3), math.cos(t3)
    sd = s3 * c1 - c3 * s1
    u = (ox - x1) * c1 + (oy - y1) * s1
    v = (ox - px) * c3 + (oy - py) * s3
    a = u / sd
    b = v / sd
    aa = a * a
    bb = b * b
    return (q00 * (aa * (c3 * c3) + bb * (c1 * c1)),
            q00 * (aa * (c3 * s3) + bb * (c1 * s1)),
            q00 * (aa * (s3 * s3) + bb * (s1 * s1)))


class Triangulating(object):
    """The rule, as a mix-in in front of GrowingOracle or a subclass of it (RetiringOracle): ``triangulate(min_parallax)`` switches
    it on, ``triangulate(None)`` back to the parent's rule.  Over a run it records
      margin    the smallest | |den| - sin_min | over every gate decision (every stored reading a blob was held against),
      excluded  (particle, reading id, blob's id) of every reading whose ray crossed the blob's and which the gate excluded,
      changed   (particle, blob's id, reading the plain rule pairs it with or None, reading this rule pairs it with or None) where
                the two differ,
      made      (particle, slot, reading id, blob's id, (Pxx, Pxy, Pyy)) of every feature made,
      longest_ring  the longest ring any particle held (before anything retires)."""

    min_parallax = None

    def triangulate(self, min_parallax):
        if min_parallax is None:
            self.min_parallax = None
            return self
        min_parallax = float(min_parallax)
        assert 0.0 <= min_parallax <= math.pi / 2
        self.min_parallax = min_parallax
        self.sin_min = math.sin(min_parallax)
        self.margin = float("inf")
        self.excluded, self.changed, self.made = [], [], []
        self.longest_ring = 0
        return self

    def add_hypothesis(self, i, blob):
        if self.min_parallax is None:
            return super(Triangulating, self).add_hypothesis(i, blob)
        f = self.f
        x, y, h = float(f.x[i]), float(f.y[i]), float(f.h[i])
        me = self.next_id[i]
        best, best_d = None, float("inf")
        plain, plain_d = None, float("inf")
        for rd in self.hyp[i]:
            crosses, den = ray_intersect_den(rd[1], rd[2], rd[4] + rd[3], x, y, blob[0] + h)
            self.margin = min(self.margin, abs(abs(den) - self.sin_min))
            if not crosses:
                continue
            d = colour_distance(rd[5:8], blob[1:4])
            if d < plain_d:
                plain, plain_d = rd, d
            if not (abs(den) >= self.sin_min):
                self.excluded.append((i, rd[0], me))
                continue
            if d < best_d:
                best, best_d = rd, d
        free = self.used[i] < self.spare

        def pairs(rd, d):
            if rd is None or not (d < self.thr) or not free:
                return None
            return cross_readings(rd[1], rd[2], rd[3] + rd[4], x, y, h + blob[0])

        xy_plain, xy = pairs(plain, plain_d), pairs(best, best_d)
        a, b = (plain[0] if xy_plain is not None else None), (best[0] if xy is not None else None)
        if a != b:
            self.changed.append((i, me, a, b))
        if xy is not None:
            slot = self.L0 + self.used[i]
            self.used[i] += 1
            pxx, pxy, pyy = triangulated_covariance(best[1], best[2], best[3] + best[4], x, y, h + blob[0], xy[0], xy[1],
                                                    float(f.Qt[0][0]))
            f.mean[i, slot] = (xy[0], xy[1], (best[5] + blob[1]) / 2, (best[6] + blob[2]) / 2, (best[7] + blob[3]) / 2)
            cov = np.identity(5)
            cov[0, 0], cov[0, 1], cov[1, 0], cov[1, 1] = pxx, pxy, pxy, pyy
            f.cov[i, slot] = cov
            f.count[i, slot] = 0
            f.potential[i, slot] = True
            self.slot_id[i][slot] = me
            self.next_id[i] += 1
            self.made.append((i, slot, best[0], me, (pxx, pxy, pyy)))
            return
        self.hyp[i].append((me, x, y, h, float(blob[0]), float(blob[1]), float(blob[2]), float(blob[3])))
        self.next_id[i] += 1
        self.longest_ring = max(self.longest_ring, len(self.hyp[i]))


class TriangulatingOracle(Triangulating, GrowingOracle):
    def __init__(self, num_particles, means, covs, spare, pair_threshold, min_parallax=0.0):
        super(TriangulatingOracle, self).__init__(num_particles, means, covs, spare, pair_threshold)
        self.triangulate(min_parallax)


class TriangulatingRetiringOracle(Triangulating, RetiringOracle):
    """The rule with retirement running behind every scan (the two compose: retirement never looks at how a feature was made)."""

    def __init__(self, num_particles, means, covs, spare, pair_threshold, reading_max_age=0, potential_max_idle=0, min_parallax=0.0):
        super(TriangulatingRetiringOracle, self).__init__(num_particles, means, covs, spare, pair_threshold, reading_max_age,
                                                          potential_max_idle)
        self.triangulate(min_parallax)


# ---------------------------------------------------------------------------------------------------------------- shared drives
class Step(object):
    """One step of ``drive``: the oracle has moved and observed; ``finish(anc)`` resamples it (by its own ancestors unless the
    caller brings the device's)."""

    def __init__(self, o, s, pose, blobs, z, u, logw, anc, gates):
        self.o, self.s, self.pose, self.blobs, self.z, self.u, self.logw, self.anc, self.gates = o, s, pose, blobs, z, u, logw, anc, gates
        self.done = False

    def finish(self, anc=None):
        if not self.done:
            if anc is not None:
                self.anc = np.asarray(anc)
            self.o.gather(self.anc)
            self.done = True


def drive(o, world, steps, seed, v, w, dt, scan, h0=0.0):
    """``steps`` steps of the drive (v, w, dt) from (0, 0, h0) on the growing oracle ``o``, resampled at every step in the log
    domain; scan(world, pose, rs) -> blobs.  Yields a Step behind every observe; the step is finished when the caller comes back."""
    P = o.f.P
    o.f.h[:] = h0
    rs = np.random.RandomState(seed)
    pose = (0.0, 0.0, h0)
    bearing = isinstance(o.f, BearingOracle)
    for s in range(steps):
        pose = truth_step(pose, v, w, dt)
        blobs = scan(world, pose, rs)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        o.f.reset_weights()
        o.f.motion(v, w, dt, z)
        gates = None
        if bearing:  # how far the association's gates are from turning over (bearing 0.5 rad, squared colour distance 300)
            sx, sy, sh = o.f.x[:, None], o.f.y[:, None], o.f.h[:, None]
            m = [gate_margins(sx, sy, sh, blobs[b], o.f.mean) for b in range(len(blobs))]
            gates = (min(float(a.min()) for a, _ in m), min(float(c.min()) for _, c in m))
        o.observe(blobs)
        logw = o.f.logw.copy()
        st = Step(o, s, pose, blobs, z, u, logw, low_variance_ancestors(np.exp(logw - np.max(logw)), u), gates)
        yield st
        st.finish()


def noise_free_wrapped(world, pose, rs):
    return wrapped_scan(world, pose)


def noise_free_unwrapped(world, pose, rs):
    return synthetic_scan(world, pose)


# The small scene of the GPU tests: 64 particles, 10 preset + 3 unknown landmarks of synthetic_world(13, seed=123), 5 spare slots,
# v = 0.8, w = 0.35, dt = 0.5, 14 steps, noise-free scans.
SMALL = dict(P=64, L0=10, U=3, spare=5, thr=30.0, v=0.8, w=0.35, dt=0.5, steps=14, world_seed=123)
GPU_SCENES = {
    # name: (model, min_parallax, reading capacity, retirement (A, M) or None, seed of the noise)
    "bearing_0.1": ("bearing", 0.1, 64, None, 6),
    "bearing_0.2": ("bearing", 0.2, 64, None, 6),
    "reference_0.1": ("reference", 0.1, 128, None, 7),
    "bearing_0.1_retiring": ("bearing", 0.1, 64, (4, 3), 6),  # (readings four scans old go: 0.2 rad are never reached)
}


def small_world():
    c = SMALL
    world, covs = synthetic_world(c["L0"] + c["U"], seed=c["world_seed"])
    return world, covs


def small_map():
    """(means, covs) of the device's map: the preset landmarks and the empty spare slots."""
    c = SMALL
    world, covs = small_world()
    L0, spare = c["L0"], c["spare"]
    means = np.zeros((L0 + spare, 5))
    means[:L0] = world[:L0]
    means[L0:, 2:] = EMPTY_COLOUR
    mcov = np.tile(np.identity(5), (L0 + spare, 1, 1))
    mcov[:L0] = covs[:L0]
    return means, mcov


def small_oracle(name, min_parallax=None, cls=None):
    """The oracle of a scene (with another min_parallax, or as another class of the same constructor, where asked)."""
    c = SMALL
    model, mp, _R, retire, _seed = GPU_SCENES[name]
    mp = mp if min_parallax is None else min_parallax
    world, covs = small_world()
    L0 = c["L0"]
    if retire:
        o = (cls or TriangulatingRetiringOracle)(c["P"], world[:L0], covs[:L0], c["spare"], c["thr"], retire[0], retire[1], min_parallax=mp)
    else:
        o = (cls or TriangulatingOracle)(c["P"], world[:L0], covs[:L0], c["spare"], c["thr"], min_parallax=mp)
    return under_bearing_model(o) if model == "bearing" else o


def small_drive(name, o):
    c = SMALL
    model, _mp, _R, _retire, seed = GPU_SCENES[name]
    world, _ = small_world()
    scan = noise_free_wrapped if model == "bearing" else noise_free_unwrapped
    return drive(o, world, c["steps"], seed, c["v"], c["w"], c["dt"], scan)


def promoted(o):
    """Spare features past update_count 5 and no longer potential, per particle."""
    L0 = o.L0
    return ((o.f.count[:, L0:] > 5) & ~o.f.potential[:, L0:]).sum(axis=1)

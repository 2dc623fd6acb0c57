"""Ranged scans on a growing map (pk_grow_ranges; DESIGN.md section 9, "Single-sighting initialisation") in plain Python: a mix-in
over grow_init_reference's TriangulatingOracle / TriangulatingRetiringOracle whose filter runs range_bearing_reference's
RangeBearingOracle -- what the device is held to, particle by particle -- and the scenes the CPU and the GPU tests share.
TEST INFRASTRUCTURE ONLY.  Needs no GPU.

Matched blobs are RangeBearingOracle's.  Per particle and unmatched blob, in scan order: a blob with a finite range, while a spare
slot is free, becomes a potential feature at once (single_sighting below; the blob's own colour, identity colour block, count 0,
slot id next_id) -- no stored reading is looked at and none is stored.  Every other unmatched blob is Triangulating.add_hypothesis'.
"""
import math

import numpy as np

from oracle.fastslam_oracle import EMPTY_COLOUR, GrowingOracle, OracleFilter

import grow_init_reference as gi
from bearing_model_reference import BearingOracle, wrapped_scan
from grow_init_reference import TriangulatingOracle, TriangulatingRetiringOracle
from grow_retire_reference import MASK32, RetiringOracle
from range_bearing_reference import RangeBearingOracle, range_scan


def single_sighting(px, py, ph, zb, rho, q_rho, q00):
    """(mx, my, Pxx, Pxy, Pyy) of the feature one ranged sighting places, operation by operation as the kernel evaluates it."""
    t = ph + zb
    s, c = math.sin(t), math.cos(t)
    a = (rho * rho) * q00
    return (px + rho * c, py + rho * s, q_rho * (c * c) + a * (s * s), (q_rho - a) * (c * s), q_rho * (s * s) + a * (c * c))


class SingleSighting(object):
    """The mix-in, in front of Triangulating (whose rule the unranged blobs go through).  ``scan_ranges`` arms the ranges of the
    next observe as pk_scan_ranges does (``observe`` takes them as arguments too); ``single`` records (particle, slot, blob's id,
    (Pxx, Pxy, Pyy)) of every single-sighting feature made, ``last_scan`` the (ranges, variances) the last observe consumed."""

    def under_ranges(self):
        """The filter runs the bearing model with ranges (RangeBearingOracle adds two records of how close its verdicts were)."""
        assert isinstance(self, GrowingOracle) and type(self.f) in (OracleFilter, BearingOracle)
        self.f.__class__ = RangeBearingOracle
        self.f.min_rel_gap = np.inf
        self.f.min_gate_margins = [np.inf, np.inf]
        self.single = []
        self.armed = None
        self.last_scan = (None, None)
        return self

    def scan_ranges(self, ranges, variances):
        self.armed = (np.asarray(ranges, dtype=np.float64), np.asarray(variances, dtype=np.float64))

    def place(self, i, blob, rho, q_rho):
        f = self.f
        mx, my, pxx, pxy, pyy = single_sighting(float(f.x[i]), float(f.y[i]), float(f.h[i]), float(blob[0]), float(rho), float(q_rho),
                                                float(f.Qt[0][0]))
        slot = self.L0 + self.used[i]
        self.used[i] += 1
        f.mean[i, slot] = (mx, my, blob[1], blob[2], blob[3])
        cov = np.identity(5)
        cov[0, 0], cov[0, 1], cov[1, 0], cov[1, 1] = pxx, pxy, pxy, pyy
        f.cov[i, slot] = cov
        f.count[i, slot] = 0
        f.potential[i, slot] = True
        self.slot_id[i][slot] = self.next_id[i]
        self.single.append((i, slot, self.next_id[i], (pxx, pxy, pyy)))
        self.next_id[i] += 1

    def observe(self, blobs, ranges=None, variances=None):
        blobs = np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
        B = len(blobs)
        if ranges is None and self.armed is not None:
            ranges, variances = self.armed
        self.armed = None  # consumed
        rng = np.full(B, np.nan) if ranges is None else np.asarray(ranges, dtype=np.float64).reshape(B)
        var = np.full(B, np.nan) if variances is None else np.asarray(variances, dtype=np.float64).reshape(B)
        self.last_scan = (rng, var)
        ids = self.f.observe(blobs, ranges=rng, variances=var)
        for i in range(self.f.P):
            for b in np.nonzero(ids[i] == 0)[0]:
                if np.isfinite(rng[b]) and self.used[i] < self.spare:
                    self.place(i, blobs[b], rng[b], var[b])
                else:
                    self.add_hypothesis(i, blobs[b])
        if isinstance(self, RetiringOracle) and B:  # RetiringOracle.observe's tail: the pass behind every non-empty scan
            self.t = (self.t + 1) & MASK32
            for i in range(self.f.P):
                self.retire_pass(i)
        return ids


class SingleSightingOracle(SingleSighting, TriangulatingOracle):
    pass


class SingleSightingRetiringOracle(SingleSighting, TriangulatingRetiringOracle):
    pass


# ---------------------------------------------------------------------------------------------------------------- shared scenes
# grow_init_reference's small scene (64 particles, 10 preset + 3 unknown landmarks, v 0.8, w 0.35, dt 0.5, 14 steps, noise seed 6,
# noise-free wrapped scans) with noise-free ranges whose variances come from sigma = SIGMA[0] + SIGMA[1] rho; the unranged blobs go
# through the triangulated rule at MIN_PARALLAX.
C = gi.SMALL
SIGMA = (0.05, 0.01)
MIN_PARALLAX = 0.1
SEED = 6
R = 64
PHANTOM_STEP = 4
PHANTOM = (0.9, 128.0, 128.0, 128.0, 6.0)  # (bearing, r, g, b, range) of a blob no landmark stands behind
SCENES = {
    # name: (every (blobs every - 1, 2 every - 1, ... have no range) or None, spare slots, retirement (A, M) or None, phantom blob)
    "all_ranged": (None, 5, None, False),
    "every_3": (3, 5, None, False),        # the unknown landmark at index 11 has no range: it is triangulated
    "spare_2": (None, 2, None, False),     # the third unknown finds every spare slot taken: a stored reading at every step
    "retiring_phantom": (None, 5, (4, 3), True),
}


def scene_map(name):
    """(means, covs) of the device's map: the preset landmarks and the scene's empty spare slots."""
    spare = SCENES[name][1]
    world, covs = gi.small_world()
    L0 = C["L0"]
    means = np.zeros((L0 + spare, 5))
    means[:L0] = world[:L0]
    means[L0:, 2:] = EMPTY_COLOUR
    mcov = np.tile(np.identity(5), (L0 + spare, 1, 1))
    mcov[:L0] = covs[:L0]
    return means, mcov


def scene_oracle(name):
    _every, spare, retire, _phantom = SCENES[name]
    world, covs = gi.small_world()
    L0 = C["L0"]
    if retire:
        o = SingleSightingRetiringOracle(C["P"], world[:L0], covs[:L0], spare, C["thr"], retire[0], retire[1], min_parallax=MIN_PARALLAX)
    else:
        o = SingleSightingOracle(C["P"], world[:L0], covs[:L0], spare, C["thr"], min_parallax=MIN_PARALLAX)
    return o.under_ranges()


def scene_scan(name, world, pose, step):
    """(blobs (B, 4), ranges (B,), variances (B,)) of the scene's scan at ``pose``, step ``step``."""
    every, _spare, _retire, phantom = SCENES[name]
    blobs = wrapped_scan(world, pose)
    rng, var = range_scan(world, pose, None, SIGMA[0], SIGMA[1], every=every)
    if phantom and step == PHANTOM_STEP:
        blobs = np.vstack([blobs, PHANTOM[:4]])
        sig = SIGMA[0] + SIGMA[1] * PHANTOM[4]
        rng, var = np.append(rng, PHANTOM[4]), np.append(var, sig * sig)
    return blobs, rng, var


def scene_drive(name, o):
    """grow_init_reference.drive on the scene: the scan arms its ranges on the oracle, whose observe consumes them; behind every
    observe ``o.last_scan`` holds them for the device."""
    world, _ = gi.small_world()
    step = [0]

    def scan(w, pose, rs):
        blobs, rng, var = scene_scan(name, w, pose, step[0])
        step[0] += 1
        o.scan_ranges(rng, var)
        return blobs

    return gi.drive(o, world, C["steps"], SEED, C["v"], C["w"], C["dt"], scan)


def unknown_errors(o):
    """Per unknown landmark: the median over the particles of the distance from the truth to the nearest spare slot in use."""
    world, _ = gi.small_world()
    L0 = C["L0"]
    out = []
    for l in range(L0, L0 + C["U"]):
        d = []
        for i in range(o.f.P):
            m = o.f.mean[i, L0:L0 + o.used[i], :2]
            d.append(float(np.hypot(m[:, 0] - world[l, 0], m[:, 1] - world[l, 1]).min()) if len(m) else np.inf)
        out.append(float(np.median(d)))
    return out

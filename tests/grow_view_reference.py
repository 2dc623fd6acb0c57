"""A field of view for the retirement pass ("A field of view for retirement"; pk_grow_view,
k_grow_retire_view) in plain Python / NumPy float64 on top of tests/grow_retire_reference.py::RetiringOracle -- what the device is held
to, particle by particle -- and a seeded scene: a robot with a forward camera on a closed loop.  Needs no GPU.

With a view (half_fov, r_min, r_max) and a bound C = confirmed_max_misses, steps 2, 3 and 5 of the pass, the compaction and the state
of a vacated slot are RetiringOracle's; two steps change:
  1'. a spare slot the last pass knew: count word changed -> seen = word, idle = 0; word unchanged and the slot IN VIEW -> idle += 1
      (saturating); word unchanged and not in view -> idle stays
  4'. a slot goes if M > 0, its seen word is potential and idle >= M, or if C > 0, its seen word is promoted and idle >= C
In view, at the particle's live pose (px, py, ph) and the slot's position mean (mx, my), in this order:
    (sn, ch) = sincos(ph);  dx = mx - px, dy = my - py;  q = dx dx + dy dy;  a = dx ch + dy sn;  c = dy ch - dx sn
    in view  iff  q > 0  and  q >= r_min^2  and  q <= r_max^2  and  |atan2(c, a)| <= half_fov
"""
import math

import numpy as np

from oracle.fastslam_oracle import EMPTY_COLOUR, low_variance_ancestors, truth_step

from grow_retire_reference import INT32_MAX, MASK32, POTENTIAL, RetiringOracle

FULL_CIRCLE = (math.pi, 0.0, float("inf"))


def in_view(view, px, py, ph, mx, my):
    """(in view, margin): the decision in the operation order above (every product and sum rounded by itself), and how far it is
    from the nearest edge of the field: | |bearing| - half_fov | (no edge at half_fov = pi: |atan2| never exceeds it) and the
    relative distance of q from r_min^2, r_max^2 (none at +inf) and 0."""
    half_fov, r_min, r_max = view
    rmin2, rmax2 = r_min * r_min, r_max * r_max
    sn, ch = math.sin(ph), math.cos(ph)
    dx, dy = mx - px, my - py
    q = dx * dx + dy * dy
    a = dx * ch + dy * sn
    c = dy * ch - dx * sn
    bearing = math.atan2(c, a)
    inside = q > 0.0 and q >= rmin2 and q <= rmax2 and abs(bearing) <= half_fov
    edges = [1.0 if q > 0.0 else 0.0]
    if half_fov < math.pi:
        edges.append(abs(abs(bearing) - half_fov))
    for e in (rmin2, rmax2):
        if e > 0.0 and not math.isinf(e):
            edges.append(abs(q - e) / max(q, e))
    margin = min(edges)
    return bool(inside), (margin if margin == margin else 0.0)


class ViewingOracle(RetiringOracle):
    """RetiringOracle with the pass of 1' / 4'.  ``view=None``: RetiringOracle's own pass.  ``stats``: [unchanged slots the last pass
    knew, those in view, potential features retired, confirmed features retired], summed over the particles (the first two restart
    with every scan, the last two with ``set_view`` switching a view on).  ``margin``: the smallest margin of any in-view decision
    taken so far.  ``created`` / ``retiring`` are hooks for a scene's own counts (nothing here)."""

    def __init__(self, num_particles, means, covs, spare, pair_threshold, reading_max_age=0, potential_max_idle=0, view=None,
                 confirmed_max_misses=0):
        super(ViewingOracle, self).__init__(num_particles, means, covs, spare, pair_threshold, reading_max_age, potential_max_idle)
        self.view, self.C = None, 0
        self.stats = [0, 0, 0, 0]
        self.margin = float("inf")
        self.retired_out_of_view = 0  # slots a pass under the view rule retired while they were not in view at that pass
        self.set_view(view, confirmed_max_misses)

    def set_view(self, view, confirmed_max_misses=0):
        if view is None:
            self.view, self.C = None, 0
            return
        if self.view is None:
            self.stats = [0, 0, 0, 0]
        self.view, self.C = tuple(float(v) for v in view), int(confirmed_max_misses)

    def slot_in_view(self, i, j):
        f = self.f
        ok, margin = in_view(self.view, float(f.x[i]), float(f.y[i]), float(f.h[i]), float(f.mean[i, self.L0 + j, 0]),
                             float(f.mean[i, self.L0 + j, 1]))
        self.margin = min(self.margin, margin)
        return ok

    def created(self, i, j):
        pass

    def retiring(self, i, j, word):
        pass

    def goes(self, word, idle):
        if word & POTENTIAL:
            return self.M > 0 and idle >= self.M
        return self.C > 0 and idle >= self.C

    def retire_pass(self, i):
        if self.view is None:
            return super(ViewingOracle, self).retire_pass(i)
        f, L0, t = self.f, self.L0, self.t
        n, used = len(self.hyp[i]), self.used[i]
        scan, seen, idle = self.scan[i], self.seen[i], self.idle[i]
        cs, cr = min(self.covered_slots[i], used), min(self.covered_readings[i], n)
        del scan[cr:], seen[cs:], idle[cs:]
        viewed = {}
        for j in range(cs):                                  # 1'
            w = self.word(i, j)
            if w != seen[j]:
                seen[j], idle[j] = w, 0
            else:
                self.stats[0] += 1
                viewed[j] = self.slot_in_view(i, j)
                if viewed[j]:
                    self.stats[1] += 1
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
        keep = [j for j in range(used) if not self.goes(seen[j], idle[j])]   # 4'
        if len(keep) < used:
            for j in range(used):
                if j not in keep:
                    self.stats[2 if seen[j] & POTENTIAL else 3] += 1
                    self.retired_out_of_view += 0 if viewed.get(j, False) else 1
                    self.retiring(i, j, seen[j])
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

    def add_hypothesis(self, i, blob):
        u0 = self.used[i]
        super(ViewingOracle, self).add_hypothesis(i, blob)
        if self.used[i] > u0:
            self.created(i, u0)

    def observe(self, blobs):
        blobs = np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
        if self.view is not None and len(blobs):
            self.stats[0] = self.stats[1] = 0
        return super(ViewingOracle, self).observe(blobs)


# ---------------------------------------------------------------------------------------------------------------- the scene
class LoopScene(object):
    """A robot with a forward camera on a closed loop: a regular polygon of ``lap`` steps inscribed in a circle of radius ``radius``
    through the origin (start pose (0, 0, 0), centre (0, radius)), driven by truth_step.  ``L0`` preset and ``U`` unknown landmarks lie
    on two rings inside and outside the track, seeded; the last two unknown landmarks share one colour (twins: the pairs from which a
    false triangulation arises).  A scan holds a blob -- noise-free wrapped bearing and colour -- for exactly the landmarks, preset
    and unknown, that lie inside the camera's field ``view`` at the true pose."""

    def __init__(self, seed, L0=6, U=4, lap=16, radius=5.0, view=(0.9, 0.5, 9.0), dt=0.5):
        rs = np.random.RandomState(seed)
        self.L0, self.U, self.lap, self.radius, self.view, self.dt = L0, U, lap, float(radius), tuple(view), dt
        L = L0 + U
        phi = 2.0 * math.pi * (np.arange(L) + rs.uniform(-0.3, 0.3, size=L)) / L
        rho = np.where(np.arange(L) % 2 == 0, rs.uniform(1.4, 1.7, size=L), rs.uniform(0.62, 0.85, size=L)) * radius
        order = rs.permutation(L)  # which ring positions are the preset ones
        means = np.empty((L, 5))
        means[:, 0] = (rho * np.cos(phi))[order]
        means[:, 1] = radius + (rho * np.sin(phi))[order]
        means[:, 2:] = rs.uniform(20.0, 235.0, size=(L, 3))
        means[L - 1, 2:] = means[L - 2, 2:]
        self.world = means
        self.covs = np.broadcast_to(0.25 * np.identity(5), (L, 5, 5)).copy()
        self.w = 2.0 * math.pi / (lap * dt)
        self.v = 2.0 * radius * math.sin(math.pi / lap) / dt

    def known(self):
        return self.world[:self.L0], self.covs[:self.L0]

    def unknown(self):
        return self.world[self.L0:, :2]

    def step(self, pose):
        return truth_step(pose, self.v, self.w, self.dt)

    def visible(self, pose):
        return [l for l in range(len(self.world)) if in_view(self.view, pose[0], pose[1], pose[2], self.world[l, 0], self.world[l, 1])[0]]

    def scan(self, pose):
        vis = self.visible(pose)
        blobs = np.empty((len(vis), 4))
        for b, l in enumerate(vis):
            d = math.atan2(self.world[l, 1] - pose[1], self.world[l, 0] - pose[0]) - pose[2]
            blobs[b, 0] = math.atan2(math.sin(d), math.cos(d))
            blobs[b, 1:] = self.world[l, 2:]
        return blobs


class SceneProbe(ViewingOracle):
    """ViewingOracle with the scene's own counts, per lineage (they follow the particles through the resample): the features a pass
    retired while their position mean lay outside the camera's field at the TRUE pose (``truth``, set by the driver before every
    observe), and the re-discoveries -- a feature made within 1 m of an unknown landmark near which this lineage had retired one.
    Retirement WITHOUT a view is run here as view=FULL_CIRCLE with C = 0, which is RetiringOracle's pass array for array
    (tests/test_grow_view_host.py), so that the hooks see it."""

    def __init__(self, scene, *args, **kwargs):
        super(SceneProbe, self).__init__(*args, **kwargs)
        self.scene, self.truth = scene, (0.0, 0.0, 0.0)
        self.lost = [set() for _ in range(self.f.P)]
        self.retired_outside_truth = 0
        self.rediscoveries = 0

    def near(self, i, j):
        d = np.hypot(*(self.scene.unknown() - self.f.mean[i, self.L0 + j, :2]).T)
        k = int(np.argmin(d))
        return k if d[k] <= 1.0 else None

    def retiring(self, i, j, word):
        mx, my = self.f.mean[i, self.L0 + j, :2]
        if not in_view(self.scene.view, self.truth[0], self.truth[1], self.truth[2], float(mx), float(my))[0]:
            self.retired_outside_truth += 1
        k = self.near(i, j)
        if k is not None:
            self.lost[i].add(k)

    def created(self, i, j):
        k = self.near(i, j)
        if k is not None and k in self.lost[i]:
            self.rediscoveries += 1
            self.lost[i].discard(k)

    def gather(self, anc):
        super(SceneProbe, self).gather(anc)
        self.lost = [set(self.lost[a]) for a in anc]


def drive(scene, o, steps, seed, on_step=None, z_scale=1.0):
    """``steps`` steps of the scene on the oracle ``o`` with the oracle's twist motion (noise seed ``seed``), every scan followed by a
    low-variance resample in the log domain.  on_step(s, pose, blobs, z, u, logw, anc) is called behind every step's gather."""
    P = o.f.P
    rs = np.random.RandomState(seed)
    pose = (0.0, 0.0, 0.0)
    for s in range(steps):
        pose = scene.step(pose)
        blobs = scene.scan(pose)
        z, u = z_scale * rs.standard_normal((P, 3)), float(rs.uniform())
        o.f.reset_weights()
        o.f.motion(scene.v, scene.w, scene.dt, z)
        if hasattr(o, "truth"):
            o.truth = pose
        o.observe(blobs)
        logw = o.f.logw.copy()
        anc = low_variance_ancestors(np.exp(logw - np.max(logw)), u)
        o.gather(anc)
        if on_step:
            on_step(s, pose, blobs, z, u, logw, anc)


# ---------------------------------------------------------------------------------------------------------------- what the mode buys
def promoted_near(o, i, xy, radius=1.0):
    """Does particle i hold a promoted spare feature within ``radius`` of the point xy?"""
    for j in range(o.used[i]):
        if not o.f.potential[i, o.L0 + j] and np.hypot(*(o.f.mean[i, o.L0 + j, :2] - xy)) <= radius:
            return True
    return False


def ghosts(o, scene, radius=1.0):
    """Confirmed spare features farther than ``radius`` from every true landmark, summed over the particles."""
    n = 0
    for i in range(o.f.P):
        for j in range(o.used[i]):
            if not o.f.potential[i, o.L0 + j]:
                d = np.hypot(*(scene.world[:, :2] - o.f.mean[i, o.L0 + j, :2]).T)
                n += int(d.min() > radius)
    return n


def measure(cfg, seed, with_view, C):
    """One run of the scene ``cfg`` (the settings block of tests/golden/grow_view_scene.json) -> its recorded figures."""
    scene = LoopScene(cfg["scene_seed"], cfg["L0"], cfg["U"], cfg["lap"], cfg["radius"], tuple(cfg["view"]), cfg["dt"])
    known, kcov = scene.known()
    view = tuple(cfg["view"]) if with_view else FULL_CIRCLE
    o = SceneProbe(scene, cfg["P"], known, kcov, cfg["spare"], cfg["pair_threshold"], cfg["A"], cfg["M"], view=view,
                   confirmed_max_misses=C if with_view else 0)
    settled = []  # per step: how many unknown landmarks at least half of the particles hold a promoted feature near

    def on_step(s, pose, blobs, z, u, logw, anc):
        settled.append(sum(2 * sum(promoted_near(o, i, xy, cfg["confirm_radius"]) for i in range(o.f.P)) >= o.f.P for xy in scene.unknown()))

    drive(scene, o, cfg["steps"], seed, on_step)
    for_good = None
    for s in range(len(settled), 0, -1):
        if settled[s - 1] < scene.U:
            break
        for_good = s - 1
    return {"retired_outside_field": o.retired_outside_truth, "rediscoveries": o.rediscoveries, "confirmed_for_good_step": for_good,
            "unknown_confirmed_at_end": int(settled[-1]), "ghosts_at_end": ghosts(o, scene, cfg["ghost_radius"]), "potential_retired": o.stats[2],
            "confirmed_retired": o.stats[3]}


def measure_all(cfg):
    """Every run the golden file records: seeds x (no view, the view with C = 0, the view with the chosen C), the same M throughout."""
    modes = (("no_view", False, 0), ("view", True, 0), ("view_C", True, cfg["C"]))
    return {name: {str(seed): measure(cfg, seed, wv, C) for seed in cfg["seeds"]} for name, wv, C in modes}

"""Host: the triangulated initialisation of growing maps ("Parallax-gated pairing") on the CPU yardsticks --
tests/grow_init_reference.py::TriangulatingOracle against GrowingOracle, its covariance against a numerical Jacobian, the gain on
the drive that motivated it, the scenes of tests/test_gpu_grow_init.py checked for what makes them worth running, and the C ABI's
entry points.  Needs no GPU."""
import copy
import math
import os
import re

import numpy as np
import pytest

from oracle.fastslam_oracle import cross_readings, synthetic_world

import grow_init_reference as gi
from bearing_model_reference import under_bearing_model, wrapped_scan
from grow_init_reference import TriangulatingOracle, TriangulatingRetiringOracle, triangulated_covariance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ 1. min_parallax = 0: the plain pairing
class _Twinned(TriangulatingOracle):
    """Before every observe of its own, a copy of its state takes the same scan under the parent's rule (GrowingOracle.add_hypothesis)."""

    twin, is_twin = None, False

    def observe(self, blobs):
        if not self.is_twin:
            self.twin = None
            t = copy.deepcopy(self)
            t.is_twin = True
            t.triangulate(None)
            t.observe(blobs)
            self.twin = t
        return super(_Twinned, self).observe(blobs)


@pytest.mark.parametrize("name", ["reference_0.1", "bearing_0.1"])
def test_without_a_minimum_parallax_the_pairing_is_the_plain_oracles_reading_for_reading(name):
    """At every step of the small scene the same state goes through one observe under both rules: counters, stored readings, slot
    ids, means, counts, flags and weights are equal, value for value; the covariances differ in the position block of the features
    made at this step and nowhere else."""
    o = gi.small_oracle(name, min_parallax=0.0, cls=_Twinned)
    made = 0
    for st in gi.small_drive(name, o):
        t = o.twin  # (behind the observe, before the resample: the drive gathers o when the loop comes back)
        assert t.hyp == o.hyp and t.used == o.used and t.next_id == o.next_id and t.slot_id == o.slot_id, st.s
        assert np.array_equal(t.f.mean, o.f.mean) and np.array_equal(t.f.count, o.f.count), st.s
        assert np.array_equal(t.f.potential, o.f.potential) and np.array_equal(t.f.logw, o.f.logw), st.s
        new = np.zeros(o.f.cov.shape, dtype=bool)
        for i, slot, _rid, _me, _p in o.made[made:]:
            new[i, slot, :2, :2] = True
            assert np.array_equal(t.f.cov[i, slot], np.identity(5)), st.s
        assert np.array_equal(t.f.cov[~new], o.f.cov[~new]), st.s
        assert len(o.made) == made or not np.array_equal(t.f.cov[new], o.f.cov[new]), st.s
        made = len(o.made)
    assert made > 0 and not o.excluded and not o.changed  # sin 0 = 0: the gate lets every crossing through


# ------------------------------------------------------------------------------------------ 2. the covariance is J Q J'
def test_the_covariance_is_the_numerical_jacobian_of_cross_readings_in_the_two_bearings():
    """P = J diag(q00, q00) J' with J the central-difference Jacobian of oracle.cross_readings in (t1, t3), step h = 3e-6.

    Tolerance, from the step: a coordinate of the crossing is N(t) / D(t) in either bearing, N and D trigonometric polynomials of
    degree one with |N^(k)| <= rho (the largest range in play, here < 40 m) and |D| = |sd| >= sd_min, |D^(k)| <= 1; differentiating
    the quotient three times gives |f'''| <= 24 rho / sd_min^4 for sd_min <= 1.  The central difference is off by h^2 / 6 of that,
    plus the rounding of cross_readings -- products of coordinates, rho^2 / sd_min in size, each good to an ulp -- over h:
        dJ = h^2 / 6 * 24 rho / sd_min^4 + 4 eps rho^2 / sd_min / h
    and P = q00 J J' moves by at most q00 (2 |J| dJ + dJ^2) summed over the two columns, |J| <= rho / sd_min."""
    rs = np.random.RandomState(12)
    h, eps, q00 = 3e-6, np.finfo(np.float64).eps, 0.1
    rho, checked, worst = 40.0, 0, 0.0
    while checked < 200:
        target = rs.uniform(-1, 1, 2)
        target *= rs.uniform(8.0, 30.0) / np.linalg.norm(target)
        x1, y1, px, py = rs.uniform(-4, 4, 4)
        t1, t3 = math.atan2(target[1] - y1, target[0] - x1), math.atan2(target[1] - py, target[0] - px)
        sd = abs(math.sin(t3 - t1))
        if sd < 0.05:
            continue
        ox, oy = cross_readings(x1, y1, t1, px, py, t3)
        J = np.empty((2, 2))
        J[:, 0] = (np.array(cross_readings(x1, y1, t1 + h, px, py, t3)) - np.array(cross_readings(x1, y1, t1 - h, px, py, t3))) / (2 * h)
        J[:, 1] = (np.array(cross_readings(x1, y1, t1, px, py, t3 + h)) - np.array(cross_readings(x1, y1, t1, px, py, t3 - h))) / (2 * h)
        want = q00 * J @ J.T
        got = triangulated_covariance(x1, y1, t1, px, py, t3, ox, oy, q00)
        sd_min = sd - 2 * h
        dJ = h * h / 6 * 24 * rho / sd_min ** 4 + 4 * eps * rho * rho / sd_min / h
        tol = 2 * q00 * (2 * rho / sd_min * dJ + dJ * dJ)
        err = max(abs(got[0] - want[0, 0]), abs(got[1] - want[0, 1]), abs(got[1] - want[1, 0]), abs(got[2] - want[1, 1]))
        assert err <= tol, (checked, err, tol, sd)
        assert tol < 1e-3 * max(want[0, 0], want[1, 1]), (tol, want)  # (the bound is worth something: a thousandth of the variance)
        worst = max(worst, err / tol)
        checked += 1
    assert worst > 0.0


def test_the_covariance_degenerates_as_the_geometry_says():
    # rays at right angles from (0, 0) along x and from (5, -5) along y: they cross at (5, 0), 5 m from both
    pxx, pxy, pyy = triangulated_covariance(0.0, 0.0, 0.0, 5.0, -5.0, math.pi / 2, 5.0, 0.0, 0.1)
    # a change of the first bearing moves the crossing along the second ray (y) by 5 m / rad, and the other way round
    assert pxx == pytest.approx(0.1 * 25.0, rel=1e-12) and pyy == pytest.approx(0.1 * 25.0, rel=1e-12) and abs(pxy) < 1e-12


# ------------------------------------------------------------------------------------------ 3. the drive that motivated it
@pytest.fixture(scope="module")
def table_drive():
    """under_bearing_model, 64 particles, synthetic_world(12, seed=5) with its last three landmarks unknown, 6 spare slots, pair
    threshold 30; v = 1.0, w = 0.35, dt = 0.5, wrapped_scan with sigma 0.01 rad and 0.3 per colour channel, 60 steps, resampled at
    every step, seeds 1-3: {(seed, rule): (errors of every spare feature in use, slots in use per particle)}."""
    world, covs = synthetic_world(12, seed=5)
    L0 = 9

    def scan(w, pose, rs):
        return wrapped_scan(w, pose, rs, 0.01, 0.3)

    out = {}
    for seed in (1, 2, 3):
        for rule, mp in (("plain", None), ("triangulated", 0.2)):
            o = under_bearing_model(TriangulatingOracle(64, world[:L0], covs[:L0], 6, 30.0, min_parallax=mp))
            if mp is None:
                assert o.min_parallax is None
            for _ in gi.drive(o, world, 60, seed, 1.0, 0.35, 0.5, scan):
                pass
            e = []
            for i in range(o.f.P):
                for k in range(o.used[i]):
                    m = o.f.mean[i, L0 + k]
                    j = int(np.argmin(np.linalg.norm(world[L0:, 2:] - m[2:], axis=1)))
                    e.append(float(np.hypot(m[0] - world[L0 + j, 0], m[1] - world[L0 + j, 1])))
            out[(seed, rule)] = (np.array(e), list(o.used))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_rule_places_the_discovered_landmarks_nearer_than_the_plain_one(table_drive, seed):
    plain, used_plain = table_drive[(seed, "plain")]
    tri, used = table_drive[(seed, "triangulated")]
    print("seed %d: plain median %.2f mean %.2f max %.1f; triangulated median %.2f mean %.2f max %.1f"
          % (seed, np.median(plain), plain.mean(), plain.max(), np.median(tri), tri.mean(), tri.max()))
    assert np.median(tri) < np.median(plain) and tri.mean() < plain.mean()
    assert used == [3] * 64 and used_plain == [3] * 64  # exactly the three unknown landmarks, in every particle


# ------------------------------------------------------------------------------------------ 4. the GPU tests' scenes
@pytest.mark.parametrize("name", sorted(gi.GPU_SCENES))
def test_the_gpu_scenes_decide_something_and_rounding_cannot_turn_it(name):
    """What tests/test_gpu_grow_init.py runs on the device, on the CPU oracle alone: no gate decision within 1e-9 of its threshold
    (an ulp of sincos cannot turn one), readings excluded, pairings changed, features made and promoted, no ring overrun."""
    o = gi.small_oracle(name)
    R = gi.GPU_SCENES[name][2]
    gates = (np.inf, np.inf)
    for st in gi.small_drive(name, o):
        if st.gates:
            gates = (min(gates[0], st.gates[0]), min(gates[1], st.gates[1]))
    print("%s: margin %.3g, %d readings excluded, %d pairings changed, %d features made, promoted per particle %d..%d, longest ring %d"
          % (name, o.margin, len(o.excluded), len(o.changed), len(o.made), gi.promoted(o).min(), gi.promoted(o).max(), o.longest_ring))
    assert o.margin > 1e-9
    assert gates[0] > 1e-9 and gates[1] > 1e-6  # (the bearing model's association gates, as test_gpu_bearing_model.py asks)
    assert len(o.excluded) > 0 and len(o.changed) > 0 and len(o.made) > 0
    assert gi.promoted(o).max() >= 1
    assert o.longest_ring <= R
    if name.startswith("bearing") and "retiring" not in name:
        assert (gi.promoted(o) == 3).all() and o.used == [3] * o.f.P  # the three unknown landmarks, promoted in every particle
    if name == "reference_0.1":
        assert o.longest_ring > 64  # the search and the gate run beyond the wave's 64 lanes
    if "retiring" in name:
        assert isinstance(o, TriangulatingRetiringOracle) and sum(o.readings_retired) > 0


# ------------------------------------------------------------------------------------------ 5. the C ABI
def test_the_header_the_library_and_the_binding_know_pk_grow_init():
    from parakeet_slam_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "parakeet_slam.h")).read()
    assert re.search(r"int\s+pk_grow_init\s*\(\s*pk_filter\s*\*\s*f\s*,\s*int32_t\s+mode\s*,\s*double\s+min_parallax\s*\)\s*;", header)
    assert re.search(r"int\s+pk_grow_init_mode\s*\(", header)
    assert re.search(r"#define\s+PK_GROW_INIT_REFERENCE\s+0\b", header) and re.search(r"#define\s+PK_GROW_INIT_TRIANGULATED\s+1\b", header)
    assert "pk_grow_init" in _lib.SIGNATURES and "pk_grow_init_mode" in _lib.SIGNATURES
    assert (_lib.PK_GROW_INIT_REFERENCE, _lib.PK_GROW_INIT_TRIANGULATED) == (0, 1)
    assert _lib.LANDMARK_INITS == {"reference": 0, "triangulated": 1}
    assert hasattr(_lib.DeviceFilter, "grow_init") and hasattr(_lib.DeviceFilter, "grow_init_mode")
    import ctypes

    so = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(so, "pk_grow_init") and hasattr(so, "pk_grow_init_mode")


def test_the_facade_refuses_before_any_device_work():
    import parakeet_slam_amd as pk

    with pytest.raises(ValueError, match="landmark_init='nearest'"):
        pk.FastSLAM([], num_particles=4, new_landmarks=True, spare_landmarks=2, landmark_init="nearest")
    for bad in (-0.1, 1.6, float("nan"), "wide"):
        with pytest.raises(ValueError, match="min_parallax"):
            pk.FastSLAM([], num_particles=4, new_landmarks=True, spare_landmarks=2, landmark_init="triangulated", min_parallax=bad)
    with pytest.raises(ValueError, match="new_landmarks=True"):
        pk.FastSLAM([], num_particles=4, landmark_init="triangulated")
    with pytest.raises(ValueError, match="new_landmarks=True"):
        pk.FastSLAM([], num_particles=4, devices=[0, 1], landmark_init="triangulated")

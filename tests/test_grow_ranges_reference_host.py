"""Host: ranged scans on a growing map (pk_grow_ranges; DESIGN.md section 9, "Single-sighting initialisation") on the CPU yardstick
tests/grow_ranges_reference.py -- the closed form against the measured point's dense covariance, the scenes of
tests/test_gpu_grow_ranges.py checked for what makes them worth running and for verdicts rounding cannot turn, the facade's
refusals and the C ABI's entry points.  Needs no GPU."""
import math
import os
import re

import numpy as np
import pytest

import grow_init_reference as gi
import grow_ranges_reference as gr
from range_bearing_reference import measured_point_covariance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = gi.SMALL
L0 = C["L0"]


def _run(name):
    """The scene on the oracle: (oracle, per step (used, promoted, ring lengths, readings made), smallest gates)."""
    o = gr.scene_oracle(name)
    rows = []
    gates = (np.inf, np.inf)
    for st in gr.scene_drive(name, o):
        gates = (min(gates[0], st.gates[0]), min(gates[1], st.gates[1]))
        rows.append((list(o.used), gi.promoted(o).copy(), [len(h) for h in o.hyp]))
    return o, rows, gates


@pytest.fixture(scope="module")
def runs():
    return {name: _run(name) for name in gr.SCENES}


def _guards(o, gates, gate_ran):
    """No verdict within 1e-9 of its threshold: an ulp of the device's sincos cannot turn one."""
    assert gates[0] > 1e-9 and gates[1] > 1e-9, gates
    assert o.f.min_gate_margins[0] > 1e-9 and o.f.min_gate_margins[1] > 1e-9, o.f.min_gate_margins
    assert o.f.min_rel_gap == np.inf  # no contested verdict
    if gate_ran:
        assert o.margin > 1e-9, o.margin


def test_the_closed_form_is_the_measured_points_covariance():
    """q_rho u u' + rho^2 q00 n n' in dense algebra (range_bearing_reference.measured_point_covariance over a zero prior) against
    the three expressions, and the point itself."""
    rs = np.random.RandomState(2)
    for _ in range(50):
        px, py, ph, zb = rs.uniform(-5, 5), rs.uniform(-5, 5), rs.uniform(-3, 3), rs.uniform(-3, 3)
        rho, q_rho, q00 = rs.uniform(0.5, 30.0), rs.uniform(1e-3, 0.2), rs.uniform(1e-4, 0.05)
        mx, my, pxx, pxy, pyy = gr.single_sighting(px, py, ph, zb, rho, q_rho, q00)
        ux, uy = math.cos(ph + zb), math.sin(ph + zb)
        S = measured_point_covariance(np.zeros((2, 2)), np.float64(ux), np.float64(uy), rho, q_rho, q00)
        assert np.allclose([[pxx, pxy], [pxy, pyy]], S, rtol=1e-12, atol=1e-15)
        assert mx == pytest.approx(px + rho * ux, rel=1e-14) and my == pytest.approx(py + rho * uy, rel=1e-14)
        assert pxx > 0 and pxx * pyy - pxy * pxy > 0


def test_all_ranged_scene_three_features_at_once_promoted_at_step_3_nearer_than_triangulated(runs):
    o, rows, gates = runs["all_ranged"]
    for s, (used, promoted, ring) in enumerate(rows):
        assert used == [3] * C["P"], s            # exactly the three unknown landmarks, from the first scan on
        assert ring == [0] * C["P"], s            # the ring stays empty
        assert (promoted == (3 if s >= 3 else 0)).all(), (s, promoted)  # made at 0, matched at 1, 2, 3: count 6 > 5
    assert len(o.single) == 3 * C["P"] and not o.made
    _guards(o, gates, gate_ran=False)
    tri = gi.small_oracle("bearing_0.1")
    for _ in gi.small_drive("bearing_0.1", tri):
        pass
    e_single, e_tri = gr.unknown_errors(o), gr.unknown_errors(tri)
    print("per-landmark median error: single sighting %s, triangulated %s" % (e_single, e_tri))
    assert all(a < b for a, b in zip(e_single, e_tri)), (e_single, e_tri)


def test_every_third_scene_runs_both_rules(runs):
    """Blobs 2, 5, 8, 11 carry no range: the unknown landmark at index 11 is triangulated, the other two placed at once."""
    o, rows, gates = runs["every_3"]
    P = C["P"]
    assert o.used == [3] * P
    # (the two logs are of events, ahead of the resamples that copy and drop their particles: told apart by the features' ids)
    single_ids, made_ids = {m[2] for m in o.single}, {m[3] for m in o.made}
    assert single_ids and made_ids and not (single_ids & made_ids)
    for i in range(P):
        ids = list(o.slot_id[i].values())
        assert sum(1 for v in ids if v in single_ids) == 2 and sum(1 for v in ids if v in made_ids) == 1, (i, ids)
    first_all = next(s for s, (_u, promoted, _r) in enumerate(rows) if (promoted == 3).all())
    print("every_3: all three promoted in every particle at step %d; margin %.3g" % (first_all, o.margin))
    assert first_all <= 11
    assert max(max(r) for _u, _p, r in rows) <= gr.R
    _guards(o, gates, gate_ran=True)


def test_two_spare_slots_leave_the_third_unknown_a_stored_reading_per_step(runs):
    o, rows, gates = runs["spare_2"]
    P = C["P"]
    for s, (used, _promoted, ring) in enumerate(rows):
        assert used == [2] * P and ring == [s + 1] * P, s  # a ranged blob with every slot taken: a reading, every step
    assert rows[-1][2] == [14] * P and 14 <= gr.R          # nothing is dropped at R = 64
    assert not o.made                                       # (no slot is free when a pairing is found)
    _guards(o, gates, gate_ran=True)


def test_the_phantom_is_made_once_and_retired_three_scans_later(runs):
    o, rows, gates = runs["retiring_phantom"]
    P, t0 = C["P"], gr.PHANTOM_STEP
    for s, (used, _promoted, ring) in enumerate(rows):
        assert used == [4 if t0 <= s < t0 + 3 else 3] * P, (s, used)
        assert ring == [0] * P
    assert sum(o.features_retired) == P and o.promoted_vacated == 0
    _guards(o, gates, gate_ran=False)


def test_the_header_the_library_and_the_binding_know_pk_grow_ranges():
    from parakeet_slam_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "parakeet_slam.h")).read()
    assert re.search(r"int\s+pk_grow_ranges\s*\(\s*pk_filter\s*\*\s*f\s*,\s*int32_t\s+on\s*\)\s*;", header)
    assert re.search(r"int\s+pk_grow_ranges_state\s*\(\s*const\s+pk_filter\s*\*\s*f\s*,\s*int32_t\s*\*\s*on\s*\)\s*;", header)
    assert "pk_grow_ranges" in _lib.SIGNATURES and "pk_grow_ranges_state" in _lib.SIGNATURES
    assert hasattr(_lib.DeviceFilter, "grow_ranges") and hasattr(_lib.DeviceFilter, "grow_ranges_state")
    assert _lib.LANDMARK_INITS == {"reference": 0, "triangulated": 1}  # a switch of its own, no third pk_grow_init mode
    import ctypes

    so = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(so, "pk_grow_ranges") and hasattr(so, "pk_grow_ranges_state")
    so.pk_grow_ranges.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    so.pk_grow_ranges_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert so.pk_grow_ranges(None, 1) == _lib.PK_ERR_INVALID and so.pk_grow_ranges_state(None, None) == _lib.PK_ERR_INVALID


def test_the_facade_refuses_before_any_device_work():
    import parakeet_slam_amd as pk

    world, covs = gi.small_world()
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L0)]
    kw = dict(num_particles=4, measurement_model="bearing")
    with pytest.raises(ValueError, match="grow_ranges=True"):  # no range_noise
        pk.FastSLAM(feats, new_landmarks=True, spare_landmarks=2, grow_ranges=True, **kw)
    with pytest.raises(ValueError, match="grow_ranges=True"):  # a preset map
        pk.FastSLAM(feats, range_noise=gr.SIGMA, grow_ranges=True, **kw)
    with pytest.raises(ValueError, match="grow_ranges=True"):  # no spare slot
        pk.FastSLAM(feats, range_noise=gr.SIGMA, new_landmarks=True, spare_landmarks=0, grow_ranges=True, **kw)
    with pytest.raises(ValueError, match="grow_ranges=True"):  # the rule is the device kernel's
        pk.FastSLAM(feats, range_noise=gr.SIGMA, new_landmarks=True, spare_landmarks=2, bookkeeping="host", grow_ranges=True, **kw)
    with pytest.raises(ValueError, match="grow_ranges=True"):
        pk.FastSLAM(feats, range_noise=gr.SIGMA, new_landmarks=True, spare_landmarks=2, proposal="measurement", grow_ranges=True, **kw)
    with pytest.raises(ValueError, match="new_landmarks=True"):  # without the keyword: the refusal as it was
        pk.FastSLAM(feats, range_noise=gr.SIGMA, new_landmarks=True, spare_landmarks=2, **kw)
    with pytest.raises(TypeError):  # the sharded facade does not take the keyword
        pk.ShardedFastSLAM(feats, num_particles=4, devices=[0, 0], grow_ranges=True)

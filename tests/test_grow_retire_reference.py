"""CPU: the retirement rule of growing maps as tests/grow_retire_reference.py::RetiringOracle states it, on the small scene
of test_gpu_grow.py run for 14 steps instead of 9 (64 particles, 10 known + 3 unknown landmarks, 5 spare slots, seed 5, 13
blobs per scan).  Without retirement that scene fills every spare slot and lets the ring pass 64 readings; with readings
older than 4 scans dropped and potential features idle for 3 scans retired, the ring is bounded by 4 scans' blobs and more
features reach promotion."""
import numpy as np
import pytest

from oracle.fastslam_oracle import GrowingOracle, low_variance_ancestors, synthetic_scan, synthetic_world, truth_step

from grow_retire_reference import RetiringOracle

P, L0, U, SPARE, STEPS, SEED, THR = 64, 10, 3, 5, 14, 5, 30.0
V, W, DT = 0.8, 0.35, 0.5


def run(oracles, steps=STEPS, each_step=None):
    world, covs = synthetic_world(L0 + U, seed=123)
    rs = np.random.RandomState(SEED)
    pose = (0.0, 0.0, 0.0)
    for s in range(steps):
        pose = truth_step(pose, V, W, DT)
        blobs = synthetic_scan(world, pose)
        z = rs.standard_normal((P, 3))
        u = float(rs.uniform())
        for o in oracles:
            o.f.reset_weights()
            o.f.motion(V, W, DT, z)
            o.observe(blobs)
            o.gather(low_variance_ancestors(np.exp(o.f.logw - np.max(o.f.logw)), u))  # pk_resample, log domain
        if each_step:
            each_step(s)


def make(cls, **kw):
    world, covs = synthetic_world(L0 + U, seed=123)
    return cls(P, world[:L0], covs[:L0], SPARE, THR, **kw)


def promoted(o):
    return int(((o.f.count[:, L0:] > 5) & ~o.f.potential[:, L0:]).sum())


@pytest.fixture(scope="module")
def runs():
    plain, off, on = make(GrowingOracle), make(RetiringOracle), make(RetiringOracle, reading_max_age=4, potential_max_idle=3)
    plain_ring = []
    run([plain, off, on], each_step=lambda s: plain_ring.append(max(len(h) for h in plain.hyp)))
    return plain, off, on, plain_ring


def test_with_both_thresholds_zero_the_subclass_is_the_plain_oracle(runs):
    plain, off, _, _ = runs
    for name in ("x", "y", "h", "logw", "mean", "cov", "count", "potential"):
        assert np.array_equal(getattr(plain.f, name), getattr(off.f, name)), name
    assert plain.hyp == off.hyp and plain.next_id == off.next_id and plain.used == off.used and plain.slot_id == off.slot_id
    assert not any(off.readings_retired) and not any(off.features_retired)
    # the clocks run all the same: every stored reading has a stamp, every slot in use its word
    assert [len(s) for s in off.scan] == [len(h) for h in off.hyp] and [len(s) for s in off.seen] == off.used


def test_retirement_bounds_the_ring_and_frees_slots_for_real_landmarks(runs):
    plain, _, on, plain_ring = runs
    assert min(on.features_retired) >= 1 and min(on.readings_retired) >= 1, "some particle retired nothing"
    assert on.max_ring <= 52, "a ring held more than 4 scans x 13 blobs"
    assert max(plain_ring) > 64, "the plain oracle's ring never passes the device's default capacity: the scene shows nothing"
    assert promoted(on) > promoted(plain), (promoted(on), promoted(plain))
    assert on.promoted_vacated == 0, "a promoted feature was vacated"

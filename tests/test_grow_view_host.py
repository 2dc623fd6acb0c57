"""CPU: the view rule of the retirement pass (tests/grow_view_reference.py::ViewingOracle; DESIGN.md section 9, "A field of view for
retirement") against RetiringOracle and against what the rule says, and what the mode buys on the loop scene
(tests/golden/grow_view_scene.json: settings and recorded results, reproduced here exactly).  Needs no GPU."""
import json
import math
import os

import numpy as np

from grow_retire_reference import INT32_MAX, POTENTIAL, RetiringOracle
from grow_view_reference import FULL_CIRCLE, LoopScene, ViewingOracle, drive, in_view, measure_all

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grow_view_scene.json")
THR = 30.0


def _state(o):
    """Everything a pass can change, in comparable form."""
    return (o.t, [list(h) for h in o.hyp], list(o.used), [dict(d) for d in o.slot_id], list(o.next_id), [list(v) for v in o.scan],
            [list(v) for v in o.seen], [list(v) for v in o.idle], o.clock_counters().tolist(), o.f.mean.copy(), o.f.cov.copy(),
            o.f.count.copy(), o.f.potential.copy(), o.f.logw.copy(), o.f.x.copy(), o.f.y.copy(), o.f.h.copy())


def _same(a, b):
    for u, v in zip(a, b):
        if isinstance(u, np.ndarray):
            assert np.array_equal(u, v)
        else:
            assert u == v


def test_the_full_circle_without_a_bound_is_the_retiring_oracle_array_for_array():
    scene = LoopScene(5, L0=8, U=4, lap=32)
    known, kcov = scene.known()
    a = RetiringOracle(8, known, kcov, 8, THR, 6, 3)
    b = ViewingOracle(8, known, kcov, 8, THR, 6, 3, view=FULL_CIRCLE, confirmed_max_misses=0)
    ra, rb = [], []
    drive(scene, a, 40, 1, lambda *x: ra.append(_state(a)))
    drive(scene, b, 40, 1, lambda *x: rb.append(_state(b)))
    assert len(ra) == len(rb) == 40
    for sa, sb in zip(ra, rb):
        _same(sa, sb)
    assert sum(a.features_retired) > 0 and sum(a.readings_retired) > 0, "the scene retires nothing: the test shows nothing"
    assert b.stats[2] > 0 and b.stats[3] == 0


def _one_particle(view, M, C, slots, pose=(0.0, 0.0, 0.0)):
    """A one-particle oracle with hand-placed spare features ``slots`` = [(x, y, word)], covered by the last pass with idle 0."""
    known = np.array([[40.0, 40.0, 250.0, 250.0, 250.0]])
    o = ViewingOracle(1, known, 0.25 * np.identity(5).reshape(1, 5, 5), 8, THR, 0, M, view=view, confirmed_max_misses=C)
    o.f.x[0], o.f.y[0], o.f.h[0] = pose
    for j, (x, y, word) in enumerate(slots):
        o.f.mean[0, 1 + j] = (x, y, 10.0 + 40.0 * j, 20.0, 30.0)
        o.f.count[0, 1 + j], o.f.potential[0, 1 + j] = word & ~POTENTIAL, bool(word & POTENTIAL)
        o.slot_id[0][1 + j] = 100 + j
        o.seen[0].append(word)
        o.idle[0].append(0)
    o.used[0] = o.covered_slots[0] = len(slots)
    return o


NOTHING = np.array([[3.0, 100.0, 50.0, 20.0]])  # a blob that matches nothing and pairs with nothing


def _scan(o):
    o.f.reset_weights()
    o.hyp[0] = []  # (no reading to pair with: the scan makes no feature)
    o.covered_readings[0] = 0
    o.observe(NOTHING)


def test_a_slot_that_is_never_in_view_keeps_its_idle_for_the_whole_run():
    view = (0.5, 1.0, 20.0)
    # behind the robot, too near, too far, just outside the cone; one ahead, which ages and goes
    slots = [(-5.0, 0.0, POTENTIAL | 2), (0.5, 0.0, POTENTIAL), (25.0, 0.0, 8), (5.0 * math.cos(0.6), 5.0 * math.sin(0.6), POTENTIAL),
             (5.0, 0.0, POTENTIAL)]
    o = _one_particle(view, 3, 0, slots)
    o.idle[0][:4] = [1, 2, INT32_MAX, 2]
    for s in range(12):
        _scan(o)
        assert o.idle[0][:4] == [1, 2, INT32_MAX, 2], s
        assert o.used[0] == (5 if s < 2 else 4), s
    assert o.stats == [4, 0, 1, 0] and o.retired_out_of_view == 0
    assert [o.slot_id[0][1 + j] for j in range(4)] == [100, 101, 102, 103]


def test_a_promoted_feature_goes_after_exactly_c_misses_in_view_and_never_with_c_zero():
    view = (0.5, 1.0, 20.0)
    for C in (1, 4):
        o = _one_particle(view, 0, C, [(6.0, 1.0, 8), (-6.0, 1.0, 8)])
        for s in range(C):
            assert o.used[0] == 2 and o.idle[0] == [s, 0], (C, s)
            _scan(o)
        assert o.used[0] == 1 and o.slot_id[0] == {1: 101} and o.stats[2:] == [0, 1], C
        assert o.features_retired[0] == 1
    o = _one_particle(view, 2, 0, [(6.0, 1.0, 8)])
    for s in range(30):
        _scan(o)
    assert o.used[0] == 1 and o.idle[0] == [30] and o.stats[3] == 0


def test_a_hit_in_between_restarts_the_count():
    o = _one_particle((0.5, 1.0, 20.0), 0, 3, [(6.0, 1.0, 8)])
    _scan(o)
    _scan(o)
    assert o.idle[0] == [2]
    o.f.count[0, 1] += 2  # a match: the count word changed
    _scan(o)
    assert o.idle[0] == [0] and o.seen[0] == [10] and o.used[0] == 1
    _scan(o)
    _scan(o)
    assert o.used[0] == 1 and o.idle[0] == [2]
    _scan(o)
    assert o.used[0] == 0 and o.stats[3] == 1


def test_under_the_view_rule_no_feature_is_retired_at_a_pass_where_it_is_out_of_view():
    scene = LoopScene(5, L0=8, U=4, lap=32)
    known, kcov = scene.known()
    o = ViewingOracle(8, known, kcov, 8, THR, 6, 3, view=scene.view, confirmed_max_misses=4)
    drive(scene, o, 64, 2)
    assert o.stats[2] > 0 and o.stats[3] > 0, "the scene retires nothing: the test shows nothing"
    assert o.retired_out_of_view == 0
    assert o.margin > 0.0


def test_in_view_edges_and_nans():
    v = (0.5, 1.0, 4.0)
    assert in_view(v, 0.0, 0.0, 0.0, 2.0, 0.0)[0]
    assert in_view(v, 0.0, 0.0, 0.0, 1.0, 0.0)[0] and in_view(v, 0.0, 0.0, 0.0, 4.0, 0.0)[0]  # the edges belong to the field
    assert not in_view(v, 0.0, 0.0, 0.0, 0.999, 0.0)[0] and not in_view(v, 0.0, 0.0, 0.0, 4.001, 0.0)[0]
    assert not in_view(v, 0.0, 0.0, math.pi, 2.0, 0.0)[0] and in_view(v, 0.0, 0.0, math.pi, -2.0, 0.0)[0]
    assert not in_view((math.pi, 0.0, float("inf")), 1.0, 1.0, 0.3, 1.0, 1.0)[0]  # q = 0: the slot sits on the sensor
    assert in_view((math.pi, 0.0, float("inf")), 1.0, 1.0, 0.3, -1e9, 1.0)[0]
    for bad in ((float("nan"), 0.0, 0.0, 2.0, 0.0), (0.0, 0.0, float("nan"), 2.0, 0.0), (0.0, 0.0, 0.0, 2.0, float("nan"))):
        assert not in_view(v, *bad)[0] and not in_view((math.pi, 0.0, float("inf")), *bad)[0]


def test_the_golden_file_reproduces_exactly_and_says_what_the_mode_buys():
    with open(GOLDEN) as fh:
        gold = json.load(fh)
    cfg = gold["settings"]
    assert cfg["seeds"] == [1, 2, 3] and cfg["C"] > 0 and cfg["M"] > 0
    assert measure_all(cfg) == gold["results"]
    # the file holds settings and recorded results only
    assert set(gold) == {"settings", "results"} and set(gold["results"]) == {"no_view", "view", "view_C"}

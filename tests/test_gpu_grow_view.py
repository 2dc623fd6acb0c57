"""GPU: a field of view for the retirement pass (pk_grow_view, k_grow_retire_view in pk_k_grow_retire.hip; DESIGN.md section 9, "A
field of view for retirement").  The checker is tests/grow_view_reference.py::ViewingOracle, particle by particle: counters, clocks,
slot ids, count words, flags and the four statistics exactly; means, covariances, readings and log-weights to the tolerances of
test_gpu_grow_retire.py (its _compare is used as it is).

The device's sincos / pk_atan2 may differ from NumPy's by an ulp, so a decision of the oracle closer than 1e-9 to an edge of the
field is not a test of the kernel: every comparison against the oracle first asserts the oracle's recorded margin.  The scenes and
hand-written states were chosen on the CPU so that the oracle alone stays above it -- a condition on the inputs, not a tolerance."""
import math
import random

import numpy as np
import pytest

from oracle.fastslam_oracle import EMPTY_COLOUR, low_variance_ancestors

import odom_reference as odo
import test_gpu_grow_retire as tgr
from grow_retire_reference import INT32_MAX, POTENTIAL
from grow_view_reference import FULL_CIRCLE, LoopScene, ViewingOracle, in_view

pytestmark = pytest.mark.gpu

THR = 30.0
MARGIN = 1e-9
ALPHAS = (0.05, 0.01, 0.05, 0.01)
# the driven scene: 8 preset + 4 unknown landmarks round a loop of 24 steps, a camera of +-1 rad between 0.5 and 10 m
SCENE = dict(seed=8, L0=8, U=4, lap=24, view=(1.0, 0.5, 10.0))
P_SCENE, SPARE, RING, A_SCENE, M_SCENE, C_SCENE = 64, 5, 64, 4, 2, 2


def _scene():
    return LoopScene(SCENE["seed"], L0=SCENE["L0"], U=SCENE["U"], lap=SCENE["lap"], view=SCENE["view"])


def _filter(lib, P, known, kcov, spare, R, A, M, view=None, C=0):
    f = tgr._device_filter(lib, P, known, kcov, spare, R, A, M)
    if view is not None:
        f.grow_view(view[0], view[1], view[2], C)
    return f


def _compare(lib, f, o, L0, step):
    assert o.margin >= MARGIN, (step, o.margin)
    tgr._compare(lib, f, o, L0, step)
    if o.view is not None:
        assert np.array_equal(f.grow_view_stats(), o.stats), (step, f.grow_view_stats(), o.stats)


def _everything(f):
    """Every download, the rows beyond what a particle stores or uses (undefined) zeroed."""
    cnt, rd, sid = f.grow_download()
    kc, sc, se, si, now = f.grow_clocks_download()
    rd, sid, sc, se, si = rd.copy(), sid.copy(), sc.copy(), se.copy(), si.copy()
    for i in range(f.P):
        rd[i, cnt[i, 0]:], sc[i, cnt[i, 0]:] = 0.0, 0
        sid[i, cnt[i, 1]:], se[i, cnt[i, 1]:], si[i, cnt[i, 1]:] = 0, 0, 0
    return [f.download_poses(), f.download_log_weights(), *f.download_landmarks(), cnt, rd, sid, kc, sc, se, si, np.array(now)]


def _oracle_step(o, prev, pose, blobs, z, u):
    d = odo.delta(prev, pose)
    o.f.reset_weights()
    o.f.x, o.f.y, o.f.h = odo.sample(o.f.x, o.f.y, o.f.h, d, ALPHAS, z)
    o.observe(blobs)
    logw = o.f.logw.copy()
    o.gather(low_variance_ancestors(np.exp(logw - np.max(logw)), u))
    return d


def _run_scene(lib, opts, route, steps=12, view=SCENE["view"], C=C_SCENE, changes=None):
    """The scene through pk_step_odom (motion, scan, bookkeeping, retirement, resample in the log domain) against the oracle at
    every step.  changes: {step: (view or None, C)} set before that step's scan."""
    sc = _scene()
    known, kcov = sc.known()
    f = _filter(lib, P_SCENE, known, kcov, SPARE, RING, A_SCENE, M_SCENE, view, C)
    for k_, v_ in opts.items():
        f.set_option(k_, v_)
    o = ViewingOracle(P_SCENE, known, kcov, SPARE, THR, A_SCENE, M_SCENE, view=view, confirmed_max_misses=C)
    rs = np.random.RandomState(5)
    pose = (0.0, 0.0, 0.0)
    for s in range(steps):
        if changes and s in changes:
            v2, c2 = changes[s]
            o.set_view(v2, c2)
            if v2 is None:
                f.grow_view(0.0)
            else:
                f.grow_view(v2[0], v2[1], v2[2], c2)
        prev, pose = pose, sc.step(pose)
        blobs = sc.scan(pose)
        assert len(blobs) > 0
        z, u = rs.standard_normal((P_SCENE, 3)), float(rs.uniform())
        d = _oracle_step(o, prev, pose, blobs, z, u)
        f.step_odom(d, ALPHAS, blobs, u, z=z, domain=lib.PK_WEIGHTS_LOG)
        assert f.observe_route() in route, (f.observe_route(), route)
        _compare(lib, f, o, sc.L0, s)
    return f, o


# ---------------------------------------------------------------------------------------------------------------- 1. the driven scene
ONE_PASS, GENERAL = ("ml_fused", "ml_regs"), ("ml_general",)


@pytest.mark.parametrize("opts,route", [({}, ONE_PASS), ({"fast_observe": 0}, GENERAL)])
def test_the_driven_scene_against_the_oracle_at_every_step(lib, opts, route):
    """64 particles, 12 steps through pk_step_odom, resample included; readings older than 4 scans, potential features with 2 and
    promoted features with 2 misses in view go."""
    f, o = _run_scene(lib, opts, route)
    kc = f.grow_clocks_download()[0]
    assert o.stats[2] > 0 and o.stats[3] > 0 and kc[:, 2].sum() > 0, "nothing of some kind was retired: the test shows less than it says"
    assert 0 < o.stats[1] < o.stats[0], "every unchanged slot was in view, or none: the view decided nothing"
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 2. hand-written states
HP, HS, HUSED, HR = 6, 70, 66, 16
H_VIEW = (1.0, 2.0, 15.0)
# the ring of slots is at angle 2 pi j / 66: slots 62..65 lie at -0.381, -0.286, -0.190, -0.095 rad.  With half_fov = 1 the first
# heading sees 62 and 63 but not 64 and 65, the second 64 and 65 but not 62 and 63, the third all four, the fourth none of them
H_HEAD = (-1.24, 0.76, -0.3, 2.5, 3.0, -2.9)
H_COVERED = (66, 66, 66, 66, 60, 66)  # (particle 4: slots 60..65 are new to the pass -- stamped, not looked at)
H_TARGETS = (5, 63, 64, 30)  # the slots the scan's blobs carry the colour of


def _slot_colour(j):
    return 10.0 + 60.0 * (j % 5), 10.0 + 60.0 * ((j // 5) % 5), 10.0 + 60.0 * (j // 25)


def _slot_xy(j):
    rad = 20.0 if j % 11 == 3 else 1.0 if j % 13 == 5 else 10.0  # beyond r_max, inside r_min, in range
    ang = 2.0 * math.pi * j / HUSED
    return rad * math.cos(ang), rad * math.sin(ang)


def _slot_clock(j, M, C, top):
    """(count word, idle) of slot j before the pass: one pass short of its bound, at ``top``, or fresh."""
    m1, c1 = max(M - 1, 0), max(C - 1, 0)
    if j % 3 == 0:  # promoted
        return 6 + 2 * (j % 4), (c1 if j % 2 else top if j % 4 == 0 else 0)
    return POTENTIAL | (j % 5), (m1 if j % 2 == 0 else top if j % 7 == 0 else 0)


def _hand_state(lib, f, o, M, C, t0=41, top=INT32_MAX):
    """HP particles at nearly one place with different headings, 66 of 70 spare slots in use on a ring round them, the clocks one
    pass short of M and C or saturated -- in the filter (pk_upload_landmarks, pk_grow_upload, pk_grow_clocks_upload) and in the
    oracle."""
    L0, L = 1, 1 + HS
    m, c, k = f.download_landmarks()
    c = c.reshape(HP, L, 25)
    cnt = np.zeros((HP, 4), dtype=np.int32)
    rd = np.zeros((HP, HR, 8))
    sid = np.zeros((HP, HS), dtype=np.int32)
    kc = np.zeros((HP, 4), dtype=np.int32)
    sc = np.zeros((HP, HR), dtype=np.uint32)
    se = np.zeros((HP, HS), dtype=np.int32)
    si = np.zeros((HP, HS), dtype=np.int32)
    xyhw = np.zeros((HP, 4))
    for i in range(HP):
        xyhw[i] = (0.11 * i, -0.07 * i, H_HEAD[i], 1.0)
        cnt[i] = (0, HUSED, 1000 + i, 0)
        kc[i] = (0, H_COVERED[i], 10 * i, 3 * i)
        for j in range(HUSED):
            m[i, L0 + j] = _slot_xy(j) + _slot_colour(j)
            cov = np.identity(5) * (1.0 + j / 128.0)
            cov[0, 1] = cov[1, 0] = 0.125
            c[i, L0 + j] = cov.reshape(25)
            word, idle = _slot_clock(j, M, C, top)
            k[i, L0 + j] = word
            se[i, j], si[i, j] = word, idle
            sid[i, j] = 100 + j
        o.f.mean[i], o.f.cov[i] = m[i], c[i].reshape(L, 5, 5)
        o.f.count[i], o.f.potential[i] = k[i] & ~POTENTIAL, (k[i] & POTENTIAL) != 0
        o.hyp[i] = []
        o.next_id[i], o.used[i] = 1000 + i, HUSED
        o.slot_id[i] = {L0 + j: 100 + j for j in range(HUSED)}
        o.scan[i], o.seen[i], o.idle[i] = [], [int(v) for v in se[i, :HUSED]], [int(v) for v in si[i, :HUSED]]
        o.covered_readings[i], o.covered_slots[i], o.readings_retired[i], o.features_retired[i] = 0, H_COVERED[i], 10 * i, 3 * i
    o.f.x, o.f.y, o.f.h = xyhw[:, 0].copy(), xyhw[:, 1].copy(), xyhw[:, 2].copy()
    o.t = t0
    f.upload_poses(xyhw)
    f.upload_landmarks(0, HP, m, c, k)
    f.grow_upload(0, HP, cnt, rd, sid)
    f.grow_clocks_upload(0, HP, kc, sc, se, si, scan_now=t0)
    return m, k, se, si


def _hand_scan(m, pose):
    """One blob in the colour of each target slot, at the bearing it has from ``pose``, and one that matches nothing."""
    blobs = [[odo.wrap(math.atan2(m[0, 1 + j, 1] - pose[1], m[0, 1 + j, 0] - pose[0]) - pose[2])] + list(m[0, 1 + j, 2:]) for j in H_TARGETS]
    return np.array(blobs + [[0.3, 600.0, 600.0, 600.0]])


HAND_KNOWN = np.array([[40.0, 40.0, 400.0, 400.0, 400.0]])
HAND_KCOV = 0.25 * np.identity(5).reshape(1, 5, 5)


@pytest.mark.parametrize("M,C", [(3, 5), (0, 4), (3, 0)])
def test_hand_written_states_across_the_waves_edges(lib, M, C):
    """6 particles (a workgroup of four waves and half of one), 70 spare slots of which 66 are in use: slots 62..65, either side of
    the 64-lane turn, hold in-view and out-of-view, potential and promoted ones, the idle values sit at M - 1, C - 1 and INT32_MAX,
    and one scan matches four of the slots.  Afterwards every array equals the oracle's, compaction across the turn included.
    (M, C) = (0, 4) and (3, 0): the saturated counts of the kind that is never retired stay where they are."""
    A = 0 if M else 1000  # (M = 0 needs a reading age to keep retirement on; no reading here is that old)
    f = _filter(lib, HP, HAND_KNOWN, HAND_KCOV, HS, HR, A, M, H_VIEW, C)
    o = ViewingOracle(HP, HAND_KNOWN, HAND_KCOV, HS, THR, A, M, view=H_VIEW, confirmed_max_misses=C)
    m, k, se, si = _hand_state(lib, f, o, M, C)
    # what the cases were written for, on the oracle's own decisions
    seen = {i: [in_view(H_VIEW, o.f.x[i], o.f.y[i], o.f.h[i], m[i, 1 + j, 0], m[i, 1 + j, 1])[0] for j in (62, 63, 64, 65)] for i in range(4)}
    assert seen == {0: [True, True, False, False], 1: [False, False, True, True], 2: [True] * 4, 3: [False] * 4}
    assert {bool(k[0, 1 + j] & POTENTIAL) for j in (62, 63, 64, 65)} == {True, False}
    blobs = _hand_scan(m, (o.f.x[2], o.f.y[2], o.f.h[2]))
    f.observe(blobs, fresh=True)
    o.f.reset_weights()
    o.observe(blobs)
    assert np.allclose(f.download_log_weights(), o.f.logw, rtol=1e-9, atol=1e-9)
    _compare(lib, f, o, 1, "M = %d, C = %d" % (M, C))
    gone = o.stats[2] + o.stats[3]
    assert (o.stats[2] > 0) == (M > 0) and (o.stats[3] > 0) == (C > 0) and gone > 0
    assert min(o.used) < 62 < max(H_COVERED), "no particle compacts across the 64-lane turn"
    assert 0 < o.stats[1] < o.stats[0]
    si2 = f.grow_clocks_download()[3]  # (rows beyond the slots in use are undefined)
    assert any((si2[i, :o.used[i]] == INT32_MAX).any() for i in range(HP)) == (M == 0 or C == 0), "a saturated count that stays"
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the full circle
def test_the_full_circle_without_a_bound_is_a_filter_without_a_view(lib):
    sc = _scene()
    known, kcov = sc.known()
    fa = _filter(lib, P_SCENE, known, kcov, SPARE, RING, A_SCENE, M_SCENE, FULL_CIRCLE, 0)
    fb = _filter(lib, P_SCENE, known, kcov, SPARE, RING, A_SCENE, M_SCENE)
    assert fa.grow_view_state() == (True, FULL_CIRCLE, 0) and fb.grow_view_state() == (False, (0.0, 0.0, 0.0), 0)
    rs = np.random.RandomState(5)
    pose = (0.0, 0.0, 0.0)
    for s in range(8):
        prev, pose = pose, sc.step(pose)
        blobs = sc.scan(pose)
        z, u = rs.standard_normal((P_SCENE, 3)), float(rs.uniform())
        for f in (fa, fb):
            f.step_odom(odo.delta(prev, pose), ALPHAS, blobs, u, z=z, domain=lib.PK_WEIGHTS_LOG)
        for a, b in zip(_everything(fa), _everything(fb)):
            assert np.array_equal(a, b), s
        st = fa.grow_view_stats()
        assert st[0] == st[1] and st[3] == 0, (s, st)
    assert fa.grow_clocks_download()[0][:, 3].sum() > 0 and fa.grow_view_stats()[2] > 0, "nothing was retired"
    fa.close()
    fb.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the proposal
def test_behind_the_proposal_the_view_is_taken_at_the_sampled_poses(lib):
    """pk_propose_odom with pk_proposal_grow on the hand-written state, M = C = 2^30 so that nothing moves: idle is what 1' gives from
    the words before and after the step and in_view at the downloaded -- sampled -- poses."""
    big = 2 ** 30
    f = lib.DeviceFilter(HP, 1 + HS)
    f.set_measurement_model("bearing")
    means = np.zeros((1 + HS, 5))
    means[:1] = HAND_KNOWN
    means[1:, 2:] = EMPTY_COLOUR
    covs = np.tile(np.identity(5).reshape(25), (1 + HS, 1))
    covs[:1] = HAND_KCOV.reshape(1, 25)
    f.upload_map(means, covs)
    f.grow_enable(1, HR, THR)
    f.grow_retire(0, big)
    f.grow_view(H_VIEW[0], H_VIEW[1], H_VIEW[2], big)
    f.proposal_grow(True)
    o = ViewingOracle(HP, HAND_KNOWN, HAND_KCOV, HS, THR, 0, big, view=H_VIEW, confirmed_max_misses=big)  # (the state's mirror only)
    m, k, se, si = _hand_state(lib, f, o, 3, 5, top=7)  # (no saturated count: INT32_MAX is beyond 2^30 and would go)
    before = f.download_poses()
    z = np.random.RandomState(3).standard_normal((HP, 3))
    delta = (0.2, 0.5, -0.1)
    aim = odo.compose(before[2, :3], delta)  # the blobs are aimed from where particle 2 is predicted to stand
    f.propose_odom(delta, ALPHAS, _hand_scan(m, aim), z=z, fresh=True)
    poses = f.download_poses()
    assert not np.allclose(poses[:, :3], before[:, :3]), "the poses did not move: sampled and prior poses cannot be told apart"
    m2, _, k2 = f.download_landmarks()
    kc2, _, se2, si2, now = f.grow_clocks_download()
    assert now == 42 and np.array_equal(kc2[:, 1], [HUSED] * HP) and not f.grow_view_stats()[2:].any()
    same = aged = changed = 0
    sampled, prior = [], []
    for i in range(HP):
        for j in range(HUSED):
            if j >= H_COVERED[i] or k2[i, 1 + j] != se[i, j]:
                want = 0
                changed += j < H_COVERED[i]
            else:
                ok, margin = in_view(H_VIEW, poses[i, 0], poses[i, 1], poses[i, 2], m2[i, 1 + j, 0], m2[i, 1 + j, 1])
                assert margin >= MARGIN, (i, j, margin)
                assert np.array_equal(m2[i, 1 + j, :2], m[i, 1 + j, :2]), "an unchanged slot's mean was touched"
                want = min(int(si[i, j]) + 1, INT32_MAX) if ok else int(si[i, j])
                same += 1
                aged += ok
                sampled.append(ok)
                prior.append(in_view(H_VIEW, before[i, 0], before[i, 1], before[i, 2], m2[i, 1 + j, 0], m2[i, 1 + j, 1])[0])
            assert si2[i, j] == want and se2[i, j] == k2[i, 1 + j], (i, j, si2[i, j], want)
    assert changed > 0 and 0 < aged < same
    assert tuple(f.grow_view_stats()[:2]) == (same, aged)
    assert prior != sampled, "the poses before the move decide the same everywhere: the test cannot tell them from the sampled ones"
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 5. mid-run changes
def test_changes_in_mid_run_hold_from_the_next_pass_and_the_view_goes_with_the_clocks(lib):
    f, o = _run_scene(lib, {}, ONE_PASS, steps=12, view=None, C=0,
                      changes={3: ((0.6, 1.0, 8.0), 1), 6: (SCENE["view"], 3), 8: (None, 0), 10: (SCENE["view"], 2)})
    assert o.stats[2] + o.stats[3] > 0
    clocks = 2 * 4 * P_SCENE * (RING + 2 * SPARE + 4)
    on = f.device_bytes()
    assert f.grow_view_state() == (True, SCENE["view"], 2)
    f.grow_retire(A_SCENE + 1, M_SCENE)  # any other pk_grow_retire call leaves the view alone
    assert f.grow_view_state() == (True, SCENE["view"], 2) and f.device_bytes() == on
    f.grow_view(0.0, 5.0, 1.0, -7)  # off: the other arguments are ignored; the counters stay until the clocks go
    assert f.grow_view_state() == (False, (0.0, 0.0, 0.0), 0) and f.device_bytes() == on
    f.grow_view(0.5, 0.0, 3.0, 9)
    assert f.grow_view_state() == (True, (0.5, 0.0, 3.0), 9) and f.device_bytes() == on
    f.grow_retire(0, 0)  # frees the clocks and clears the view with them
    assert f.grow_view_state() == (False, (0.0, 0.0, 0.0), 0)
    base = f.device_bytes()
    assert on - base == clocks + lib.PK_GROW_VIEW_STATS_BYTES
    f.grow_retire(A_SCENE, M_SCENE)  # the clocks alone: what the filter held before a view was first set
    assert f.grow_view_state() == (False, (0.0, 0.0, 0.0), 0) and f.device_bytes() == base + clocks
    f.grow_view(0.0)  # off while off: nothing is allocated
    assert f.device_bytes() == base + clocks
    f.grow_view(*SCENE["view"], 1)
    assert f.device_bytes() == on
    f.grow_retire(0, 0)
    assert f.device_bytes() == base
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 6. arguments and state
def test_arguments_and_state(lib):
    sc = _scene()
    known, kcov = sc.known()
    g = lib.DeviceFilter(4, 5)
    for call in (lambda: g.grow_view(1.0, 0.0, 5.0, 0), g.grow_view_stats):
        with pytest.raises(lib.PkError, match="pk_grow_enable was not called") as e:
            call()
        assert e.value.status == lib.PK_ERR_STATE
    assert g.grow_view_state() == (False, (0.0, 0.0, 0.0), 0)
    g.close()
    f = _filter(lib, 8, known, kcov, 3, 8, 0, 0)
    for call in (lambda: f.grow_view(1.0, 0.0, 5.0, 0), lambda: f.grow_view(0.0), f.grow_view_stats):
        with pytest.raises(lib.PkError, match="nothing is being retired") as e:  # retirement is off: no clocks
            call()
        assert e.value.status == lib.PK_ERR_STATE
    assert f.grow_view_state() == (False, (0.0, 0.0, 0.0), 0)
    f.grow_retire(4, 3)
    with pytest.raises(lib.PkError, match="without a field of view") as e:  # stats before a view
        f.grow_view_stats()
    assert e.value.status == lib.PK_ERR_STATE
    nan, inf = float("nan"), float("inf")
    bad = [(nan, 0.0, 5.0, 0), (-0.1, 0.0, 5.0, 0), (3.2, 0.0, 5.0, 0), (inf, 0.0, 5.0, 0),
           (1.0, nan, 5.0, 0), (1.0, -1.0, 5.0, 0), (1.0, inf, inf, 0),
           (1.0, 1.0, nan, 0), (1.0, 2.0, 2.0, 0), (1.0, 2.0, 1.0, 0),
           (1.0, 0.0, 5.0, -1), (1.0, 0.0, 5.0, 2 ** 30 + 1)]
    for state in ((False, (0.0, 0.0, 0.0), 0), (True, (0.7, 0.25, inf), 2 ** 30)):
        if state[0]:
            f.grow_view(0.7, 0.25, inf, 2 ** 30)  # (+inf for the far range and C = 2^30 are allowed)
        bytes0 = f.device_bytes()
        for args in bad:
            with pytest.raises(lib.PkError, match="pk_grow_view: ") as e:
                f.grow_view(*args)
            assert e.value.status == lib.PK_ERR_INVALID, args
            assert f.grow_view_state() == state and f.device_bytes() == bytes0, args
    f.grow_view(math.pi, 0.0, 1e-3, 0)
    assert f.grow_view_state() == (True, (math.pi, 0.0, 1e-3), 0)
    assert not f.grow_view_stats().any()
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 7. the facade
def test_facade_runs_the_scene_saves_and_restores(lib, tmp_path):
    """FastSLAM(..., view=, confirmed_max_misses=) on the scene under the twist model (rng='global': the motion noise comes from
    numpy's global stream, the resample draw from random.random()), against the oracle; save_state at step 6, load_state into a new
    filter, and both continue identically."""
    import parakeet_slam_amd as pk

    sc = _scene()
    known, kcov = sc.known()
    P, steps = 32, 13
    feats = [pk.Feature(mean=known[l].copy(), covar=kcov[l].copy()) for l in range(sc.L0)]
    kw = dict(num_particles=P, weight_domain="log", rng="global", new_landmarks=True, spare_landmarks=SPARE,
              reading_max_age=A_SCENE, potential_max_idle=M_SCENE, view=SCENE["view"], confirmed_max_misses=C_SCENE)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = sc.v, sc.w

    def make(now):
        pk.msgs.Time.set_now(now)
        fs_ = pk.FastSLAM(feats, device=0, **kw)
        fs_.last_control = tw
        return fs_

    fs = make(0.0)
    assert fs._filter.grow_view_state() == (True, SCENE["view"], C_SCENE)
    o = ViewingOracle(P, known, kcov, SPARE, THR, A_SCENE, M_SCENE, view=SCENE["view"], confirmed_max_misses=C_SCENE)
    pose, fs2, path = (0.0, 0.0, 0.0), None, str(tmp_path / "view.npz")
    for s in range(steps):
        pose = sc.step(pose)
        blobs = sc.scan(pose)
        for who in (fs, fs2):
            if who is not None:
                np.random.seed(100 + s)
                random.seed(200 + s)
                pk.msgs.Time.set_now(sc.dt * (s + 1))
                who.cam_cb(tgr._View(pk, blobs))
        # against the oracle, on the same numbers
        z, u = np.random.RandomState(100 + s).standard_normal((P, 3)), random.Random(200 + s).random()
        o.f.reset_weights()
        o.f.motion(sc.v, sc.w, sc.dt, z)
        o.observe(blobs)
        o.gather(low_variance_ancestors(np.exp(o.f.logw - np.max(o.f.logw)), u))
        _compare(lib, fs._filter, o, sc.L0, "facade %d" % s)
        assert fs.view_stats() == tuple(o.stats)
        if s == 5:  # six steps done
            fs.save_state(path)
            fs2 = make(sc.dt * (s + 1))
            fs2.load_state(path)
        if fs2 is not None:
            for a, b in zip(_everything(fs._filter), _everything(fs2._filter)):
                assert np.array_equal(a, b), s
            assert fs.view_stats()[:2] == fs2.view_stats()[:2]
    assert sum(fs.view_stats()[2:]) > 0 and fs.retired()[1] == sum(o.features_retired) > 0
    assert fs2.retired() == fs.retired()
    assert "view" not in " ".join(np.load(path).files), "the view is configuration: no snapshot holds it"
    fs.close()
    fs2.close()


def test_facade_value_errors():
    import parakeet_slam_amd as pk

    sc = _scene()
    known, kcov = sc.known()
    feats = [pk.Feature(mean=known[l].copy(), covar=kcov[l].copy()) for l in range(4)]
    pk.msgs.Time.set_now(0.0)
    grow = dict(num_particles=8, new_landmarks=True, spare_landmarks=2)
    v = (1.0, 0.5, 10.0)
    with pytest.raises(ValueError, match="reading_max_age=... or potential_max_idle"):
        pk.FastSLAM(feats, view=v, **grow)
    with pytest.raises(ValueError, match="bookkeeping='host'"):
        pk.FastSLAM(feats, view=v, bookkeeping="host", **grow)
    with pytest.raises(ValueError, match="bookkeeping='host'"):
        pk.FastSLAM(feats, num_particles=8, view=v, potential_max_idle=3)
    with pytest.raises(ValueError, match="one GPU only"):
        pk.FastSLAM(feats, view=v, potential_max_idle=3, devices=[0, 0], **grow)
    with pytest.raises(ValueError, match="give view="):
        pk.FastSLAM(feats, confirmed_max_misses=3, potential_max_idle=3, **grow)
    for bad in ((0.0, 0.5, 10.0), (4.0, 0.5, 10.0), (1.0, -1.0, 10.0), (1.0, 5.0, 5.0), (1.0, 0.5), "wide", (float("nan"), 0.0, 1.0)):
        with pytest.raises(ValueError, match="half_fov, r_min, r_max"):
            pk.FastSLAM(feats, view=bad, potential_max_idle=3, **grow)
    for bad in (-1, 2 ** 30 + 1):
        with pytest.raises(ValueError, match="0..2\\^30"):
            pk.FastSLAM(feats, view=v, confirmed_max_misses=bad, potential_max_idle=3, **grow)
    fs = pk.FastSLAM(feats, potential_max_idle=3, **grow)
    with pytest.raises(ValueError, match="without view="):
        fs.view_stats()
    fs.close()

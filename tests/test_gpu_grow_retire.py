"""GPU: growing maps that also shrink (pk_grow_retire, k_grow_retire in pk_k_grow_retire.hip).  Behind the
bookkeeping of every scan each particle drops the stale prefix of its reading ring and retires the potential features that went
unmatched, compacting its spare slots.  The checker is tests/grow_retire_reference.py::RetiringOracle, particle by particle at
every step: counters, readings and slot ids in use, count words, potential flags and the clocks exactly; means, covariances and
log-weights to the tolerances of test_gpu_grow.py."""
import random

import numpy as np
import pytest

from oracle.fastslam_oracle import EMPTY_COLOUR, low_variance_ancestors, synthetic_scan, synthetic_world, truth_step

from grow_retire_reference import POTENTIAL, RetiringOracle

pytestmark = pytest.mark.gpu

THR = 30.0
V, W, DT = 0.8, 0.35, 0.5
A_SCENE, M_SCENE = 4, 3


def _scene(L0, U, seed=123):
    world, covs = synthetic_world(L0 + U, seed=seed)
    return world, covs, world[:L0], covs[:L0]


def _device_filter(lib, P, known, kcov, spare, R, A=0, M=0):
    L0 = len(known)
    f = lib.DeviceFilter(P, L0 + spare)
    means = np.zeros((L0 + spare, 5))
    means[:L0] = known
    means[L0:, 2:] = EMPTY_COLOUR
    covs = np.tile(np.identity(5).reshape(25), (L0 + spare, 1))
    covs[:L0] = np.asarray(kcov).reshape(L0, 25)
    f.upload_map(means, covs)
    f.grow_enable(L0, R, THR)
    if A or M:
        f.grow_retire(A, M)
    return f


def _empty_beyond_used(m, c, k, used, L0):
    """Every spare slot beyond the ones in use -- never used, or vacated -- is the empty state, bit for bit."""
    P, L = k.shape
    beyond = np.arange(L - L0)[None, :] >= np.asarray(used)[:, None]
    em = np.array([0.0, 0.0, EMPTY_COLOUR, EMPTY_COLOUR, EMPTY_COLOUR])
    assert np.array_equal(m[:, L0:][beyond], np.broadcast_to(em, (int(beyond.sum()), 5)))
    assert np.array_equal(c.reshape(P, L, 25)[:, L0:][beyond], np.broadcast_to(np.identity(5).reshape(25), (int(beyond.sum()), 25)))
    assert not k[:, L0:][beyond].any()


def _compare(lib, f, o, L0, step):
    cnt, rd, sid = f.grow_download()
    assert np.array_equal(cnt[:, 0], [len(h) for h in o.hyp]), "step %s: readings stored" % (step,)
    assert np.array_equal(cnt[:, 1], o.used), "step %s: spare slots in use" % (step,)
    assert np.array_equal(cnt[:, 2], o.next_id), "step %s: next_id" % (step,)
    assert not cnt[:, 3].any(), "step %s: readings dropped" % (step,)
    kc, sc, se, si, now = f.grow_clocks_download()
    assert now == o.t, (step, now, o.t)
    assert np.array_equal(kc, o.clock_counters()), "step %s: covered / retired counters" % (step,)
    for i in range(f.P):
        n, used = int(cnt[i, 0]), int(cnt[i, 1])
        if n:
            assert np.allclose(rd[i, :n], np.asarray(o.hyp[i]), rtol=1e-12, atol=1e-12), (step, i)
            assert np.array_equal(rd[i, :n, 0], [h[0] for h in o.hyp[i]]), (step, i, "reading ids")
        assert [int(v) for v in sid[i, :used]] == [o.slot_id[i][L0 + k] for k in range(used)], (step, i)
        assert [int(v) for v in sc[i, :n]] == o.scan[i], (step, i, "stamps")
        assert [int(v) for v in se[i, :used]] == o.seen[i], (step, i, "seen")
        assert [int(v) for v in si[i, :used]] == o.idle[i], (step, i, "idle")
    m, c, k = f.download_landmarks()
    assert np.array_equal((k & lib.PK_LANDMARK_POTENTIAL) != 0, o.f.potential), step
    assert np.array_equal(k & ~lib.PK_LANDMARK_POTENTIAL, o.f.count), step
    assert np.allclose(m, o.f.mean, rtol=1e-8, atol=1e-8), step
    assert np.allclose(c.reshape(o.f.cov.shape), o.f.cov, rtol=1e-8, atol=1e-9), step
    _empty_beyond_used(m, c, k, cnt[:, 1], L0)


def _oracle_step(o, z, blobs, u):
    o.f.reset_weights()
    o.f.motion(V, W, DT, z)
    o.observe(blobs)
    logw = o.f.logw.copy()
    anc = low_variance_ancestors(np.exp(logw - np.max(logw)), u)
    o.gather(anc)
    return logw, anc


def _run_scene(lib, opts, route, A=A_SCENE, M=M_SCENE, steps=14, change_at=None):
    P, L0, U, spare, R = 64, 10, 3, 5, 64
    world, covs, known, kcov = _scene(L0, U)
    f = _device_filter(lib, P, known, kcov, spare, R, A, M)
    for k_, v_ in opts.items():
        f.set_option(k_, v_)
    o = RetiringOracle(P, known, kcov, spare, THR, A, M)
    rs = np.random.RandomState(5)
    pose = (0.0, 0.0, 0.0)
    for s in range(steps):
        if change_at and s in change_at:  # other thresholds in mid-run: from the next pass on
            o.A, o.M = change_at[s]
            f.grow_retire(*change_at[s])
        pose = truth_step(pose, V, W, DT)
        blobs = synthetic_scan(world, pose)
        z = rs.standard_normal((P, 3))
        f.motion(V, W, DT, z=z)
        f.observe(blobs, fresh=True)
        assert f.observe_route() == route, (f.observe_route(), route)
        u = float(rs.uniform())
        logw, anc = _oracle_step(o, z, blobs, u)
        assert np.allclose(f.download_log_weights(), logw, rtol=1e-9, atol=1e-9), s
        assert np.array_equal(f.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), s
        _compare(lib, f, o, L0, s)
    kc = f.grow_clocks_download()[0]
    f.close()
    return kc, o


@pytest.mark.parametrize("opts,route", [({}, "ml_fused"), ({"fast_observe": 0}, "ml_general")])
def test_the_scene_against_the_oracle_at_every_step(lib, opts, route):
    """64 particles, 10 known + 3 unknown landmarks, 5 spare slots, seed 5, 14 steps, R = 64: readings older than 4 scans and
    potential features idle for 3 go.  Without retirement this scene fills the ring (test_grow_retire_reference.py): here nothing is
    dropped, and every particle retired both readings and features."""
    kc, o = _run_scene(lib, opts, route)
    assert (kc[:, 2] > 0).all() and (kc[:, 3] > 0).all(), "some particle retired nothing"
    assert o.promoted_vacated == 0


def test_thresholds_changed_in_mid_run_hold_from_the_next_pass(lib):
    kc, o = _run_scene(lib, {}, "ml_fused", A=0, M=6, steps=12, change_at={5: (3, 2), 9: (0, 4)})
    assert kc[:, 2].sum() > 0 and kc[:, 3].sum() > 0


def test_one_pass_against_general_on_a_larger_map(lib):
    """12 particles, 700 + 3 landmarks, 5 spare slots, R = 128, retirement on: the bit rows k_step_pub leaves must give the
    bookkeeping and the retirement behind it exactly what the general association's ids give them, array for array -- compaction
    does not disturb the route."""
    P, L0, U, spare, steps = 12, 700, 3, 5, 9
    world, covs, known, kcov = _scene(L0, U)
    fa = _device_filter(lib, P, known, kcov, spare, 128, A_SCENE, M_SCENE)
    fb = _device_filter(lib, P, known, kcov, spare, 128, A_SCENE, M_SCENE)
    fb.set_option("fast_observe", 0)
    rs = np.random.RandomState(7 + L0)
    pose, on_kernel = (0.0, 0.0, 0.0), 0
    for s in range(steps):
        pose = truth_step(pose, V, W, DT)
        blobs = synthetic_scan(world, pose)
        z = rs.standard_normal((P, 3))
        for f in (fa, fb):
            f.motion(V, W, DT, z=z)
            f.observe(blobs, fresh=True)
        assert fa.observe_route() == "ml_regs" and fa.observe_published() and fb.observe_route() == "ml_general"
        on_kernel += P - fa.observe_flagged()[0]
        (ca, ra, sa), (cb, rb, sb) = fa.grow_download(), fb.grow_download()
        ka, kb = fa.grow_clocks_download(), fb.grow_clocks_download()
        assert np.array_equal(ca, cb) and np.array_equal(ka[0], kb[0]) and ka[4] == kb[4] == s + 1, s
        for i in range(P):
            n, used = ca[i, 0], ca[i, 1]
            assert np.array_equal(ra[i, :n], rb[i, :n]) and np.array_equal(sa[i, :used], sb[i, :used]), (s, i)
            assert np.array_equal(ka[1][i, :n], kb[1][i, :n]), (s, i)
            assert np.array_equal(ka[2][i, :used], kb[2][i, :used]) and np.array_equal(ka[3][i, :used], kb[3][i, :used]), (s, i)
        la, lb = fa.download_landmarks(), fb.download_landmarks()
        for xa, xb in zip(la, lb):
            assert np.array_equal(xa, xb), s
        _empty_beyond_used(la[0], la[1], la[2], ca[:, 1], L0)
        assert np.allclose(fa.download_log_weights(), fb.download_log_weights(), rtol=1e-11, atol=1e-9), s
        u = float(rs.uniform())
        assert np.array_equal(fa.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), fb.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True))
    kc = fa.grow_clocks_download()[0]
    assert on_kernel >= P * 2, "hardly any particle stayed on the one-pass kernel"
    assert kc[:, 2].sum() > 0 and kc[:, 3].sum() > 0, "nothing was retired: the test shows nothing about compaction"
    fa.close()
    fb.close()


# ---- hand-written states: S = 70 spare slots and a ring of R = 150, the smallest shapes that cross the wave's edges
HS, HR, HM, HA = 70, 150, 3, 4
SLOT_CASES = [  # (slots in use, the ones that retire)
    (67, (0, 63, 64, 66)),
    (67, ()),
    (67, tuple(range(67))),
    (67, (66,)),
    (64, (0,)),
    (65, (64,)),
    (70, (1, 2, 3, 62, 65, 69)),
    (0, ()),
    (1, (0,)),
]
READING_CASES = [  # (readings stored, ages at the pass in ring order)
    (140, [5] * 1 + [2] * 139),
    (140, [7] * 64 + [3] * 76),
    (140, [7] * 65 + [1] * 75),
    (140, [6] * 140),
    (140, [1, 1, 9] + [1] * 137),             # a stale reading behind fresh ones stays: only the prefix goes
    (140, [4] * 3 + [1] + [8] * 5 + [2] * 131),  # ... the prefix of 3 goes, the stale five behind the fresh one stay
    (0, []),
    (63, [4] * 63),
    (149, [5] * 100 + [3] * 49),
]


def _hand_state(lib, t0):
    """One particle per case, put in place through pk_upload_landmarks, pk_grow_upload and pk_grow_clocks_upload, and the same state
    in the oracle.  One blob that matches nothing and pairs with nothing (colours far from every feature and reading) then runs
    the pass: t = t0 + 1 (mod 2^32), every particle stores one more reading."""
    P, L0 = len(SLOT_CASES), 1
    known = np.array([[40.0, 40.0, 250.0, 250.0, 250.0]])
    kcov = 0.25 * np.identity(5).reshape(1, 5, 5)
    f = _device_filter(lib, P, known, kcov, HS, HR, HA, HM)
    o = RetiringOracle(P, known, kcov, HS, THR, HA, HM)
    rs = np.random.RandomState(31)
    t1 = (t0 + 1) & 0xFFFFFFFF
    L = L0 + HS
    m, c, k = f.download_landmarks()
    c = c.reshape(P, L, 25)
    cnt = np.zeros((P, 4), dtype=np.int32)
    rd = np.zeros((P, HR, 8))
    sid = np.zeros((P, HS), dtype=np.int32)
    kc = np.zeros((P, 4), dtype=np.int32)
    sc = np.zeros((P, HR), dtype=np.uint32)
    se = np.zeros((P, HS), dtype=np.int32)
    si = np.zeros((P, HS), dtype=np.int32)
    for i, ((used, gone), (n, ages)) in enumerate(zip(SLOT_CASES, READING_CASES)):
        cnt[i] = (n, used, 1000 + i, 0)
        kc[i] = (n, used, 10 * i, 3 * i)
        for j in range(used):
            ang = 1.0 + 4.0 * j / HS  # (away from the blob's bearing 0)
            m[i, L0 + j] = (20.0 * np.cos(ang), 20.0 * np.sin(ang), 200.0 + (j % 7), 150.0 + i, 220.0 - (j % 5))
            cov = np.identity(5) * (1.0 + j / 128.0)
            cov[0, 1] = cov[1, 0] = 0.125
            c[i, L0 + j] = cov.reshape(25)
            if j in gone:        # potential, unchanged, one pass short of M
                word, seen, idle = POTENTIAL | (j % 5), None, HM - 1
            elif j % 9 == 4:     # promoted AND idle for long: stays
                word, seen, idle = 7 + (j % 3), None, 2 ** 31 - 1 if j % 2 else 40
            elif j % 9 == 5:     # potential and idle, but its word changed since the last pass: idle restarts
                word, seen, idle = POTENTIAL | 3, POTENTIAL | 2, 50
            else:                # potential, idle for fewer passes
                word, seen, idle = POTENTIAL | (j % 6), None, j % (HM - 1)
            k[i, L0 + j] = word
            se[i, j], si[i, j] = (word if seen is None else seen), idle
            sid[i, j] = 100 + j
        for r in range(n):
            rd[i, r] = (500 + r, rs.uniform(-3, -1), rs.uniform(-3, 3), rs.uniform(-0.3, 0.3), rs.uniform(-0.5, 0.5),
                        200.0 + r % 11, 210.0, 190.0 + i)
            sc[i, r] = (t1 - ages[r]) & 0xFFFFFFFF
        # the oracle's copy
        o.f.mean[i], o.f.cov[i] = m[i], c[i].reshape(L, 5, 5)
        o.f.count[i], o.f.potential[i] = k[i] & ~POTENTIAL, (k[i] & POTENTIAL) != 0
        o.hyp[i] = [(int(r[0]),) + tuple(float(v) for v in r[1:]) for r in rd[i, :n]]
        o.next_id[i], o.used[i] = 1000 + i, used
        o.slot_id[i] = {L0 + j: 100 + j for j in range(used)}
        o.scan[i], o.seen[i], o.idle[i] = [int(v) for v in sc[i, :n]], [int(v) for v in se[i, :used]], [int(v) for v in si[i, :used]]
        o.covered_readings[i], o.covered_slots[i], o.readings_retired[i], o.features_retired[i] = n, used, 10 * i, 3 * i
    o.t = t0
    f.upload_landmarks(0, P, m, c, k)
    f.grow_upload(0, P, cnt, rd, sid)
    f.grow_clocks_upload(0, P, kc, sc, se, si, scan_now=t0)
    back = f.grow_clocks_download()
    assert np.array_equal(back[0], kc) and np.array_equal(back[1], sc) and np.array_equal(back[2], se) and np.array_equal(back[3], si) and back[4] == t0
    return f, o, L0


@pytest.mark.parametrize("t0", [1000, 2 ** 32 - 3, 2 ** 32 - 1, 1])
def test_hand_written_states_across_the_waves_edges_and_the_clocks_wrap(lib, t0):
    """t0 = 2^32 - 3: t stays just below 2^32; 2^32 - 1: t wraps to 0 in this pass, every stamp lies on the other side; 1: the
    stamps straddle the wrap (ages up to 9 from t = 2)."""
    f, o, L0 = _hand_state(lib, t0)
    blobs = np.array([[0.0, 100.0, 50.0, 20.0]])
    f.observe(blobs, fresh=True)
    o.f.reset_weights()
    o.observe(blobs)
    assert o.t == (t0 + 1) & 0xFFFFFFFF
    assert np.allclose(f.download_log_weights(), o.f.logw, rtol=1e-9, atol=1e-9)
    _compare(lib, f, o, L0, "t0 = %d" % t0)
    # what the cases were written for
    kc = f.grow_clocks_download()[0]
    cnt = f.grow_download()[0]
    assert [int(v) for v in kc[:, 3]] == [3 * i + len(g) for i, (_, g) in enumerate(SLOT_CASES)]
    assert [int(v) for v in kc[:, 2] - 10 * np.arange(len(SLOT_CASES))] == [1, 64, 65, 140, 0, 3, 0, 63, 100]
    assert [int(v) for v in cnt[:, 0]] == [n + 1 - g for (n, _), g in zip(READING_CASES, [1, 64, 65, 140, 0, 3, 0, 63, 100])]
    assert o.promoted_vacated == 0
    f.close()


def _small_state(lib, A=HA, M=HM, P=24, spare=5, R=16, seed=3):
    """A filter with retirement on and different bookkeeping and clocks in every particle (hand-written)."""
    world, covs, known, kcov = _scene(4, 0)
    f = _device_filter(lib, P, known, kcov, spare, R, A, M)
    rs = np.random.RandomState(seed)
    cnt = np.stack([rs.randint(0, R + 1, P), rs.randint(0, spare + 1, P), rs.randint(7, 30, P), np.zeros(P, dtype=np.int64)], axis=1).astype(np.int32)
    rd = rs.normal(size=(P, R, 8))
    sid = rs.randint(7, 30, size=(P, spare)).astype(np.int32)
    f.grow_upload(0, P, cnt, rd, sid)
    kc = np.stack([cnt[:, 0] - (rs.uniform(size=P) < 0.3) * (cnt[:, 0] > 0), cnt[:, 1], rs.randint(0, 99, P), rs.randint(0, 99, P)], axis=1).astype(np.int32)
    sc = rs.randint(0, 2 ** 32, size=(P, R), dtype=np.uint64).astype(np.uint32)
    se = rs.randint(0, 9, size=(P, spare)).astype(np.int32) | POTENTIAL
    si = rs.randint(0, 5, size=(P, spare)).astype(np.int32)
    f.grow_clocks_upload(0, P, kc, sc, se, si, scan_now=77)
    return f, (cnt, rd, sid), (kc, sc, se, si)


def _clocks_follow(f, cnt, clocks, anc):
    kc, sc, se, si = clocks
    c2 = f.grow_download()[0]
    k2, s2, e2, i2, now = f.grow_clocks_download()
    assert now == 77
    assert np.array_equal(c2, cnt[anc]) and np.array_equal(k2, kc[anc])
    for p, a in enumerate(anc):
        n, used = cnt[a, 0], cnt[a, 1]
        assert np.array_equal(s2[p, :n], sc[a, :n]), p
        assert np.array_equal(e2[p, :used], se[a, :used]) and np.array_equal(i2[p, :used], si[a, :used]), p


def test_the_clocks_follow_the_ancestors_through_pk_resample(lib):
    f, (cnt, rd, sid), clocks = _small_state(lib)
    rs = np.random.RandomState(8)
    f.upload_log_weights(rs.normal(scale=2.0, size=f.P))
    anc = f.resample(0.37, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
    assert len(set(anc.tolist())) < f.P and len(set(anc.tolist())) > 2, "the ancestors show nothing"
    _clocks_follow(f, cnt, clocks, anc)
    # twice: both buffers of the pair have been current
    cnt2 = cnt[anc]
    clocks2 = tuple(x[anc] for x in clocks)
    f.upload_log_weights(rs.normal(scale=2.0, size=f.P))
    anc2 = f.resample(0.81, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
    _clocks_follow(f, cnt2, clocks2, anc2)
    f.close()


@pytest.mark.parametrize("threshold,kept", [(0.0, True), (1.0, False)])
def test_the_clocks_follow_through_pk_resample_adaptive_kept_and_resampled(lib, threshold, kept):
    f, (cnt, rd, sid), clocks = _small_state(lib)
    f.upload_log_weights(np.random.RandomState(9).normal(scale=2.0, size=f.P))
    anc = f.resample_adaptive(0.37, threshold, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
    assert np.array_equal(anc, np.arange(f.P)) == kept
    _clocks_follow(f, cnt, clocks, anc)
    f.close()


def test_pk_grow_upload_restarts_the_clocks_of_exactly_the_particles_it_wrote(lib):
    f, (cnt, rd, sid), (kc, sc, se, si) = _small_state(lib)
    f.grow_upload(5, 9, cnt[5:9], rd[5:9], sid[5:9])
    k2, s2, e2, i2, now = f.grow_clocks_download()
    want = kc.copy()
    want[5:9, :2] = 0  # covered_* restart; the retired counters stay
    assert np.array_equal(k2, want) and now == 77
    assert np.array_equal(s2, sc) and np.array_equal(e2, se) and np.array_equal(i2, si)
    # counters alone restart them too
    f.grow_upload(0, 1, cnt[:1], None, None)
    want[0, :2] = 0
    assert np.array_equal(f.grow_clocks_download()[0], want)
    # and the next pass stamps everything those particles hold as new: nothing of theirs is stale, nothing idle
    blobs = synthetic_scan(_scene(4, 0)[0], (0.0, 0.0, 0.0))[:2]
    f.observe(blobs, fresh=True)
    c3 = f.grow_download()[0]
    k3, s3, e3, i3, now = f.grow_clocks_download()
    assert now == 78
    for p in (0, 5, 6, 7, 8):
        assert k3[p, 2] == kc[p, 2] and k3[p, 3] == kc[p, 3] and c3[p, 0] >= cnt[p, 0] and c3[p, 1] >= cnt[p, 1], p
        assert (s3[p, :c3[p, 0]] == 78).all() and not i3[p, :c3[p, 1]].any(), p
    f.close()


def test_lifecycle_and_device_bytes(lib):
    world, covs, known, kcov = _scene(6, 2)
    P, spare, R = 16, 3, 8
    plain = _device_filter(lib, P, known, kcov, spare, R)
    f = _device_filter(lib, P, known, kcov, spare, R)
    base = f.device_bytes()
    assert base == plain.device_bytes()
    f.grow_retire(0, 0)  # off already: nothing happens
    assert f.device_bytes() == base
    with pytest.raises(lib.PkError, match="nothing is being retired") as e:
        f.grow_clocks_download()
    assert e.value.status == lib.PK_ERR_STATE
    f.grow_retire(4, 0)
    on = f.device_bytes()
    # two buffers of: stamps (R words), seen and idle (spare words each), four counters, per particle
    assert on - base == 2 * 4 * P * (R + 2 * spare + 4)
    f.grow_retire(0, 3)  # only the thresholds change
    assert f.device_bytes() == on
    kc, _, _, _, now = f.grow_clocks_download()
    assert not kc.any() and now == 0
    f.grow_retire(0, 0)
    assert f.device_bytes() == base
    # an empty scan runs nothing and advances no clock; a scan does
    f.grow_retire(2, 2)
    f.observe(np.zeros((0, 4)), fresh=True)
    assert f.grow_clocks_download()[4] == 0
    f.observe(synthetic_scan(world, (0.0, 0.0, 0.0)), fresh=True)
    assert f.grow_clocks_download()[4] == 1
    f.close()
    plain.close()


def test_refusals_and_arguments(lib):
    world, covs, known, kcov = _scene(6, 2)
    g = lib.DeviceFilter(4, 5)
    with pytest.raises(lib.PkError, match="pk_grow_retire: pk_grow_enable was not called") as e:
        g.grow_retire(4, 3)
    assert e.value.status == lib.PK_ERR_STATE
    with pytest.raises(lib.PkError, match="pk_grow_clocks_download: pk_grow_enable was not called"):
        g.grow_clocks_download()
    g.close()
    f = _device_filter(lib, 16, known, kcov, 3, 8)
    for bad in ((-1, 0), (0, -1), (2 ** 30 + 1, 0), (0, 2 ** 30 + 1)):
        with pytest.raises(lib.PkError, match="outside 0..2\\^30") as e:
            f.grow_retire(*bad)
        assert e.value.status == lib.PK_ERR_INVALID
    f.grow_retire(2 ** 30, 2 ** 30)
    with pytest.raises(lib.PkError, match="particles \\[") as e:
        f.grow_clocks_download(3, 17)
    assert e.value.status == lib.PK_ERR_INVALID
    # covered_* beyond what the particle holds
    cnt = np.tile(np.array([[3, 2, 9, 0]], dtype=np.int32), (16, 1))
    f.grow_upload(0, 16, cnt, None, None)
    for col, v in ((0, 4), (1, 3), (0, -1), (2, -1)):
        kc = np.tile(np.array([[3, 2, 0, 0]], dtype=np.int32), (16, 1))
        kc[7, col] = v
        with pytest.raises(lib.PkError, match="pk_grow_clocks_upload: particle 7") as e:
            f.grow_clocks_upload(0, 16, kc)
        assert e.value.status == lib.PK_ERR_INVALID
    assert not f.grow_clocks_download()[0].any(), "a refused upload wrote something"
    # what moves particles between filters is refused while retirement is on, ahead of every other check (any address will do)
    table = np.zeros(6, dtype=np.int64)
    calls = {
        "pk_pack_particles": lambda: f.pack_particles([0, 1], 4096),
        "pk_adopt_particles": lambda: f.adopt_particles(np.arange(16), 4096, 0),
        "pk_shard_pack_dev": lambda: f.shard_pack_dev([0, 0], 1, 0, 4096),
        "pk_shard_pack_slots_dev": lambda: f.shard_pack_slots_dev(0, 0, 0, 0, 4096),
        "pk_shard_adopt_dev": lambda: f.shard_adopt_dev(0, 4096, 0),
        "pk_shard_adopt_local_dev": lambda: f.shard_adopt_local_dev(0),
        "pk_shard_adopt_remote_dev": lambda: f.shard_adopt_remote_dev(0, 4096, 0),
        "pk_shard_state_dev": lambda: f.shard_state_dev(4096),
        "pk_shard_pack_balanced_dev": lambda: f.shard_pack_balanced_dev(table, 1, 0, 4096),
        "pk_shard_pack_balanced_loop_dev": lambda: f.shard_pack_balanced_loop_dev(0, 0, 0, 4096),
        "pk_shard_adopt_balanced_dev": lambda: f.shard_adopt_balanced_dev(table, 1, 0, 4096, 0, 0),
    }
    for name, call in calls.items():
        with pytest.raises(lib.PkError, match="%s: readings and features are being retired \\(pk_grow_retire\\)" % name) as e:
            call()
        assert e.value.status == lib.PK_ERR_STATE, name
    # off again: the refusal of before is back (the contiguous exchange carries no bookkeeping)
    f.grow_retire(0, 0)
    with pytest.raises(lib.PkError, match="balanced placement only"):
        f.pack_particles([0, 1], 4096)
    f.close()


# ---- the facade
class _View(object):
    def __init__(self, pk, blobs):
        class Scan(object):
            pass

        self.last_sensor_reading = Scan()
        obs = []
        for b in blobs:
            o = pk.msgs.Blob()
            o.bearing = float(b[0])
            o.color.r, o.color.g, o.color.b = float(b[1]), float(b[2]), float(b[3])
            obs.append(o)
        self.last_sensor_reading.observes = obs


def test_facade_runs_the_scene_saves_and_restores_the_clocks(lib, tmp_path):
    """FastSLAM(..., reading_max_age=4, potential_max_idle=3) on the scene: rng='global' takes the motion noise from numpy's global
    stream and the resample draw from random.random(), so the oracle and a filter driven through the ABI see the same numbers."""
    import parakeet_slam_amd as pk

    P, L0, U, spare, steps = 64, 10, 3, 5, 14
    world, covs, known, kcov = _scene(L0, U)
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L0)]
    kw = dict(num_particles=P, weight_domain="log", rng="global", new_landmarks=True, spare_landmarks=spare,
              reading_max_age=A_SCENE, potential_max_idle=M_SCENE)
    np.random.seed(11)
    random.seed(7)
    pk.msgs.Time.set_now(0.0)
    fs = pk.FastSLAM(feats, device=0, **kw)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = V, W
    fs.last_control = tw
    f = _device_filter(lib, P, known, kcov, spare, 64, A_SCENE, M_SCENE)
    o = RetiringOracle(P, known, kcov, spare, THR, A_SCENE, M_SCENE)
    rs, pr = np.random.RandomState(11), random.Random(7)
    pose = (0.0, 0.0, 0.0)

    def step(fs_, s):
        pk.msgs.Time.set_now(DT * (s + 1))
        blobs = synthetic_scan(world, truth_step(pose, V, W, DT))
        fs_.cam_cb(_View(pk, blobs))
        z, u = rs.standard_normal((P, 3)), pr.random()
        _oracle_step(o, z, blobs, u)
        return blobs, z, u

    for s in range(steps):
        blobs, z, u = step(fs, s)
        pose = truth_step(pose, V, W, DT)
        f.motion(V, W, DT, z=z)
        f.observe(blobs, fresh=True)
        f.resample(u, domain=lib.PK_WEIGHTS_LOG)
    kc = f.grow_clocks_download()[0]
    assert fs.retired() == (int(kc[:, 2].sum()), int(kc[:, 3].sum())) == (sum(o.readings_retired), sum(o.features_retired))
    assert fs.retired()[0] > 0 and fs.retired()[1] > 0 and fs.readings_dropped() == 0
    f.close()
    _compare(lib, fs._filter, o, L0, "facade")
    path = str(tmp_path / "retire.npz")
    fs.save_state(path)
    d = np.load(path)
    assert {"nl_clock_counters", "nl_clock_scan", "nl_clock_seen", "nl_clock_idle", "nl_clock_now"} <= set(d.files)
    assert int(d["nl_clock_now"]) == steps
    # into a fresh filter: the clocks come back, and the next step still agrees with the oracle
    pk.msgs.Time.set_now(DT * steps)
    fs2 = pk.FastSLAM(feats, device=0, **kw)
    fs2.last_control = tw
    fs2.load_state(path)
    _compare(lib, fs2._filter, o, L0, "restored")
    assert fs2.retired() == fs.retired()
    fs.close()
    step(fs2, steps)
    _compare(lib, fs2._filter, o, L0, "the step after the restore")
    # a snapshot without the clocks loads, and restarts them
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, **{k: d[k] for k in d.files if not k.startswith("nl_clock_")})
    before = fs2.retired()
    fs2.load_state(bare)
    kc2 = fs2._filter.grow_clocks_download()[0]
    assert not kc2[:, :2].any() and fs2.retired() == before
    fs2.close()


def test_facade_refuses_host_bookkeeping_and_several_devices():
    import parakeet_slam_amd as pk

    world, covs = synthetic_world(6)
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(4)]
    pk.msgs.Time.set_now(0.0)
    with pytest.raises(ValueError, match="bookkeeping='host'"):
        pk.FastSLAM(feats, num_particles=8, new_landmarks=True, spare_landmarks=2, bookkeeping="host", reading_max_age=4)
    with pytest.raises(ValueError, match="one GPU only"):
        pk.FastSLAM(feats, num_particles=8, new_landmarks=True, spare_landmarks=2, devices=[0, 0], potential_max_idle=3)
    with pytest.raises(ValueError, match=">= 0"):
        pk.FastSLAM(feats, num_particles=8, new_landmarks=True, spare_landmarks=2, reading_max_age=-1)
    fs = pk.FastSLAM(feats, num_particles=8, new_landmarks=True, spare_landmarks=2)
    assert fs.retired() == (0, 0)
    fs.close()

"""GPU: the bearing measurement model (pk_set_measurement_model(f, PK_MODEL_BEARING); DESIGN.md section 4, "The bearing model")
against tests/bearing_model_reference.py -- the probe rows, supplied ids, the general route through both association kernels,
growing maps with and without retirement, the facade; and the reference model left bit for bit what it was.

Tolerances: the ones tests/test_gpu_parity.py holds the reference model to against OracleFilter -- the probe's probabilities and
weight 1e-10 relative, closest point 1e-12, updated means 1e-12, covariances rtol 1e-10 / atol 1e-13; a filter's weights 1e-9
relative (log-weights 1e-9 absolute), means 1e-9 relative, covariances rtol 1e-9 / atol 1e-13, counts and ids exactly.

Every scene is checked, on the reference's state, to hold no |wrapped bearing difference| within 1e-9 of 0.5 and no squared colour
distance within 1e-6 of 300 before anything is compared: rounding cannot turn a gate."""
import math
import random

import numpy as np
import pytest

from conftest import relerr
from oracle.fastslam_oracle import EMPTY_COLOUR, GrowingOracle, low_variance_ancestors, synthetic_world, truth_step

import bearing_model_reference as ref
from bearing_model_reference import BearingOracle, under_bearing_model, wrap, wrapped_scan
from grow_retire_reference import RetiringOracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
V, W, DT = 1.0, 0.35, 0.5  # the turning drive: a full turn in 36 steps
H0 = 2.9                   # the heading it starts from here, so that it wraps inside six steps
SIGMA_B, SIGMA_C = 0.01, 0.3
THR = 30.0


# ---------------------------------------------------------------------------------------------------------------- helpers
def _assert_margins(o, blobs, what):
    """No gate of any (particle, landmark, blob) of the oracle's current state can be turned by rounding."""
    sx, sy, sh = o.x[:, None], o.y[:, None], o.h[:, None]
    for b in range(len(blobs)):
        mb, mc = ref.gate_margins(sx, sy, sh, blobs[b], o.mean)
        assert mb.min() > 1e-9 and mc.min() > 1e-6, (what, b, mb.min(), mc.min())


def _device(lib, P, means, covs, immutable=None, model="bearing", opts=None, heading=H0):
    L = len(means)
    f = lib.DeviceFilter(P, L)
    if model is not None:
        f.set_measurement_model(model)
    for k, v in (opts or {}).items():
        f.set_option(k, v)
    f.upload_map(means, np.asarray(covs).reshape(L, 25), immutable)
    xyhw = np.zeros((P, 4))
    xyhw[:, 2] = heading
    xyhw[:, 3] = 1.0
    f.upload_poses(xyhw)
    return f


def _compare_state(lib, f, o, what, logw=None):
    if logw is not None:
        assert np.allclose(f.download_log_weights(), logw, rtol=0, atol=RTOL), (what, np.abs(f.download_log_weights() - logw).max())
    m, c, k = f.download_landmarks()
    assert np.array_equal((k & lib.PK_LANDMARK_POTENTIAL) != 0, o.potential), what
    assert np.array_equal(k & ~lib.PK_LANDMARK_POTENTIAL, o.count), what
    assert relerr(m, o.mean) < RTOL, (what, relerr(m, o.mean))
    assert np.allclose(c.reshape(o.cov.shape), o.cov, rtol=RTOL, atol=1e-13), what


def _drive(lib, f, o, world, sees, steps, rs, ids_of=None, twins=()):
    """`steps` steps of the turning drive on device filter f and oracle o (and on the twins, which must stay bit-identical to f):
    the scan shows the landmarks `sees`; ids_of(step, B) -> supplied ids or None (maximum likelihood)."""
    pose = (0.0, 0.0, H0)
    P = o.P
    for s in range(steps):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world[sees], pose, rs, SIGMA_B, SIGMA_C)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        ids = ids_of(s, len(blobs)) if ids_of else None
        o.reset_weights()
        o.motion(V, W, DT, z)
        _assert_margins(o, blobs, ("step", s))
        want = o.observe(blobs, ids)
        logw = o.logw.copy()
        anc = low_variance_ancestors(np.exp(logw - np.max(logw)), u)
        o.gather(anc)
        for g in (f,) + tuple(twins):
            g.motion(V, W, DT, z=z)
            if ids is None:
                got = g.observe(blobs, return_ids=True, fresh=True)
                assert np.array_equal(got, want), (s, int((got != want).sum()))
                assert g.observe_route() == "ml_general"
            else:
                g.observe(blobs, ids=ids, fresh=True)
                assert g.observe_route() == "known_ids"
        assert np.allclose(f.download_log_weights(), logw, rtol=0, atol=RTOL), (s, np.abs(f.download_log_weights() - logw).max())
        for g in twins:
            assert np.array_equal(g.download_log_weights(), f.download_log_weights()), s
        for g in (f,) + tuple(twins):
            assert np.array_equal(g.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), s
        _compare_state(lib, f, o, ("step", s))
        for g in twins:
            for a, b in zip(g.download_landmarks(), f.download_landmarks()):
                assert np.array_equal(a, b), s
        assert np.allclose(f.download_poses()[:, :3], np.stack([o.x, o.y, o.h], axis=1), rtol=1e-12, atol=1e-13), s
    return pose


# ---------------------------------------------------------------------------------------------------------------- the probe
def _probe_rows():
    """(pose, landmark mean, wrapped-difference target, heading) rows: differences just inside and outside the gate on both sides of
    0 and of +-2 pi, headings at +-pi, bearings at +-pi, the landmark under the robot."""
    rs = np.random.RandomState(3)
    rows = []
    for k in (-1, 0, 1):
        for side in (-1.0, 1.0):
            for eps in (-1e-6, 1e-6, -0.2, 0.3):  # |difference| = 0.5 + eps (eps <= -0.2: well inside)
                for h in (rs.uniform(-3, 3), math.pi, -math.pi):
                    sx, sy = rs.uniform(-3, 3, 2)
                    phi, rho = rs.uniform(-math.pi, math.pi), rs.uniform(4.0, 25.0)
                    fx, fy = sx + rho * math.cos(phi), sy + rho * math.sin(phi)
                    beta = (math.atan2(fy - sy, fx - sx) - h) + side * (0.5 + eps) + k * 2 * math.pi
                    rows.append((sx, sy, h, fx, fy, beta))
    for beta in (math.pi, -math.pi):  # a blob at the cut, seen by a robot that looks the other way
        for d in (0.1, -0.3):
            sx, sy = rs.uniform(-3, 3, 2)
            phi, rho = rs.uniform(-1.0, 1.0), rs.uniform(4.0, 25.0)
            fx, fy = sx + rho * math.cos(phi), sy + rho * math.sin(phi)
            h = math.atan2(fy - sy, fx - sx) - beta + d
            rows.append((sx, sy, float(wrap(h)), fx, fy, beta))
    sx, sy = 1.25, -0.5
    rows.append((sx, sy, 0.7, sx, sy, -0.7 + 0.1))  # q = 0: pse = atan2(0, 0) = 0
    return rs, np.array(rows)


def _landmark_rows(rs, n):
    cov = np.zeros((n, 5, 5))
    for i in range(n):
        a, c = rs.standard_normal((2, 2)), rs.standard_normal((3, 3))
        cov[i, :2, :2] = 0.3 * (a @ a.T) + 0.05 * np.identity(2)
        cov[i, 2:, 2:] = c @ c.T + 0.5 * np.identity(3)
    return rs.uniform(0, 255, (n, 3)), cov


def _fields14(mean, cov):
    return np.concatenate([mean, [cov[0, 0], cov[0, 1], cov[1, 1], cov[2, 2], cov[2, 3], cov[2, 4], cov[3, 3], cov[3, 4], cov[4, 4]]])


def test_probe_match_rows_against_the_reference(lib):
    rs, rows = _probe_rows()
    n = len(rows)
    col, cov = _landmark_rows(rs, n)
    inp, want = np.empty((n, 23)), np.empty((n, 5))
    for i, (sx, sy, h, fx, fy, beta) in enumerate(rows):
        mean = np.array([fx, fy, *col[i]])
        blob = np.array([beta, *(col[i] + rs.uniform(-6, 6, 3))])
        mb, mc = ref.gate_margins(sx, sy, h, blob, mean)
        assert mb > 1e-9 and mc > 1e-6, i
        cb, sb = math.cos(beta), math.sin(beta)
        ln = math.sqrt(cb * cb + sb * sb + 0.0)
        inp[i] = np.concatenate([[sx, sy, h], _fields14(mean, cov[i]), blob, [cb * (1.0 / ln), sb * (1.0 / ln)]])
        wx, wy = ref.world_ray(beta, h)
        mag = (fx - sx) * wx + (fy - sy) * wy
        want[i] = [ref.probability_of_match(sx, sy, h, blob, mean, cov[i]),
                   ref.prob_position_match(fx, fy, (cov[i, 0, 0], cov[i, 0, 1], cov[i, 1, 1]), sx, sy, h, beta),
                   ref.prob_color_match(mean[2:], (cov[i, 2, 2], cov[i, 2, 3], cov[i, 2, 4], cov[i, 3, 3], cov[i, 3, 4], cov[i, 4, 4]), blob[1:]),
                   sx + wx * mag, sy + wy * mag]
    got = lib.probe_bearing(0, inp)
    inside = want[:, 0] > 0
    assert inside.sum() >= 20 and (~inside).sum() >= 20  # both verdicts of the gate, on every side
    assert np.array_equal(got[:, 0] > 0, inside)
    assert np.array_equal(got[~inside, 0], np.zeros((~inside).sum()))
    for j in range(3):
        assert relerr(got[:, j], want[:, j], floor=1e-280) < 1e-10, (j, relerr(got[:, j], want[:, j], floor=1e-280))
    assert np.allclose(got[:, 3:], want[:, 3:], rtol=1e-12, atol=1e-12)


def test_probe_update_rows_against_the_reference(lib):
    rs, rows = _probe_rows()
    POT = lib.PK_LANDMARK_POTENTIAL
    # every geometry as a plain landmark; then immutable, and potential at counts 2, 4 and 6, zhat0 supplied or not
    variants = [(0, 0, 0)] * len(rows) + [(1, 0, 4), (1, 2, 0), (0, 0, POT | 2), (0, 2, POT | 4), (0, 0, POT | 6), (1, 0, POT | 4)]
    rows = np.concatenate([rows, rows[[5, 17, 29, 41, 44, len(rows) - 1]]])
    n = len(rows)
    col, cov = _landmark_rows(rs, n)
    qt = np.array([0.1, 0.1, 0.0, 0.0, 0.1, 0.0, 0.1])
    Qt = 0.1 * np.identity(4)
    inp = np.empty((n, 32))
    for i, (sx, sy, h, fx, fy, beta) in enumerate(rows):
        imm, known, count = variants[i]
        mean = np.array([fx, fy, *col[i]])
        blob = np.array([beta, *(col[i] + rs.uniform(-6, 6, 3))])
        pse = math.atan2(fy - sy, fx - sx)
        inp[i] = np.concatenate([[sx, sy, h], _fields14(mean, cov[i]), [count], blob, qt, [pse if known else 123.0, imm | known, 7.5]])
    got = lib.probe_bearing(1, inp)
    for i, (sx, sy, h, fx, fy, beta) in enumerate(rows):
        imm, known, count = variants[i]
        mean, blob = inp[i, 3:8], inp[i, 18:22]
        nm, nc, lw, aux = ref.ekf_update_dense(sx, sy, h, mean, cov[i], blob, Qt)
        assert abs(aux["delz"][0]) <= math.pi * (1 + 1e-15), i
        pot = bool(count & POT)
        want_lw = math.log(0.1) if pot else float(lw)
        assert abs(got[i, 0] - want_lw) < 1e-10 * max(1.0, abs(want_lw)), (i, got[i, 0], want_lw)
        if imm:
            assert np.array_equal(got[i, 1:15], inp[i, 3:17]) and got[i, 15] == count, i
        else:
            assert np.allclose(got[i, 1:6], nm, rtol=1e-12, atol=1e-12), (i, got[i, 1:6] - nm)
            assert np.allclose(got[i, 6:15], _fields14(nm, nc)[5:], rtol=1e-10, atol=1e-13), i
            c2 = (count & ~POT) + 2
            assert got[i, 15] == (c2 | POT if pot and c2 <= 5 else c2), (i, got[i, 15])
        assert got[i, 16] == 7.5
    # the refusals of the entry point itself; the math probe still has no op 11
    for what, arr in ((2, inp), (-1, inp)):
        with pytest.raises(lib.PkError) as e:
            lib.probe_bearing(what, arr[:1, :1])
        assert e.value.status == lib.PK_ERR_INVALID and "neither 0" in str(e.value)
    bad = inp[:1].copy()
    bad[0, 30] = 4.0
    with pytest.raises(lib.PkError) as e:
        lib.probe_bearing(1, bad)
    assert e.value.status == lib.PK_ERR_INVALID and "bit 0" in str(e.value)
    out = np.empty(64)
    assert lib.load().pk_probe_math(0, 11, 1, lib.dptr(np.zeros(64)), lib.dptr(out)) == lib.PK_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- supplied ids
def test_supplied_ids_against_the_reference_while_the_heading_wraps(lib):
    P, L = 64, 12
    world, covs = synthetic_world(L, seed=5)
    imm = np.zeros(L, dtype=np.uint8)
    imm[7] = 1
    f = _device(lib, P, world, covs, imm)
    assert f.measurement_model() == "bearing"
    o = BearingOracle(P, world, covs, immutable=imm)
    o.h[:] = H0

    def ids_of(s, B):
        ids = np.arange(1, B + 1, dtype=np.int32)
        if s % 2:
            ids[5] = 0   # an unmatched blob
            ids[9] = 9   # and a landmark seen twice: blobs 8 and 9
        return ids

    pose = _drive(lib, f, o, world, np.arange(L), 6, np.random.RandomState(1), ids_of)
    assert pose[2] < 0 < H0, "the heading did not wrap inside the run"
    f.close()


# ---------------------------------------------------------------------------------------------------------------- general route
def _scene(L, seed=5):
    world, covs = synthetic_world(L, seed=seed)
    if L >= 65:
        # S3: two landmarks of one colour 0.1 rad apart as the robot sees them; S4: six of one colour within 0.15 rad
        phi = math.atan2(world[10, 1], world[10, 0])
        world[11, :2] = 14.0 * math.cos(phi + 0.1), 14.0 * math.sin(phi + 0.1)
        world[11, 2:] = world[10, 2:]
        phi = math.atan2(world[20, 1], world[20, 0])
        for i in range(1, 6):
            world[20 + i, :2] = (12.0 + 2.0 * i) * math.cos(phi + 0.03 * i), (12.0 + 2.0 * i) * math.sin(phi + 0.03 * i)
            world[20 + i, 2:] = world[20, 2:]
    return world, covs


REFERENCE_ROUTE = {3: "ml_fused", 65: "ml_fused", 600: "ml_regs"}  # what a reference-model filter of these shapes says today


@pytest.mark.parametrize("L,B,P", [(3, 3, 64), (65, 65, 64), (600, 70, 32)])
def test_general_route_against_the_reference_through_both_association_kernels(lib, L, B, P):
    world, covs = _scene(L)
    sees = np.arange(L) if B == L else (np.arange(B) * 8) % L
    f = _device(lib, P, world, covs)
    brute = _device(lib, P, world, covs, opts={"assoc_kernel": 1})
    o = BearingOracle(P, world, covs)
    o.h[:] = H0
    rs = np.random.RandomState(2)
    # pk_associate runs the same model, and touches nothing
    blobs0 = wrapped_scan(world[sees], truth_step((0.0, 0.0, H0), V, W, DT), np.random.RandomState(9), SIGMA_B, SIGMA_C)
    _assert_margins(o, blobs0, "associate")
    want0 = o.associate(blobs0)
    assert np.array_equal(f.associate(blobs0), want0) and np.array_equal(brute.associate(blobs0), want0)
    if L == 65:
        assert (want0[:, 10:12] > 0).all() and (want0[:, 20:26] > 0).all()  # the contested blobs are settled, not dropped
    pose = _drive(lib, f, o, world, sees, 6, rs, twins=(brute,))
    assert pose[2] < 0 < H0
    # a reference-model filter of this shape takes the route it always took
    r = _device(lib, P, world, covs, model=None)
    assert r.measurement_model() == "reference"
    r.observe(blobs0, fresh=True)
    assert r.observe_route() == REFERENCE_ROUTE[L]
    r.close()
    if L == 3:  # B = 1 and B = 0
        for nb in (1, 0):
            blobs = wrapped_scan(world[:nb], pose, rs, SIGMA_B, SIGMA_C).reshape(nb, 4)
            o.reset_weights()
            if nb:
                _assert_margins(o, blobs, ("B", nb))
            want = o.observe(blobs)
            for g in (f, brute):
                got = g.observe(blobs, return_ids=True, fresh=True)
                assert got.shape == (P, nb) and np.array_equal(got, want.reshape(P, nb))
                assert g.observe_route() == ("ml_general" if nb else "known_ids")
                _compare_state(lib, g, o, ("B", nb), o.logw)
    f.close()
    brute.close()


# ---------------------------------------------------------------------------------------------------------------- the reference model
def test_the_reference_model_is_bit_for_bit_what_it_was(lib):
    """A one-pass shape (L = 600): a filter told PK_MODEL_REFERENCE, and one switched to the bearing model and back between scans
    (with a pk_associate under it in between), are the filter that was never told."""
    P, L, B = 64, 600, 70
    world, covs = _scene(L)
    sees = (np.arange(B) * 8) % L
    never = _device(lib, P, world, covs, model=None, heading=0.0)
    told = _device(lib, P, world, covs, model="reference", heading=0.0)
    back = _device(lib, P, world, covs, model=None, heading=0.0)
    rs = np.random.RandomState(4)
    pose = (0.0, 0.0, 0.0)
    for s in range(4):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world[sees], pose, rs, SIGMA_B, SIGMA_C)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        back.set_measurement_model("bearing")
        assert back.measurement_model() == "bearing"
        back.associate(blobs)
        back.set_measurement_model(lib.PK_MODEL_REFERENCE)
        for g in (never, told, back):
            g.motion(V, W, DT, z=z)
            g.observe(blobs, fresh=True)
            assert g.observe_route() == REFERENCE_ROUTE[L], (s, g.observe_route())
        lw = never.download_log_weights()
        for g in (told, back):
            assert np.array_equal(g.download_log_weights(), lw), s
        anc = never.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
        for g in (told, back):
            assert np.array_equal(g.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), s
            assert np.array_equal(g.download_poses(), never.download_poses()), s
            for a, b in zip(g.download_landmarks(), never.download_landmarks()):
                assert np.array_equal(a, b), s
    for g in (never, told, back):
        g.close()


# ---------------------------------------------------------------------------------------------------------------- growing maps
def _compare_growing(lib, f, o, L0, step, clocks):
    cnt, rd, sid = f.grow_download()
    assert np.array_equal(cnt[:, 0], [len(h) for h in o.hyp]), "step %s: readings stored" % (step,)
    assert np.array_equal(cnt[:, 1], o.used), "step %s: spare slots in use" % (step,)
    assert np.array_equal(cnt[:, 2], o.next_id), "step %s: next_id" % (step,)
    assert not cnt[:, 3].any(), "step %s: readings dropped" % (step,)
    for i in range(f.P):
        n, used = int(cnt[i, 0]), int(cnt[i, 1])
        if n:
            assert np.array_equal(rd[i, :n, 0], [h[0] for h in o.hyp[i]]), (step, i, "reading ids")
            assert np.allclose(rd[i, :n], np.asarray(o.hyp[i]), rtol=1e-12, atol=1e-12), (step, i)
        assert [int(v) for v in sid[i, :used]] == [o.slot_id[i][L0 + k] for k in range(used)], (step, i)
    if clocks:
        kc, sc, se, si, now = f.grow_clocks_download()
        assert now == o.t and np.array_equal(kc, o.clock_counters()), step
        for i in range(f.P):
            n, used = int(cnt[i, 0]), int(cnt[i, 1])
            assert [int(v) for v in sc[i, :n]] == o.scan[i] and [int(v) for v in se[i, :used]] == o.seen[i], (step, i)
            assert [int(v) for v in si[i, :used]] == o.idle[i], (step, i)
    _compare_state(lib, f, o.f, step)


@pytest.mark.parametrize("retire", [False, True])
def test_growing_map_against_the_reference(lib, retire):
    """64 particles, 10 preset + 3 unknown landmarks, 5 spare slots, 13 blobs, 14 steps of the turning drive; with retirement
    (reading_max_age 4, potential_max_idle 3) running behind every scan."""
    P, L0, U, spare, R = 64, 10, 3, 5, 64
    A, M = (4, 3) if retire else (0, 0)
    world, covs = synthetic_world(L0 + U, seed=5)
    means = np.zeros((L0 + spare, 5))
    means[:L0] = world[:L0]
    means[L0:, 2:] = EMPTY_COLOUR
    mcov = np.tile(np.identity(5), (L0 + spare, 1, 1))
    mcov[:L0] = covs[:L0]
    f = _device(lib, P, means, mcov)
    f.grow_enable(L0, R, THR)
    if retire:
        f.grow_retire(A, M)
    o = under_bearing_model(RetiringOracle(P, world[:L0], covs[:L0], spare, THR, A, M) if retire
                            else GrowingOracle(P, world[:L0], covs[:L0], spare, THR))
    o.f.h[:] = H0
    rs = np.random.RandomState(6)
    pose = (0.0, 0.0, H0)
    for s in range(14):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        o.f.reset_weights()
        o.f.motion(V, W, DT, z)
        _assert_margins(o.f, blobs, ("step", s))
        o.observe(blobs)
        logw = o.f.logw.copy()
        anc = low_variance_ancestors(np.exp(logw - np.max(logw)), u)
        o.gather(anc)
        f.motion(V, W, DT, z=z)
        f.observe(blobs, fresh=True)
        assert f.observe_route() == "ml_general"
        assert np.allclose(f.download_log_weights(), logw, rtol=0, atol=RTOL), (s, np.abs(f.download_log_weights() - logw).max())
        assert np.array_equal(f.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), s
        _compare_growing(lib, f, o, L0, s, retire)
    assert o.used == [3] * P  # the three unknown landmarks, and nothing else, were discovered
    f.close()


# ---------------------------------------------------------------------------------------------------------------- the facade
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


def test_facade_runs_the_turning_drive_and_keeps_the_model_in_its_snapshots(lib, tmp_path):
    import parakeet_slam_amd as pk

    P, L, steps = 64, 12, 8
    world, covs = synthetic_world(L, seed=5)
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L)]
    kw = dict(num_particles=P, weight_domain="log", rng="global")
    np.random.seed(11)
    random.seed(7)
    pk.msgs.Time.set_now(0.0)
    fs = pk.FastSLAM(feats, device=0, measurement_model="bearing", **kw)
    assert fs._filter.measurement_model() == "bearing"
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = V, W
    fs.last_control = tw
    o = BearingOracle(P, world, covs)
    rs, pr, noise = np.random.RandomState(11), random.Random(7), np.random.RandomState(8)
    pose = (0.0, 0.0, 0.0)
    for s in range(steps):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world, pose, noise, SIGMA_B, SIGMA_C)
        pk.msgs.Time.set_now(DT * (s + 1))
        fs.cam_cb(_View(pk, blobs))
        z, u = rs.standard_normal((P, 3)), pr.random()
        o.reset_weights()
        o.motion(V, W, DT, z)
        _assert_margins(o, blobs, ("step", s))
        o.observe(blobs)
        o.gather(low_variance_ancestors(np.exp(o.logw - np.max(o.logw)), u))
        assert fs._filter.observe_route() == "ml_general"
        assert np.allclose(fs.summary(), o.summary(), rtol=1e-12, atol=1e-14), (s, fs.summary(), o.summary())
    err = math.hypot(fs.summary()[0] - pose[0], fs.summary()[1] - pose[1])
    assert err < 0.5, err  # (it localises: the reference model is a metre off on this drive)
    _compare_state(lib, fs._filter, o, "facade")
    # the snapshot carries the model's name; the other model refuses it; one without the field is the reference model's
    path = str(tmp_path / "bearing.npz")
    fs.save_state(path)
    d = np.load(path)
    assert str(d["measurement_model"]) == "bearing"
    fs2 = pk.FastSLAM(feats, device=0, measurement_model="bearing", **kw)
    fs2.load_state(path)
    _compare_state(lib, fs2._filter, o, "restored")
    fs2.close()
    fr = pk.FastSLAM(feats, device=0, **kw)
    with pytest.raises(ValueError, match="measurement_model='bearing'"):
        fr.load_state(path)
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, **{k: d[k] for k in d.files if k != "measurement_model"})
    fr.load_state(bare)
    with pytest.raises(ValueError, match="measurement_model='reference'"):
        fs.load_state(bare)
    rpath = str(tmp_path / "reference.npz")
    fr.save_state(rpath)
    assert str(np.load(rpath)["measurement_model"]) == "reference"
    fr.close()
    fs.close()


def test_refusals_each_with_its_status_and_text(lib):
    import parakeet_slam_amd as pk

    world, covs = synthetic_world(600, seed=5)
    f = _device(lib, 16, world, covs, model=None, heading=0.0)
    for bad in (2, -1, 7):
        with pytest.raises(lib.PkError) as e:
            f.set_measurement_model(bad)
        assert e.value.status == lib.PK_ERR_INVALID and "PK_MODEL_BEARING" in str(e.value)
        assert f.measurement_model() == "reference"
    with pytest.raises(ValueError):
        f.set_measurement_model("textbook")
    # the ranged and split observes of the sharded step
    blobs = wrapped_scan(world[:70], (0.0, 0.0, 0.0))
    f.stage_scan(blobs)
    assert f.staged_takes_regs()
    f.set_measurement_model("bearing")
    assert not f.staged_takes_regs()
    with pytest.raises(lib.PkError) as e:
        f.observe_staged_range(True, 0, 16, True, True)
    assert e.value.status == lib.PK_ERR_UNSUPPORTED and "ranged and split observes" in str(e.value)
    f.observe_staged(fresh=True)  # the staged scan itself serves the model
    assert f.observe_route() == "ml_general"
    # the dense layout: a Qt that couples bearing and colour
    Qt = 0.1 * np.identity(4)
    Qt[0, 1] = Qt[1, 0] = 0.01
    f.set_measurement_noise(Qt)
    for call in (lambda: f.observe(blobs), lambda: f.associate(blobs), lambda: f.observe(blobs, ids=np.arange(1, 71, dtype=np.int32))):
        with pytest.raises(lib.PkError) as e:
            call()
        assert e.value.status == lib.PK_ERR_UNSUPPORTED and "dense layout" in str(e.value)
    f.set_measurement_model("reference")
    f.observe(blobs)
    assert f.observe_route() == "dense"
    f.close()
    # the facade: several devices, an unknown name
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(4)]
    pk.msgs.Time.set_now(0.0)
    with pytest.raises(ValueError, match="one GPU"):
        pk.FastSLAM(feats, num_particles=8, devices=[0, 0], measurement_model="bearing")
    with pytest.raises(ValueError, match="measurement_model"):
        pk.FastSLAM(feats, num_particles=8, devices=[0, 0], measurement_model="textbook")
    with pytest.raises(ValueError, match="'reference' \\(default\\) or 'bearing'"):
        pk.FastSLAM(feats, num_particles=8, measurement_model="textbook")

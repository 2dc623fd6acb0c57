"""GPU: range-bearing scans (pk_scan_ranges; DESIGN.md section 4, "Range-bearing scans") against tests/range_bearing_reference.py --
the probe rows, every kind of scan through both association kernels and every entry point that takes blobs, an armed scan without a
finite range against a filter never armed, the refusals, the facade.

Shapes, scenes and tolerances are those of tests/test_gpu_bearing_model.py (its helpers are used as they are): the probe's
probabilities, weight and covariances rtol 1e-10 / atol 1e-13; a filter's log-weights 1e-9 absolute, means 1e-9 relative, covariances
rtol 1e-9 / atol 1e-13, counts and ids exactly.  The scenes add a depth pair -- two landmarks of one colour on one ray -- to that
file's contested landmarks.  Before anything is compared the reference's own margins are checked: no gate within 1e-9 rad / 1e-6 of
turning over, and the best probability of a contested blob at least 1e-6 (relative) above the second best -- four decades above what
the probe rows hold the device's probabilities to.  tests/test_range_bearing_host.py runs the same check without a GPU."""
import math
import random

import numpy as np
import pytest

from oracle.fastslam_oracle import low_variance_ancestors, synthetic_world, truth_step

import bearing_model_reference as bref
import range_bearing_reference as rref
import test_gpu_bearing_model as tb
from bearing_model_reference import wrapped_scan
from range_bearing_reference import RangeBearingOracle, range_scan

pytestmark = pytest.mark.gpu

V, W, DT, H0 = tb.V, tb.W, tb.DT, tb.H0
SIGMA_B, SIGMA_C, SIGMA_R = tb.SIGMA_B, tb.SIGMA_C, (0.05, 0.01)
SHAPES = [(3, 3, 64), (65, 65, 64), (600, 70, 32)]
GAP = 1e-6


# ---------------------------------------------------------------------------------------------------------------- scenes
def scene(L, B):
    """tb._scene's world and the landmarks the scan shows; from 65 landmarks on, blobs 30 and 31 see a depth pair: the second
    landmark 1.6 times as far as the first on the ray from where the first scan is taken, in the first one's colour."""
    world, covs = tb._scene(L)
    sees = np.arange(L) if B == L else (np.arange(B) * 8) % L
    if L >= 65:
        x, y, _ = truth_step((0.0, 0.0, H0), V, W, DT)
        a, b = sees[30], sees[31]
        world[b, :2] = x + 1.6 * (world[a, 0] - x), y + 1.6 * (world[a, 1] - y)
        world[b, 2:] = world[a, 2:]
    return world, covs, sees


def scans(world, sees, steps, kind, seed=2):
    """The drive's inputs, step by step: (pose, blobs, ranges, variances, z-seed, u).  kind "all": every blob ranged; "mixed": every
    third blob has none; "none": NaN everywhere."""
    rs, rr = np.random.RandomState(seed), np.random.RandomState(100 + seed)
    pose = (0.0, 0.0, H0)
    out = []
    for s in range(steps):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world[sees], pose, rs, SIGMA_B, SIGMA_C)
        rho, var = range_scan(world[sees], pose, rr, SIGMA_R[0], SIGMA_R[1], 3 if kind == "mixed" else None)
        if kind == "none":
            rho[:] = np.nan
        out.append((pose, blobs, rho, var, rs.randint(1 << 30), float(rs.uniform())))
    return out


def oracle_drive(L, B, P, kind, steps=6):
    """The reference's half of the drive (no GPU): per step (blobs, rho, var, z, u, ids, logw before the resample, ancestors), the
    oracle states behind each step, and the oracle itself, with the margins it met."""
    world, covs, sees = scene(L, B)
    o = RangeBearingOracle(P, world, covs)
    o.h[:] = H0
    rows = []
    for pose, blobs, rho, var, zseed, u in scans(world, sees, steps, kind):
        z = np.random.RandomState(zseed).standard_normal((P, 3))
        o.reset_weights()
        o.motion(V, W, DT, z)
        ids = o.observe(blobs, None, rho, var)
        logw = o.logw.copy()
        anc = low_variance_ancestors(np.exp(logw - np.max(logw)), u)
        o.gather(anc)
        rows.append(dict(pose=pose, blobs=blobs, rho=rho, var=var, z=z, u=u, ids=ids, logw=logw, anc=anc, mean=o.mean.copy(),
                         cov=o.cov.copy(), count=o.count.copy(), potential=o.potential.copy(), xyh=np.stack([o.x, o.y, o.h], axis=1)))
    return world, covs, rows, o


def assert_margins(o, what):
    assert o.min_gate_margins[0] > 1e-9 and o.min_gate_margins[1] > 1e-6, (what, o.min_gate_margins)
    assert o.min_rel_gap > GAP, (what, o.min_rel_gap)


class _State(object):
    """What tb._compare_state wants of an oracle, from a row of oracle_drive."""

    def __init__(self, row):
        self.mean, self.cov, self.count, self.potential = row["mean"], row["cov"], row["count"], row["potential"]


# ---------------------------------------------------------------------------------------------------------------- the probe
RANGES = (0.1, 200.0, None, None, None)   # None: the landmark's own distance, a little off
VARIANCES = (1e-4, 1e-3, 1e-2, 1e-1, 1.0, 1e2)


def _probe_cases():
    rs, rows = tb._probe_rows()
    n = len(rows)
    col, cov = tb._landmark_rows(rs, n)
    rho = np.empty(n)
    for i, (sx, sy, h, fx, fy, beta) in enumerate(rows):
        r = RANGES[i % len(RANGES)]
        rho[i] = math.hypot(fx - sx, fy - sy) + rs.uniform(-0.4, 0.4) if r is None else r
    rho[-1] = 0.7  # the q = 0 row
    var = np.array([VARIANCES[i % len(VARIANCES)] for i in range(n)])
    return rs, rows, col, cov, rho, var


def test_probe_match_rows_against_the_reference(lib):
    rs, rows, col, cov, rho, var = _probe_cases()
    n = len(rows)
    inp, want = np.empty((2 * n, 26)), np.empty((2 * n, 5))
    for i, (sx, sy, h, fx, fy, beta) in enumerate(rows):
        mean = np.array([fx, fy, *col[i]])
        blob = np.array([beta, *(col[i] + rs.uniform(-6, 6, 3))])
        mb, mc = bref.gate_margins(sx, sy, h, blob, mean)
        assert mb > 1e-9 and mc > 1e-6, i
        q00 = (0.1, 1e-4)[i % 2]
        cb, sb = math.cos(beta), math.sin(beta)
        ln = math.sqrt(cb * cb + sb * sb + 0.0)
        head = np.concatenate([[sx, sy, h], tb._fields14(mean, cov[i]), blob, [cb * (1.0 / ln), sb * (1.0 / ln)]])
        wx, wy = bref.world_ray(beta, h)
        colour = bref.prob_color_match(mean[2:], (cov[i, 2, 2], cov[i, 2, 3], cov[i, 2, 4], cov[i, 3, 3], cov[i, 3, 4], cov[i, 4, 4]), blob[1:])
        inp[i] = np.concatenate([head, [rho[i], var[i], q00]])
        want[i] = [rref.probability_of_match(sx, sy, h, blob, rho[i], var[i], q00, mean, cov[i]),
                   rref.prob_position_match(fx, fy, cov[i, :2, :2], sx, sy, h, beta, rho[i], var[i], q00), colour,
                   sx + rho[i] * wx, sy + rho[i] * wy]
        # the same row without a range: the bearing model's own functions
        mag = (fx - sx) * wx + (fy - sy) * wy
        inp[n + i] = np.concatenate([head, [np.nan, 0.0, q00]])
        want[n + i] = [bref.probability_of_match(sx, sy, h, blob, mean, cov[i]),
                       bref.prob_position_match(fx, fy, (cov[i, 0, 0], cov[i, 0, 1], cov[i, 1, 1]), sx, sy, h, beta), colour,
                       sx + wx * mag, sy + wy * mag]
    got = lib.probe_range(0, inp)
    inside = want[:, 0] > 0
    assert inside[:n].sum() >= 10 and (~inside[:n]).sum() >= 20
    assert np.array_equal(got[:, 0] > 0, inside)
    assert np.array_equal(got[~inside, 0], np.zeros((~inside).sum()))
    for j in range(3):
        assert np.allclose(got[:, j], want[:, j], rtol=1e-10, atol=1e-13), (j, np.abs(got[:, j] - want[:, j]).max())
    assert (want[:n, 1] > 1e-6).sum() >= 10  # some of the densities compared are not negligible
    assert np.allclose(got[:, 3:], want[:, 3:], rtol=1e-12, atol=1e-12)
    assert np.array_equal(got[n:], lib.probe_bearing(0, inp[n:, :23]))  # and a NaN range is the bearing model's probe, bit for bit


def test_probe_update_rows_against_the_reference(lib):
    rs, rows, col, cov, rho, var = _probe_cases()
    POT = lib.PK_LANDMARK_POTENTIAL
    extra = [5, 17, 29, 41, 44, len(rows) - 1]
    variants = [(0, 0, 0)] * len(rows) + [(1, 0, 4), (1, 2, 0), (0, 0, POT | 2), (0, 2, POT | 4), (0, 0, POT | 6), (1, 0, POT | 4)]
    rows = np.concatenate([rows, rows[extra]])
    n = len(rows)
    col, cov = tb._landmark_rows(rs, n)
    rho, var = np.concatenate([rho, rho[extra]]), np.concatenate([var, var[extra]])
    qt = np.array([0.1, 0.1, 0.0, 0.0, 0.1, 0.0, 0.1])
    Qt = 0.1 * np.identity(4)
    inp = np.empty((n, 33))
    for i, (sx, sy, h, fx, fy, beta) in enumerate(rows):
        imm, known, count = variants[i]
        mean = np.array([fx, fy, *col[i]])
        blob = np.array([beta, *(col[i] + rs.uniform(-6, 6, 3))])
        pse = math.atan2(fy - sy, fx - sx)
        inp[i] = np.concatenate([[sx, sy, h], tb._fields14(mean, cov[i]), [count], blob, qt, [pse if known else 123.0, imm | known], [rho[i], var[i]]])
    got = lib.probe_range(1, inp)
    assert got.shape == (n, 16)
    for i, (sx, sy, h, fx, fy, beta) in enumerate(rows):
        imm, known, count = variants[i]
        mean, blob = inp[i, 3:8], inp[i, 18:22]
        nm, nc, lw, aux = rref.ekf_update_dense(sx, sy, h, mean, cov[i], blob, rho[i], var[i], Qt)
        pot = bool(count & POT)
        want_lw = math.log(0.1) if pot else float(lw)
        assert abs(got[i, 0] - want_lw) < 1e-10 * max(1.0, abs(want_lw)), (i, got[i, 0], want_lw)
        if imm:
            assert np.array_equal(got[i, 1:15], inp[i, 3:17]) and got[i, 15] == count, i
        else:
            assert np.allclose(got[i, 1:6], nm, rtol=1e-12, atol=1e-12), (i, got[i, 1:6] - nm)
            assert np.allclose(got[i, 6:15], tb._fields14(nm, nc)[5:], rtol=1e-10, atol=1e-13), (i, got[i, 6:15] - tb._fields14(nm, nc)[5:])
            c2 = (count & ~POT) + 2
            assert got[i, 15] == (c2 | POT if pot and c2 <= 5 else c2), (i, got[i, 15])
    # a NaN range: the bearing model's update, bit for bit
    nan = inp.copy()
    nan[:, 31] = np.nan
    plain = lib.probe_bearing(1, np.concatenate([inp[:, :31], np.zeros((n, 1))], axis=1))
    assert np.array_equal(lib.probe_range(1, nan), plain[:, :16])
    # the refusals of the entry point itself; the bearing probe still has no what = 2, the model no value 2
    for what in (2, -1):
        with pytest.raises(lib.PkError) as e:
            lib.probe_range(what, inp[:1, :1])
        assert e.value.status == lib.PK_ERR_INVALID and "neither 0" in str(e.value)
    bad = inp[:1].copy()
    bad[0, 30] = 4.0
    with pytest.raises(lib.PkError) as e:
        lib.probe_range(1, bad)
    assert e.value.status == lib.PK_ERR_INVALID and "bit 0" in str(e.value)
    with pytest.raises(lib.PkError) as e:
        lib.probe_bearing(2, inp[:1, :1])
    assert e.value.status == lib.PK_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- the drive
def _observe(lib, g, mode, row, P):
    """One step of the drive on device filter g through one of the entry points that take blobs; the ids where the call gives them."""
    blobs, rho, var, z, u = row["blobs"], row["rho"], row["var"], row["z"], row["u"]
    B = len(blobs)
    if mode == "step":  # pk_step: motion, observe and resample in one call
        g.scan_ranges(rho, var)
        g.step(V, W, DT, blobs, u, z=z, domain=lib.PK_WEIGHTS_LOG)
        return None
    g.motion(V, W, DT, z=z)
    if mode == "staged":  # pk_stage_scan consumes the ranges; the staged scan keeps them
        g.scan_ranges(rho, var)
        g.stage_scan(blobs)
        assert g.scan_ranges_state() == (0, B)
        g.observe_staged(fresh=True)
        assert g.scan_ranges_state() == (0, 0)
        return None
    if mode == "associate":  # pk_associate runs the same rule and touches nothing; then the observe
        g.scan_ranges(rho, var)
        assert g.scan_ranges_state() == (B, 0)
        assert np.array_equal(g.associate(blobs), row["ids"])
        assert g.scan_ranges_state() == (0, 0)
    g.scan_ranges(rho, var)
    return g.observe(blobs, return_ids=True, fresh=True)


MODES = ("associate", "staged", "step", "observe", "staged", "step")


@pytest.mark.parametrize("kind", ["all", "mixed"])
@pytest.mark.parametrize("L,B,P", SHAPES)
def test_general_route_against_the_reference_through_both_association_kernels(lib, L, B, P, kind):
    world, covs, rows, o = oracle_drive(L, B, P, kind)
    assert_margins(o, (L, kind))
    if L >= 65:  # the depth pair is contested in every scan, and the range settles it
        for r in rows:
            assert (r["ids"][:, 30] == 31 if B == L else r["ids"][:, 30] > 0).all() and (r["ids"][:, 30] != r["ids"][:, 31]).all()
    f = tb._device(lib, P, world, covs)
    brute = tb._device(lib, P, world, covs, opts={"assoc_kernel": 1})
    for s, r in enumerate(rows):
        for g in (f, brute):
            got = _observe(lib, g, MODES[s], r, P)
            if got is not None:
                assert np.array_equal(got, r["ids"]), (s, int((got != r["ids"]).sum()))
            assert g.observe_route() == "ml_general"
            if MODES[s] != "step":
                lw = g.download_log_weights()
                assert np.allclose(lw, r["logw"], rtol=0, atol=tb.RTOL), (s, np.abs(lw - r["logw"]).max())
                assert np.array_equal(g.resample(r["u"], domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), r["anc"]), s
            tb._compare_state(lib, g, _State(r), ("step", s))
            assert np.allclose(g.download_poses()[:, :3], r["xyh"], rtol=1e-12, atol=1e-13), s
        for a, b in zip(brute.download_landmarks(), f.download_landmarks()):
            assert np.array_equal(a, b), s
    assert rows[-1]["pose"][2] < 0 < H0, "the heading did not wrap inside the run"
    f.close()
    brute.close()


def test_one_blob_supplied_ids_and_a_landmark_seen_with_and_without_a_range(lib):
    P, L = 64, 12
    world, covs = synthetic_world(L, seed=5)
    imm = np.zeros(L, dtype=np.uint8)
    imm[7] = 1
    f = tb._device(lib, P, world, covs, imm)
    o = RangeBearingOracle(P, world, covs, immutable=imm)
    o.h[:] = H0
    rs, rr = np.random.RandomState(1), np.random.RandomState(2)
    pose = (0.0, 0.0, H0)
    for s in range(6):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
        rho, var = range_scan(world, pose, rr, *SIGMA_R)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        ids = np.arange(1, L + 1, dtype=np.int32)
        ids[5] = 0                      # an unmatched blob
        ids[9] = 9                      # landmark 9 seen twice, by blobs 8 and 9:
        rho[8 + s % 2] = np.nan         # ranged then unranged, and the other way round
        if s >= 4:
            rho[::3] = np.nan
        o.reset_weights()
        o.motion(V, W, DT, z)
        o.observe(blobs, ids, rho, var)
        logw = o.logw.copy()
        anc = low_variance_ancestors(np.exp(logw - np.max(logw)), u)
        o.gather(anc)
        f.motion(V, W, DT, z=z)
        f.scan_ranges(rho, var)
        f.observe(blobs, ids=ids, fresh=True)
        assert f.observe_route() == "known_ids" and f.scan_ranges_state() == (0, 0)
        lw = f.download_log_weights()
        assert np.allclose(lw, logw, rtol=0, atol=tb.RTOL), (s, np.abs(lw - logw).max())
        assert np.array_equal(f.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), s
        tb._compare_state(lib, f, o, ("step", s))
    # maximum likelihood: landmark 3 shown by two blobs, the first ranged and the second not, then the other way round; and B = 1
    for order in (0, 1):
        blobs = wrapped_scan(world[[0, 3, 3, 6]], pose, rs, SIGMA_B, SIGMA_C)
        rho, var = range_scan(world[[0, 3, 3, 6]], pose, rr, *SIGMA_R)
        rho[1 + order] = np.nan
        o.reset_weights()
        want = o.observe(blobs, None, rho, var)
        assert (want[:, 1] == 4).all() and (want[:, 2] == 4).all()
        f.scan_ranges(rho, var)
        assert np.array_equal(f.observe(blobs, return_ids=True, fresh=True), want)
        tb._compare_state(lib, f, o, ("twice", order), o.logw)
    blobs = wrapped_scan(world[2:3], pose, rs, SIGMA_B, SIGMA_C)
    rho, var = range_scan(world[2:3], pose, rr, *SIGMA_R)
    o.reset_weights()
    want = o.observe(blobs, None, rho, var)
    assert (want == 3).all()
    f.scan_ranges(rho, var)
    assert np.array_equal(f.observe(blobs, return_ids=True, fresh=True), want)
    tb._compare_state(lib, f, o, "B = 1", o.logw)
    assert_margins(o, "supplied ids")
    f.close()


def test_the_step_that_uploads_its_scan_with_the_motion_launch_carries_the_ranges(lib):
    """pk_step without supplied normals stages the scan itself and sends it with the motion kernel: the same bits as the three calls."""
    L, B, P = 65, 65, 64
    world, covs, sees = scene(L, B)
    a, b = tb._device(lib, P, world, covs), tb._device(lib, P, world, covs)
    for s, (pose, blobs, rho, var, zseed, u) in enumerate(scans(world, sees, 3, "mixed")):
        a.scan_ranges(rho, var)
        a.step(V, W, DT, blobs, u, seed=7, draw=s, domain=lib.PK_WEIGHTS_LOG)
        b.motion(V, W, DT, seed=7, draw=s)
        b.scan_ranges(rho, var)
        b.observe(blobs, fresh=True)
        b.resample(u, domain=lib.PK_WEIGHTS_LOG)
        assert a.scan_ranges_state() == (0, 0)
        assert np.array_equal(a.download_poses(), b.download_poses()), s
        for x, y in zip(a.download_landmarks(), b.download_landmarks()):
            assert np.array_equal(x, y), s
    # ... and differs from the step without ranges (the ranges were used)
    c = tb._device(lib, P, world, covs)
    for s, (pose, blobs, rho, var, zseed, u) in enumerate(scans(world, sees, 3, "mixed")):
        c.step(V, W, DT, blobs, u, seed=7, draw=s, domain=lib.PK_WEIGHTS_LOG)
    assert not np.array_equal(c.download_landmarks()[0], a.download_landmarks()[0])
    for g in (a, b, c):
        g.close()


# ---------------------------------------------------------------------------------------------------------------- no finite range
@pytest.mark.parametrize("assoc_kernel", [0, 1])
def test_an_armed_scan_without_a_finite_range_is_the_scan_never_armed(lib, assoc_kernel):
    L, B, P = 65, 65, 64
    world, covs, sees = scene(L, B)
    armed = tb._device(lib, P, world, covs, opts={"assoc_kernel": assoc_kernel})
    never = tb._device(lib, P, world, covs, opts={"assoc_kernel": assoc_kernel})
    for s, (pose, blobs, rho, var, zseed, u) in enumerate(scans(world, sees, 4, "none")):
        z = np.random.RandomState(zseed).standard_normal((P, 3))
        ids = None if s != 2 else np.arange(1, B + 1, dtype=np.int32)
        got = []
        for g in (armed, never):
            g.motion(V, W, DT, z=z)
            if g is armed:
                g.scan_ranges(rho, None if s == 1 else var)  # (no variance is read where no range is finite)
                assert g.scan_ranges_state() == (B, 0)
            got.append(g.observe(blobs, ids=ids, return_ids=True, fresh=True))
        assert np.array_equal(got[0], got[1]), s
        assert armed.observe_route() == never.observe_route() and armed.device_bytes() == never.device_bytes(), s
        assert np.array_equal(armed.download_log_weights(), never.download_log_weights()), s
        for g in (armed, never):
            g.resample(u, domain=lib.PK_WEIGHTS_LOG)
        assert np.array_equal(armed.download_poses(), never.download_poses()), s
        for x, y in zip(armed.download_landmarks(), never.download_landmarks()):
            assert np.array_equal(x, y), s
    armed.close()
    never.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def _snapshot(f):
    return [f.download_log_weights(), f.download_poses()] + list(f.download_landmarks())


def _refused(lib, f, call, status, text, before):
    with pytest.raises(lib.PkError) as e:
        call()
    assert e.value.status == status and text in str(e.value), (status, text, e.value.status, str(e.value))
    assert f.scan_ranges_state()[0] == 0, "a refused call disarms"
    for a, b in zip(_snapshot(f), before):
        assert np.array_equal(a, b), text


def test_refusals_each_with_its_status_and_text(lib):
    import parakeet_slam_amd as pk

    P, L, B = 16, 12, 12
    world, covs = synthetic_world(L, seed=5)
    blobs = wrapped_scan(world, (0.0, 0.0, 0.0))
    rho, var = range_scan(world, (0.0, 0.0, 0.0))
    var[:] = 0.01
    ids = np.arange(1, B + 1, dtype=np.int32)
    f = tb._device(lib, P, world, covs, heading=0.0)
    f.observe(blobs, fresh=True)
    before = _snapshot(f)
    # the arming call itself: nothing is armed behind a refusal, and what was armed is gone
    for bad_r, bad_v in ((-1.0, 0.01), (0.0, 0.01), (np.inf, 0.01), (5.0, 0.0), (5.0, -1.0), (5.0, np.nan), (5.0, np.inf)):
        f.scan_ranges(rho, var)
        r2, v2 = rho.copy(), var.copy()
        r2[3], v2[3] = bad_r, bad_v
        _refused(lib, f, lambda: f.scan_ranges(r2, v2), lib.PK_ERR_INVALID, "pk_scan_ranges", before)
    f.scan_ranges(rho, var)
    _refused(lib, f, lambda: f.scan_ranges(rho, None), lib.PK_ERR_INVALID, "variances[0]", before)
    f.scan_ranges(rho, var)
    assert f.scan_ranges_state() == (B, 0)
    f.scan_ranges(None)
    assert f.scan_ranges_state() == (0, 0)
    # another number of blobs, through every consuming entry point
    calls = [lambda: f.observe(blobs[:5]), lambda: f.observe(blobs[:5], fresh=True), lambda: f.observe(blobs[:5], ids=ids[:5]),
             lambda: f.associate(blobs[:5]), lambda: f.stage_scan(blobs[:5]),
             lambda: f.step(V, W, DT, blobs[:5], 0.5, z=np.zeros((P, 3))), lambda: f.step(V, W, DT, blobs[:5], 0.5, seed=1),
             lambda: f.step_odom((0.0, 0.5, 0.0), (0.01, 0.01, 0.01, 0.01), blobs[:5], 0.5, seed=1)]
    for call in calls:
        f.scan_ranges(rho, var)
        _refused(lib, f, call, lib.PK_ERR_INVALID, "named the ranges of a scan of 12 blobs, this one has 5", before)
    # the proposal
    for call in (lambda: f.propose(V, W, DT, blobs, seed=1), lambda: f.propose(V, W, DT, blobs, seed=1, ids=ids)):
        f.scan_ranges(rho, var)
        _refused(lib, f, call, lib.PK_ERR_UNSUPPORTED, "not part of the measurement-informed proposal", before)
    # a staged scan keeps its ranges, and a filter that changed under it refuses it and discards it
    f.scan_ranges(rho, var)
    f.stage_scan(blobs)
    f.set_measurement_model("reference")
    _refused(lib, f, lambda: f.observe_staged(fresh=True), lib.PK_ERR_UNSUPPORTED, "option of the bearing model", before)
    assert f.scan_ranges_state() == (0, 0)
    # the reference model (it comes before the dense layout and growing maps; the number of blobs before it)
    for call in (lambda: f.observe(blobs), lambda: f.observe(blobs, ids=ids), lambda: f.associate(blobs), lambda: f.stage_scan(blobs),
                 lambda: f.step(V, W, DT, blobs, 0.5, seed=1)):
        f.scan_ranges(rho, var)
        _refused(lib, f, call, lib.PK_ERR_UNSUPPORTED, "option of the bearing model", before)
    f.scan_ranges(rho, var)
    _refused(lib, f, lambda: f.observe(blobs[:5]), lib.PK_ERR_INVALID, "this one has 5", before)
    f.set_measurement_model("bearing")
    f.close()
    # growing maps
    g = tb._device(lib, P, world, covs, heading=0.0)
    g.grow_enable(L - 2, 16, 30.0)
    before = _snapshot(g)
    for call in (lambda: g.observe(blobs), lambda: g.step(V, W, DT, blobs, 0.5, seed=1)):
        g.scan_ranges(rho, var)
        _refused(lib, g, call, lib.PK_ERR_UNSUPPORTED, "no kernel for growing maps", before)
    g.close()
    # the dense layout: the bearing model's own refusal, in its own words
    d = tb._device(lib, P, world, covs, heading=0.0)
    Qt = 0.1 * np.identity(4)
    Qt[0, 1] = Qt[1, 0] = 0.01
    d.set_measurement_noise(Qt)
    before = _snapshot(d)
    for call in (lambda: d.observe(blobs), lambda: d.associate(blobs), lambda: d.observe(blobs, ids=ids), lambda: d.stage_scan(blobs)):
        d.scan_ranges(rho, var)
        _refused(lib, d, call, lib.PK_ERR_UNSUPPORTED, "has no kernel for the dense layout", before)
    d.close()
    # what stays as it was
    h = tb._device(lib, P, world, covs, heading=0.0)
    with pytest.raises(lib.PkError) as e:
        h.set_measurement_model(2)
    assert e.value.status == lib.PK_ERR_INVALID
    assert sorted(lib.MEASUREMENT_MODELS) == ["bearing", "reference"]
    h.close()
    # the facade
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(4)]
    pk.msgs.Time.set_now(0.0)
    kw = dict(num_particles=8, measurement_model="bearing")
    for bad, text in (((0.0, 0.0), "cannot both be 0"), ((-0.1, 0.0), "finite and >= 0"), ((0.1, np.inf), "finite and >= 0"),
                      ((np.nan, 0.1), "finite and >= 0"), ((0.1,), "sigma0, sigma1"), (0.1, "sigma0, sigma1")):
        with pytest.raises(ValueError, match=text):
            pk.FastSLAM(feats, range_noise=bad, **kw)
    with pytest.raises(ValueError, match="measurement_model='bearing'"):
        pk.FastSLAM(feats, num_particles=8, range_noise=SIGMA_R)
    with pytest.raises(ValueError, match="proposal='measurement'"):
        pk.FastSLAM(feats, range_noise=SIGMA_R, proposal="measurement", **kw)
    with pytest.raises(ValueError, match="new_landmarks=True"):
        pk.FastSLAM(feats, range_noise=SIGMA_R, new_landmarks=True, spare_landmarks=2, **kw)
    with pytest.raises(ValueError, match="one GPU"):
        pk.FastSLAM(feats, range_noise=SIGMA_R, devices=[0, 0], **kw)
    with pytest.raises(ValueError, match="'reference' \\(default\\) or 'bearing'"):
        pk.FastSLAM(feats, num_particles=8, measurement_model="textbook")
    fs = pk.FastSLAM(feats, **kw)
    view = tb._View(pk, blobs[:4])
    view.last_sensor_reading.observes = np.concatenate([blobs[:4], rho[:4, None]], axis=1)
    with pytest.raises(ValueError, match="needs range_noise"):
        fs.cam_cb(view)
    fs.close()


# ---------------------------------------------------------------------------------------------------------------- the facade
def _view(pk, blobs, rho, as_array):
    v = tb._View(pk, blobs)
    if as_array:
        v.last_sensor_reading.observes = np.concatenate([blobs, rho[:, None]], axis=1)
    else:
        for o, r in zip(v.last_sensor_reading.observes, rho):
            if r == r:
                o.range = float(r)
            elif int(o.bearing * 1e6) % 2:
                o.range = None  # (absent, None and NaN all mean "none")
    return v


def test_facade_runs_the_pushed_map_drive_with_message_objects_and_with_arrays(lib):
    import parakeet_slam_amd as pk

    P, L, steps = 64, 12, 8
    world, covs = synthetic_world(L, seed=5)
    start = world.copy()
    start[:, :2] += 0.5 * np.random.RandomState(101).standard_normal((L, 2))
    feats = [pk.Feature(mean=start[l].copy(), covar=covs[l].copy()) for l in range(L)]
    kw = dict(num_particles=P, weight_domain="log", rng="global", measurement_model="bearing")
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = V, W
    filters = []
    for as_array in (False, True, None):  # None: message objects with ranges on a filter WITHOUT range_noise -- they are ignored
        np.random.seed(11)
        random.seed(7)
        pk.msgs.Time.set_now(0.0)
        fs = pk.FastSLAM(feats, device=0, range_noise=None if as_array is None else SIGMA_R, **kw)
        fs.last_control = tw
        o = RangeBearingOracle(P, start, covs)
        rs, pr, noise, rr = np.random.RandomState(11), random.Random(7), np.random.RandomState(8), np.random.RandomState(9)
        pose = (0.0, 0.0, 0.0)
        for s in range(steps):
            pose = truth_step(pose, V, W, DT)
            blobs = wrapped_scan(world, pose, noise, SIGMA_B, SIGMA_C)
            rho, _ = range_scan(world, pose, rr, SIGMA_R[0], SIGMA_R[1], 3 if s % 2 else None)
            sig = SIGMA_R[0] + SIGMA_R[1] * rho
            pk.msgs.Time.set_now(DT * (s + 1))
            fs.cam_cb(_view(pk, blobs, rho, bool(as_array)))
            z, u = rs.standard_normal((P, 3)), pr.random()
            o.reset_weights()
            o.motion(V, W, DT, z)
            if as_array is None:
                o.observe(blobs)
            else:
                o.observe(blobs, None, rho, sig * sig)
            o.gather(low_variance_ancestors(np.exp(o.logw - np.max(o.logw)), u))
            assert fs._filter.observe_route() == "ml_general"
            assert np.allclose(fs.summary(), o.summary(), rtol=1e-12, atol=1e-14), (as_array, s, fs.summary(), o.summary())
        assert_margins(o, ("facade", as_array))
        tb._compare_state(lib, fs._filter, o, ("facade", as_array))
        est = o.mean[:, :, :2].mean(axis=0)
        print("facade, %s: landmarks' mean distance from the truth after %d steps %.3f m"
              % ("no ranges" if as_array is None else "ranges", steps, float(np.mean(np.hypot(*(est - world[:, :2]).T)))))
        filters.append(fs)
    # message objects and the (B, 5) array: the same filter, bit for bit (the same ids, the same updates)
    for a, b in zip(_snapshot(filters[0]._filter), _snapshot(filters[1]._filter)):
        assert np.array_equal(a, b)
    assert not np.array_equal(filters[0]._filter.download_landmarks()[0], filters[2]._filter.download_landmarks()[0])
    for fs in filters:
        fs.close()

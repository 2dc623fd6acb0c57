"""GPU: the path estimate by the weights and the most likely particle (pk_path_summary_weighted, pk_best_particle;
pk_k_path_weighted.hip; DESIGN.md section 4, "The weighted path estimate").

No map and no scan anywhere but in the facade test: DeviceFilter(P, 0), rings built by hand through path_upload or driven by
motion and resample_adaptive, chosen log-weights.  The reference is path_weighted_reference.py, where the tolerances are stated;
every check prints the errors it measured."""
import random

import numpy as np
import pytest

import path_reference as pr
import path_weighted_reference as pw
from conftest import load_golden
from test_gpu_adaptive import facade_filter, giants, run_facade
from test_gpu_path import raises, same_bits, start_poses

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1  # PK_ERR_STATE, PK_ERR_INVALID
LIN, LOG = 0, 1          # PK_WEIGHTS_LINEAR, PK_WEIGHTS_LOG


def spread_logw(rs, P):
    """Log-weights over thirteen decades, a tenth of the particles at weight 0."""
    logw = rs.uniform(-30.0, 0.0, P)
    logw[rs.permutation(P)[:P // 10]] = -np.inf
    return logw


def ring_filter(lib, rs, P, held, cap=8, make=start_poses):
    """A filter whose ring holds `held` rows of its own poses and random, unsorted ancestor maps."""
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(make(rs, P))
    f.path_enable(cap)
    poses = np.stack([make(rs, P)[:, :3] for _ in range(held)]) if held else np.empty((0, P, 3))
    anc = rs.randint(0, P, (held, P)).astype(np.int32)
    if held:
        f.path_upload(poses, anc)
    return f, poses, anc


def same_summary(a, b):
    return same_bits(a.mean, b.mean) and same_bits(a.spread, b.spread) and a.n_eff == b.n_eff


def check_call(f, dom, poses, anc, logw, what):
    """The call against the reference."""
    got = f.path_summary_weighted(dom)
    pw.check(got, poses, anc, f.download_poses()[:, :3], logw, dom == LOG, what=what)
    return got


# ---- 1. hand-built rings: sizes that straddle a wave, a workgroup and the grid (65 793 = 256 x 256 + 257: a second turn of the
# grid-stride loop), an empty ring, one row, several
@pytest.mark.parametrize("held", [0, 1, 5])
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 257, 4097, 65793])
def test_hand_built_rings(lib, P, held):
    rs = np.random.RandomState(1000 * held + P % 997)
    f, poses, anc = ring_filter(lib, rs, P, held)
    logw = spread_logw(rs, P)
    f.upload_log_weights(logw)
    assert f.path_shape()[:2] == (8, held)
    for dom in (LIN, LOG):
        got = check_call(f, dom, poses, anc, logw, "P = %d, %d rows, domain %d" % (P, held, dom))
        assert got.held == held and got.first_step == 0
    if P > 1 and held == 5:  # particle 0, whose lineage is the reference pose, has no weight
        logw[0] = -np.inf
        logw[1] = -0.5
        f.upload_log_weights(logw)
        for dom in (LIN, LOG):
            check_call(f, dom, poses, anc, logw, "P = %d, particle 0 at weight 0, domain %d" % (P, dom))
    f.close()


def test_a_deep_ring_of_many_particles(lib):
    """Eleven rows of 65 793 particles: eight rows at a time by threads that hold two particles, then three rows one by one."""
    P, held = 65793, 11
    rs = np.random.RandomState(12)
    f, poses, anc = ring_filter(lib, rs, P, held, cap=12)
    logw = spread_logw(rs, P)
    f.upload_log_weights(logw)
    check_call(f, LOG, poses, anc, logw, "P = %d, %d rows" % (P, held))
    f.close()


# ---- 2. a coalesced row: its pose bit for bit, exactly no spread
def test_a_coalesced_row(lib):
    P, held = 257, 3
    rs = np.random.RandomState(21)
    f, poses, anc = ring_filter(lib, rs, P, held)
    anc[0][:] = 7
    f.path_upload(poses, anc)
    logw = spread_logw(rs, P)
    f.upload_log_weights(logw)
    for dom in (LIN, LOG):
        got = check_call(f, dom, poses, anc, logw, "coalesced row, domain %d" % dom)
        assert got.mean[0, 0] == poses[0, 7, 0] and got.mean[0, 1] == poses[0, 7, 1]
        assert pr.angle_diff(got.mean[0, 2], poses[0, 7, 2]) <= 1e-12
        assert got.spread[0, :3].tolist() == [0.0, 0.0, 0.0]
        assert abs(got.spread[0, 3] - 1.0) <= 1e-12
        assert np.all(got.spread[1:, [0, 2]] > 0.0)
    f.close()


# ---- 3. a driven filter: motion and resample_adaptive, kept and resampled in turn as in test_gpu_adaptive.test_with_the_ring
def test_a_driven_filter(lib):
    P = 1025
    rs = np.random.RandomState(31)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(rs, P, rs.uniform(0.1, 1.0, P) ** 4))
    f.path_enable(8)
    poses, anc = [], []
    for s in range(6):
        f.motion(0.3, 0.1, 0.1, z=rs.standard_normal((P, 3)))
        if s % 2 == 1:
            giants(f, rs, P)
        before = f.download_poses()
        a = f.resample_adaptive(float(rs.uniform(0.0, 1.0)), 0.0 if s % 2 == 0 else 2.0, domain=LOG, return_ancestors=True)
        poses.append(before[:, :3].copy())
        anc.append(a.astype(np.int32))
        assert f.resample_stats().resampled == (s % 2 == 1)
        if s % 2 == 1:  # (a resample leaves unit weights: others, so that the estimate is not the plain one)
            f.upload_log_weights(spread_logw(rs, P))
        logw = f.download_log_weights()
        for dom in (LIN, LOG):
            check_call(f, dom, np.array(poses), np.array(anc), logw, "driven, step %d, domain %d" % (s, dom))
    assert f.path_shape() == (8, 6, 6)
    surv = pr.survivors(np.array(anc), P)
    assert np.any(surv < P), surv  # some row has fewer than P distinct ancestors
    f.close()


# ---- 4. the ring wraps: capacity 3 with seven rows recorded; and 19 with 23, where the kernel takes eight rows at a time -- two
# such turns, the second across the ring's seam, and three rows one by one
@pytest.mark.parametrize("cap,steps", [(3, 7), (19, 23)])
def test_ring_wrap(lib, cap, steps):
    P = 300
    rs = np.random.RandomState(41)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(rs, P, rs.uniform(0.1, 1.0, P) ** 3))
    f.path_enable(cap)
    poses, anc = [], []
    for s in range(steps):
        f.motion(0.3, 0.1, 0.1, z=rs.standard_normal((P, 3)))
        before = f.download_poses()
        a = f.resample(float(rs.uniform(0.0, 1.0)), return_ancestors=True)
        poses.append(before[:, :3].copy())
        anc.append(a.astype(np.int32))
        f.upload_log_weights(spread_logw(rs, P))  # (the next resample's weights too)
    assert f.path_shape() == (cap, cap, steps)
    logw = f.download_log_weights()
    for dom in (LIN, LOG):
        got = check_call(f, dom, np.array(poses[-cap:]), np.array(anc[-cap:]), logw, "wrapped ring, domain %d" % dom)
        assert got.first_step == steps - cap and got.steps().tolist() == list(range(steps - cap, steps + 1))
    f.close()


# ---- 5. equal log-weights: path_summary's estimate
@pytest.mark.parametrize("P", [65, 4097])
def test_equal_log_weights_are_the_plain_summary(lib, P):
    rs = np.random.RandomState(50 + P)
    f, poses, anc = ring_filter(lib, rs, P, 5)
    f.upload_log_weights(np.full(P, -2.5))
    plain = f.path_summary()
    for dom in (LIN, LOG):
        got = f.path_summary_weighted(dom)
        errs = pw.errors(got.mean, got.spread, plain.mean, plain.spread)
        e_n = abs(got.n_eff - P) / P
        print("P = %d, domain %d against path_summary: mean %.2e, var %.2e, cov %.2e, R %.2e, heading %.2e; n_eff %.2e" % ((P, dom) + errs + (e_n,)))
        assert max(errs) <= pw.TOL and e_n <= pw.TOL
    f.close()


# ---- 6. row `held` is pk_summary_weighted's estimate, n_eff its n_eff
@pytest.mark.parametrize("P", [63, 1025, 65793])
def test_row_held_against_summary_weighted(lib, P):
    rs = np.random.RandomState(60 + P % 997)
    f, poses, anc = ring_filter(lib, rs, P, 5)
    f.upload_log_weights(spread_logw(rs, P))
    for dom in (LIN, LOG):
        got, now = f.path_summary_weighted(dom), f.summary_weighted(dom)
        errs = pw.errors(got.mean[5:], got.spread[5:], now.mean[None], now.spread[None])
        print("P = %d, domain %d, row held against summary_weighted: mean %.2e, var %.2e, cov %.2e, R %.2e, heading %.2e" % ((P, dom) + errs))
        assert max(errs) <= pw.TOL
        assert got.n_eff == now.n_eff
    f.close()


# ---- 7. far from the origin: poses near 1e6 with a spread of 1e-3, the covariance to the same tolerance
def far_poses(rs, P, weights=None):
    return np.column_stack([1e6 + 1e-3 * rs.standard_normal(P), -2e6 + 1e-3 * rs.standard_normal(P), rs.uniform(-0.3, 0.3, P), np.ones(P)])


def test_far_from_the_origin(lib):
    P = 4097
    rs = np.random.RandomState(71)
    f, poses, anc = ring_filter(lib, rs, P, 5, make=far_poses)
    logw = spread_logw(rs, P)
    f.upload_log_weights(logw)
    for dom in (LIN, LOG):
        check_call(f, dom, poses, anc, logw, "1e6 from the origin, domain %d" % dom)
    f.close()


# ---- 8. log-weights near -800: the log domain carries on, the linear one has nothing left
def test_underflow(lib):
    P = 1025
    rs = np.random.RandomState(81)
    f, poses, anc = ring_filter(lib, rs, P, 5)
    logw = rs.uniform(-805.0, -795.0, P)
    f.upload_log_weights(logw)
    check_call(f, LOG, poses, anc, logw, "log-weights near -800")
    assert "sum to" in raises(lib, STATE, f.path_summary_weighted, LIN)
    f.close()


# ---- 9. the same bits twice, and nothing of the filter changes
def test_determinism_and_purity(lib):
    P = 4097
    rs = np.random.RandomState(91)
    f, poses, anc = ring_filter(lib, rs, P, 5)
    f.resample(0.3)  # (map sources that are not the identity, a sixth row)
    f.upload_log_weights(spread_logw(rs, P))
    before = (f.download_poses()[:, :3], f.download_log_weights(), f.download_sources()) + f.path_download()
    plain = f.path_summary()
    for dom in (LIN, LOG):
        a, b = f.path_summary_weighted(dom), f.path_summary_weighted(dom)
        assert same_summary(a, b)
    after = (f.download_poses()[:, :3], f.download_log_weights(), f.download_sources()) + f.path_download()
    for x, y in zip(before, after):
        assert same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y)
    again = f.path_summary()
    assert same_bits(plain.mean, again.mean) and same_bits(plain.spread, again.spread) and np.array_equal(plain.survivors, again.survivors)
    assert f.path_shape() == (8, 6, 6)
    f.close()


# ---- 10. refusals, NULL outputs, memory
def test_refusals_and_memory(lib):
    P, cap = 1000, 5
    rs = np.random.RandomState(101)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(rs, P, rs.uniform(0.1, 1.0, P)))
    assert "pk_path_enable" in raises(lib, STATE, f.path_summary_weighted, LOG)  # recording is off
    b0 = f.device_bytes()
    f.path_enable(cap)
    b1 = f.device_bytes()
    f.resample(0.5)
    f.resample(0.25)
    f.best_particle()
    assert f.device_bytes() == b1                  # nothing until the first call
    raises(lib, INVALID, f.path_summary_weighted, 2)  # a bad domain
    raises(lib, INVALID, f.path_summary_weighted, -1)
    assert f.device_bytes() == b1
    f.upload_log_weights(np.full(P, -np.inf))      # weights that sum to nothing
    assert "sum to" in raises(lib, STATE, f.path_summary_weighted, LIN)
    assert "sum to" in raises(lib, STATE, f.path_summary_weighted, LOG)
    f.upload_log_weights(spread_logw(rs, P))
    got = f.path_summary_weighted(LOG)
    b2 = f.device_bytes()
    assert b2 >= b1 + 12 * P                       # (the scratch: counted while held ...)
    f.path_summary_weighted(LIN)
    assert f.device_bytes() == b2
    # any output may be NULL
    c = f._lib
    mean, n_eff = np.empty((3, 3)), np.empty(1)
    assert c.pk_path_summary_weighted(f._h, LOG, None, None, None) == 0
    assert c.pk_path_summary_weighted(f._h, LOG, lib.dptr(mean), None, None) == 0 and same_bits(mean, got.mean)
    assert c.pk_path_summary_weighted(f._h, LOG, None, None, lib.dptr(n_eff)) == 0 and n_eff[0] == got.n_eff
    assert c.pk_best_particle(f._h, None, None) == 0
    f.path_enable(0)                               # (... and given back with the ring)
    assert f.device_bytes() == b0
    assert "pk_path_enable" in raises(lib, STATE, f.path_summary_weighted, LOG)
    f.best_particle()                              # needs no ring
    assert f.device_bytes() == b0
    f.close()


# ---- 11. the most likely particle
def upload_raw_log_weights(f, logw):
    """Log-weights the checked uploads refuse (NaN), by the way the sharded protocol's records come in: every particle adopted from
    a record of its own pose and the given log-weight.  Returns the owner of the record buffer, which must outlive the filter's use
    of it (``free_all``)."""
    from test_gpu_refusals import Hip

    stride = f.particle_bytes()
    assert stride % 8 == 0
    rec = np.zeros((f.P, stride // 8))
    rec[:, :3] = f.download_poses()[:, :3]
    rec[:, 3] = logw
    hip = Hip()
    buf = hip.zeros(rec.nbytes)
    assert hip.rt.hipMemcpy(buf, rec.ctypes.data, rec.nbytes, 1) == 0  # hipMemcpyHostToDevice
    f.adopt_particles(-(np.arange(f.P) + 1), buf, f.P)
    return hip


@pytest.mark.parametrize("P", [1, 65, 1025, 262145])
def test_best_particle(lib, P):
    rs = np.random.RandomState(110 + P % 997)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(rs, P))
    base = rs.uniform(-30.0, -1.0, P)
    for at in (0, 255, 256, 1023, 1024, P - 1):
        if at >= P:
            continue
        logw = base.copy()
        logw[at] = -0.25
        f.upload_log_weights(logw)
        assert f.best_particle() == (at, -0.25), at
        assert f.best_particle() == f.best_particle()
    # equal maxima: the lowest index
    several = sorted(set(int(i) for i in rs.randint(0, P, 5)) | {P - 1})
    logw = base.copy()
    logw[several] = 0.5
    f.upload_log_weights(logw)
    assert f.best_particle() == (several[0], 0.5)
    # all at weight 0: index 0
    f.upload_log_weights(np.full(P, -np.inf))
    assert f.best_particle() == (0, -np.inf)
    # NaN never wins, wherever it stands; all NaN: nothing to hand out
    logw = base.copy()
    nans = sorted(set(int(i) for i in rs.randint(0, P, 7)) | {0})
    logw[nans] = np.nan
    f.close()
    cases = [(np.full(P, np.nan), None)]
    if P > len(nans):
        at = int(np.flatnonzero(~np.isnan(logw))[-1])
        logw[at] = -0.125
        cases.append((logw.copy(), (at, -0.125)))
        logw[~np.isnan(logw)] = -np.inf  # weight 0 beside NaN: the lowest index that is a number
        cases.append((logw.copy(), (int(np.flatnonzero(~np.isnan(logw))[0]), -np.inf)))
    for raw, want in cases:  # (a filter each: one adoption, nothing folded back)
        f = lib.DeviceFilter(P, 0)
        f.upload_poses(start_poses(rs, P))
        keep = upload_raw_log_weights(f, raw)
        assert np.array_equal(np.isnan(f.download_log_weights()), np.isnan(raw))
        if want is None:
            assert "NaN" in raises(lib, STATE, f.best_particle)
        else:
            assert f.best_particle() == want and f.best_particle() == want
        f.close()
        keep.free_all()


# ---- 12. the facade
def test_facade():
    import parakeet_slam_amd as pk
    from parakeet_slam_amd import msgs, path as pkpath

    pk.msgs = msgs
    g = load_golden("step_small")
    np.random.seed(3)
    random.seed(3)
    msgs.Time.set_now(0.0)
    fs = facade_filter(pk, g, weight_domain="log", record_path=8, resample_threshold=0.5)
    run_facade(pk, fs, g, 5)
    filt = fs._filter
    assert filt.path_shape() == (8, 5, 5)
    plain = fs.path_summary()
    assert isinstance(plain, pkpath.PathSummary)
    got = fs.path_summary(weighting="weights")
    assert isinstance(got, pkpath.WeightedPathSummary) and got.mean.shape == (6, 3) and got.spread.shape == (6, 4) and got.first_step == 0
    ring_p, ring_a = filt.path_download()
    logw = filt.download_log_weights()
    assert len(np.unique(logw)) > 1  # (the filter kept: the weights are mid-way, not all equal)
    pw.check(got, ring_p, ring_a, filt.download_poses()[:, :3], logw, True, what="facade")
    assert got.n_eff == fs.pose_summary().n_eff
    assert pkpath.as_poses(got)[5] == tuple(float(v) for v in got.mean[5])
    for again in (fs.path_summary(), fs.path_summary(weighting="uniform"), fs.path_summary("uniform")):
        assert same_bits(plain.mean, again.mean) and same_bits(plain.spread, again.spread) and np.array_equal(plain.survivors, again.survivors)
    best = fs.best_particle()
    assert isinstance(best, int) and logw[best] == np.max(logw) and best == int(np.argmax(logw))
    assert same_bits(fs.best_path(), fs.particle_paths([best])[0]) and fs.best_path().shape == (6, 3)
    for bad in ("weighted", None, 1):
        with pytest.raises(ValueError, match="weighting"):
            fs.path_summary(weighting=bad)
    fs.close()
    plain_fs = facade_filter(pk, g, weight_domain="log")
    assert plain_fs.best_particle() == 0  # (unit weights: the lowest index)
    with pytest.raises(ValueError, match="record_path"):
        plain_fs.best_path()
    with pytest.raises(ValueError, match="record_path"):
        plain_fs.path_summary(weighting="weights")
    plain_fs.close()

"""GPU: adaptive resampling (pk_resample_adaptive, pk_step_adaptive, pk_resample_stats, pk_weight_sums, pk_summary_weighted;
pk_k_adaptive.hip; DESIGN.md section 4, "Adaptive resampling") -- the effective sample size and the verdict on the device, the
resample that can decline, and the pose summary by the weights.

Most tests need no map: DeviceFilter(P, 0) with chosen weights, as test_gpu_path.py does.  The reference is adaptive_reference.py
(where the tolerances are stated), fed with the log-weights and poses downloaded in front of the call.  Sizes straddle a wave, a
256-lane workgroup, the 1 024-particle scan block and the 256 scan blocks up to which the gated kernel scans the block totals itself."""
import math
import random

import numpy as np
import pytest

import adaptive_reference as ar
import path_reference as pr
from conftest import load_golden
from resample_reference import SCAN_BLOCK, ancestors_match_exact, true_weights
from test_gpu_path import View, raises, same_bits, start_poses

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1  # PK_ERR_STATE, PK_ERR_INVALID
LIN, LOG = 0, 1          # PK_WEIGHTS_LINEAR, PK_WEIGHTS_LOG
SIZES = [1, 63, 65, 1000, 1025, 4097, 262145]  # 262 145: 257 scan blocks, the path beyond kAncestorsScanMaxBlocks
GIANT = 1e3


def wide_weights(rs, P):
    """Weights over 12 decades; ``giants`` re-uploads a few of them a thousand times heavier than any."""
    return rs.uniform(0.1, 1.0, P) ** 12


def giants(f, rs, P):
    now = f.download_poses()
    for i in rs.randint(0, P, size=min(P, 3)):
        f.upload_pose(int(i), np.append(now[i, :3], GIANT * float(rs.uniform(0.5, 1.0))))


def new_filter(lib, P, seed, weights=None, shuffle_sources=True):
    """A filter with the given weights whose map sources are not the identity (one resample in front of the upload)."""
    rs = np.random.RandomState(seed)
    f = lib.DeviceFilter(P, 0)
    if shuffle_sources:
        f.upload_poses(start_poses(rs, P, rs.uniform(0.2, 1.0, P)))
        f.resample(0.37)
    f.upload_poses(start_poses(rs, P, weights))
    return f


def state(f):
    return f.download_poses()[:, :3], f.download_log_weights(), f.download_sources()


# ---- 1. a threshold above 1 is pk_resample
@pytest.mark.parametrize("dom", [LIN, LOG])
@pytest.mark.parametrize("P", SIZES)
def test_always_resampling_is_pk_resample(lib, P, dom):
    rs = np.random.RandomState(10 + P)
    w, u = wide_weights(rs, P), float(rs.uniform(0.0, 1.0))
    a, b = new_filter(lib, P, P, w), new_filter(lib, P, P, w)
    for f in (a, b):
        giants(f, np.random.RandomState(P), P)
    anc_a = a.resample(u, domain=dom, return_ancestors=True)
    anc_b = b.resample_adaptive(u, 2.0, domain=dom, return_ancestors=True)
    pa, _, sa = state(a)
    pb, lb, sb = state(b)
    assert np.array_equal(anc_a, anc_b)
    assert same_bits(pa, pb) and np.array_equal(sa, sb)
    assert same_bits(lb, np.zeros(P))  # unit weights, +0.0
    st = b.resample_stats()
    assert st.resampled and (st.calls, st.resamples) == (1, 1)
    if P > 65:
        assert np.unique(anc_b).size < P  # (the resample did select)
    a.close()
    b.close()


# ---- 2. threshold 0 keeps
@pytest.mark.parametrize("dom", [LIN, LOG])
@pytest.mark.parametrize("P", SIZES)
def test_threshold_zero_keeps(lib, P, dom):
    rs = np.random.RandomState(20 + P)
    f = new_filter(lib, P, P, wide_weights(rs, P))
    giants(f, rs, P)
    p0, l0, s0 = state(f)
    anc = f.resample_adaptive(float(rs.uniform(0.0, 1.0)), 0.0, domain=dom, return_ancestors=True)
    p1, l1, s1 = state(f)
    assert np.array_equal(anc, np.arange(P))
    assert same_bits(p0, p1) and np.array_equal(s0, s1)
    assert same_bits(l1, l0 - l0.max() if dom == LOG else l0)  # one rounded subtraction of the scan's shift
    st = f.resample_stats()
    assert not st.resampled and (st.calls, st.resamples) == (1, 0)
    assert st.shift == (l0.max() if dom == LOG else 0.0)
    if P > 1:
        assert not np.array_equal(s0, np.arange(P))  # (the sources that were carried over were not the identity)
    f.close()


# ---- 3. n_eff: the sums against the reference, S1 the resample's own sum, the same bits twice
def comb_is_consistent(anc, logw, u, domain_is_log, s1):
    """Every comb point u r + k r taken with r = s1 / P lies on its ancestor's cumulative weight, inside ``ancestors_match_exact``'s
    window ((nb + 20) eps): the resample divided THIS sum by P."""
    P = len(anc)
    c = np.cumsum(true_weights(logw, domain_is_log))
    r = s1 / float(P)
    t = (u * r + np.arange(P, dtype=np.float64) * r).astype(np.longdouble)
    win = (int(math.ceil(P / float(SCAN_BLOCK))) + 20) * np.finfo(np.float64).eps
    assert np.all(c[anc] >= t * (1.0 - win))
    below = anc > 0
    assert np.all(c[anc[below] - 1] <= t[below] * (1.0 + win))
    return True


@pytest.mark.parametrize("dom", [LIN, LOG])
@pytest.mark.parametrize("P", SIZES)
def test_n_eff_against_the_reference(lib, P, dom):
    ar.need_longdouble()
    rs = np.random.RandomState(30 + P)
    f = new_filter(lib, P, P, wide_weights(rs, P), shuffle_sources=False)
    giants(f, rs, P)
    logw = f.download_log_weights()
    s1, s2 = f.weight_sums(dom)
    ar.check_sums(s1, s2, f.n_eff(dom), logw, dom == LOG, what="P = %d, domain %d" % (P, dom))
    assert f.weight_sums(dom) == (s1, s2)            # the same bits on every call
    assert same_bits(f.download_log_weights(), logw)  # ... which changes no state
    u = float(rs.uniform(0.0, 1.0))
    anc = f.resample_adaptive(u, 2.0, domain=dom, return_ancestors=True)
    st = f.resample_stats()
    assert (st.s1, st.s2) == (s1, s2) and st.n_eff == s1 / s2 * s1  # the gate's sums are those, and its one expression
    ancestors_match_exact(anc, logw, u, dom == LOG)
    assert comb_is_consistent(anc, logw, u, dom == LOG, st.s1)
    if dom == LOG:  # a maximum given from outside (what a sharded filter would pass) is the handle's own
        f.upload_poses(start_poses(rs, P, wide_weights(rs, P)))
        lw = f.download_log_weights()
        assert f.weight_sums(LOG, gmax=float(lw.max())) == f.weight_sums(LOG)
    f.close()


# ---- 4. the verdict at the edge, exactly
@pytest.mark.parametrize("dom", [LIN, LOG])
@pytest.mark.parametrize("P,m", [(1024, 300), (4096, 2049)])
def test_the_verdict_at_the_edge(lib, P, m, dom):
    rs = np.random.RandomState(P + m)
    theta = m / float(P)  # exact in binary
    ones = rs.permutation(P)
    for n_ones, keep in ((m, True), (m - 1, False)):
        w = np.zeros(P)
        w[ones[:n_ones]] = 1.0
        f = new_filter(lib, P, P, w)
        anc = f.resample_adaptive(0.5, theta, domain=dom, return_ancestors=True)
        st = f.resample_stats()
        assert (st.n_eff, st.s1, st.s2) == (float(n_ones), float(n_ones), float(n_ones))
        assert st.resampled == (not keep)
        assert np.array_equal(anc, np.arange(P)) == keep
        if not keep:
            assert np.all(w[anc] == 1.0)  # only particles with weight were chosen
        f.close()


# ---- 5. the verdict away from the edge
THETA = 0.5


def ladder_weights(rs, P, share):
    """About share * P particles near weight 1, the others four decades below: n_eff / P near ``share``."""
    m = max(1, int(round(share * P)))
    w = 1e-4 * rs.uniform(0.5, 1.0, P)
    w[rs.permutation(P)[:m]] = rs.uniform(0.9, 1.1, m)
    return w


@pytest.mark.parametrize("dom", [LIN, LOG])
@pytest.mark.parametrize("P", SIZES)
def test_the_verdict_away_from_the_edge(lib, P, dom):
    ar.need_longdouble()
    f = lib.DeviceFilter(P, 0)
    seen = set()
    for share in (0.1, 0.3, 0.5, 0.7, 0.9):
        rs = np.random.RandomState(int(1000 * share) + P)
        f.upload_poses(start_poses(rs, P, ladder_weights(rs, P, share)))
        logw = f.download_log_weights()
        assert ar.margin(logw, dom == LOG, THETA) >= ar.MARGIN, (P, share)  # a condition on the input, not a tolerance
        keep = ar.keeps(logw, dom == LOG, THETA)
        f.resample_adaptive(float(rs.uniform(0.0, 1.0)), THETA, domain=dom)
        st = f.resample_stats()
        assert st.resampled == (not keep), (P, share, st)
        ar.check_sums(st.s1, st.s2, st.n_eff, logw, dom == LOG, what="P = %d, share %.1f" % (P, share))
        seen.add(keep)
    if P >= 63:
        assert seen == {True, False}  # (the ladder crosses the threshold)
    f.close()


# ---- 6. all weights zero: the call resamples, as pk_resample does
@pytest.mark.parametrize("dom", [LIN, LOG])
@pytest.mark.parametrize("P", [65, 1025])
def test_all_weights_zero(lib, P, dom):
    a, b = new_filter(lib, P, P, np.zeros(P)), new_filter(lib, P, P, np.zeros(P))
    anc_a = a.resample(0.3, domain=dom, return_ancestors=True)
    anc_b = b.resample_adaptive(0.3, THETA, domain=dom, return_ancestors=True)
    pa, _, sa = state(a)
    pb, lb, sb = state(b)
    assert np.array_equal(anc_a, anc_b) and same_bits(pa, pb) and np.array_equal(sa, sb)
    assert same_bits(lb, np.zeros(P))
    st = b.resample_stats()
    assert st.resampled and math.isnan(st.n_eff) and st.s1 == 0.0 and st.s2 == 0.0 and st.shift == 0.0
    assert b.n_eff(dom) == P  # (the new generation has unit weights)
    a.close()
    b.close()


# ---- 7. the weighted pose summary
@pytest.mark.parametrize("dom", [LIN, LOG])
@pytest.mark.parametrize("P", SIZES)
def test_weighted_pose_summary_against_the_reference(lib, P, dom):
    ar.need_longdouble()
    rs = np.random.RandomState(70 + P)
    f = new_filter(lib, P, P, wide_weights(rs, P), shuffle_sources=False)
    giants(f, rs, P)
    poses, logw, _ = state(f)
    got = f.summary_weighted(dom)
    ar.check_pose_summary(got, poses, logw, dom == LOG, what="P = %d, domain %d" % (P, dom))
    again = f.summary_weighted(dom)
    assert same_bits(got.mean, again.mean) and same_bits(got.spread, again.spread) and got.n_eff == again.n_eff
    assert same_bits(f.download_log_weights(), logw) and same_bits(f.download_poses()[:, :3], poses)  # no state changed
    f.close()


@pytest.mark.parametrize("P", [63, 1025, 4097])
def test_weighted_pose_summary_special_populations(lib, P):
    ar.need_longdouble()
    rs = np.random.RandomState(80 + P)
    f = lib.DeviceFilter(P, 0)
    # equal weights: pk_summary's estimate
    f.upload_poses(start_poses(rs, P, np.full(P, 0.25)))
    got, (sx, sy, sh) = f.summary_weighted(LOG), f.summary()
    assert abs(got.mean[0] - sx) <= 1e-12 * abs(sx) and abs(got.mean[1] - sy) <= 1e-12 * abs(sy)
    assert pr.angle_diff(got.mean[2], sh) <= 1e-12 and ar.rel(got.n_eff, P) <= 1e-12
    # all poses equal, any weights: the pose bit for bit, exactly no variance
    one = np.array([1e6 + 0.1, -3.3, 0.7])
    f.upload_poses(np.column_stack([np.tile(one, (P, 1)), wide_weights(rs, P)]))
    for dom in (LIN, LOG):
        got = f.summary_weighted(dom)
        assert got.mean[0] == one[0] and got.mean[1] == one[1] and pr.angle_diff(got.mean[2], one[2]) <= 1e-12
        assert np.all(got.spread[:3] == 0.0) and abs(got.spread[3] - 1.0) <= 1e-12
    # 1e6 from the origin with a spread of 1e-3: the covariance keeps eight digits (the conditioning case of test_gpu_mapsum.py)
    far = np.column_stack([1e6 + 1e-3 * rs.standard_normal(P), -2e6 + 1e-3 * rs.standard_normal(P), rs.uniform(-0.3, 0.3, P),
                           rs.uniform(0.1, 1.0, P) ** 3])
    f.upload_poses(far)
    poses, logw, _ = state(f)
    got = f.summary_weighted(LOG)
    _, spread, _ = ar.pose_summary(poses, logw, True)
    assert np.all(np.abs(got.spread[:3] - spread[:3]) <= 1e-8 * np.abs(spread[:3])), (got.spread, spread)
    # weights that sum to nothing
    f.upload_poses(start_poses(rs, P, np.zeros(P)))
    assert "sum to" in raises(lib, STATE, f.summary_weighted, LIN)
    assert "sum to" in raises(lib, STATE, f.summary_weighted, LOG)
    f.close()


# ---- 8. with the ring: one row per call, kept or not
@pytest.mark.parametrize("P", [65, 1025])
def test_with_the_ring(lib, P):
    rs = np.random.RandomState(90 + P)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(rs, P, rs.uniform(0.1, 1.0, P) ** 4))
    f.path_enable(8)
    poses, anc, kept = [], [], []
    for s in range(6):
        f.motion(0.3, 0.1, 0.1, z=rs.standard_normal((P, 3)))
        if s % 2 == 1:
            giants(f, rs, P)
        before = f.download_poses()
        a = f.resample_adaptive(float(rs.uniform(0.0, 1.0)), 0.0 if s % 2 == 0 else 2.0, domain=LOG, return_ancestors=True)
        poses.append(before[:, :3].copy())
        anc.append(a.astype(np.int32))
        kept.append(s % 2 == 0)
        assert f.resample_stats().resampled == (s % 2 == 1)
    assert f.path_shape() == (8, 6, 6)
    rp, ra = f.path_download()
    assert same_bits(rp, np.array(poses)) and np.array_equal(ra, np.array(anc))
    for t in range(6):
        assert np.array_equal(ra[t], np.arange(P)) == kept[t]
    current = f.download_poses()[:, :3]
    assert same_bits(f.path_trace(np.arange(P)), pr.paths(np.array(poses), np.array(anc), current))
    got = f.path_summary()
    _, _, surv = pr.check_summary(got, np.array(poses), np.array(anc), current, what="alternating, P = %d" % P)
    for t in range(6):
        if kept[t]:
            assert got.survivors[t] == got.survivors[t + 1]
    assert np.any(surv < P)
    f.close()


# ---- 9. with growing maps: the bookkeeping follows the ancestors, the identity when the call kept
def grow_equal(a, b):
    (ca, ra, sa), (cb, rb, sb) = a, b
    if not np.array_equal(ca, cb):
        return False
    for i in range(ca.shape[0]):  # (rows beyond what is stored / in use are undefined)
        if not (same_bits(ra[i, :ca[i, 0]], rb[i, :cb[i, 0]]) and np.array_equal(sa[i, :ca[i, 1]], sb[i, :cb[i, 1]])):
            return False
    return True


def test_with_growing_maps(lib):
    from oracle.fastslam_oracle import synthetic_scan, truth_step
    from test_gpu_grow import _device_filter, _scene

    P, L0, U, spare = 64, 10, 3, 5
    world, covs, known, kcov = _scene(L0, U)
    fs = [_device_filter(lib, P, known, kcov, spare, 30.0, 64) for _ in range(3)]
    rs = np.random.RandomState(5)
    pose = (0.0, 0.0, 0.0)
    for s in range(4):  # a few plain steps: readings stored, slots in use, different from particle to particle
        pose = truth_step(pose, 0.8, 0.35, 0.5)
        blobs, z, u = synthetic_scan(world, pose), rs.standard_normal((P, 3)), float(rs.uniform())
        for f in fs:
            f.motion(0.8, 0.35, 0.5, z=z)
            f.observe(blobs, fresh=True)
            if s < 3:
                f.resample(u, domain=LOG)
    keep, plain, gated = fs
    before = keep.grow_download()
    assert before[0][:, 0].min() > 0  # every particle has stored readings (at its own poses: they differ)
    m0 = keep.download_landmarks()
    a = keep.resample_adaptive(0.6, 0.0, domain=LOG, return_ancestors=True)
    assert np.array_equal(a, np.arange(P)) and grow_equal(keep.grow_download(), before)
    for x, y in zip(m0, keep.download_landmarks()):
        assert np.array_equal(x, y)
    a1 = plain.resample(0.6, domain=LOG, return_ancestors=True)
    a2 = gated.resample_adaptive(0.6, 2.0, domain=LOG, return_ancestors=True)
    assert np.array_equal(a1, a2) and np.unique(a1).size < P
    g1, g2 = plain.grow_download(), gated.grow_download()
    assert grow_equal(g1, g2)
    assert np.array_equal(g2[0], before[0][a2])  # gathered by the ancestors
    for x, y in zip(plain.download_landmarks(), gated.download_landmarks()):
        assert np.array_equal(x, y)
    for f in fs:
        f.close()


# ---- 10. whole steps
STEPS = 12


def step_scene(L, B=8, seed=123):
    """A map of L landmarks on a ring and the B of them the robot sees: (means, covs, the seen rows)."""
    from oracle.fastslam_oracle import synthetic_world

    means, covs = synthetic_world(L, seed=seed)
    return means, covs, np.linspace(0, L - 1, B).astype(int)


STEP_V, STEP_W, STEP_DT = 0.8, 0.35, 0.5


def step_blobs(means, seen, n=STEPS):
    from oracle.fastslam_oracle import synthetic_scan, truth_step

    pose, out = (0.0, 0.0, 0.0), []
    for _ in range(n):
        pose = truth_step(pose, STEP_V, STEP_W, STEP_DT)
        out.append(synthetic_scan(means[seen], pose))
    return out


def full_state(f):
    return state(f) + tuple(f.download_landmarks())


def copy_state(src, dst, P, L):
    dst.upload_poses(src.download_poses())
    m, c, k = src.download_landmarks()
    dst.upload_landmarks(0, P, m, c.reshape(P, L, 25), k)


@pytest.mark.parametrize("L", [16, 513])
def test_whole_steps(lib, L):
    ar.need_longdouble()
    P = 256
    means, covs, seen = step_scene(L)
    scans = step_blobs(means, seen)
    us = np.random.RandomState(L).uniform(0.0, 1.0, STEPS)

    def fresh_filter():
        f = lib.DeviceFilter(P, L)
        f.upload_map(means, covs.reshape(L, 25))
        return f

    one, parts, plain = fresh_filter(), fresh_filter(), fresh_filter()
    verdicts, acc, run = [], None, 0
    for s in range(STEPS):
        blobs, u = scans[s], float(us[s])
        if run == 0:  # the particles were just made or resampled: the twin of (c) starts a run on copies of them
            if s:
                copy_state(parts, plain, P, L)
            acc = np.zeros(P)
        # (a) the step in one call == its three parts, bit for bit
        one.step_adaptive(STEP_V, STEP_W, STEP_DT, blobs, u, THETA, seed=7, draw=s, domain=LOG)
        parts.motion(STEP_V, STEP_W, STEP_DT, seed=7, draw=s)
        parts.observe(blobs, fresh=False)
        logw = parts.download_log_weights()
        # (c) over a run of kept steps the carried weights are the product of the per-scan weights of a twin that restarts them
        plain.motion(STEP_V, STEP_W, STEP_DT, seed=7, draw=s)
        plain.observe(blobs, fresh=True)
        acc = acc + plain.download_log_weights()
        assert np.allclose(logw - logw.max(), acc - acc.max(), rtol=1e-12), (s, run)
        # (b) the verdict is the reference's, from the log-weights in front of the call
        assert ar.margin(logw, True, THETA) >= ar.MARGIN, s
        keep = ar.keeps(logw, True, THETA)
        anc = parts.resample_adaptive(u, THETA, domain=LOG, return_ancestors=True)
        st = parts.resample_stats()
        assert st.resampled == (not keep), (s, st)
        ar.check_sums(st.s1, st.s2, st.n_eff, logw, True, what="L = %d, step %d" % (L, s))
        assert np.array_equal(anc, np.arange(P)) == keep
        st1 = one.resample_stats()
        assert (st1.n_eff, st1.s1, st1.s2, st1.shift, st1.resampled, st1.calls, st1.resamples) == \
               (st.n_eff, st.s1, st.s2, st.shift, st.resampled, st.calls, st.resamples)
        a, b = (full_state(one), full_state(parts)) if (L == 16 or s == STEPS - 1) else (state(one), state(parts))
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]), s
        for x, y in zip(a[3:], b[3:]):
            assert np.array_equal(x, y), s
        verdicts.append(keep)
        run = run + 1 if keep else 0
    # (d) both verdicts occurred, and some run of kept steps was longer than one
    assert True in verdicts and False in verdicts, verdicts
    assert any(verdicts[i] and verdicts[i + 1] for i in range(STEPS - 1)), verdicts
    assert parts.resample_stats().calls == STEPS and parts.resample_stats().resamples == verdicts.count(False)
    for f in (one, parts, plain):
        f.close()


# ---- 11. the facade
def facade_filter(pk, g, **kw):
    L = int(g["L"])
    fs = pk.FastSLAM([pk.Feature(mean=g["means0"][l], covar=g["covs0"][l]) for l in range(L)], num_particles=64, **kw)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = 0.2, 0.1
    fs.last_control = tw
    return fs


def run_facade(pk, fs, g, steps, first=0):
    nb = len(g["blobs"])
    out = []
    for s in range(first, first + steps):
        pk.msgs.Time.set_now(0.1 * (s + 1))
        fs.cam_cb(View(pk, g["blobs"][s % nb]))
        out.append(fs._filter.download_poses())
    return out


def test_facade(tmp_path):
    import parakeet_slam_amd as pk
    from parakeet_slam_amd import adaptive, msgs

    pk.msgs = msgs
    g = load_golden("step_small")
    with pytest.raises(ValueError, match="one GPU"):  # (before any process starts)
        pk.FastSLAM([], num_particles=512, devices=[0, 1], resample_threshold=0.5)
    with pytest.raises(ValueError, match="one GPU"):
        pk.ShardedFastSLAM([], num_particles=512, devices=[0, 1], resample_threshold=0.5)
    for bad in (-0.5, float("nan"), float("inf"), "often"):
        with pytest.raises(ValueError, match="resample_threshold"):
            pk.FastSLAM([], num_particles=8, resample_threshold=bad)

    def seeded(**kw):
        np.random.seed(3)
        random.seed(3)
        msgs.Time.set_now(0.0)
        return facade_filter(pk, g, weight_domain="log", **kw)

    # None is today's filter, bit for bit
    a, b = seeded(), seeded(resample_threshold=None)
    ra = run_facade(pk, a, g, 4)
    np.random.seed(3)
    random.seed(3)
    b.last_update = msgs.Time(0.0)
    rb = run_facade(pk, b, g, 4)
    for x, y in zip(ra, rb):
        assert same_bits(x, y)
    assert a.summary() == b.summary() == a._filter.summary()
    for asked in (a.resample_stats, a.pose_summary):
        with pytest.raises(ValueError, match="resample_threshold"):
            asked()
    a.close()
    b.close()

    fs = seeded(resample_threshold=0.5)
    steps = 8
    resampled = []
    for s in range(steps):
        run_facade(pk, fs, g, 1, first=s)
        st = fs.resample_stats()
        assert isinstance(st, adaptive.ResampleStats) and st.calls == s + 1
        assert st.resampled == (not st.n_eff >= 0.5 * 64)  # the verdict is the gate's comparison on the figures it reports
        resampled.append(st.resampled)
    # (this scene is nearly noise-free: on the host oracle n_eff / P stays above 0.99 over these steps, so the filter keeps)
    assert st.resamples == sum(resampled) == 0, resampled
    always = seeded(resample_threshold=2.0)  # ... and the other verdict: a threshold above 1 resamples at every step
    run_facade(pk, always, g, 3)
    st = always.resample_stats()
    assert st.resampled and (st.calls, st.resamples) == (3, 3)
    assert same_bits(always._filter.download_log_weights(), np.zeros(64))
    sw, su = always.summary(), always._filter.summary()  # unit weights: the plain mean
    assert all(abs(x - y) <= 1e-12 * abs(y) for x, y in zip(sw, su))
    always.close()
    got = fs.pose_summary()
    assert isinstance(got, adaptive.PoseSummary)
    assert fs.summary() == got.pose() == fs._filter.summary_weighted(LOG).pose()
    poses, logw = fs._filter.download_poses()[:, :3], fs._filter.download_log_weights()
    ar.check_pose_summary(got, poses, logw, True, what="facade")
    assert fs.map_summary().n_eff == fs.map_summary("weights").n_eff
    assert ar.rel(fs.map_summary().n_eff, got.n_eff) <= 1e-12

    # a snapshot between two resamples (the last step kept): save, reload into a fresh filter, go on to the same bits
    s = steps
    assert not fs.resample_stats().resampled
    assert len(np.unique(fs._filter.download_log_weights())) > 1  # the weights are mid-way: not all equal
    snap = str(tmp_path / "snap.npz")
    fs.save_state(snap)
    assert "log_weights" in np.load(snap).files
    other = seeded(resample_threshold=0.5)
    other.load_state(snap)
    assert same_bits(other._filter.download_log_weights(), fs._filter.download_log_weights())
    outs = []
    for f in (fs, other):
        np.random.seed(9)
        random.seed(9)
        f.last_update = msgs.Time(0.1 * s)
        outs.append(run_facade(pk, f, g, 3, first=s))
        outs[-1].append(f._filter.download_log_weights())
    for x, y in zip(*outs):
        assert same_bits(x, y)
    # the identity on a kept step: last_ancestors when they are asked for
    grow = seeded(resample_threshold=0.0, new_landmarks=True, spare_landmarks=2, record_ids=True)
    run_facade(pk, grow, g, 2)
    assert np.array_equal(grow.last_ancestors, np.arange(64)) and not grow.resample_stats().resampled
    for f in (fs, other, grow):
        f.close()


# ---- 12. refusals, and a filter that uses none of this
def test_refusals(lib):
    from oracle.fastslam_oracle import synthetic_world
    from test_gpu_colour_table import scan_of
    from test_gpu_pub import poses_around

    P = 64
    f, untouched = lib.DeviceFilter(P, 0), lib.DeviceFilter(P, 0)
    assert "pk_resample_adaptive" in raises(lib, STATE, f.resample_stats)
    for theta in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert "threshold" in raises(lib, INVALID, f.resample_adaptive, 0.5, theta)
        assert "threshold" in raises(lib, INVALID, f.step_adaptive, 0.2, 0.1, 0.1, np.zeros((0, 4)), 0.5, theta)
    before = f.download_poses()
    for u in (1.0, -0.25, float("nan")):
        assert "outside [0,1)" in raises(lib, INVALID, f.resample_adaptive, u, 0.5)
    assert "weight_domain" in raises(lib, INVALID, f.resample_adaptive, 0.5, 0.5, 2)
    assert "outside [0,1)" in raises(lib, INVALID, f.resample_adaptive, 1.0, 0.5, 2)  # precedence as pk_resample: u first
    assert "weight_domain" in raises(lib, INVALID, f.weight_sums, 2)
    assert "weight_domain" in raises(lib, INVALID, f.summary_weighted, -1)
    raises(lib, STATE, f.resample_stats)  # (nothing of that was a gated call)
    assert np.array_equal(f.download_poses(), before)
    # a filter that used none of this holds the bytes of one created alongside it; the first call allocates, later ones do not
    b0 = untouched.device_bytes()
    assert f.device_bytes() == b0
    f.resample(0.5)
    f.summary()
    assert f.device_bytes() == b0
    f.resample_adaptive(0.5, 0.5)
    b1 = f.device_bytes()
    assert b0 < b1 <= b0 + 64 * 1024
    f.resample_adaptive(0.25, 0.5)
    f.weight_sums(LOG)
    f.summary_weighted(LOG)
    assert f.device_bytes() == b1
    # the balanced placement: pk_resample's status and wording
    f.upload_logical(np.arange(P, dtype=np.int64))
    said_plain = raises(lib, STATE, f.resample, 0.5)
    said = raises(lib, STATE, f.resample_adaptive, 0.5, 0.5)
    assert said.replace("pk_resample_adaptive", "pk_resample") == said_plain
    f.close()
    untouched.close()
    # a split observe in progress
    L = 1030
    means, covs = synthetic_world(L)
    g = lib.DeviceFilter(P, L)
    g.upload_map(means, covs.reshape(L, 25))
    g.upload_poses(poses_around(np.random.RandomState(1), P))
    g.stage_scan(scan_of(means, (0.0, 0.0, 0.0), np.linspace(0, L - 1, 40).astype(int)))
    g.observe_staged_range(False, 0, 24, True, False)
    said_plain = raises(lib, STATE, g.resample, 0.5)
    said = raises(lib, STATE, g.resample_adaptive, 0.5, 0.5)
    assert "split observe" in said and said.replace("pk_resample_adaptive", "pk_resample") == said_plain
    g.observe_staged_range(False, 24, P, False, True)
    g.resample_adaptive(0.5, 0.5, domain=LOG)
    assert g.resample_stats().calls == 1
    g.close()

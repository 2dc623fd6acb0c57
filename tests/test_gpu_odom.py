"""GPU: the odometry motion model (k_motion_odom, pk_motion_odom / pk_motion_odom_range / pk_step_odom, FastSLAM(motion="odometry"))
against tests/odom_reference.py in numpy.longdouble, against k_motion's own Philox layout (test_gpu_parity.device_normals), and
against the same filter driven call by call.

The pose bound, rtol 1e-12 / atol 1e-13, is the one test_gpu_parity.py holds the twist model to: sincos and atan2 are the only inexact
steps in both.  Headings are compared by their wrapped difference, so +pi and -pi are one value."""
import math
import random

import numpy as np
import pytest

import odom_reference as ref
from conftest import load_golden
from oracle.fastslam_oracle import synthetic_scan, synthetic_world, truth_step
from test_gpu_parity import device_normals

pytestmark = pytest.mark.gpu

ALPHAS = (0.3, 0.02, 0.1, 0.05)
# (rot1, trans, rot2): forward, backward, a turn in place, a zero delta, a large arc
DELTAS = ((0.0, 0.8, 0.0), (math.pi, 0.5, -math.pi), (0.0, 0.0, 1.2), (0.0, 0.0, 0.0), (0.9, 1.5, 1.1))
# noise for the whole steps: wide enough that blobs go unmatched for some particles and not for others, so that the weights
# degenerate within four scans -- a resample that copies particles, and a gate at 0.5 that gives both verdicts
STEP_ALPHAS = (4.0, 0.3, 1.0, 0.3)
ONE_PASS = ("ml_regs", "ml_fused", "ml_pub_big")


def spread_poses(P, seed=1):
    """Poses over +-50 with headings within 0.05 rad of +-pi (and the two ends themselves), weight 1."""
    rs = np.random.RandomState(seed)
    h = np.where(rs.uniform(size=P) < 0.5, 1.0, -1.0) * (math.pi - rs.uniform(0.0, 0.05, P))
    h[0] = math.pi
    if P > 1:
        h[1] = -math.pi
    return np.stack([rs.uniform(-50, 50, P), rs.uniform(-50, 50, P), h, np.ones(P)], 1)


def assert_poses(got, want_xyh, what):
    ok, worst = ref.poses_close(got, *want_xyh)
    print("%s: worst excess over the bound (<= 0 passes) x %.3g y %.3g heading %.3g" % ((what,) + worst))
    assert ok, (what, worst)


@pytest.mark.parametrize("P", [4097, 1])
def test_supplied_normals_match_the_longdouble_reference(lib, P):
    f = lib.DeviceFilter(P, 1)
    f.upload_poses(spread_poses(P))
    rs = np.random.RandomState(3)
    for k, d in enumerate(DELTAS):
        before = f.download_poses()
        z = rs.standard_normal((P, 3))
        f.motion_odom(d, ALPHAS, z=z)
        assert_poses(f.download_poses(), ref.sample_ld(before[:, 0], before[:, 1], before[:, 2], d, ALPHAS, z), "delta %d, P %d" % (k, P))
        assert np.array_equal(f.download_poses()[:, 3], before[:, 3])  # the weights are not the motion's
    f.close()


def test_device_noise_is_k_motions_philox_layout_whatever_the_shards_and_ranges(lib):
    P, seed, draw = 4097, 0x1234ABCD5678, 17
    start, d = spread_poses(P, 2), DELTAS[4]
    f = lib.DeviceFilter(P, 1)
    f.upload_poses(start)
    f.motion_odom(d, ALPHAS, seed=seed, draw=draw)
    got = f.download_poses()
    assert_poses(got, ref.sample_ld(start[:, 0], start[:, 1], start[:, 2], d, ALPHAS, device_normals(P, seed, draw)), "device noise")
    # the counters are the particle's index in the WHOLE filter: two shards reproduce the one filter bit for bit
    parts = []
    for off, n in ((0, 2048), (2048, 2049)):
        s = lib.DeviceFilter(n, 1)
        s.set_shard(off)
        s.upload_poses(start[off:off + n])
        s.motion_odom(d, ALPHAS, seed=seed, draw=draw)
        parts.append(s.download_poses())
        s.close()
    assert np.array_equal(np.vstack(parts), got)
    # ... and so do the pieces of a range launch
    f.upload_poses(start)
    for p0, p1 in ((0, 100), (100, 3000), (3000, 4097)):
        f.motion_odom_range(d, ALPHAS, seed, draw, p0, p1)
    f.motion_odom_range(d, ALPHAS, seed, draw, 50, 50)  # an empty range: nothing
    assert np.array_equal(f.download_poses(), got)
    # draw and seed each change every particle
    for s2, d2 in ((seed, draw + 1), (seed + 1, draw), (seed, draw | (1 << 40))):
        f.upload_poses(start)
        f.motion_odom(d, ALPHAS, seed=s2, draw=d2)
        other = f.download_poses()
        assert np.all(np.any(other[:, :3] != got[:, :3], axis=1)), (s2, d2)
    f.close()


def test_zero_alphas_move_every_particle_by_exactly_the_rigid_delta(lib):
    P = 4097
    prev, now = (12.5, -7.25, 3.0), (11.9, -6.6, -2.9)
    start = spread_poses(P, 4)
    start[0, :3] = prev
    d = lib.odom_delta(prev, now, 0.01)
    f = lib.DeviceFilter(P, 1)
    f.upload_poses(start)
    f.motion_odom(d, np.zeros(4), seed=5, draw=1)  # (device noise: multiplied by sigmas of exactly zero)
    got = f.download_poses()
    assert_poses(got, ref.sample_ld(start[:, 0], start[:, 1], start[:, 2], d, np.zeros(4), np.zeros((P, 3))), "alpha = 0")
    assert abs(got[0, 0] - now[0]) <= 1e-12 and abs(got[0, 1] - now[1]) <= 1e-12 and ref.angle_diff(got[0, 2], now[2]) <= 1e-12
    f.motion_odom(d, np.zeros(4), z=np.random.RandomState(1).standard_normal((P, 3)))  # supplied normals: the same rigid move
    again = lib.DeviceFilter(P, 1)
    again.upload_poses(got)
    again.motion_odom(d, np.zeros(4), seed=99, draw=7)
    assert np.array_equal(f.download_poses(), again.download_poses())
    f.close()
    again.close()


def scene(L, steps, B=6):
    """A drive past L landmarks on a ring: per step the odometry delta of the true motion and a scan of B blobs."""
    means, covs = synthetic_world(L)
    pick = np.linspace(0, L - 1, B).astype(int)
    pose, out = (0.0, 0.0, 0.0), []
    for s in range(steps):
        nxt = truth_step(pose, 0.9, 0.4 if s % 2 == 0 else -0.7, 0.5)
        out.append((ref.delta(pose, nxt), synthetic_scan(means, nxt)[pick]))
        pose = nxt
    return means, covs, out


def whole_state(f):
    """Poses, log-weights, map sources (the ancestors, behind a resample), then the maps (which reads them through the sources)."""
    poses, logw, src = f.download_poses(), f.download_log_weights(), f.download_sources()
    return (poses[:, :3], logw, src) + tuple(f.download_landmarks())


def assert_same_state(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, k)


@pytest.mark.parametrize("L", [8, 160])
@pytest.mark.parametrize("threshold", [None, 0.5])
def test_step_odom_is_motion_odom_observe_and_the_resample(lib, L, threshold):
    """threshold None: pk_step's reset and resample; 0.5: pk_step_adaptive's carried weights and gate, with equal resample_stats."""
    P, steps = 2049, 4
    means, covs, run = scene(L, steps)
    a, b = lib.DeviceFilter(P, L), lib.DeviceFilter(P, L)
    for f in (a, b):
        f.upload_map(means, covs.reshape(L, 25))
    kept = resampled = copied = 0
    for s, (d, blobs) in enumerate(run):
        u = 0.17 + 0.21 * s
        a.step_odom(d, STEP_ALPHAS, blobs, u, threshold=threshold, seed=11, draw=s, domain=lib.PK_WEIGHTS_LOG)
        b.motion_odom(d, STEP_ALPHAS, seed=11, draw=s)
        if threshold is None:
            b.observe(blobs, fresh=True)
            anc = b.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
        else:
            b.observe(blobs)
            anc = b.resample_adaptive(u, threshold, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
            sa, sb = a.resample_stats(), b.resample_stats()
            assert vars(sa) == vars(sb), (s, vars(sa), vars(sb))
            resampled += int(sb.resampled)
            kept += int(not sb.resampled)
        assert a.observe_route() == b.observe_route()
        if L == 160:
            assert a.observe_route() in ONE_PASS, a.observe_route()
        assert np.array_equal(a.download_sources(), anc), s
        copied += int(not np.array_equal(anc, np.arange(P)))
        assert_same_state(whole_state(a), whole_state(b), "step %d" % s)
    if threshold is not None:
        print("L %d: %d steps resampled, %d kept" % (L, resampled, kept))
        assert resampled >= 1 and kept >= 1 and copied == resampled, "the scene must show both verdicts of the gate"
    else:
        assert copied == steps, "every resample of the scene must copy some particle"
    assert len(np.unique(a.download_poses()[:, 0])) > 1
    a.close()
    b.close()


def test_the_pose_sums_of_motion_odom_are_the_candidates_own(lib):
    """k_motion_odom leaves the per-block pose sums k_candidates reads.  The same state rebuilt through upload_poses has none, so
    the candidates' own launches form them: the observe must come out the same, flagged particles included."""
    P, L = 2049, 160
    means, covs, run = scene(L, 1)
    d, blobs = run[0]
    a, b = lib.DeviceFilter(P, L), lib.DeviceFilter(P, L)
    for f in (a, b):
        f.upload_map(means, covs.reshape(L, 25))
    a.motion_odom(d, ALPHAS, seed=3, draw=0)
    moved = a.download_poses()
    b.upload_poses(moved)
    a.observe(blobs, fresh=True)
    b.observe(blobs, fresh=True)
    assert a.observe_route() == b.observe_route() and a.observe_route() in ONE_PASS
    assert a.observe_flagged() == b.observe_flagged()
    assert_same_state(whole_state(a), whole_state(b), "pose sums")
    assert np.ptp(a.download_log_weights()) > 0
    a.close()
    b.close()


class View(object):
    def __init__(self, pk, blobs):
        class Scan(object):
            pass

        self.last_sensor_reading = Scan()
        obs = []
        for bl in blobs:
            o = pk.msgs.Blob()
            o.bearing = float(bl[0])
            o.color.r, o.color.g, o.color.b = float(bl[1]), float(bl[2]), float(bl[3])
            obs.append(o)
        self.last_sensor_reading.observes = obs


def odometry_messages(n, v=0.9, dt=0.25, with_truth=False):
    """n odometry poses of a drive that stands still once and turns in place once.  The odometry frame is not the map's (it starts
    near the seam of the heading); with_truth: also the same drive in the map's frame, where the particles start."""
    from parakeet_slam_amd.core import _make_state

    pose, truth, out, truths = (0.3, -0.2, math.pi - 0.1), (0.0, 0.0, 0.0), [], []
    for k in range(n):
        out.append(_make_state(*pose))
        truths.append(truth)
        if k == 3:
            continue  # the robot stands still: the next message repeats the pose
        pose, truth = truth_step(pose, 0.0 if k == 5 else v, 0.8, dt), truth_step(truth, 0.0 if k == 5 else v, 0.8, dt)
    return (out, truths) if with_truth else out


def golden_features(pk, g):
    feats = []
    for l in range(int(g["L"])):
        ft = pk.Feature(mean=g["means0"][l], covar=g["covs0"][l])
        ft.__immutable__ = bool(g["immutable"][l])
        feats.append(ft)
    return feats


def test_facade_in_odometry_mode_is_the_hand_driven_filter(lib, tmp_path):
    import parakeet_slam_amd as pk
    from parakeet_slam_amd.core import _state_pose

    g = load_golden("step_small")
    L, P, seed = int(g["L"]), 512, 9
    feats, msgs8 = golden_features(pk, g), odometry_messages(8)
    random.seed(4)
    pk.msgs.Time.set_now(0.0)
    fs = pk.FastSLAM(feats, num_particles=P, rng="device", seed=seed, motion="odometry", odom_alphas=ALPHAS, weight_domain="log")
    hand = lib.DeviceFilter(P, L)
    hand.upload_map(g["means0"], g["covs0"].reshape(L, 25), np.asarray(g["immutable"], dtype=np.uint8))
    us = random.Random(4)
    prev, draw, twin = None, 0, None
    path = str(tmp_path / "odom.npz")
    tw = pk.msgs.Twist()
    tw.linear.x = 5.0
    for k, m in enumerate(msgs8):
        before = fs._filter.download_poses()
        fs.odom_motion_update(m)
        if k == 0 or k == 4:  # the first message only stores the pose; a robot that stood still launches nothing
            assert np.array_equal(fs._filter.download_poses(), before) and fs._draw == draw
        now = _state_pose(m)
        if prev is not None:
            d = lib.odom_delta(prev, now, 0.01)
            if np.any(d != 0.0):
                hand.motion_odom(d, ALPHAS, seed=seed, draw=draw)
                draw += 1
        prev = now
        assert fs._draw == draw
        if k % 2 == 1:
            pk.msgs.Time.set_now(0.25 * (k + 1))
            fs.motion_update(tw)  # odometry mode: records the control, moves nothing
            assert fs.last_control is tw and np.array_equal(fs._filter.download_poses()[:, :3], hand.download_poses()[:, :3])
            blobs = g["blobs"][k // 2]
            fs.cam_cb(View(pk, blobs))
            hand.set_measurement_noise(fs.Qt)
            hand.observe(blobs, fresh=True)
            hand.resample(us.random(), domain=lib.PK_WEIGHTS_LOG)
            assert_same_state(whole_state(fs._filter), whole_state(hand), "message %d" % k)
        if k == 3:  # a snapshot in mid-run goes into a second facade, which must continue identically
            fs.save_state(path)
            assert "odom_prev" in np.load(path).files
            twin = pk.FastSLAM(feats, num_particles=P, rng="device", seed=seed, motion="odometry", odom_alphas=ALPHAS, weight_domain="log")
            twin.load_state(path)
            assert twin._odom_prev == fs._odom_prev and twin._draw == fs._draw
    assert draw == 6 and len(np.unique(hand.download_poses()[:, 0])) > 1
    final = whole_state(fs._filter)
    random.seed(4)
    for _ in range(2):
        random.random()  # the two draws the first facade made before the snapshot
    for k in range(4, 8):
        twin.odom_motion_update(msgs8[k])
        if k % 2 == 1:
            twin.motion_update(tw)
            twin.cam_cb(View(pk, g["blobs"][k // 2]))
    # (reading fs's maps above made its sources the identity; the twin's still name the last ancestors: everything but them)
    got = whole_state(twin._filter)
    assert_same_state(got[:2] + got[3:], final[:2] + final[3:], "the snapshot's continuation")
    # a snapshot without the stored pose makes the next message the first
    d = dict(np.load(path))
    d.pop("odom_prev")
    np.savez_compressed(path, **d)
    twin.load_state(path)
    assert twin._odom_prev is None
    before = twin._filter.download_poses()
    twin.odom_motion_update(msgs8[6])
    assert np.array_equal(twin._filter.download_poses(), before) and twin._odom_prev == _state_pose(msgs8[6])
    # a message that is not finite: ValueError, nothing stored, nothing moved; the next good message carries on from the last good one
    stored, before = twin._odom_prev, twin._filter.download_poses()
    bad = odometry_messages(1)[0]
    bad.pose.pose.position.y = float("inf")
    with pytest.raises(ValueError):
        twin.odom_motion_update(bad)
    assert twin._odom_prev == stored and np.array_equal(twin._filter.download_poses(), before)
    twin.odom_motion_update(msgs8[7])
    assert twin._odom_prev == _state_pose(msgs8[7]) and not np.array_equal(twin._filter.download_poses()[:, :2], before[:, :2])
    for f in (fs, twin):
        f.close()
    hand.close()
    # the default mode: odom_motion_update stays the reference's no-op, and its snapshots keep their key set
    fs = pk.FastSLAM(feats, num_particles=64, rng="device", seed=seed)
    before = fs._filter.download_poses()
    for m in msgs8[:3]:
        fs.odom_motion_update(m)
    assert np.array_equal(fs._filter.download_poses(), before) and fs._draw == 0 and fs._odom_prev is None
    fs.save_state(path)
    assert "odom_prev" not in np.load(path).files
    fs.close()
    for bad in (dict(motion="odom"), dict(motion=None), dict(odom_alphas=(0.1, 0.1, 0.1)), dict(odom_alphas=(0.1, -0.1, 0.1, 0.1)),
                dict(odom_alphas=(0.1, float("nan"), 0.1, 0.1)), dict(odom_alphas=0.1), dict(odom_min_trans=-0.01),
                dict(odom_min_trans=float("inf")), dict(odom_min_trans=None)):
        with pytest.raises(ValueError):
            pk.FastSLAM(feats, num_particles=64, motion=bad.get("motion", "odometry"), **{k: v for k, v in bad.items() if k != "motion"})


def test_two_ranks_on_one_gpu_in_odometry_mode_match_the_single_gpu_facade():
    """FastSLAM(devices=[0, 0], motion="odometry"): one child per entry, gloo between them, the Philox counters of one filter.
    Compared with the one-GPU facade in logical order, as
    test_fastslam_devices_keyword_two_ranks_on_one_gpu_match_the_single_gpu_facade compares."""
    import parakeet_slam_amd as pk

    L, P, steps = 8, 2 * 1280, 4
    means, covs = synthetic_world(L)
    feats = [pk.Feature(mean=means[l].copy(), covar=covs[l].copy()) for l in range(L)]
    msgs, truths = odometry_messages(steps + 1, v=0.8, dt=0.5, with_truth=True)

    out = []
    for devices in ([0, 0], None):
        random.seed(5)
        pk.msgs.Time.set_now(0.0)
        kw = dict(num_particles=P, weight_domain="log", rng="device", seed=3, motion="odometry", odom_alphas=ALPHAS)
        if devices:
            fs = pk.FastSLAM(feats, devices=devices, backend="gloo", **kw)
            assert isinstance(fs, pk.ShardedFastSLAM)
        else:
            fs = pk.FastSLAM(feats, device=0, **kw)
        fs.odom_motion_update(msgs[0])
        sums = []
        for s in range(steps):
            pk.msgs.Time.set_now(0.5 * (s + 1))
            fs.odom_motion_update(msgs[s + 1])
            fs.cam_cb(View(pk, synthetic_scan(means, truths[s + 1])))
            sums.append(fs.summary())
        poses = fs.download_poses() if devices else fs._filter.download_poses()
        p0 = fs.particles[P - 1]
        out.append((np.array(sums), np.asarray(p0.feature_set[3].mean, dtype=np.float64).copy(), p0.state.pose.pose.position.x, poses, fs._draw))
        fs.close()
    assert np.allclose(out[0][0], out[1][0], rtol=1e-12, atol=1e-13)
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert np.array_equal(out[0][3][:, :3], out[1][3][:, :3])
    assert out[0][4] == out[1][4] == 3  # (message 4 repeats message 3: the robot stood still)


def test_the_filter_calls_refuse_what_the_header_says(lib):
    import ctypes as C

    so = lib.load()
    P, L = 300, 4
    means, covs = synthetic_world(L)
    f = lib.DeviceFilter(P, L)
    f.upload_map(means, covs.reshape(L, 25))
    f.upload_poses(spread_poses(P))
    before = whole_state(f)
    blobs = synthetic_scan(means, (0.0, 0.0, 0.0))
    nan, inf = float("nan"), float("inf")
    good = (0.1, 0.5, -0.2)
    bad_deltas = [(nan, 0.5, 0.0), (0.1, inf, 0.0), (0.1, 0.5, -inf), (0.1, -1e-9, 0.0)]
    bad_alphas = [(0.1, 0.1, 0.1, nan), (inf, 0.1, 0.1, 0.1), (0.1, -1e-12, 0.1, 0.1)]

    def refused(call):
        with pytest.raises(lib.PkError) as e:
            call()
        assert e.value.status == lib.PK_ERR_INVALID

    for d in bad_deltas:
        refused(lambda: f.motion_odom(d, ALPHAS))
        refused(lambda: f.motion_odom_range(d, ALPHAS, 0, 0, 0, P))
        refused(lambda: f.step_odom(d, ALPHAS, blobs, 0.5))
    for a in bad_alphas:
        refused(lambda: f.motion_odom(good, a))
        refused(lambda: f.motion_odom_range(good, a, 0, 0, 0, P))
        refused(lambda: f.step_odom(good, a, blobs, 0.5))
    for p0, p1 in ((-1, 10), (10, 5), (0, P + 1)):
        refused(lambda: f.motion_odom_range(good, ALPHAS, 0, 0, p0, p1))
    for thr in (-0.5, inf):
        refused(lambda: f.step_odom(good, ALPHAS, blobs, 0.5, threshold=thr))
    dp = C.POINTER(C.c_double)
    g3, a4 = (C.c_double * 3)(*good), (C.c_double * 4)(*ALPHAS)
    null = C.cast(None, dp)
    assert so.pk_motion_odom(f._h, null, a4, null, 0, 0) == lib.PK_ERR_INVALID
    assert so.pk_motion_odom(f._h, g3, null, null, 0, 0) == lib.PK_ERR_INVALID
    assert so.pk_motion_odom_range(f._h, null, a4, 0, 0, 0, P) == lib.PK_ERR_INVALID
    assert so.pk_step_odom(f._h, g3, null, null, 0, 0, blobs.ctypes.data_as(dp), len(blobs), None, 0.5, 0, nan) == lib.PK_ERR_INVALID
    assert_same_state(whole_state(f), before, "nothing changed")
    f.close()

"""CPU, worlds of 2 and 3 over gloo, balanced placement, 12 particles per rank: the odometry motion model through the sharded
filter (ShardedFilter.motion_odom, step(motion=...)) and through the multi-GPU front end (FastSLAM(devices=[...],
motion="odometry")).  The exchange, the command pipes and the front end are the product's; the per-particle arithmetic is the
test-only OracleShard with the reference's sample (tests/odom_reference.py).  Six steps of odometry messages and scans must leave
what ONE NumPy filter holding every particle leaves, with the supplied normals in logical order, array for array."""
import random

import numpy as np
import pytest
import torch.multiprocessing as mp

import odom_reference as ref
from oracle.fastslam_oracle import OracleFilter, low_variance_ancestors, synthetic_scan, synthetic_world, truth_step
from sharded_common import OracleShard, init_gloo, store_file

ALPHAS = (0.3, 0.02, 0.1, 0.05)
P_LOCAL, L, STEPS = 12, 6, 6


class OdomOracleShard(OracleShard):
    """OracleShard with the odometry motion model: the reference's sample on this rank's particles."""

    def motion_odom(self, delta, alphas, z=None, seed=0, draw=0):
        assert z is not None, "the oracle shard has no Philox: the test supplies the normals"
        o = self.o
        o.x, o.y, o.h = ref.sample(o.x, o.y, o.h, np.asarray(delta, dtype=np.float64), alphas, z)


def make_odom_oracle_shard(P, means, covs, immutable=None):
    """Shard factory for ShardedFastSLAM's CPU rehearsal (module-level: picklable for the spawned ranks)."""
    return OdomOracleShard(P, means, covs, immutable)


def drive(steps):
    """Odometry poses of a drive that turns in place once and reverses once, and one scan per pose.  The odometry frame is not the
    map's (it starts near the heading's seam, as odometry starts wherever it was switched on); the scans are taken from the same
    drive in the map's frame, where the particles start."""
    means, covs = synthetic_world(L)
    pose, truth, poses, scans = (0.4, -0.3, 3.0), (0.0, 0.0, 0.0), [], []
    for s in range(steps + 1):
        poses.append(pose)
        scans.append(synthetic_scan(means, truth))
        v = {2: 0.0, 4: -0.6}.get(s, 0.8)
        pose, truth = truth_step(pose, v, 0.9, 0.5), truth_step(truth, v, 0.9, 0.5)
    return means, covs, poses, scans


def one_filter(P, world_seed):
    """The single NumPy filter: what every sharded run below must leave, per step."""
    means, covs, poses, scans = drive(STEPS)
    rs = np.random.RandomState(world_seed)
    z, us = rs.standard_normal((STEPS, P, 3)), rs.uniform(0, 1, STEPS)
    o = OracleFilter(P, means, covs)
    out = []
    for s in range(STEPS):
        d = ref.delta(poses[s], poses[s + 1])
        o.reset_weights()
        o.x, o.y, o.h = ref.sample(o.x, o.y, o.h, d, ALPHAS, z[s])
        o.observe(scans[s + 1])
        sh = OracleShard(P, means, covs)  # the canonical blocked scan, as tests/test_sharded_gloo.py takes its ancestors
        sh.o = o
        hi = sh.shard_offspring(sh.shard_block_totals(float(o.logw.max()), 1), 0, P, float(us[s]), True)
        anc = np.minimum(np.searchsorted(np.maximum.accumulate(hi[1:]), np.arange(P), side="right"), P - 1)
        o.gather(anc)
        out.append((o.x.copy(), o.y.copy(), o.h.copy(), o.logw.copy(), o.mean.copy(), o.cov.copy(), o.count.copy()))
    return out, z, us


def worker(rank, world, store, q):
    try:
        init_gloo(rank, world, store)
        from parakeet_slam_amd.sharded import ShardedFilter, TorchComm

        means, covs, poses, scans = drive(STEPS)
        P = P_LOCAL * world
        _ref, z, us = one_filter(P, 11)
        sf = ShardedFilter(P_LOCAL, L, comm=TorchComm(), shard=OdomOracleShard(P_LOCAL, means, covs), placement="balanced")
        res = []
        for s in range(STEPS):
            d = ref.delta(poses[s], poses[s + 1])
            if s % 3 == 0:  # call by call
                sf.reset_weights()
                sf.motion_odom(d, ALPHAS, z=z[s])  # the whole filter's normals in logical order: the rank takes its rows
                sf.observe(scans[s + 1])
                sf.resample(float(us[s]), domain=1)
            elif s % 3 == 1:  # the step with an odometry delta for its motion (v, w, dt are not read)
                sf.step(9.0, 9.0, 9.0, scans[s + 1], float(us[s]), z=z[s], domain=1, motion=("odom", d, ALPHAS))
            else:  # moved already: a step without motion
                sf.motion_odom(d, ALPHAS, z=z[s])
                sf.step(9.0, 9.0, 9.0, scans[s + 1], float(us[s]), domain=1, motion="none")
            lg = sf.logical_index()  # (completes the pending exchange)
            o = sf.f.o
            res.append((o.x.copy(), o.y.copy(), o.h.copy(), o.logw.copy(), o.mean.copy(), o.cov.copy(), o.count.copy(), lg))
        try:
            sf.step(0.0, 0.0, 0.0, scans[0], 0.5, motion="odom")
            bad = "a bad motion description was accepted"
        except ValueError:
            bad = None
        q.put((rank, res if bad is None else "ERR " + bad))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "ERR " + traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_filter_with_odometry_motion_is_the_single_filter(world):
    ctx = mp.get_context("spawn")
    q, store = ctx.Queue(), store_file()
    procs = [ctx.Process(target=worker, args=(r, world, store, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        r, res = q.get(timeout=300)
        assert not isinstance(res, str), res
        got[r] = res
    for p in procs:
        p.join(timeout=60)
    P = world * P_LOCAL
    want, _z, _us = one_filter(P, 11)
    moved = False
    for s in range(STEPS):
        logical = np.concatenate([got[r][s][7] for r in range(world)])
        assert np.array_equal(np.sort(logical), np.arange(P))
        moved = moved or not np.array_equal(logical, np.arange(P))
        for fld in range(7):
            cat = np.concatenate([got[r][s][fld] for r in range(world)])
            whole = np.empty_like(cat)
            whole[logical] = cat
            assert np.array_equal(whole, want[s][fld]), (s, fld)
    assert len(np.unique(want[-1][0])) > 1 and moved, "the run shows nothing: no spread, or no particle ever changed rank"


class View(object):
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


@pytest.mark.parametrize("world", [2, 3])
def test_front_end_in_odometry_mode_is_the_single_filter(world, tmp_path):
    import parakeet_slam_amd as pk
    from parakeet_slam_amd.core import _make_state, _state_pose

    P = P_LOCAL * world
    means, covs, poses, scans = drive(STEPS)
    np.random.seed(5)
    random.seed(5)
    pk.msgs.Time.set_now(0.0)
    feats = [pk.Feature(mean=m.copy(), covar=c.copy()) for m, c in zip(means, covs)]
    fs = pk.FastSLAM(feats, num_particles=P, devices=list(range(world)), weight_domain="log", rng="global", backend="gloo",
                     motion="odometry", odom_alphas=ALPHAS, _shard_factory=make_odom_oracle_shard)
    try:
        from parakeet_slam_amd.multi import ShardedFastSLAM

        assert isinstance(fs, ShardedFastSLAM) and fs._motion == "odometry" and fs._odom_alphas == ALPHAS
        o = OracleFilter(P, means, covs)
        np_rs, py_rs = np.random.RandomState(5), random.Random(5)
        path = str(tmp_path / "odom.npz")
        msgs = [_make_state(*p) for p in poses]
        start = fs.download_poses().copy()
        fs.odom_motion_update(msgs[0])  # the first message only stores its pose
        assert np.array_equal(fs.download_poses(), start) and fs._draw == 0 and fs._odom_prev == _state_pose(msgs[0])
        tw = pk.msgs.Twist()
        tw.linear.x, tw.angular.z = 3.0, 1.0
        pk.msgs.Time.set_now(0.5)
        fs.motion_update(tw)  # odometry mode: the control is recorded, nothing moves, no draw is made
        assert fs.last_control is tw and np.array_equal(fs.download_poses(), start) and fs._draw == 0
        fs.odom_motion_update(msgs[0])  # the robot stood still: nothing
        assert np.array_equal(fs.download_poses(), start) and fs._draw == 0
        for s in range(STEPS):
            pk.msgs.Time.set_now(0.5 * (s + 2))
            fs.odom_motion_update(msgs[s + 1])
            fs.cam_cb(View(pk, scans[s + 1]))
            d = ref.delta(_state_pose(msgs[s]), _state_pose(msgs[s + 1]))
            o.reset_weights()
            o.x, o.y, o.h = ref.sample(o.x, o.y, o.h, d, ALPHAS, np_rs.standard_normal((P, 3)))
            o.observe(scans[s + 1])
            o.gather(low_variance_ancestors(np.exp(o.logw - o.logw.max()), py_rs.random()))
            fs.save_state(path)
            snap = np.load(path)
            assert np.array_equal(snap["poses"][:, :3], np.stack([o.x, o.y, o.h], 1)), s
            assert np.allclose(snap["poses"][:, 3], np.exp(o.logw), rtol=1e-12, atol=0.0)
            assert np.array_equal(snap["means"], o.mean) and np.array_equal(snap["covs"], o.cov) and np.array_equal(snap["counts"], o.count)
            assert np.array_equal(snap["odom_prev"], _state_pose(msgs[s + 1]))
        assert fs._draw == STEPS and len(np.unique(o.x)) > 1
        # the snapshot goes back in: the stored odometry pose with it
        fs._odom_prev = None
        fs.load_state(path)
        assert fs._odom_prev == _state_pose(msgs[STEPS])
        # a message that is not finite is refused in the front end: nothing stored, nothing moved, no rank fails, and the next
        # good message moves the particles by the change since the last good one
        before = fs.download_poses().copy()
        bad = _make_state(1.0, 2.0, 0.5)
        bad.pose.pose.position.x = float("nan")
        with pytest.raises(ValueError):
            fs.odom_motion_update(bad)
        assert fs._odom_prev == _state_pose(msgs[STEPS]) and fs._draw == STEPS and np.array_equal(fs.download_poses(), before)
        fs.odom_motion_update(_make_state(*truth_step(poses[STEPS], 0.8, 0.9, 0.5)))
        assert fs._draw == STEPS + 1 and not np.array_equal(fs.download_poses()[:, :2], before[:, :2])
        # a malformed stored pose in a snapshot: ValueError before anything is assigned, as FastSLAM.load_state
        after = fs.download_poses().copy()
        snap = dict(np.load(path))
        for wrong in (np.array([1.0, 2.0]), np.array([1.0, float("inf"), 0.0])):
            snap["odom_prev"] = wrong
            np.savez_compressed(path, **snap)
            with pytest.raises(ValueError):
                fs.load_state(path)
            assert np.array_equal(fs.download_poses(), after)
    finally:
        fs.close()


def test_the_default_mode_ignores_odometry_messages_and_bad_keywords_are_refused_before_anything_starts():
    import parakeet_slam_amd as pk
    from parakeet_slam_amd.core import _make_state

    pk.msgs.Time.set_now(0.0)
    feats = [pk.Feature(mean=np.array([5.0 + l, 1.0 - l, 10.0 * l, 20.0, 30.0]), covar=0.25 * np.identity(5)) for l in range(3)]
    fs = pk.FastSLAM(feats, 8, devices=[0, 1], backend="gloo", _shard_factory=make_odom_oracle_shard)
    try:
        before = fs.download_poses().copy()
        for p in ((0.0, 0.0, 0.0), (1.0, 0.5, 0.3), (2.0, 1.5, 0.9)):
            fs.odom_motion_update(_make_state(*p))
        assert fs._motion == "twist" and np.array_equal(fs.download_poses(), before) and fs._draw == 0 and fs._odom_prev is None
    finally:
        fs.close()
    for bad in (dict(motion="odom"), dict(motion="odometry", odom_alphas=(1, 2, 3)), dict(motion="odometry", odom_alphas=(0.1, 0.1, 0.1, -1.0)),
                dict(motion="odometry", odom_min_trans=-1.0), dict(motion="odometry", odom_min_trans=float("nan"))):
        with pytest.raises(ValueError):
            pk.FastSLAM(feats, 8, devices=[0, 1], backend="gloo", _shard_factory=make_odom_oracle_shard, **bad)
        with pytest.raises(ValueError):
            pk.ShardedFastSLAM(feats, 8, devices=[0, 1], backend="gloo", _shard_factory=make_odom_oracle_shard, **bad)

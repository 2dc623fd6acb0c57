"""GPU: the path estimate (pk_path_*, pk_k_path.hip; DESIGN.md section 4, "The path estimate") -- a ring of the generations every
resample worked on, the lineages traced back through it, their moments and the number of distinct ancestors left per step.

No map and no scan anywhere but in the facade test: DeviceFilter(P, 0), chosen weights and resample(u) drive everything.  The
reference is path_reference.py (where the tolerances are stated), fed with what the host saw happen: download_poses() before
every resample and the ancestors it returned."""
import random

import numpy as np
import pytest

import path_reference as pr
from conftest import load_golden
from resample_reference import exact_ancestors

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1  # PK_ERR_STATE, PK_ERR_INVALID


def start_poses(rs, P, weights=None):
    """Poses away from the origin with y following x (no moment of the population is small against its scale)."""
    x = rs.uniform(10.0, 20.0, P)
    y = 0.5 * x + rs.uniform(-1.0, 1.0, P)
    h = rs.uniform(-0.6, 0.6, P)
    return np.column_stack([x, y, h, np.ones(P) if weights is None else weights])


class Run(object):
    """A filter and the host's record of what happened to it: the poses in front of every resample and its ancestors."""

    def __init__(self, lib, P, capacity, seed, weights=None):
        self.rs = np.random.RandomState(seed)
        self.P = P
        self.f = lib.DeviceFilter(P, 0)
        self.f.upload_poses(start_poses(self.rs, P, weights))
        if capacity:
            self.f.path_enable(capacity)
        self.poses, self.anc = [], []

    def move(self):
        self.f.motion(0.3, 0.1, 0.1, z=self.rs.standard_normal((self.P, 3)))

    def set_one(self, i, weight):
        """One particle re-uploaded (pk_upload_pose: only the present changes) at a new pose and weight."""
        row = np.append(start_poses(self.rs, 1)[0, :3], weight)
        self.f.upload_pose(i, row)

    def resample(self, u):
        before = self.f.download_poses()
        a = self.f.resample(u, return_ancestors=True)
        self.poses.append(before[:, :3].copy())
        self.anc.append(a.astype(np.int32))
        return before, a

    def current(self):
        return self.f.download_poses()[:, :3]

    def last(self, n):
        return np.array(self.poses[len(self.poses) - n:]).reshape(n, self.P, 3), np.array(self.anc[len(self.anc) - n:]).reshape(n, self.P)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. recording is what happened: sizes that straddle a wave, a 256-lane block and the 1024-particle scan block
@pytest.mark.parametrize("P", [1, 63, 65, 1000, 1025, 4097])
def test_recording_is_what_happened(lib, P):
    rs = np.random.RandomState(100 + P)
    r = Run(lib, P, 8, seed=P, weights=rs.uniform(0.1, 1.0, P) ** 4)
    for s in range(6):
        if s % 2 == 0:
            r.move()
        else:
            for i in rs.randint(0, P, size=min(P, 5)):
                r.set_one(int(i), float(rs.uniform(0.5, 3.0)))
        r.resample(float(rs.uniform(0.0, 1.0)))
    assert r.f.path_shape() == (8, 6, 6)
    poses, anc = r.f.path_download()
    assert poses.shape == (6, P, 3) and anc.shape == (6, P) and anc.dtype == np.int32
    want_p, want_a = r.last(6)
    assert same_bits(poses, want_p)
    assert np.array_equal(anc, want_a)
    p23, a23 = r.f.path_download(2, 4)  # a range of rows
    assert same_bits(p23, want_p[2:4]) and np.array_equal(a23, want_a[2:4])
    if P > 1:
        assert any(np.unique(a).size < P for a in want_a)  # (the resamples did select)
    r.f.close()


# ---- 2. the ring wraps: the newest rows are kept, oldest first, and the count of rows ever recorded stays exact
@pytest.mark.parametrize("capacity,steps", [(4, 11), (1, 3)])
def test_ring_wrap(lib, capacity, steps):
    P = 300
    rs = np.random.RandomState(7)
    r = Run(lib, P, capacity, seed=3, weights=rs.uniform(0.1, 1.0, P) ** 3)
    for s in range(steps):
        r.move()
        r.resample(float(rs.uniform(0.0, 1.0)))
        held = min(s + 1, capacity)
        assert r.f.path_shape() == (capacity, held, s + 1)
    poses, anc = r.f.path_download()
    want_p, want_a = r.last(capacity)
    assert same_bits(poses, want_p) and np.array_equal(anc, want_a)
    got = r.f.path_summary()
    assert got.first_step == steps - capacity and got.held == capacity
    assert got.steps().tolist() == list(range(steps - capacity, steps + 1))
    pr.check_summary(got, want_p, want_a, r.current(), what="wrapped ring of %d" % capacity)
    assert same_bits(r.f.path_trace(np.arange(P)), pr.paths(want_p, want_a, r.current()))
    r.f.close()


# ---- 3. trace and summary against the reference, on a run with all three kinds of row
HEAVY = 1e7  # a heavy particle among weights of 1: the issue's "few heavy particles among 1e-7 ones", scaled


def heavy_plan(P, steps=8):
    """Per step the particles that are heavy in front of its resample: one, then three, then forty, then none (uniform weights)."""
    return [[7 % P], [P // 10, P // 2, P - P // 10 - 1], list(range(3, P, max(1, P // 40)))[:40]] + [[] for _ in range(steps - 3)]


@pytest.mark.parametrize("P", [1000, 4097])
def test_trace_and_summary_against_the_reference(lib, P):
    plan = heavy_plan(P)
    us = np.random.RandomState(P).uniform(0.05, 0.95, len(plan))
    # before the GPU is touched: the run, as the host's exact resampler sees it, holds a row with one survivor, one with several but
    # not all, and one with all -- nothing below can pass vacuously
    host_anc = []
    for heavy, u in zip(plan, us):
        w = np.ones(P)
        w[heavy] = HEAVY
        host_anc.append(exact_ancestors(np.log(w), float(u), False)[0])
    host_surv = pr.survivors(np.array(host_anc), P)
    assert np.any(host_surv == 1) and np.any((host_surv > 1) & (host_surv < P)) and np.any(host_surv == P), host_surv

    r = Run(lib, P, 16, seed=P + 1)
    for heavy, u in zip(plan, us):
        r.move()
        r.f.reset_weights()
        now = r.f.download_poses()
        for i in heavy:
            r.f.upload_pose(i, np.append(now[i, :3], HEAVY))
        r.resample(float(u))
    T = len(plan)
    poses, anc = r.last(T)
    rp, ra = r.f.path_download()
    assert same_bits(rp, poses) and np.array_equal(ra, anc)
    current = r.current()
    surv = pr.survivors(anc, P)
    assert np.any(surv == 1) and np.any((surv > 1) & (surv < P)) and np.any(surv == P), surv  # (the device's run too)

    got_paths = r.f.path_trace(np.arange(P))
    assert got_paths.shape == (P, T + 1, 3)
    assert same_bits(got_paths, pr.paths(poses, anc, current))
    some = np.array([P - 1, 0, P // 2, 0])  # any order, repeats
    assert same_bits(r.f.path_trace(some), got_paths[some])

    got = r.f.path_summary()
    mean, spread, _ = pr.check_summary(got, poses, anc, current, what="P = %d" % P)
    sx, sy, sh = r.f.summary()  # row `held` is the current generation: pk_summary's estimate
    assert abs(got.mean[T, 0] - sx) <= 1e-12 * abs(sx) and abs(got.mean[T, 1] - sy) <= 1e-12 * abs(sy)
    assert pr.angle_diff(got.mean[T, 2], sh) <= 1e-12
    again = r.f.path_summary()
    assert same_bits(got.mean, again.mean) and same_bits(got.spread, again.spread) and np.array_equal(got.survivors, again.survivors)
    r.f.close()


# ---- 4. ancestors in any order: uploaded maps, reversed and random with repeats
def test_unsorted_ancestors(lib):
    P, T = 300, 5
    rs = np.random.RandomState(11)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(rs, P))
    f.path_enable(6)
    poses = np.stack([start_poses(rs, P)[:, :3] for _ in range(T)])
    anc = np.stack([np.arange(P)[::-1],               # reversed
                    rs.randint(0, P, P),              # random, with repeats
                    rs.permutation(P),                # a permutation
                    rs.randint(0, 9, P) * 31,         # nine parents, unsorted
                    rs.randint(0, P, P)]).astype(np.int32)
    f.path_upload(poses, anc, recorded=12)
    assert f.path_shape() == (6, T, 12)
    rp, ra = f.path_download()
    assert same_bits(rp, poses) and np.array_equal(ra, anc)
    current = f.download_poses()[:, :3]
    assert same_bits(f.path_trace(np.arange(P)), pr.paths(poses, anc, current))
    got = f.path_summary()
    assert got.first_step == 7
    _, _, surv = pr.check_summary(got, poses, anc, current, what="uploaded maps")
    assert np.any((surv > 1) & (surv < P))
    # ... and one survivor through a constant map, in a ring that then goes on recording
    anc[2] = 123
    f.path_upload(poses, anc)
    f.motion(0.2, 0.0, 0.1, z=rs.standard_normal((P, 3)))
    before = f.download_poses()[:, :3]
    a = f.resample(0.3, return_ancestors=True)
    poses6, anc6 = np.concatenate([poses, before[None]]), np.concatenate([anc, a[None].astype(np.int32)])
    assert f.path_shape() == (6, 6, 6)
    got = f.path_summary()
    _, _, surv = pr.check_summary(got, poses6, anc6, f.download_poses()[:, :3], what="constant map")
    assert surv[:3].tolist() == [1, 1, 1]
    f.close()


# ---- 5. life cycle
def raises(lib, status, fn, *args):
    with pytest.raises(lib.PkError) as e:
        fn(*args)
    assert e.value.status == status, e.value
    return str(e.value)


def test_memory_is_counted_and_given_back(lib):
    P, cap = 1000, 5
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(np.random.RandomState(0), P))
    b0 = f.device_bytes()
    f.path_enable(cap)
    b1 = f.device_bytes()
    assert b1 - b0 >= cap * P * 28
    f.resample(0.5)
    f.resample(0.25)
    f.path_summary()                 # (scratch of the summary and the trace: counted while held ...)
    f.path_trace(np.arange(P))
    assert f.device_bytes() > b1
    f.path_enable(0)                 # (... and given back with the ring)
    assert f.device_bytes() == b0
    raises(lib, STATE, f.path_shape)
    f.path_enable(3)
    assert f.path_shape() == (3, 0, 0)
    f.resample(0.5)
    assert f.path_shape() == (3, 1, 1)
    f.path_enable(7)                 # another capacity: an empty ring
    assert f.path_shape() == (7, 0, 0)
    assert f.device_bytes() - b0 >= 7 * P * 28
    f.close()


def test_what_empties_the_ring(lib):
    P = 200
    r = Run(lib, P, 4, seed=5)
    r.move()
    r.resample(0.4)
    r.move()
    r.resample(0.6)
    assert r.f.path_shape() == (4, 2, 2)
    r.set_one(17, 2.0)               # one particle: only the present changes
    assert r.f.path_shape() == (4, 2, 2)
    poses, anc = r.last(2)
    assert same_bits(r.f.path_trace(np.arange(P)), pr.paths(poses, anc, r.current()))
    assert r.current()[17].tolist() == r.f.path_trace([17])[0, 2].tolist()
    r.f.upload_poses(start_poses(r.rs, P))  # a replaced population has no lineage
    assert r.f.path_shape()[:2] == (4, 0)
    got = r.f.path_summary()         # held == 0 is a valid input: the current generation alone
    assert got.mean.shape == (1, 3) and got.survivors.tolist() == [P]
    pr.check_summary(got, np.empty((0, P, 3)), np.empty((0, P), dtype=np.int32), r.current(), what="empty ring")
    assert r.f.path_trace(np.zeros(0, dtype=np.int64)).shape == (0, 1, 3)  # n == 0 too
    r.f.close()


def test_one_particle(lib):
    r = Run(lib, 1, 3, seed=2)
    for u in (0.1, 0.9):
        r.move()
        r.resample(u)
    poses, anc = r.last(2)
    assert np.array_equal(anc, np.zeros((2, 1), dtype=np.int32))
    got = r.f.path_summary()
    pr.check_summary(got, poses, anc, r.current(), what="P = 1")
    assert got.survivors.tolist() == [1, 1, 1]
    assert same_bits(r.f.path_trace([0]), pr.paths(poses, anc, r.current()))
    r.f.close()


def test_refusals(lib):
    P = 64
    f = lib.DeviceFilter(P, 0)
    some_poses, some_anc = np.zeros((1, P, 3)), np.zeros((1, P), dtype=np.int32)
    # before pk_path_enable
    for fn, args in ((f.path_shape, ()), (f.path_download, ()), (f.path_upload, (some_poses, some_anc)), (f.path_trace, ([0],)),
                     (f.path_summary, ())):
        assert "pk_path_enable" in raises(lib, STATE, fn, *args)
    raises(lib, INVALID, f.path_enable, -1)
    f.path_enable(2)
    f.resample(0.5)
    # bad ranges, particles and ancestors
    raises(lib, INVALID, f.path_download, 1, 0)
    raises(lib, INVALID, f.path_download, 0, 2)
    raises(lib, INVALID, f.path_download, -1, 1)
    raises(lib, INVALID, f.path_trace, [P])
    raises(lib, INVALID, f.path_trace, [0, -1])
    for bad in (P, -1):
        a = some_anc.copy()
        a[0, 5] = bad
        raises(lib, INVALID, f.path_upload, some_poses, a)
    raises(lib, INVALID, f.path_upload, np.zeros((3, P, 3)), np.zeros((3, P), dtype=np.int32))  # more rows than the ring has
    raises(lib, INVALID, f.path_upload, some_poses, some_anc, 0)                                # recorded < rows
    assert f.path_shape() == (2, 1, 1)  # (nothing of that changed the ring)
    # the sharded protocol and the split step, refused ahead of anything else they do
    table = np.zeros(6, dtype=np.int64)
    for fn, args in ((f.pack_particles, ([0], 0)), (f.adopt_particles, (np.arange(P), 0, 0)), (f.shard_adopt_dev, (0, 0, 0)),
                     (f.shard_adopt_local_dev, (0,)), (f.shard_adopt_remote_dev, (0, 0, 0)),
                     (f.shard_adopt_balanced_dev, (table, 1, 0, 0, 0, 0)), (f.shard_state_dev, (0,)),
                     (f.observe_staged_range, (True, 0, P, True, True))):
        assert "pk_path_enable" in raises(lib, STATE, fn, *args)
    f.path_enable(0)
    raises(lib, INVALID, f.shard_state_dev, 0)  # the refusal went with the ring: the call's own argument check speaks again
    f.close()


def test_a_filter_that_never_recorded_resamples_as_before(lib):
    P = 1025
    rs = np.random.RandomState(4)
    w = rs.uniform(0.1, 1.0, P) ** 4
    a, b = Run(lib, P, 0, seed=9, weights=w), Run(lib, P, 5, seed=9, weights=w)
    for u in (0.3, 0.7, 0.05):
        for r in (a, b):
            r.move()
            r.resample(u)
    for x, y in zip(a.anc, b.anc):
        assert np.array_equal(x, y)
    assert same_bits(a.f.download_poses(), b.f.download_poses())
    raises(lib, STATE, a.f.path_shape)
    a.f.close()
    b.f.close()


# ---- 6. the facade
class View(object):
    def __init__(self, pk, rows):
        class Scan(object):
            pass

        self.last_sensor_reading = Scan()
        self.last_sensor_reading.observes = [blob(pk, *r) for r in rows]


def blob(pk, bearing=0.0, r=0, g=0, b=0):
    if pk.msgs.Blob is pk.msgs._Blob:
        return pk.msgs.Blob(bearing, r, g, b)
    z = pk.msgs.Blob()
    z.bearing = bearing
    z.color.r, z.color.g, z.color.b = r, g, b
    return z


def small_scene_filter(pk, g, **kw):
    L = int(g["L"])
    fs = pk.FastSLAM([pk.Feature(mean=g["means0"][l], covar=g["covs0"][l]) for l in range(L)], num_particles=512, **kw)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = 0.2, 0.1
    fs.last_control = tw
    return fs


def test_facade(tmp_path):
    import parakeet_slam_amd as pk
    from parakeet_slam_amd import msgs, path as pkpath

    pk.msgs = msgs
    g = load_golden("step_small")
    np.random.seed(3)
    random.seed(3)
    msgs.Time.set_now(0.0)
    with pytest.raises(ValueError, match="one GPU"):  # (before any process starts)
        pk.FastSLAM([], num_particles=512, devices=[0, 1], record_path=8)
    with pytest.raises(ValueError, match="one GPU"):
        pk.ShardedFastSLAM([], num_particles=512, devices=[0, 1], record_path=8)
    fs = small_scene_filter(pk, g, record_path=8)
    nb = len(g["blobs"])
    for s in range(5):
        msgs.Time.set_now(0.1 * (s + 1))
        fs.cam_cb(View(pk, g["blobs"][s % nb]))
    P = 512
    got = fs.path_summary()
    assert isinstance(got, pkpath.PathSummary)
    assert got.mean.shape == (6, 3) and got.spread.shape == (6, 4) and got.survivors.shape == (6,) and got.first_step == 0
    assert got.survivors[5] == P and np.all(got.survivors[:-1] <= got.survivors[1:]) and got.survivors[0] >= 1
    sx, sy, sh = fs.summary()
    assert abs(got.mean[5, 0] - sx) <= 1e-12 * abs(sx) and abs(got.mean[5, 1] - sy) <= 1e-12 * abs(sy)
    assert pr.angle_diff(got.mean[5, 2], sh) <= 1e-12
    track = pkpath.as_poses(got)
    assert len(track) == 6 and track[5] == tuple(float(v) for v in got.mean[5])
    idx = [0, 17, P - 1]
    paths = fs.particle_paths(idx)
    assert paths.shape == (3, 6, 3)
    for row, i in zip(paths, idx):
        p = fs.particles[i]
        assert row[5, 0] == p.state.pose.pose.position.x and row[5, 1] == p.state.pose.pose.position.y
        assert pr.angle_diff(row[5, 2], msgs.quaternion_to_heading(p.state.pose.pose.orientation)) <= 1e-12
    ring_p, ring_a = fs._filter.path_download()
    pr.check_summary(got, ring_p, ring_a, fs._filter.download_poses()[:, :3], what="facade")
    # save -> a fresh filter -> load: an equal ring; a filter that does not record writes the snapshot it always wrote
    snap = str(tmp_path / "snap.npz")
    fs.save_state(snap)
    assert {"path_poses", "path_ancestors", "path_recorded"} <= set(np.load(snap).files)
    other = small_scene_filter(pk, g, record_path=8)
    other.load_state(snap)
    assert other._filter.path_shape() == fs._filter.path_shape() == (8, 5, 5)
    op, oa = other._filter.path_download()
    assert same_bits(op, ring_p) and np.array_equal(oa, ring_a)
    assert same_bits(other.particle_paths(idx), paths)
    plain = small_scene_filter(pk, g)
    with pytest.raises(ValueError, match="record_path"):
        plain.path_summary()
    plain.load_state(snap)           # (a snapshot with a path into a filter without a ring: the path is not read)
    plain_snap = str(tmp_path / "plain.npz")
    plain.save_state(plain_snap)
    assert not any(k.startswith("path_") for k in np.load(plain_snap).files)
    other.load_state(plain_snap)     # a snapshot without a path: the ring is left empty
    assert other._filter.path_shape()[:2] == (8, 0)
    for f in (fs, other, plain):
        f.close()

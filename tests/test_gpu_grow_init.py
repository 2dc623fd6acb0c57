"""GPU: the triangulated initialisation of growing maps (pk_grow_init(f, PK_GROW_INIT_TRIANGULATED, min_parallax); k_new_landmarks_tri,
pk_k_grow.hip; DESIGN.md section 9, "Parallax-gated pairing") against tests/grow_init_reference.py, particle by particle at every
step: counters, stored readings, slot ids, flags, counts, means, covariances, log-weights.

Tolerances: under the reference model the ones tests/test_gpu_grow.py holds the plain rule to (readings 1e-12, means 1e-8,
covariances rtol 1e-8 / atol 1e-9, log-weights 1e-9); under the bearing model the ones tests/test_gpu_bearing_model.py holds its
growing maps to (means 1e-9 relative, covariances rtol 1e-9 / atol 1e-13, log-weights 1e-9 absolute).

The scenes are tests/grow_init_reference.py's; tests/test_grow_init_reference_host.py checks each of them on the CPU for a gate
margin above 1e-9, for readings excluded, pairings changed, features made and promoted, and for rings that are never overrun."""
import random

import numpy as np
import pytest

from conftest import relerr
from oracle.fastslam_oracle import EMPTY_COLOUR, synthetic_scan, synthetic_world, truth_step

import grow_init_reference as gi
from bearing_model_reference import wrapped_scan
from grow_init_reference import TriangulatingOracle

pytestmark = pytest.mark.gpu

C = gi.SMALL
L0 = C["L0"]


# ---------------------------------------------------------------------------------------------------------------- helpers
def _device(lib, name, opts=None, init=True):
    model, mp, R, retire, _seed = gi.GPU_SCENES[name]
    means, mcov = gi.small_map()
    f = lib.DeviceFilter(C["P"], len(means))
    if model == "bearing":
        f.set_measurement_model("bearing")
    for k, v in (opts or {}).items():
        f.set_option(k, v)
    f.upload_map(means, mcov.reshape(len(means), 25))
    f.grow_enable(L0, R, C["thr"])
    if retire:
        f.grow_retire(*retire)
    if init:
        f.grow_init("triangulated", mp)
        assert f.grow_init_mode() == ("triangulated", mp)
    return f


def _compare(lib, f, o, step, bearing, clocks=False):
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
    m, c, k = f.download_landmarks()
    assert np.array_equal((k & lib.PK_LANDMARK_POTENTIAL) != 0, o.f.potential), step
    assert np.array_equal(k & ~lib.PK_LANDMARK_POTENTIAL, o.f.count), step
    if bearing:
        assert relerr(m, o.f.mean) < 1e-9, (step, relerr(m, o.f.mean))
        assert np.allclose(c.reshape(o.f.cov.shape), o.f.cov, rtol=1e-9, atol=1e-13), step
    else:
        assert np.allclose(m, o.f.mean, rtol=1e-8, atol=1e-8), step
        assert np.allclose(c.reshape(o.f.cov.shape), o.f.cov, rtol=1e-8, atol=1e-9), step


def _propagated(o):
    """Position blocks of the features the oracle made that are no identity: the covariance is in play."""
    return sum(1 for _i, _slot, _rid, _me, p in o.made if abs(p[0] - 1.0) > 1e-3 or abs(p[2] - 1.0) > 1e-3 or abs(p[1]) > 1e-3)


# ---------------------------------------------------------------------------------------------------------------- the small scene
@pytest.mark.parametrize("name", ["bearing_0.1", "bearing_0.2", "bearing_0.1_retiring"])
def test_bearing_model_small_scene_against_the_oracle(lib, name):
    """64 particles, 10 + 3 landmarks, 5 spare slots, noise-free wrapped scans, 14 steps; with retirement (reading_max_age 4,
    potential_max_idle 3) against the composed oracle, clocks included."""
    retiring = gi.GPU_SCENES[name][3] is not None
    f = _device(lib, name)
    o = gi.small_oracle(name)
    for st in gi.small_drive(name, o):
        f.motion(C["v"], C["w"], C["dt"], z=st.z)
        f.observe(st.blobs, fresh=True)
        assert f.observe_route() == "ml_general"
        got = f.download_log_weights()
        assert np.allclose(got, st.logw, rtol=0, atol=1e-9), (st.s, np.abs(got - st.logw).max())
        assert np.array_equal(f.resample(st.u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), st.anc), st.s
        st.finish()
        _compare(lib, f, o, st.s, True, clocks=retiring)
    assert o.used == [3] * C["P"] and (gi.promoted(o) == 3).all()  # the three unknown landmarks, and nothing else, in every particle
    assert o.margin > 1e-9
    assert len(o.excluded) > 0 and len(o.changed) > 0 and _propagated(o) == len(o.made) > 0
    if retiring:
        assert sum(o.readings_retired) > 0
    f.close()


def test_reference_model_small_scene_on_both_routes(lib):
    """The same scene under the reference model, unwrapped scans, rings of 128 (they reach about 110 readings: the search and the
    gate run beyond the wave's 64 lanes): the one-pass route of its size, whose bit rows the kernel reads, and the general route,
    whose ids it reads -- both against the oracle, and against each other array for array."""
    name = "reference_0.1"
    fa, fb = _device(lib, name), _device(lib, name, opts={"fast_observe": 0})
    o = gi.small_oracle(name)
    for st in gi.small_drive(name, o):
        for f in (fa, fb):
            f.motion(C["v"], C["w"], C["dt"], z=st.z)
            f.observe(st.blobs, fresh=True)
        assert fa.observe_route() == "ml_fused" and fa.observe_published() and fb.observe_route() == "ml_general"
        for f in (fa, fb):
            assert np.allclose(f.download_log_weights(), st.logw, rtol=1e-9, atol=1e-9), st.s
        assert np.allclose(fa.download_log_weights(), fb.download_log_weights(), rtol=1e-11, atol=1e-9), st.s
        (ca, ra, sa), (cb, rb, sb) = fa.grow_download(), fb.grow_download()
        assert np.array_equal(ca, cb), st.s
        for i in range(C["P"]):
            assert np.array_equal(ra[i, :ca[i, 0]], rb[i, :cb[i, 0]]) and np.array_equal(sa[i, :ca[i, 1]], sb[i, :cb[i, 1]]), (st.s, i)
        for xa, xb in zip(fa.download_landmarks(), fb.download_landmarks()):
            assert np.array_equal(xa, xb), st.s
        # (the ancestors are the device's: the oracle's log-weights agree with it to 1e-9, which a resample may feel)
        anc = fa.resample(st.u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
        assert np.array_equal(fb.resample(st.u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), st.s
        st.finish(anc)
        _compare(lib, fa, o, st.s, False)
        _compare(lib, fb, o, st.s, False)
    assert o.margin > 1e-9  # (of the run as the device's ancestors made it)
    assert o.longest_ring > 64 and len(o.excluded) > 0 and len(o.changed) > 0 and _propagated(o) > 0 and gi.promoted(o).max() >= 1
    fa.close()
    fb.close()


# ---------------------------------------------------------------------------------------------------------------- hand-written rings
def test_hand_written_rings(lib):
    """One unmatched blob against rings written by hand (pk_grow_upload), min_parallax 0.2 (sin 0.1987).  The robot looks along +x at
    a landmark 10 m ahead.  A reading taken from behind the robot, close to its line of sight, meets the blob's ray at 0.05 rad at
    the most (|den| <= 0.05); one taken from 3-5 m to the side at 0.29 rad or more (|den| >= 0.28): every |den| is 0.08 or more
    away from the threshold.
      particle 0: the nearest colour is ineligible -- the second nearest is taken (index 66, beyond the first 64 lanes);
      particle 1: every reading is ineligible -- the blob is stored;
      particle 2: the nearest colour three times, ineligible at 10, eligible at 20 and 75 -- 20 wins;
      particle 3: 150 readings, the only eligible one at index 130;
      particle 4: no reading at all -- stored."""
    P, L0_, spare, R, thr, mp = 5, 1, 2, 150, 30.0, 0.2
    known = np.array([[40.0, 40.0, 250.0, 250.0, 250.0]])
    kcov = 0.25 * np.identity(5).reshape(1, 5, 5)
    f = lib.DeviceFilter(P, L0_ + spare)
    means = np.zeros((L0_ + spare, 5))
    means[:L0_] = known
    means[L0_:, 2:] = EMPTY_COLOUR
    covs = np.tile(np.identity(5).reshape(25), (L0_ + spare, 1))
    covs[:L0_] = kcov.reshape(L0_, 25)
    f.upload_map(means, covs)
    f.grow_enable(L0_, R, thr)
    f.grow_init(lib.PK_GROW_INIT_TRIANGULATED, mp)
    o = TriangulatingOracle(P, known, kcov, spare, thr, min_parallax=mp)
    rs = np.random.RandomState(8)
    poses = np.zeros((P, 4))
    poses[:, 0] = rs.uniform(-0.2, 0.2, P)
    poses[:, 1] = rs.uniform(-0.05, 0.05, P)
    poses[:, 3] = 1.0
    f.upload_poses(poses)
    o.f.x[:], o.f.y[:], o.f.h[:] = poses[:, 0], poses[:, 1], poses[:, 2]
    target = np.array([10.0, 0.0])
    colour = np.array([100.0, 50.0, 20.0])

    def reading(eligible, offset):
        if eligible:
            ox, oy = rs.uniform(0.0, 3.0), rs.uniform(3.0, 5.0) * rs.choice([-1.0, 1.0])
        else:
            ox, oy = rs.uniform(-3.0, -1.0), rs.uniform(0.2, 0.4) * rs.choice([-1.0, 1.0])
        oh = rs.uniform(-0.3, 0.3)
        col = colour + offset * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
        return (ox, oy, oh, np.arctan2(target[1] - oy, target[0] - ox) - oh, col[0], col[1], col[2])

    def far():  # a colour distance no one wins with
        return rs.uniform(8.0, 14.0)

    rings = [
        [reading(True, far()) for _ in range(70)],
        [reading(False, rs.uniform(1.0, 14.0)) for _ in range(100)],
        [reading(True, far()) for _ in range(100)],
        [reading(False, rs.uniform(1.0, 14.0)) for _ in range(150)],
        [],
    ]
    rings[0][40] = reading(False, 1.0)
    rings[0][66] = reading(True, 2.0)
    rings[2][10] = reading(False, 1.5)
    rings[2][20] = reading(True, 1.5)
    rings[2][75] = reading(True, 1.5)
    rings[3][130] = reading(True, 9.0)
    cnt = np.zeros((P, 4), dtype=np.int32)
    rd = np.zeros((P, R, 8))
    for i, ring in enumerate(rings):
        n = len(ring)
        cnt[i] = (n, 0, L0_ + 1 + n, 0)
        for r, row in enumerate(ring):
            rd[i, r] = (L0_ + 1 + r,) + row
        o.hyp[i] = [(int(r[0]),) + tuple(float(v) for v in r[1:]) for r in rd[i, :n]]
        o.next_id[i] = L0_ + 1 + n
    f.grow_upload(0, P, cnt, rd, np.zeros((P, spare), dtype=np.int32))
    blobs = np.zeros((1, 4))
    blobs[0, 1:] = colour
    f.observe(blobs, fresh=True)
    o.f.reset_weights()
    o.observe(blobs)
    # the oracle decided what the docstring says, nowhere near the threshold
    assert o.margin > 0.08, o.margin
    assert o.used == [1, 0, 1, 1, 0] and [len(h) for h in o.hyp] == [70, 101, 100, 150, 1]
    assert [(i, rid - (L0_ + 1)) for i, _slot, rid, _me, _p in o.made] == [(0, 66), (2, 20), (3, 130)]
    assert (0, L0_ + 1 + 40, L0_ + 1 + 70) in o.excluded and (2, L0_ + 1 + 10, L0_ + 1 + 100) in o.excluded
    c2, r2, s2 = f.grow_download()
    assert np.array_equal(c2[:, 0], [len(h) for h in o.hyp]) and np.array_equal(c2[:, 1], o.used) and np.array_equal(c2[:, 2], o.next_id)
    assert not c2[:, 3].any()
    for i in (1, 4):  # the stored blob, as the last reading
        assert np.allclose(r2[i, c2[i, 0] - 1], np.asarray(o.hyp[i][-1]), rtol=1e-12, atol=1e-12), i
    m, c, k = f.download_landmarks()
    assert np.allclose(m[:, L0_:], o.f.mean[:, L0_:], rtol=1e-9, atol=1e-9)
    assert np.allclose(c.reshape(o.f.cov.shape), o.f.cov, rtol=1e-9, atol=1e-12)
    for i in (0, 2, 3):
        assert int(s2[i, 0]) == o.slot_id[i][L0_] and k[i, L0_] == lib.PK_LANDMARK_POTENTIAL
        assert c.reshape(o.f.cov.shape)[i, L0_, 0, 0] != 1.0
    f.close()


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_a_filter_told_the_reference_rule_is_one_never_told(lib):
    """PK_GROW_INIT_REFERENCE, with a min_parallax it must ignore, against a filter that never called pk_grow_init: every array equal,
    bit for bit, over 9 steps -- and a filter switched to the new rule and back before the first scan."""
    name = "reference_0.1"
    never, told, back = _device(lib, name, init=False), _device(lib, name, init=False), _device(lib, name, init=False)
    assert never.grow_init_mode() == ("reference", 0.0)
    told.grow_init(lib.PK_GROW_INIT_REFERENCE, 0.3)
    assert told.grow_init_mode() == ("reference", 0.3)
    back.grow_init("triangulated", 0.3)
    back.grow_init("reference")
    world, _ = gi.small_world()
    rs = np.random.RandomState(5)
    pose = (0.0, 0.0, 0.0)
    for s in range(9):
        pose = truth_step(pose, C["v"], C["w"], C["dt"])
        blobs = synthetic_scan(world, pose)
        z, u = rs.standard_normal((C["P"], 3)), float(rs.uniform())
        for g in (never, told, back):
            g.motion(C["v"], C["w"], C["dt"], z=z)
            g.observe(blobs, fresh=True)
        want = (never.download_log_weights(),) + never.grow_download() + never.download_landmarks()
        cn = want[1]
        for g in (told, back):
            got = (g.download_log_weights(),) + g.grow_download() + g.download_landmarks()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), s
            for i in range(C["P"]):  # (beyond what a particle holds nothing was ever written)
                assert np.array_equal(got[2][i, :cn[i, 0]], want[2][i, :cn[i, 0]]) and np.array_equal(got[3][i, :cn[i, 1]], want[3][i, :cn[i, 1]]), (s, i)
            for a, b in zip(got[4:], want[4:]):
                assert np.array_equal(a, b), s
        anc = never.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
        for g in (told, back):
            assert np.array_equal(g.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), s
    assert never.grow_download()[0][:, 1].max() >= 2, "nothing was triangulated"
    m, c, k = never.download_landmarks()
    made = (k[:, L0:] & lib.PK_LANDMARK_POTENTIAL) != 0
    assert made.any()
    for g in (never, told, back):
        g.close()


def test_refusals_change_nothing(lib):
    f = lib.DeviceFilter(8, 4)
    with pytest.raises(lib.PkError, match="pk_grow_enable was not called") as e:
        f.grow_init("triangulated", 0.2)
    assert e.value.status == lib.PK_ERR_STATE
    means = np.zeros((4, 5))
    means[2:, 2:] = EMPTY_COLOUR
    f.upload_map(means, np.tile(np.identity(5).reshape(25), (4, 1)))
    f.grow_enable(2, 8, 30.0)
    before = f.device_bytes() if hasattr(f, "device_bytes") else None
    f.grow_init("triangulated", 0.25)
    for mode, angle in ((2, 0.1), (-1, 0.1), (1, float("nan")), (1, -1e-9), (1, np.pi / 2 + 1e-9), (0, 2.0), (1, float("inf"))):
        with pytest.raises(lib.PkError) as e:
            f.grow_init(mode, angle)
        assert e.value.status == lib.PK_ERR_INVALID, (mode, angle)
        assert f.grow_init_mode() == ("triangulated", 0.25)
    with pytest.raises(ValueError, match="grow_init"):
        f.grow_init("nearest", 0.1)
    f.grow_init("triangulated", np.pi / 2)
    f.grow_init("triangulated", 0.0)
    assert f.grow_init_mode() == ("triangulated", 0.0)
    if before is not None:
        assert f.device_bytes() == before  # it holds no device state
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


def _facade_run(pk, steps=14, P=C["P"], **kw):
    world, covs = gi.small_world()
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L0)]
    np.random.seed(11)
    random.seed(7)
    pk.msgs.Time.set_now(0.0)
    args = dict(num_particles=P, weight_domain="log", rng="global", new_landmarks=True, spare_landmarks=C["spare"], device=0,
                measurement_model="bearing")
    args.update(kw)
    fs = pk.FastSLAM(feats, **args)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = C["v"], C["w"]
    fs.last_control = tw
    pose = (0.0, 0.0, 0.0)
    for s in range(steps):
        pose = truth_step(pose, C["v"], C["w"], C["dt"])
        pk.msgs.Time.set_now(C["dt"] * (s + 1))
        fs.cam_cb(_View(pk, wrapped_scan(world, pose)))
    return fs, feats


def test_facade_device_and_host_bookkeeping_agree_and_the_snapshot_carries_the_rule(lib, tmp_path):
    import parakeet_slam_amd as pk

    kw = dict(landmark_init="triangulated", min_parallax=0.1)
    fd, feats = _facade_run(pk, **kw)
    assert fd._filter.grow_init_mode() == ("triangulated", 0.1)
    fh, _ = _facade_run(pk, bookkeeping="host", **kw)
    pd, ph = str(tmp_path / "device.npz"), str(tmp_path / "host.npz")
    fd.save_state(pd)
    fh.save_state(ph)
    a, b = np.load(pd), np.load(ph)
    assert str(a["landmark_init"]) == "triangulated" and float(a["min_parallax"]) == 0.1
    assert set(a.files) == set(b.files)
    # (the host path takes its sines and cosines from libm, the kernel from the device library: an ulp or two apart)
    for k in ("nl_offsets", "nl_next_id", "nl_used", "nl_slot_id", "counts", "landmark_init", "min_parallax"):
        assert np.array_equal(a[k], b[k]), k
    assert np.allclose(a["nl_readings"], b["nl_readings"], rtol=1e-12, atol=1e-12)
    assert np.allclose(a["poses"][:, :3], b["poses"][:, :3], rtol=1e-12, atol=1e-13)
    assert relerr(a["means"], b["means"]) < 1e-9 and np.allclose(a["covs"], b["covs"], rtol=1e-9, atol=1e-13)
    assert int(a["nl_used"].min()) == 3 and int(a["nl_used"].max()) == 3
    # the round trip: a filter built with the default rule takes the snapshot's; one without the fields is the reference's
    f2 = pk.FastSLAM(feats, num_particles=C["P"], weight_domain="log", rng="global", new_landmarks=True, spare_landmarks=C["spare"],
                     device=0, measurement_model="bearing")
    assert f2._filter.grow_init_mode() == ("reference", 0.0)
    f2.load_state(pd)
    assert (f2._landmark_init, f2._min_parallax) == ("triangulated", 0.1) and f2._filter.grow_init_mode() == ("triangulated", 0.1)
    p2 = str(tmp_path / "again.npz")
    f2.save_state(p2)
    c = np.load(p2)
    assert set(c.files) == set(a.files)
    for k in a.files:
        if k == "poses":  # (the weights go through log and exp on their way in and out)
            assert np.array_equal(a[k][:, :3], c[k][:, :3]) and np.allclose(a[k][:, 3], c[k][:, 3], rtol=1e-12, atol=0.0)
        elif k != "last_update":
            assert np.array_equal(a[k], c[k]), k
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, **{k: a[k] for k in a.files if k not in ("landmark_init", "min_parallax")})
    f2.load_state(bare)
    assert f2._landmark_init == "reference" and f2._filter.grow_init_mode()[0] == "reference"
    fh.load_state(bare)
    assert fh._landmark_init == "reference"
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, **dict({k: a[k] for k in a.files if k != "landmark_init"}, landmark_init=np.array("nearest")))
    with pytest.raises(ValueError, match="landmark_init='nearest'"):
        fd.load_state(bad)
    assert fd._landmark_init == "triangulated"
    for f in (fd, fh, f2):
        f.close()


def test_discovered_landmarks_carry_the_propagated_covariances(lib):
    """With the three unknown landmarks in every particle's map (one slot each, the same order in every particle),
    discovered_landmarks()' cov_within is the mean over a feature's holders of their EKFs' covariances: the propagated ones, updated
    since."""
    import parakeet_slam_amd as pk

    fs, _ = _facade_run(pk, landmark_init="triangulated", min_parallax=0.1)
    d = fs.discovered_landmarks(radius=3.0)
    m, c, k = fs._filter.download_landmarks()
    assert d.mean.shape[0] == 3 and (d.support > 0.9).all()
    ref = int(d.reference_particle)
    assert sorted(int(v) for v in d.slots) == [L0, L0 + 1, L0 + 2]
    for j, slot in enumerate(int(v) for v in d.slots):
        assert np.linalg.norm(m[:, slot, 2:] - m[0, slot, 2:], axis=1).max() < 1.0  # the same feature in every particle
        # its holders: the particles whose feature lies within the radius of the reference particle's (uniform weights behind a resample)
        holds = np.hypot(m[:, slot, 0] - m[ref, slot, 0], m[:, slot, 1] - m[ref, slot, 1]) < 3.0
        assert holds.mean() == d.support[j], (j, holds.mean(), d.support[j])
        want = c.reshape(C["P"], -1, 5, 5)[holds, slot].mean(axis=0)
        assert abs(want[0, 1]) > 1e-6  # (no identity's descendant: an EKF update of a bearing keeps a diagonal block diagonal only by accident)
        assert np.allclose(d.cov_within[j], want, rtol=1e-9, atol=1e-12), j
    fs.close()


def test_three_ranks_grow_the_same_maps_as_one_filter_under_the_rule(tmp_path):
    """FastSLAM(..., landmark_init='triangulated', devices=[0, 0, 0]) against one filter, as tests/test_gpu_grow.py does for the plain
    rule: both keywords reach every shard, the rule keeps no per-particle state, so the snapshots are equal array for array."""
    import parakeet_slam_amd as pk

    U, P, spare, steps = 3, 600, 5, 10
    v, w, dt = 0.8, 0.35, 0.5
    world, covs = synthetic_world(L0 + U)
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L0)]
    snaps = []
    for devices in ([0, 0, 0], None):
        random.seed(7)
        pk.msgs.Time.set_now(0.0)
        kw = dict(num_particles=P, weight_domain="log", rng="device", seed=3, new_landmarks=True, spare_landmarks=spare,
                  landmark_init="triangulated", min_parallax=0.1, reading_capacity=128)
        if devices:
            fs = pk.FastSLAM(feats, devices=devices, backend="gloo", **kw)
            assert isinstance(fs, pk.ShardedFastSLAM)
        else:
            fs = pk.FastSLAM(feats, device=0, **kw)
        tw = pk.msgs.Twist()
        tw.linear.x, tw.angular.z = v, w
        fs.last_control = tw
        pose = (0.0, 0.0, 0.0)
        for s in range(steps):
            pose = truth_step(pose, v, w, dt)
            pk.msgs.Time.set_now(dt * (s + 1))
            fs.cam_cb(_View(pk, synthetic_scan(world, pose)))
        path = str(tmp_path / ("grow_init_%d.npz" % len(snaps)))
        fs.save_state(path)
        snaps.append(path)
        fs.close()
    a, b = np.load(snaps[0]), np.load(snaps[1])
    assert set(a.files) == set(b.files) and str(a["landmark_init"]) == "triangulated" and float(a["min_parallax"]) == 0.1
    for k in a.files:
        if k == "poses":  # (as tests/test_gpu_grow.py: a shard's candidate lists are its own; the log-weight's terms in another order)
            assert np.array_equal(a[k][:, :3], b[k][:, :3]) and np.allclose(a[k][:, 3], b[k][:, 3], rtol=1e-11, atol=0.0), k
            continue
        assert np.array_equal(a[k], b[k]), k
    assert int(a["nl_used"].max()) >= 2, "nothing was triangulated"
    L = a["means"].shape[1]
    spare_cov = a["covs"].reshape(P, L, 5, 5)[:, L0:]
    in_use = np.arange(spare)[None, :] < a["nl_used"][:, None]
    assert (np.abs(spare_cov[in_use][:, 0, 1]) > 1e-6).any(), "no propagated covariance in the snapshot: the rule did not reach the shards"

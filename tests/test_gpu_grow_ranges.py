"""GPU: ranged scans on a growing map (pk_grow_ranges; k_new_landmarks_ranged / k_new_landmarks_tri_ranged, pk_k_grow.hip; DESIGN.md
section 9, "Single-sighting initialisation") against tests/grow_ranges_reference.py, particle by particle at every step: counters,
stored readings, slot ids, flags, counts, means, covariances, log-weights, ancestors.

Tolerances: the ones tests/test_gpu_grow_init.py holds the bearing model's growing maps to (readings 1e-12, means 1e-9 relative,
covariances rtol 1e-9 / atol 1e-13, log-weights 1e-9 absolute); the kernel alone against its closed form at 1e-12.

The scenes are tests/grow_ranges_reference.py's; tests/test_grow_ranges_reference_host.py checks each of them on the CPU for gate
margins above 1e-9, uncontested verdicts, and for what they are meant to exercise."""
import random

import numpy as np
import pytest

from oracle.fastslam_oracle import EMPTY_COLOUR, truth_step

import grow_init_reference as gi
import grow_ranges_reference as gr
from bearing_model_reference import wrapped_scan
from range_bearing_reference import range_scan
from test_gpu_grow_init import _compare, _View

pytestmark = pytest.mark.gpu

C = gi.SMALL
L0 = C["L0"]


# ---------------------------------------------------------------------------------------------------------------- helpers
def _device(lib, name, ranges=True):
    _every, _spare, retire, _phantom = gr.SCENES[name]
    means, mcov = gr.scene_map(name)
    f = lib.DeviceFilter(C["P"], len(means))
    f.set_measurement_model("bearing")
    f.upload_map(means, mcov.reshape(len(means), 25))
    f.grow_enable(L0, gr.R, C["thr"])
    if retire:
        f.grow_retire(*retire)
    f.grow_init("triangulated", gr.MIN_PARALLAX)
    if ranges is not None:
        assert f.grow_ranges_state() is False
        f.grow_ranges(ranges)
        assert f.grow_ranges_state() is bool(ranges)
    return f


def _arrays(f):
    """Everything a step leaves, rows beyond what a particle holds zeroed (nothing was ever written there)."""
    cnt, rd, sid = f.grow_download()
    rd, sid = rd.copy(), sid.copy()
    rd[np.arange(rd.shape[1])[None, :] >= cnt[:, :1]] = 0.0
    sid[np.arange(sid.shape[1])[None, :] >= cnt[:, 1:2]] = 0
    return (f.download_log_weights(), f.download_poses()[:, :3], cnt, rd, sid) + tuple(f.download_landmarks())


def _equal(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, k)


# ---------------------------------------------------------------------------------------------------------------- the scenes
@pytest.mark.parametrize("name,staged", [("all_ranged", False), ("every_3", True), ("spare_2", False), ("retiring_phantom", False)])
def test_small_scenes_against_the_oracle(lib, name, staged):
    """64 particles, 10 + 3 landmarks, 14 steps, noise-free wrapped scans with ranges: all ranged (three features at once, an empty
    ring); every third blob unranged (both rules run; through pk_stage_scan + pk_observe_staged); two spare slots (the third unknown
    is a stored reading at every step); retirement (4, 3) with a phantom ranged blob in one scan, made and gone three scans later,
    clocks included."""
    retiring = gr.SCENES[name][2] is not None
    f = _device(lib, name)
    before = f.device_bytes()
    o = gr.scene_oracle(name)
    used = []
    for st in gr.scene_drive(name, o):
        rng, var = o.last_scan
        f.motion(C["v"], C["w"], C["dt"], z=st.z)
        f.scan_ranges(rng, var)
        assert f.scan_ranges_state() == (len(rng), 0)
        if staged:
            f.stage_scan(st.blobs)
            assert f.scan_ranges_state() == (0, len(rng))
            f.observe_staged(fresh=True)
        else:
            f.observe(st.blobs, fresh=True)
        assert f.scan_ranges_state() == (0, 0)
        assert f.observe_route() == "ml_general"
        got = f.download_log_weights()
        assert np.allclose(got, st.logw, rtol=0, atol=1e-9), (st.s, np.abs(got - st.logw).max())
        assert np.array_equal(f.resample(st.u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), st.anc), st.s
        st.finish()
        _compare(lib, f, o, st.s, True, clocks=retiring)
        used.append(list(o.used))
    P = C["P"]
    if name == "all_ranged":
        assert o.used == [3] * P and (gi.promoted(o) == 3).all() and not any(o.hyp) and not o.made
    elif name == "every_3":
        assert o.used == [3] * P and (gi.promoted(o) == 3).all() and o.made and o.single and o.margin > 1e-9
    elif name == "spare_2":
        assert o.used == [2] * P and [len(h) for h in o.hyp] == [14] * P
    else:
        t0 = gr.PHANTOM_STEP
        assert used[t0 - 1] == [3] * P and used[t0] == [4] * P and used[t0 + 2] == [4] * P and used[t0 + 3] == [3] * P
        assert f.grow_clocks_download()[0][:, 3].sum() == P  # every lineage retired one feature: the phantom
    assert f.device_bytes() >= before  # (the per-scan block may grow with the first ranged scan; the mode itself holds nothing)
    f.close()


# ---------------------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("init", ["reference", "triangulated"])
def test_the_kernel_alone_at_its_smallest_shapes(lib, init):
    """5 particles (a block takes four) at poses of their own, one scan of 70 blobs (two turns of the 64-lane vote) whose colours gate
    out against every preset landmark, 3 spare slots, a ring of 1; ranges on blobs 2, 5, 65, 67 and 69, NaN elsewhere.  In scan
    order: blob 0 fills the ring, blobs 2, 5 and 65 become features (their rows the closed form's, their ids the next_ids they met),
    everything else -- the ranged blobs 67 and 69 too: no slot is free -- is counted as dropped.  Colours 3 apart and a pair
    threshold of 1 keep the two-bearing rule from pairing anything."""
    P, L0_, S, R_, B = 5, 2, 3, 1, 70
    means = np.zeros((L0_ + S, 5))
    means[:L0_] = [[30.0, 5.0, 900.0, 900.0, 900.0], [-20.0, 12.0, 900.0, 900.0, 900.0]]
    means[L0_:, 2:] = EMPTY_COLOUR
    covs = np.tile(np.identity(5).reshape(25), (L0_ + S, 1))
    f = lib.DeviceFilter(P, L0_ + S)
    f.set_measurement_model("bearing")
    f.upload_map(means, covs)
    f.grow_enable(L0_, R_, 1.0)
    f.grow_init(init, 0.1)
    f.grow_ranges(True)
    rs = np.random.RandomState(4)
    poses = np.ones((P, 4))
    poses[:, 0], poses[:, 1], poses[:, 2] = rs.uniform(-3, 3, P), rs.uniform(-3, 3, P), rs.uniform(-3, 3, P)
    f.upload_poses(poses)
    blobs = np.zeros((B, 4))
    blobs[:, 0] = rs.uniform(-3.1, 3.1, B)
    blobs[:, 1] = 10.0 + 3.0 * np.arange(B)
    blobs[:, 2], blobs[:, 3] = 20.0, 40.0
    ranged = [2, 5, 65, 67, 69]
    rho, var = np.full(B, np.nan), np.zeros(B)
    rho[ranged] = rs.uniform(2.0, 25.0, len(ranged))
    var[ranged] = (0.05 + 0.01 * rho[ranged]) ** 2
    Qt = np.diag([0.02, 0.1, 0.1, 0.1])
    f.set_measurement_noise(Qt)
    f.scan_ranges(rho, var)
    ids = f.observe(blobs, fresh=True, return_ids=True)
    assert not ids.any() and f.observe_route() == "ml_general"
    cnt, rd, sid = f.grow_download()
    assert np.array_equal(cnt, [[1, 3, L0_ + 1 + B, B - 4]] * P)
    m, c, k = f.download_landmarks()
    c = c.reshape(P, L0_ + S, 5, 5)
    for i in range(P):
        want0 = (L0_ + 1, poses[i, 0], poses[i, 1], poses[i, 2]) + tuple(blobs[0])
        assert np.allclose(rd[i, 0], want0, rtol=1e-12, atol=1e-12), i
        assert [int(v) for v in sid[i]] == [L0_ + 1 + b for b in ranged[:3]], i
        for j, b in enumerate(ranged[:3]):
            mx, my, pxx, pxy, pyy = gr.single_sighting(poses[i, 0], poses[i, 1], poses[i, 2], blobs[b, 0], rho[b], var[b], Qt[0, 0])
            assert np.allclose(m[i, L0_ + j], (mx, my) + tuple(blobs[b, 1:]), rtol=1e-12, atol=1e-12), (i, j)
            want = np.identity(5)
            want[0, 0], want[0, 1], want[1, 0], want[1, 1] = pxx, pxy, pxy, pyy
            assert np.allclose(c[i, L0_ + j], want, rtol=1e-12, atol=1e-12), (i, j)
            assert k[i, L0_ + j] == lib.PK_LANDMARK_POTENTIAL
    assert np.array_equal(m[:, :L0_], np.broadcast_to(means[:L0_], (P, L0_, 5))) and not k[:, :L0_].any()
    f.close()


# ---------------------------------------------------------------------------------------------------------------- off means off
def test_the_mode_on_without_a_finite_range_is_a_filter_never_told(lib):
    """The all-ranged scene's drive with no ranges at all: a filter that never called pk_grow_ranges, one with the mode on, and one
    with the mode on whose every scan arms ranges that are all NaN -- every array equal, bit for bit, over the 14 steps."""
    name = "all_ranged"
    never, on, nan = _device(lib, name, ranges=None), _device(lib, name), _device(lib, name)
    world, _ = gi.small_world()
    rs = np.random.RandomState(5)
    pose = (0.0, 0.0, 0.0)
    for s in range(C["steps"]):
        pose = truth_step(pose, C["v"], C["w"], C["dt"])
        blobs = wrapped_scan(world, pose)
        z, u = rs.standard_normal((C["P"], 3)), float(rs.uniform())
        nan.scan_ranges(np.full(len(blobs), np.nan), np.zeros(len(blobs)))
        for g in (never, on, nan):
            g.motion(C["v"], C["w"], C["dt"], z=z)
            g.observe(blobs, fresh=True)
        want = _arrays(never)
        _equal(want, _arrays(on), ("on", s))
        _equal(want, _arrays(nan), ("nan", s))
        anc = never.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
        for g in (on, nan):
            assert np.array_equal(g.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), s
    cnt = never.grow_download()[0]
    assert cnt[:, 1].min() >= 1 and cnt[:, 0].max() >= 1, "the bookkeeping had nothing to do"
    for g in (never, on, nan):
        g.close()


def test_the_step_consumes_the_ranges_as_the_observe_does(lib):
    """pk_step against pk_motion + pk_observe_fresh + pk_resample on the every-third scene: every array equal over 5 steps."""
    name = "every_3"
    a, b = _device(lib, name), _device(lib, name)
    world, _ = gi.small_world()
    rs = np.random.RandomState(5)
    pose = (0.0, 0.0, 0.0)
    for s in range(5):
        pose = truth_step(pose, C["v"], C["w"], C["dt"])
        blobs, rng, var = gr.scene_scan(name, world, pose, s)
        z, u = rs.standard_normal((C["P"], 3)), float(rs.uniform())
        a.motion(C["v"], C["w"], C["dt"], z=z)
        a.scan_ranges(rng, var)
        a.observe(blobs, fresh=True)
        a.resample(u, domain=lib.PK_WEIGHTS_LOG)
        b.scan_ranges(rng, var)
        b.step(C["v"], C["w"], C["dt"], blobs, u, z=z, domain=lib.PK_WEIGHTS_LOG)
        assert b.scan_ranges_state() == (0, 0)
        _equal(_arrays(a), _arrays(b), s)
    assert a.grow_download()[0][:, 1].min() >= 2
    a.close()
    b.close()


def test_switching_and_refusals_change_nothing(lib):
    f = lib.DeviceFilter(8, 4)
    with pytest.raises(lib.PkError, match="pk_grow_enable was not called") as e:
        f.grow_ranges(True)
    assert e.value.status == lib.PK_ERR_STATE and f.grow_ranges_state() is False
    f.close()
    name = "all_ranged"
    f = _device(lib, name, ranges=None)
    bytes_before = f.device_bytes()
    f.grow_ranges(True)
    for bad in (2, -1):
        with pytest.raises(lib.PkError) as e:
            f.grow_ranges(bad)
        assert e.value.status == lib.PK_ERR_INVALID and f.grow_ranges_state() is True
    f.grow_ranges(0)
    assert f.grow_ranges_state() is False
    f.grow_ranges(1)
    assert f.grow_ranges_state() is True and f.device_bytes() == bytes_before  # it holds no device state
    world, _ = gi.small_world()
    pose = truth_step((0.0, 0.0, 0.0), C["v"], C["w"], C["dt"])
    blobs, rng, var = gr.scene_scan(name, world, pose, 0)
    f.scan_ranges(rng, var)
    f.observe(blobs, fresh=True)  # taken
    before = _arrays(f)
    assert before[2][:, 1].min() == 3

    def refused(call, status, text):
        f.scan_ranges(rng, var)
        with pytest.raises(lib.PkError, match=text) as e:
            call()
        assert e.value.status == status and f.scan_ranges_state() == (0, 0)  # refused, and the ranges are gone
        _equal(before, _arrays(f), text)

    # on, the other refusals stay, in their order: the number of blobs, then the model
    refused(lambda: f.observe(blobs[:5]), lib.PK_ERR_INVALID, "this one has 5")
    f.set_measurement_model("reference")
    refused(lambda: f.observe(blobs), lib.PK_ERR_UNSUPPORTED, "option of the bearing model")
    f.set_measurement_model("bearing")
    # the proposal refuses growing maps as ever, with ranges in the proposal too
    f.proposal_ranges(True)
    refused(lambda: f.propose(C["v"], C["w"], C["dt"], blobs, seed=1), lib.PK_ERR_UNSUPPORTED, "measurement-informed proposal has no kernel for growing maps")
    f.proposal_ranges(False)
    # on, then off: the refusal as it was, for armed ranges and for a scan staged while the mode was on
    f.grow_ranges(False)
    for call in (lambda: f.observe(blobs), lambda: f.step(C["v"], C["w"], C["dt"], blobs, 0.5, seed=1), lambda: f.stage_scan(blobs)):
        refused(call, lib.PK_ERR_UNSUPPORTED, "no kernel for growing maps")
    f.grow_ranges(True)
    f.scan_ranges(rng, var)
    f.stage_scan(blobs)
    f.grow_ranges(False)
    with pytest.raises(lib.PkError, match="no kernel for growing maps"):
        f.observe_staged(fresh=True)
    assert f.scan_ranges_state() == (0, 0)
    _equal(before, _arrays(f), "staged")
    f.close()


# ---------------------------------------------------------------------------------------------------------------- the facade
def _facade(pk, **kw):
    world, covs = gi.small_world()
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L0)]
    args = dict(num_particles=C["P"], weight_domain="log", rng="global", new_landmarks=True, spare_landmarks=C["spare"], device=0,
                measurement_model="bearing", landmark_init="triangulated", min_parallax=gr.MIN_PARALLAX, range_noise=gr.SIGMA,
                grow_ranges=True)
    args.update(kw)
    return pk.FastSLAM(feats, **args), feats


def test_facade_agrees_with_the_device_filter_driven_by_hand_and_the_snapshot_carries_the_flag(lib, tmp_path):
    import parakeet_slam_amd as pk

    name = "all_ranged"
    world, _ = gi.small_world()
    np.random.seed(11)
    random.seed(7)
    pk.msgs.Time.set_now(0.0)
    fs, feats = _facade(pk)
    assert fs._filter.grow_ranges_state() is True and fs._filter.grow_init_mode() == ("triangulated", gr.MIN_PARALLAX)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = C["v"], C["w"]
    fs.last_control = tw
    f = _device(lib, name)
    f.set_measurement_noise(fs.Qt)
    rs, pr = np.random.RandomState(11), random.Random(7)
    pose = (0.0, 0.0, 0.0)
    for s in range(C["steps"]):
        pose = truth_step(pose, C["v"], C["w"], C["dt"])
        blobs = wrapped_scan(world, pose)
        rho, _ = range_scan(world, pose, None, gr.SIGMA[0], gr.SIGMA[1])
        pk.msgs.Time.set_now(C["dt"] * (s + 1))
        view = _View(pk, blobs)
        view.last_sensor_reading.observes = np.concatenate([blobs, rho[:, None]], axis=1)  # a (B, 5) scan
        fs.cam_cb(view)
        z, u = rs.standard_normal((C["P"], 3)), pr.random()
        sig = gr.SIGMA[0] + gr.SIGMA[1] * rho
        f.motion(C["v"], C["w"], C["dt"], z=z)
        f.scan_ranges(rho, sig * sig)
        f.observe(blobs, fresh=True)
        f.resample(u, domain=lib.PK_WEIGHTS_LOG)
        assert fs._filter.observe_route() == "ml_general"
        _equal(_arrays(f), _arrays(fs._filter), s)
    d = fs.discovered_landmarks(radius=3.0)
    assert d.mean.shape[0] == 3 and sorted(int(v) for v in d.slots) == [L0, L0 + 1, L0 + 2]
    # one per unknown landmark: the scans' colours are noise-free, so each feature holds its landmark's colour
    seen = sorted(int(np.argmin(np.linalg.norm(world[L0:, 2:] - d.mean[j, 2:5], axis=1))) for j in range(3))
    assert seen == [0, 1, 2] and all(np.linalg.norm(world[L0:, 2:] - d.mean[j, 2:5], axis=1).min() < 1e-6 for j in range(3))
    # the snapshot carries the flag; one without it restores as off
    path = str(tmp_path / "ranged.npz")
    fs.save_state(path)
    a = np.load(path)
    assert bool(a["grow_ranges"]) is True
    np.random.seed(11)
    f2, _ = _facade(pk, grow_ranges=False, range_noise=None)
    with pytest.raises(ValueError, match="grow_ranges=True"):
        f2.load_state(path)
    f2.close()
    f3, _ = _facade(pk)
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, **{k: a[k] for k in a.files if k != "grow_ranges"})
    f3.load_state(bare)
    assert f3._grow_ranges is False and f3._filter.grow_ranges_state() is False
    f3.load_state(path)
    assert f3._grow_ranges is True and f3._filter.grow_ranges_state() is True
    _equal(_arrays(fs._filter)[1:], _arrays(f3._filter)[1:], "restored")  # (the weights go through exp and log on their way)
    again = str(tmp_path / "again.npz")
    f3.save_state(again)
    assert bool(np.load(again)["grow_ranges"]) is True
    f.close()
    fs.close()
    f3.close()


def test_facade_refusals(lib):
    import parakeet_slam_amd as pk

    # (the default landmark_init: with new_landmarks=False "triangulated" has a refusal of its own, which comes first)
    for kw in (dict(range_noise=None), dict(new_landmarks=False), dict(spare_landmarks=0), dict(bookkeeping="host"),
               dict(proposal="measurement")):
        with pytest.raises(ValueError, match="grow_ranges=True"):
            _facade(pk, landmark_init="reference", **kw)
    with pytest.raises(ValueError, match="new_landmarks=True"):  # without the keyword: the refusal as it was
        _facade(pk, grow_ranges=False)

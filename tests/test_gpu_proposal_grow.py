"""GPU: the measurement-informed proposal on growing maps (pk_proposal_grow with pk_propose / pk_propose_odom on a filter with
pk_grow_enable / pk_grow_retire / pk_grow_ranges; DESIGN.md section 4, "The proposal on growing maps") against
tests/proposal_grow_reference.py, particle by particle at every step.

Tolerances: none is stated here.  The step's own results (xi, the weight increments, `used`, poses, log-weights, landmarks) go
through tests/test_gpu_range_proposal.py's comparison (its tp._compare_step: xi, increments and log-weights 1e-9 absolute, poses
rtol 1e-12 and the pose invariant bit for bit, means 1e-9 relative, covariances rtol 1e-9 / atol 1e-13, ids and `used` exactly,
cond_2(Lambda) <= 1e4 asserted first); the bookkeeping (the ring, the four counters, the slot ids, the clocks, flags and counts)
goes through tests/test_gpu_grow_ranges.py's (its _compare: readings 1e-12, the rest exactly).  Before ids are compared exactly the
reference's own margins are asserted (assert_margins of tests/test_gpu_range_bearing.py); tests/test_proposal_grow_host.py runs that
check on every scene here without a GPU.

Shapes: the scenes are 64 particles x (10 + 5 or 10 + 2) landmarks, 13 or 14 blobs -- one workgroup per particle in k_propose and
k_observe_proposed, sixteen blocks of four particles in k_new_landmarks; 67 particles leave that kernel's last block partly empty
and the particle count off a multiple of the wave."""
import random

import numpy as np
import pytest

from oracle.fastslam_oracle import truth_step

import grow_init_reference as gi
import grow_ranges_reference as gr
import proposal_grow_reference as pg
import proposal_reference as pr
import test_gpu_grow_ranges as tgr
import test_gpu_range_proposal as trp
from bearing_model_reference import wrapped_scan
from range_bearing_reference import range_scan
from test_gpu_range_bearing import assert_margins

pytestmark = pytest.mark.gpu

tp = trp.tp  # tests/test_gpu_proposal.py's helpers, as tests/test_gpu_range_proposal.py uses them
C = gi.SMALL
L0 = C["L0"]
V, W, DT = C["v"], C["w"], C["dt"]
PARTIAL = ("all_ranged", "twist", 67, 4)


def oracle_scenes():
    """Every run of this file that is held to the oracle, as (scene, motion, particles or None, steps or None): what
    tests/test_proposal_grow_host.py checks the margins of."""
    for name in pg.RANGED + pg.UNRANGED:
        for motion in pg.MOTIONS:
            yield name, motion, None, None
    yield PARTIAL


# ---------------------------------------------------------------------------------------------------------------- helpers
def _device(lib, name, P=None, grow=True, proposal_ranges=None, grow_ranges=None):
    spare, R, retire, mp = pg.scene_shape(name)
    ranged = name in pg.RANGED
    means, mcov = pg.scene_map(name)
    f = lib.DeviceFilter(C["P"] if P is None else P, len(means))
    f.set_measurement_model("bearing")
    f.upload_map(means, mcov.reshape(len(means), 25))
    f.grow_enable(L0, R, C["thr"])
    if retire:
        f.grow_retire(*retire)
    f.grow_init("triangulated", mp)
    if ranged if grow_ranges is None else grow_ranges:
        f.grow_ranges(True)
    if ranged if proposal_ranges is None else proposal_ranges:
        f.proposal_ranges(True)
    assert f.proposal_grow_state() is False  # the default
    if grow:
        f.proposal_grow(True)
        assert f.proposal_grow_state() is True
    return f


def _twin(lib, name, P=None):
    """A filter of the scene's shape that only ever moves: the pose invariant's."""
    means, mcov = pg.scene_map(name)
    P = C["P"] if P is None else P
    return tp._device(lib, P, means, mcov, np.zeros((P, 3)))


def _step(f, st, **kw):
    if st.rng is not None:
        f.scan_ranges(st.rng, st.var)
    return tp._propose(f, st.control, st.blobs, fresh=True, **kw)


def _everything(f, clocks=False):
    out = tgr._arrays(f) + tuple(f.proposal_download())
    if clocks:
        kc, sc, se, si, now = f.grow_clocks_download()
        cnt = out[2]
        sc, se, si = sc.copy(), se.copy(), si.copy()
        sc[np.arange(sc.shape[1])[None, :] >= cnt[:, :1]] = 0
        se[np.arange(se.shape[1])[None, :] >= cnt[:, 1:2]] = 0
        si[np.arange(si.shape[1])[None, :] >= cnt[:, 1:2]] = 0
        out += (kc, sc, se, si, np.array(now))
    return out


def _against_the_oracle(lib, name, motion, P=None, steps=None):
    retiring = pg.scene_shape(name)[2] is not None
    f, twin, o = _device(lib, name, P), _twin(lib, name, P), pg.scene_oracle(name, P=P)
    before = f.device_bytes()
    for st in pg.drive(name, o, motion, steps=steps):
        what = (name, motion, st.s)
        assert_margins(o.f, what)
        twin.upload_poses(f.download_poses())
        got = _step(f, st, z=st.z, return_ids=True)
        assert np.array_equal(got, st.ids), (what, int((got != st.ids).sum()))
        assert f.observe_route() == "ml_general" and f.scan_ranges_state() == (0, 0)
        tp._compare_step(lib, f, o.f, what, twin, st.control)
        assert np.array_equal(f.resample(st.u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), st.anc), what
        st.finish()
        tgr._compare(lib, f, o, what, True, clocks=retiring)
    assert f.device_bytes() >= before  # (the scan's buffers and the proposal's 84 P bytes; the mode itself holds nothing)
    f.close()
    twin.close()
    return o


# ---------------------------------------------------------------------------------------------------------------- the scenes
@pytest.mark.parametrize("motion", pg.MOTIONS)
@pytest.mark.parametrize("name", pg.RANGED)
def test_ranged_scenes_against_the_oracle(lib, name, motion):
    """grow_ranges_reference's four scenes under both motion models, pk_resample between the steps: all blobs ranged (three features
    at once, at the SAMPLED pose), every third blob unranged (both rules), two spare slots (a stored reading at every step),
    retirement (4, 3) with a phantom made in one scan and gone three scans later, clocks included."""
    o = _against_the_oracle(lib, name, motion)
    P, spare = C["P"], pg.scene_shape(name)[0]
    assert o.used == [min(3, spare)] * P and (gi.promoted(o) == min(3, spare)).all()
    if name == "all_ranged":
        assert len(o.single) == 3 * P and not o.made and not any(o.hyp)
    elif name == "every_3":
        assert o.made and o.single
    elif name == "spare_2":
        assert [len(h) for h in o.hyp] == [C["steps"]] * P
    else:
        assert sum(o.features_retired) == P


@pytest.mark.parametrize("motion", pg.MOTIONS)
@pytest.mark.parametrize("name", pg.UNRANGED)
def test_unranged_triangulated_scenes_against_the_oracle(lib, name, motion):
    """grow_init_reference's bearing_0.1 and bearing_0.1_retiring: no ranges anywhere -- k_propose, k_observe_proposed and
    k_new_landmarks_tri at the sampled poses, with the retirement pass behind them."""
    o = _against_the_oracle(lib, name, motion)
    assert o.used == [3] * C["P"] and (gi.promoted(o) == 3).all() and o.made and not o.single
    if pg.scene_shape(name)[2]:
        assert sum(o.readings_retired) > 0


def test_a_last_workgroup_that_is_not_full(lib):
    """67 particles: k_new_landmarks' blocks take four, so the last holds three; 67 is off every multiple of the wave."""
    name, motion, P, steps = PARTIAL
    o = _against_the_oracle(lib, name, motion, P, steps)
    assert o.used == [3] * P and (gi.promoted(o) == 3).all()


# ---------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("motion", pg.MOTIONS)
def test_the_same_bits_every_run(lib, motion):
    """Two filters, the same calls, the step's own Philox normals (no z supplied): every array equal after every step."""
    name = "retiring_phantom"
    world, _ = gi.small_world()
    a, b = _device(lib, name), _device(lib, name)
    rs = np.random.RandomState(9)
    pose = (0.0, 0.0, 0.0)
    for s in range(6):
        prev, pose = pose, truth_step(pose, V, W, DT)
        blobs, rng, var = pg.scene_scan(name, world, pose, s)
        control, u = pg.control_of(motion, prev, pose), float(rs.uniform())
        for g in (a, b):
            g.scan_ranges(rng, var)
            tp._propose(g, control, blobs, seed=77, draw=s, fresh=True)
        tgr._equal(_everything(a, clocks=True), _everything(b, clocks=True), (motion, s))
        anc = a.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
        assert np.array_equal(b.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc)
    cnt = a.grow_download()[0]
    assert cnt[:, 1].min() >= 3 and a.grow_clocks_download()[4] == 6
    a.close()
    b.close()


def test_the_mode_on_a_preset_map_is_the_mode_off(lib):
    """A filter that does not grow: pk_proposal_grow changes no bit of a step -- ranged scans, both motion models, maximum-likelihood
    and supplied ids -- nor pk_device_bytes, nor the route."""
    L, B, P = 65, 12, 16
    world, covs, xyh, sees, rows = trp.shape_scene(L, B, P, "mixed", 2)
    for name, control in sorted(tp._controls().items()):
        for ids in (None, trp.supplied_ids(sees, B)):
            out = []
            for on in (False, True):
                f = trp._device(lib, P, world, covs, xyh)
                held = f.device_bytes()
                f.proposal_grow(on)
                assert f.proposal_grow_state() is on and f.device_bytes() == held
                for s, (blobs, rho, var, z) in enumerate(rows):
                    trp._propose(f, control, blobs, rho, var, z=z, ids=ids, fresh=s == 0)
                out.append(trp._everything(f) + (np.array(f.device_bytes()), np.array(f.observe_route())))
                f.close()
            tgr._equal(out[0], out[1], (name, ids is None))


# ---------------------------------------------------------------------------------------------------------------- refusals
def _scan(name, step=0):
    world, _ = gi.small_world()
    return pg.scene_scan(name, world, truth_step((0.0, 0.0, 0.0), V, W, DT), step)


def _refused(lib, f, blobs, rng, var, status, text, before, **kw):
    for call in (lambda: f.propose(V, W, DT, blobs, seed=1, **kw), lambda: f.propose_odom(tp.DELTA, tp.ALPHAS, blobs, seed=1, **kw)):
        if rng is not None:
            f.scan_ranges(rng, var)
            assert f.scan_ranges_state() == (len(rng), 0)
        with pytest.raises(lib.PkError) as e:
            call()
        assert e.value.status == status and text in str(e.value), str(e.value)
        assert f.scan_ranges_state() == (0, 0)  # refused, and the ranges are gone
        tgr._equal(before, tgr._arrays(f), text)


def test_the_mode_off_refuses_a_growing_filter_as_ever(lib):
    name = "retiring_phantom"
    blobs, rng, var = _scan(name)
    text = "measurement-informed proposal has no kernel for growing maps"
    f = _device(lib, name, grow=False)
    f.scan_ranges(rng, var)
    f.observe(blobs, fresh=True)  # (a state worth comparing: three features made)
    before = tgr._arrays(f)
    assert before[2][:, 1].min() == 3
    _refused(lib, f, blobs, None, None, lib.PK_ERR_UNSUPPORTED, text, before)
    _refused(lib, f, blobs, rng, var, lib.PK_ERR_UNSUPPORTED, text, before)
    f.grow_retire(0, 0)  # growing without retirement: the same clause
    _refused(lib, f, blobs, None, None, lib.PK_ERR_UNSUPPORTED, text, before)
    for bad in (2, -1):  # the switch takes 0 or 1 and nothing else
        with pytest.raises(lib.PkError) as e:
            f.proposal_grow(bad)
        assert e.value.status == lib.PK_ERR_INVALID and f.proposal_grow_state() is False
    f.proposal_grow(1)
    f.proposal_grow(0)  # on, then off: refused as ever
    _refused(lib, f, blobs, None, None, lib.PK_ERR_UNSUPPORTED, text, before)
    f.close()


def test_refusals_with_the_mode_on_carry_their_status_and_text_and_change_nothing(lib):
    name = "all_ranged"
    blobs, rng, var = _scan(name)
    B = len(blobs)
    ids = np.zeros(B, dtype=np.int32)
    ids[:L0] = np.arange(1, L0 + 1)
    f = _device(lib, name)
    f.scan_ranges(rng, var)
    tp._propose(f, pr.twist(V, W, DT), blobs, seed=1, fresh=True)  # taken: three features made
    before = tgr._arrays(f)
    assert before[2][:, 1].min() == 3
    # supplied ids: the bookkeeping follows the maximum-likelihood association, in pk_observe's words -- with and without ranges
    _refused(lib, f, blobs, None, None, lib.PK_ERR_STATE, "follows the maximum-likelihood association: no ids", before, ids=ids)
    _refused(lib, f, blobs, rng, var, lib.PK_ERR_STATE, "follows the maximum-likelihood association: no ids", before, ids=ids)
    # the ranges' own refusals come first: the number of blobs, then (below) the two modes they need
    _refused(lib, f, blobs, rng[:5], var[:5], lib.PK_ERR_INVALID, "named the ranges of a scan of 5 blobs", before, ids=ids)
    f.grow_ranges(False)  # armed ranges without pk_grow_ranges: pk_scan_ranges' refusal 4
    _refused(lib, f, blobs, rng, var, lib.PK_ERR_UNSUPPORTED, "per-blob ranges (pk_scan_ranges) have no kernel for growing maps", before)
    f.grow_ranges(True)
    f.proposal_ranges(False)  # armed ranges without pk_proposal_ranges: the proposal's refusal of ranges
    _refused(lib, f, blobs, rng, var, lib.PK_ERR_UNSUPPORTED, "not part of the measurement-informed proposal", before)
    f.proposal_ranges(True)
    f.stage_scan(blobs)  # the proposal's other clauses keep their place: a staged scan in flight
    _refused(lib, f, blobs, None, None, lib.PK_ERR_STATE, "staged scan", before)
    f.close()


# ---------------------------------------------------------------------------------------------------------------- edges
def test_an_empty_scan_leaves_the_bookkeeping_and_the_retirement_clock_alone(lib):
    name = "retiring_phantom"
    f, o = _device(lib, name), pg.scene_oracle(name)
    for st in pg.drive(name, o, "twist", steps=3):
        _step(f, st, z=st.z)
        f.resample(st.u, domain=lib.PK_WEIGHTS_LOG)
    tgr._compare(lib, f, o, "before", True, clocks=True)
    grow, clocks = f.grow_download(), f.grow_clocks_download()
    assert clocks[4] == 3
    z = np.random.RandomState(3).standard_normal((C["P"], 3))
    control = pr.twist(V, W, DT)
    o.propose(control, z, np.zeros((0, 4)))
    got = tp._propose(f, control, np.zeros((0, 4)), z=z, return_ids=True, fresh=True)
    assert got.shape == (C["P"], 0)
    xi, dl, used = f.proposal_download()
    assert np.array_equal(xi, z) and not dl.any() and not used.any()
    tgr._equal(grow, f.grow_download(), "bookkeeping")
    for a, b in zip(clocks, f.grow_clocks_download()):
        assert np.array_equal(a, b)
    tp._compare_step(lib, f, o.f, "empty scan")
    tgr._compare(lib, f, o, "after", True, clocks=True)
    f.close()


def test_the_mode_holds_no_device_memory(lib):
    """Switching it on and off leaves pk_device_bytes where it was, and a ranged proposal step on a growing filter holds what the
    plain growing observe of that scan holds plus the proposal's 84 P bytes."""
    name = "all_ranged"
    blobs, rng, var = _scan(name)
    P = C["P"]
    g = _device(lib, name, grow=False)
    g.scan_ranges(rng, var)
    g.observe(blobs, fresh=True)
    held = g.device_bytes()
    g.close()
    f = _device(lib, name, grow=False)
    b0 = f.device_bytes()
    f.proposal_grow(True)
    assert f.device_bytes() == b0
    for control in (pr.twist(V, W, DT), pr.odom(tp.DELTA, tp.ALPHAS)):
        f.scan_ranges(rng, var)
        tp._propose(f, control, blobs, seed=1, fresh=True)
        assert f.device_bytes() == held + 84 * P
    f.proposal_grow(False)
    assert f.device_bytes() == held + 84 * P
    f.close()


# ---------------------------------------------------------------------------------------------------------------- the facade
@pytest.mark.parametrize("motion", pg.MOTIONS)
def test_facade_agrees_with_the_device_filter_driven_by_hand(lib, motion):
    """cam_cb with proposal_grow=True on (B, 5) scans against pk_scan_ranges + pk_propose / pk_propose_odom + pk_resample by hand,
    array for array at every step; then discovered_landmarks() yields the three unknown landmarks."""
    import parakeet_slam_amd as pk
    from parakeet_slam_amd.core import _make_state

    name = "all_ranged"
    world, covs = gi.small_world()
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L0)]
    np.random.seed(11)
    random.seed(7)
    pk.msgs.Time.set_now(0.0)
    kw = dict(motion="odometry", odom_alphas=pg.ALPHAS) if motion == "odometry" else {}
    fs = pk.FastSLAM(feats, num_particles=C["P"], weight_domain="log", rng="global", new_landmarks=True, spare_landmarks=C["spare"],
                     device=0, measurement_model="bearing", landmark_init="triangulated", min_parallax=gr.MIN_PARALLAX,
                     range_noise=gr.SIGMA, grow_ranges=True, proposal="measurement", proposal_ranges=True, proposal_grow=True, **kw)
    assert fs._filter.proposal_grow_state() and fs._filter.proposal_ranges_state() and fs._filter.grow_ranges_state()
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = V, W
    fs.last_control = tw
    f = _device(lib, name)
    f.set_measurement_noise(fs.Qt)
    rs, prn = np.random.RandomState(11), random.Random(7)
    pose = (0.0, 0.0, 0.0)
    if motion == "odometry":
        fs.odom_motion_update(_make_state(*pose))
    for s in range(C["steps"]):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world, pose)
        rho, _ = range_scan(world, pose, None, gr.SIGMA[0], gr.SIGMA[1])
        sig = gr.SIGMA[0] + gr.SIGMA[1] * rho
        pk.msgs.Time.set_now(DT * (s + 1))
        delta = None
        if motion == "odometry":
            fs.odom_motion_update(_make_state(*pose))
            delta = lib.odom_delta(fs._odom_applied, fs._odom_prev, fs._odom_min_trans)  # what cam_cb is about to move by
        view = tgr._View(pk, blobs)
        view.last_sensor_reading.observes = np.concatenate([blobs, rho[:, None]], axis=1)  # a (B, 5) scan
        fs.cam_cb(view)
        z, u = rs.standard_normal((C["P"], 3)), prn.random()
        f.scan_ranges(rho, sig * sig)
        if delta is None:
            f.propose(V, W, DT, blobs, z=z, fresh=True)
        else:
            f.propose_odom(delta, pg.ALPHAS, blobs, z=z, fresh=True)
        f.resample(u, domain=lib.PK_WEIGHTS_LOG)
        assert fs._filter.observe_route() == "ml_general"
        tgr._equal(tgr._arrays(f), tgr._arrays(fs._filter), (motion, s))
    d = fs.discovered_landmarks(radius=3.0)
    assert d.mean.shape[0] == 3 and sorted(int(v) for v in d.slots) == [L0, L0 + 1, L0 + 2]
    # one per unknown landmark: the scans' colours are noise-free, so each feature holds its landmark's colour
    seen = sorted(int(np.argmin(np.linalg.norm(world[L0:, 2:] - d.mean[j, 2:5], axis=1))) for j in range(3))
    assert seen == [0, 1, 2] and all(np.linalg.norm(world[L0:, 2:] - d.mean[j, 2:5], axis=1).min() < 1e-6 for j in range(3))
    f.close()
    fs.close()


def test_facade_odometry_scan_without_new_odometry_is_the_plain_growing_observe(lib):
    """Odometry mode, two scans on one odometry message: the second moves nothing and is pk_observe on the growing filter -- the
    bookkeeping and all -- array for array."""
    import parakeet_slam_amd as pk
    from parakeet_slam_amd.core import _make_state

    name = "all_ranged"
    world, covs = gi.small_world()
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L0)]
    np.random.seed(11)
    random.seed(7)
    pk.msgs.Time.set_now(0.0)
    fs = pk.FastSLAM(feats, num_particles=C["P"], weight_domain="log", rng="global", new_landmarks=True, spare_landmarks=C["spare"],
                     device=0, measurement_model="bearing", landmark_init="triangulated", min_parallax=gr.MIN_PARALLAX,
                     range_noise=gr.SIGMA, grow_ranges=True, proposal="measurement", proposal_ranges=True, proposal_grow=True,
                     motion="odometry", odom_alphas=pg.ALPHAS)
    f = _device(lib, name)
    f.set_measurement_noise(fs.Qt)
    rs, prn = np.random.RandomState(11), random.Random(7)
    start = (0.0, 0.0, 0.0)
    pose = truth_step(start, V, W, DT)
    fs.odom_motion_update(_make_state(*start))
    fs.odom_motion_update(_make_state(*pose))
    delta = lib.odom_delta(fs._odom_applied, fs._odom_prev, fs._odom_min_trans)
    blobs = wrapped_scan(world, pose)
    rho, _ = range_scan(world, pose, None, gr.SIGMA[0], gr.SIGMA[1])
    sig = gr.SIGMA[0] + gr.SIGMA[1] * rho
    view = tgr._View(pk, blobs)
    view.last_sensor_reading.observes = np.concatenate([blobs, rho[:, None]], axis=1)
    for s in range(2):
        pk.msgs.Time.set_now(DT * (s + 1))
        fs.cam_cb(view)
        f.scan_ranges(rho, sig * sig)
        if s == 0:
            f.propose_odom(delta, pg.ALPHAS, blobs, z=rs.standard_normal((C["P"], 3)), fresh=True)
        else:
            f.observe(blobs, fresh=True)
        f.resample(prn.random(), domain=lib.PK_WEIGHTS_LOG)
        tgr._equal(tgr._arrays(f), tgr._arrays(fs._filter), s)
    assert tgr._arrays(f)[2][:, 1].min() == 3
    f.close()
    fs.close()

"""GPU: the measurement-informed proposal (pk_propose, pk_propose_odom, pk_proposal_download; DESIGN.md section 4, "The
measurement-informed proposal") against tests/proposal_reference.py.

Tolerances: the filter tolerances of tests/test_gpu_bearing_model.py -- xi, the weight increments and the log-weights 1e-9 absolute,
poses rtol 1e-12, means 1e-9 relative, covariances rtol 1e-9 / atol 1e-13, ids and counts exactly.

Every comparison first asserts from the reference alone that cond_2(Lambda) <= 1e4 for every particle (the 3 x 3 solve loses at most
~1e-12) and, where ids are associated, that no gate is within 1e-6 of turning and no two candidates of a blob tie within 1e-6
(_safe_ml_ids says which pairs a gate's margin counts for, and why)."""
import math
import random

import numpy as np
import pytest

from conftest import relerr
from oracle.fastslam_oracle import low_variance_ancestors, synthetic_world, truth_step

import bearing_model_reference as ref
import odom_reference as odo
import proposal_reference as pr
from bearing_model_reference import BearingOracle, wrapped_scan
from proposal_reference import ProposalOracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
V, W, DT = 1.0, 0.35, 0.5
H0 = 2.9
SIGMA_B, SIGMA_C = 0.01, 0.3
ALPHAS = (0.5, 0.05, 0.05, 0.05)
DELTA = (0.0875, 0.5, 0.0875)  # one move of the turning drive as an odometry delta
LOG_LOW = math.log(0.1)


# ---------------------------------------------------------------------------------------------------------------- helpers
def _controls():
    return {"twist": pr.twist(V, W, DT), "odom": pr.odom(DELTA, ALPHAS)}


def _device(lib, P, means, covs, xyh, immutable=None, model="bearing", opts=None):
    L = len(means)
    f = lib.DeviceFilter(P, L)
    if model is not None:
        f.set_measurement_model(model)
    for k, v in (opts or {}).items():
        f.set_option(k, v)
    f.upload_map(means, np.asarray(covs).reshape(L, 25), immutable)
    xyhw = np.ones((P, 4))
    xyhw[:, :3] = xyh
    f.upload_poses(xyhw)
    return f


def _oracle(P, means, covs, xyh, immutable=None):
    o = ProposalOracle(P, means, covs, immutable=immutable)
    o.x, o.y, o.h = xyh[:, 0].copy(), xyh[:, 1].copy(), xyh[:, 2].copy()
    return o


def _poses(P, seed, heading=H0, spread=(0.05, 0.05, 0.02)):
    rs = np.random.RandomState(seed)
    xyh = rs.standard_normal((P, 3)) * np.asarray(spread)
    xyh[:, 2] += heading
    return xyh


def _propose(f, control, blobs, **kw):
    if control[0] == "twist":
        return f.propose(control[1], control[2], control[3], blobs, **kw)
    return f.propose_odom(control[1], control[2], blobs, **kw)


def _move(f, control, **kw):
    if control[0] == "twist":
        return f.motion(control[1], control[2], control[3], **kw)
    return f.motion_odom(control[1], control[2], **kw)


def _safe_ml_ids(o, control, blobs, what):
    """The maximum-likelihood ids at the predicted poses of the oracle's current state, with the scene's safety asserted: no gate
    within 1e-6 of turning and no tie between the two best candidates of a blob within 1e-6.

    A gate's margin counts for the pairs the other gate does not itself reject by more than that margin: a pair the colour gate
    rejects outright has probability 0 whatever rounding does to its bearing difference (of the 46 million pairs of 257 x 600 x
    300 some thirty lie within 1e-6 of the bearing gate whatever the seed, every one of them a colour gate apart).  The expected
    bearings are formed once for all blobs, and the probabilities -- bearing_model_reference.probability_of_match, as
    BearingOracle.associate calls it -- only for the pairs inside both gates: every other pair's is exactly 0."""
    P, B = o.P, len(blobs)
    x, y, h = pr.move(o.x, o.y, o.h, control, np.zeros((P, 3)))
    sx, sy, sh = x[:, None], y[:, None], h[:, None]
    expected = np.arctan2(o.mean[..., 1] - sy, o.mean[..., 0] - sx) - sh
    mr, mg, mbl = o.mean[..., 2], o.mean[..., 3], o.mean[..., 4]
    ids = np.zeros((P, B), dtype=np.int32)
    for b in range(B):
        delb = np.abs(ref.wrap(blobs[b, 0] - expected))
        cd = np.power(blobs[b, 1] - mr, 2) + np.power(blobs[b, 2] - mg, 2) + np.power(blobs[b, 3] - mbl, 2)
        mb, mc = np.abs(delb - 0.5), np.abs(cd - 300.0)
        colour_rejects, bearing_rejects = (cd > 300.0) & (mc > 1e-6), (delb > 0.5) & (mb > 1e-6)
        close = ((mb <= 1e-6) & ~colour_rejects) | ((mc <= 1e-6) & ~bearing_rejects)
        assert not close.any(), (what, b, "a gate within 1e-6 of turning")
        pi, li = np.nonzero((delb <= 0.5) & (cd <= 300.0))
        p = np.zeros((P, o.L))
        if len(pi):
            v = ref.probability_of_match(x[pi], y[pi], h[pi], blobs[b], o.mean[pi, li], o.cov[pi, li])
            p[pi, li] = np.where(np.isnan(v), 0.0, v)
        best = np.argmax(p, axis=1)
        top = p[np.arange(P), best]
        if len(pi):
            p[np.arange(P), best] = -1.0
            second = p.max(axis=1)
            tie = (second > 0) & (top - second <= 1e-6 * top)
            assert not tie.any(), (what, b, "a tie between two candidates")
        ids[:, b] = np.where(top > 0, best + 1, 0)
    return ids


def _assert_conditioned(o, what):
    c = np.linalg.cond(o.Lambda)
    assert c.max() <= 1e4, (what, c.max())


def _compare_state(lib, f, o, what):
    m, c, k = f.download_landmarks()
    assert np.array_equal((k & lib.PK_LANDMARK_POTENTIAL) != 0, o.potential), what
    assert np.array_equal(k & ~lib.PK_LANDMARK_POTENTIAL, o.count), what
    assert relerr(m, o.mean) < RTOL, (what, relerr(m, o.mean))
    assert np.allclose(c.reshape(o.cov.shape), o.cov, rtol=RTOL, atol=1e-13), what


def _compare_step(lib, f, o, what, twin=None, control=None, shifted=False):
    """The last proposal step of device filter f against the oracle's; twin (a filter at the poses f had before the step): moved by
    the plain motion call with the downloaded xi as its normals it stands where f does, bit for bit.  shifted: the log-weights are
    compared about their maximum (a gated call that keeps the particles leaves the carried weights shifted by a constant)."""
    _assert_conditioned(o, what)
    xi, dl, used = f.proposal_download()
    assert np.array_equal(used, o.used), (what, used, o.used)
    assert np.allclose(xi, o.xi, rtol=0, atol=RTOL), (what, np.abs(xi - o.xi).max())
    assert np.allclose(dl, o.dlogw, rtol=0, atol=RTOL), (what, np.abs(dl - o.dlogw).max())
    lw, ow = f.download_log_weights(), o.logw
    if shifted:
        lw, ow = lw - lw.max(), ow - ow.max()
    assert np.allclose(lw, ow, rtol=0, atol=RTOL), (what, np.abs(lw - ow).max())
    got = f.download_poses()
    assert np.allclose(got[:, :3], np.stack([o.x, o.y, o.h], axis=1), rtol=1e-12, atol=1e-13), what
    if twin is not None:
        _move(twin, control, z=xi)
        assert np.array_equal(twin.download_poses()[:, :3], got[:, :3]), (what, "the pose invariant")
    _compare_state(lib, f, o, what)


# ---------------------------------------------------------------------------------------------------------------- 1, 3
@pytest.mark.parametrize("P", [1, 3, 257])
@pytest.mark.parametrize("L,B", [(3, 1), (65, 13), (600, 300)])
def test_k_propose_against_the_reference(lib, P, L, B):
    """Both motion models; supplied z; maximum-likelihood ids through both association kernels, and supplied ids; two steps on the
    small shapes, so that the second gathers from maps that differ between particles.  And the pose invariant."""
    world, covs = synthetic_world(L, seed=5)
    sees = (np.arange(B) * (L // B)) % L
    xyh = _poses(P, 3)
    rs = np.random.RandomState(100 * L + P)
    steps = 2 if L < 600 else 1
    for name, control in sorted(_controls().items()):
        fs = {"grid": _device(lib, P, world, covs, xyh), "brute": _device(lib, P, world, covs, xyh, opts={"assoc_kernel": 1}),
              "ids": _device(lib, P, world, covs, xyh)}
        twin = _device(lib, P, world, covs, xyh)
        o_ml, o_ids = _oracle(P, world, covs, xyh), _oracle(P, world, covs, xyh)
        pose = (0.0, 0.0, H0)
        for s in range(steps):
            pose = truth_step(pose, V, W, DT)
            blobs = wrapped_scan(world[sees], pose, rs, SIGMA_B, SIGMA_C)
            z = rs.standard_normal((P, 3))
            what = (name, P, L, B, s)
            want = _safe_ml_ids(o_ml, control, blobs, what)
            o_ml.propose(control, z, blobs, ids=want)
            for kind in ("grid", "brute"):
                twin.upload_poses(fs[kind].download_poses())
                got = _propose(fs[kind], control, blobs, z=z, return_ids=True, fresh=True)
                assert np.array_equal(got, want), (what, kind, int((got != want).sum()))
                assert fs[kind].observe_route() == "ml_general"
                _compare_step(lib, fs[kind], o_ml, what + (kind,), twin, control)
            supplied = (sees + 1).astype(np.int32)
            if B > 1:
                supplied[1] = 0            # an unmatched blob
                supplied[2] = supplied[3]  # and a landmark seen twice
            o_ids.propose(control, z, blobs, ids=supplied)
            twin.upload_poses(fs["ids"].download_poses())
            got = _propose(fs["ids"], control, blobs, z=z, ids=supplied, return_ids=True, fresh=True)
            assert np.array_equal(got, np.broadcast_to(supplied, (P, B)))
            assert fs["ids"].observe_route() == "known_ids"
            _compare_step(lib, fs["ids"], o_ids, what + ("ids",), twin, control)
        for g in list(fs.values()) + [twin]:
            g.close()


def test_k_propose_walks_more_particles_than_its_grid(lib):
    """launch_propose caps the grid at 16 384 workgroups and walks the particles with a grid stride: 20 000 particles, so that some
    workgroups take a second particle, against the oracle and against pk_motion_odom with xi as its normals."""
    P, L = 20000, 3
    world, covs = synthetic_world(L, seed=5)
    xyh = _poses(P, 13)
    rs = np.random.RandomState(14)
    control = _controls()["odom"]
    blobs = wrapped_scan(world[:2], truth_step((0.0, 0.0, H0), V, W, DT), rs, SIGMA_B, SIGMA_C)
    z = rs.standard_normal((P, 3))
    f, twin, o = _device(lib, P, world, covs, xyh), _device(lib, P, world, covs, xyh), _oracle(P, world, covs, xyh)
    want = _safe_ml_ids(o, control, blobs, "grid stride")
    o.propose(control, z, blobs, ids=want)
    got = _propose(f, control, blobs, z=z, return_ids=True, fresh=True)
    assert np.array_equal(got, want) and (o.used == 2).all()
    _compare_step(lib, f, o, "grid stride", twin, control)
    f.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def _edge(lib, control, world, covs, xyh, blobs, ids, what, immutable=None, potential=None, ml=False):
    """One hand-built step, supplied ids (ml: the association must find the same), against the oracle."""
    P, L = len(xyh), len(world)
    f, twin = _device(lib, P, world, covs, xyh, immutable), _device(lib, P, world, covs, xyh, immutable)
    o = _oracle(P, world, covs, xyh, immutable)
    for l, count in (potential or {}).items():
        o.potential[:, l], o.count[:, l] = True, count
        k = np.zeros((P, L), dtype=np.int32)
        k[:, l] = count | lib.PK_LANDMARK_POTENTIAL
        for g in (f, twin):
            g.upload_landmarks(0, P, counts=np.where(k != 0, k, 0))
    z = np.random.RandomState(17).standard_normal((P, 3))
    if ml:
        want = _safe_ml_ids(o, control, blobs, what)
        assert np.array_equal(want, np.broadcast_to(ids, want.shape)), (what, want[0], ids)
        o.propose(control, z, blobs, ids=want)
        got = _propose(f, control, blobs, z=z, return_ids=True, fresh=True)
        assert np.array_equal(got, want), what
    else:
        o.propose(control, z, blobs, ids=ids)
        _propose(f, control, blobs, z=z, ids=ids, fresh=True)
    _compare_step(lib, f, o, what, twin, control)
    f.close()
    twin.close()
    return o


@pytest.mark.parametrize("name", ["twist", "odom"])
def test_hand_built_edges(lib, name):
    control = _controls()[name]
    world, covs = synthetic_world(6, seed=5)
    P = 3
    xyh = _poses(P, 5)
    pose = truth_step((0.0, 0.0, H0), V, W, DT)
    rs = np.random.RandomState(2)
    # a landmark matched by two and by three blobs, a potential feature, an immutable landmark, an unmatched blob
    sees = np.array([0, 0, 1, 1, 1, 2, 3, 4])
    blobs = wrapped_scan(world[sees], pose, rs, SIGMA_B, SIGMA_C)
    blobs[7, 1:] += 60.0  # (landmark 4's sighting in another colour: unmatched)
    ids = np.array([1, 1, 2, 2, 2, 3, 4, 0], dtype=np.int32)
    imm = np.zeros(6, dtype=np.uint8)
    imm[3] = 1
    for ml in (False, True):
        o = _edge(lib, control, world, covs, xyh, blobs, ids, (name, "several", ml), immutable=imm, potential={2: 2}, ml=ml)
        assert (o.used == 6).all() and (o.count[:, 0] == 4).all() and (o.count[:, 1] == 6).all() and (o.count[:, 3] == 0).all()
    # every blob unmatched; no blob
    off = blobs.copy()
    off[:, 1:] += 60.0
    o = _edge(lib, control, world, covs, xyh, off, np.zeros(8, dtype=np.int32), (name, "none"), ml=True)
    assert not o.used.any() and np.array_equal(o.logw, np.full(P, 8 * LOG_LOW))
    o = _edge(lib, control, world, covs, xyh, np.zeros((0, 4)), np.zeros(0, dtype=np.int32), (name, "B = 0"))
    assert not o.logw.any()
    # a heading within 1e-3 of +-pi, before and after the move
    turn = control[2] * control[3] if name == "twist" else control[1][0] + control[1][2]
    for h in (math.pi - 5e-4, -math.pi + 5e-4, math.pi - 5e-4 - turn, -math.pi + 5e-4 - turn):
        near = _poses(P, 6, heading=h, spread=(0.05, 0.05, 1e-4))
        p2 = truth_step((0.0, 0.0, h), V, W, DT)
        b2 = wrapped_scan(world, p2, rs, SIGMA_B, SIGMA_C)
        _edge(lib, control, world, covs, near, b2, np.arange(1, 7, dtype=np.int32), (name, "heading", h), ml=True)


def test_zero_sigmas_and_a_landmark_at_the_predicted_pose(lib):
    world, covs = synthetic_world(6, seed=5)
    P = 3
    rs = np.random.RandomState(3)
    pose = truth_step((0.0, 0.0, 0.0), V, W, DT)
    blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
    ids = np.arange(1, 7, dtype=np.int32)
    xyh = _poses(P, 7, heading=0.0)
    # two zero sigmas (both rotations), and one (rot1 = 0 under a2 = 0)
    for delta, alphas in (((0.0875, 0.5, 0.0875), (0.0, 0.0, 0.05, 0.05)), ((0.0, 0.5, 0.0875), (0.5, 0.0, 0.05, 0.05))):
        s = odo.sigmas(np.array(delta), alphas)
        assert (s == 0).sum() == (2 if alphas[0] == 0.0 else 1)
        o = _edge(lib, pr.odom(delta, alphas), world, covs, xyh, blobs, ids, ("zero sigmas", alphas), ml=True)
        assert np.array_equal(o.Lambda[:, s == 0][:, :, s == 0], np.broadcast_to(np.identity(int((s == 0).sum())), (P,) + (int((s == 0).sum()),) * 2))
    # q = 0: every particle at the origin looking along x, moved 0.5 m with no rotation -- cos 0 = 1, sin 0 = 0: the predicted pose is
    # (0.5, 0, 0) exactly, on the host and on the device -- and landmark 0 put there
    at = world.copy()
    at[0, :2] = 0.5, 0.0
    b3 = wrapped_scan(at, (0.5, 0.0, 0.0), rs, SIGMA_B, SIGMA_C)
    b3[0, 0] = 0.3
    o = _edge(lib, pr.odom((0.0, 0.5, 0.0), ALPHAS), at, covs, np.zeros((P, 3)), b3, ids, "q = 0")
    assert np.array_equal(o.xhat, np.broadcast_to([0.5, 0.0, 0.0], (P, 3))) and (o.used == 6).all()


# ---------------------------------------------------------------------------------------------------------------- 4, 5
@pytest.mark.parametrize("name", ["twist", "odom"])
def test_a_scan_that_tells_nothing_is_the_plain_step(lib, name):
    control = _controls()[name]
    world, covs = synthetic_world(12, seed=5)
    P, B = 257, 12
    xyh = _poses(P, 8)
    blobs = wrapped_scan(world, truth_step((0.0, 0.0, H0), V, W, DT))
    blobs[:, 1:] += 60.0
    z = np.random.RandomState(5).standard_normal((P, 3))
    for kw in (dict(z=z), dict(seed=12345, draw=7)):  # host normals; the device's Philox draws
        f, g = _device(lib, P, world, covs, xyh), _device(lib, P, world, covs, xyh)
        ids = _propose(f, control, blobs, return_ids=True, fresh=True, **kw)
        assert not ids.any()
        _move(g, control, **kw)
        xi, dl, used = f.proposal_download()
        if "z" in kw:
            assert np.array_equal(xi, z)
        assert not used.any()
        assert np.array_equal(f.download_poses()[:, :3], g.download_poses()[:, :3])
        assert np.allclose(f.download_log_weights(), B * LOG_LOW, rtol=0, atol=RTOL)
        f.close()
        g.close()


def test_zero_alphas_are_the_plain_odometry_step(lib):
    world, covs = synthetic_world(12, seed=5)
    P = 64
    xyh = _poses(P, 9)
    rs = np.random.RandomState(6)
    blobs = wrapped_scan(world, truth_step((0.0, 0.0, H0), V, W, DT), rs, SIGMA_B, SIGMA_C)
    z = rs.standard_normal((P, 3))
    f, g = _device(lib, P, world, covs, xyh), _device(lib, P, world, covs, xyh)
    zero = np.zeros(4)
    ids = f.propose_odom(DELTA, zero, blobs, z=z, return_ids=True, fresh=True)
    g.motion_odom(DELTA, zero, z=z)
    want = g.observe(blobs, return_ids=True, fresh=True)
    assert np.array_equal(ids, want) and (want == np.arange(1, 13)).all()
    assert np.array_equal(f.download_poses()[:, :3], g.download_poses()[:, :3])
    for a, b in zip(f.download_landmarks(), g.download_landmarks()):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-300)
    assert np.allclose(f.download_log_weights(), g.download_log_weights(), rtol=0, atol=RTOL)
    f.close()
    g.close()


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("mode", ["resample", "adaptive", "path"])
def test_a_run_against_the_reference(lib, mode):
    """64 particles x 12 landmarks x 8 steps of the turning drive under the odometry model, compared at every step: resampled every
    step, gated by n_eff (threshold 0.99: some steps keep, some resample), and with the path recorded."""
    P, L, steps, theta = 64, 12, 8, 0.99
    world, covs = synthetic_world(L, seed=5)
    xyh = np.zeros((P, 3))
    xyh[:, 2] = H0
    f, o = _device(lib, P, world, covs, xyh), _oracle(P, world, covs, xyh)
    if mode == "path":
        f.path_enable(16)
    rs = np.random.RandomState(21)
    pose = (0.0, 0.0, H0)
    kept = 0
    for s in range(steps):
        prev, pose = pose, truth_step(pose, V, W, DT)
        control = pr.odom(odo.delta(prev, pose), ALPHAS)
        blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        fresh = mode != "adaptive"
        want = _safe_ml_ids(o, control, blobs, (mode, s))
        o.propose(control, z, blobs, ids=want, fresh=fresh)
        got = _propose(f, control, blobs, z=z, return_ids=True, fresh=fresh)
        assert np.array_equal(got, want), (mode, s)
        _compare_step(lib, f, o, (mode, s), shifted=mode == "adaptive")
        w = np.exp(o.logw - np.max(o.logw))
        anc = low_variance_ancestors(w, u)
        if mode == "adaptive":
            ne = w.sum() ** 2 / (w * w).sum()
            assert abs(ne - theta * P) > 1e-6
            if ne < theta * P:
                o.gather(anc)
                o.logw[:] = 0.0
            else:
                anc = np.arange(P)
                kept += 1
            assert np.array_equal(f.resample_adaptive(u, theta, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), s
        else:
            o.gather(anc)
            assert np.array_equal(f.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), s
        _compare_state(lib, f, o, (mode, s, "resampled"))
    if mode == "adaptive":
        assert 0 < kept < steps, kept
    if mode == "path":
        assert f.path_shape()[1:] == (steps, steps)
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def _snapshot(f):
    return (f.download_poses(),) + tuple(f.download_landmarks())


def test_refusals_leave_the_filter_untouched(lib):
    world, covs = synthetic_world(12, seed=5)
    P = 16
    xyh = _poses(P, 4)
    blobs = wrapped_scan(world, truth_step((0.0, 0.0, H0), V, W, DT))

    def refused(f, status, text):
        before = _snapshot(f)
        for call in (lambda: f.propose(V, W, DT, blobs, seed=1), lambda: f.propose_odom(DELTA, ALPHAS, blobs, seed=1)):
            with pytest.raises(lib.PkError) as e:
                call()
            assert e.value.status == status and text in str(e.value), str(e.value)
        for a, b in zip(before, _snapshot(f)):
            assert np.array_equal(a, b)

    f = _device(lib, P, world, covs, xyh, model=None)  # the reference model
    refused(f, lib.PK_ERR_UNSUPPORTED, "bearing model")
    with pytest.raises(lib.PkError) as e:
        f.proposal_download()
    assert e.value.status == lib.PK_ERR_STATE
    f.close()
    f = _device(lib, P, world, covs, xyh)  # the dense layout: a Qt that couples bearing and colour
    Qt = 0.1 * np.identity(4)
    Qt[0, 1] = Qt[1, 0] = 0.01
    f.set_measurement_noise(Qt)
    refused(f, lib.PK_ERR_UNSUPPORTED, "dense layout")
    f.close()
    for retire in (False, True):  # growing maps, retirement
        f = _device(lib, P, world, covs, xyh)
        f.grow_enable(10, 16, 30.0)
        if retire:
            f.grow_retire(4, 3)
        refused(f, lib.PK_ERR_UNSUPPORTED, "growing maps")
        f.close()
    # a shard of a sharded filter.  (A split step in progress is refused by the same clause, which no call can reach today: only a
    # reference-model filter can enter a split step -- pk_observe_staged_range refuses the bearing model -- and pk_set_measurement_model
    # refuses to change the model inside one, so such a filter is refused for its model first.)
    f = _device(lib, P, world, covs, xyh)
    f.set_shard(64)
    refused(f, lib.PK_ERR_UNSUPPORTED, "one whole filter")
    f.close()
    f = _device(lib, P, world, covs, xyh)  # a staged scan in flight
    f.stage_scan(blobs)
    refused(f, lib.PK_ERR_STATE, "staged scan")
    f.observe_staged(fresh=True)
    f.propose(V, W, DT, blobs, seed=1)  # ... and once it is taken the call goes through
    f.close()


def test_memory_and_isolation(lib):
    world, covs = synthetic_world(12, seed=5)
    P = 64
    xyh = _poses(P, 4)
    rs = np.random.RandomState(12)
    blobs = wrapped_scan(world, truth_step((0.0, 0.0, H0), V, W, DT), rs, SIGMA_B, SIGMA_C)
    z = rs.standard_normal((P, 3))

    def plain(f):
        f.motion(V, W, DT, z=z)
        f.observe(blobs, fresh=True)
        return (f.download_log_weights(),) + _snapshot(f)

    before = _device(lib, P, world, covs, xyh)
    want = plain(before)
    b0 = before.device_bytes()
    before.close()
    f = _device(lib, P, world, covs, xyh)
    f.associate(blobs)  # (the scan's own buffers: what a pk_observe of this scan holds)
    held = f.device_bytes()
    assert held == b0
    f.propose(V, W, DT, blobs, z=z, fresh=True)
    assert f.device_bytes() == held + 84 * P
    f.propose_odom(DELTA, ALPHAS, blobs, z=z, fresh=True)
    assert f.device_bytes() == held + 84 * P
    f.close()
    g = _device(lib, P, world, covs, xyh)  # supplied ids: the scan's block is pk_observe's (the id row fits its slack)
    ids = np.arange(1, 13, dtype=np.int32)
    g.observe(blobs, ids=ids, fresh=True)
    held = g.device_bytes()
    g.propose(V, W, DT, blobs, z=z, ids=ids, fresh=True)
    assert g.device_bytes() == held + 84 * P
    g.close()
    after = _device(lib, P, world, covs, xyh)  # a bearing-model filter after a twin has used the proposal: the same bits
    for a, b in zip(want, plain(after)):
        assert np.array_equal(a, b)
    assert after.device_bytes() == b0
    after.close()


def test_supplied_ids_have_no_limit_of_the_association(lib):
    """20 000 blobs on a map of 3 landmarks: more than the per-particle LDS chains of a maximum-likelihood scan hold (pk_propose
    refuses that scan without ids, as pk_observe does) and no hindrance with supplied ids, which pk_observe takes too.  Three blobs
    are matched; the others weigh log 0.1 each."""
    P, L, B = 2, 3, 20000
    world, covs = synthetic_world(L, seed=5)
    xyh = _poses(P, 15)
    rs = np.random.RandomState(16)
    control = _controls()["twist"]
    blobs = np.zeros((B, 4))
    blobs[:, 0] = rs.uniform(-3.0, 3.0, B)
    blobs[:3] = wrapped_scan(world, truth_step((0.0, 0.0, H0), V, W, DT), rs, SIGMA_B, SIGMA_C)
    ids = np.zeros(B, dtype=np.int32)
    ids[:3] = 1, 2, 3
    z = rs.standard_normal((P, 3))
    f, o = _device(lib, P, world, covs, xyh), _oracle(P, world, covs, xyh)
    with pytest.raises(lib.PkError) as e:
        _propose(f, control, blobs, z=z, fresh=True)
    assert e.value.status == lib.PK_ERR_UNSUPPORTED and "LDS" in str(e.value)
    assert np.array_equal(f.download_poses()[:, :3], xyh)
    o.propose(control, z, blobs[:3], ids=ids[:3])  # the oracle on the matched blobs; the others add (B - 3) log 0.1
    o.dlogw += (B - 3) * LOG_LOW
    o.logw += (B - 3) * LOG_LOW
    _propose(f, control, blobs, z=z, ids=ids, fresh=True)
    _compare_step(lib, f, o, "20 000 supplied ids")
    f.close()


def test_the_facade_refuses_what_the_proposal_cannot_do(lib):
    import parakeet_slam_amd as pk

    world, covs = synthetic_world(4, seed=5)
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(4)]
    pk.msgs.Time.set_now(0.0)
    with pytest.raises(ValueError, match="measurement_model='bearing'"):
        pk.FastSLAM(feats, num_particles=8, proposal="measurement")
    with pytest.raises(ValueError, match="new_landmarks"):
        pk.FastSLAM(feats, num_particles=8, measurement_model="bearing", proposal="measurement", new_landmarks=True, spare_landmarks=2)
    with pytest.raises(ValueError, match="one GPU"):
        pk.FastSLAM(feats, num_particles=8, devices=[0, 0], measurement_model="bearing", proposal="measurement")
    with pytest.raises(ValueError, match="'motion' \\(default\\) or 'measurement'"):
        pk.FastSLAM(feats, num_particles=8, measurement_model="bearing", proposal="scan")


# ---------------------------------------------------------------------------------------------------------------- 8
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


@pytest.mark.parametrize("motion", ["twist", "odometry"])
def test_facade_against_the_reference(lib, motion):
    import parakeet_slam_amd as pk
    from parakeet_slam_amd.core import _make_state

    P, L, steps = 64, 12, 5
    world, covs = synthetic_world(L, seed=5)
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L)]
    np.random.seed(11)
    random.seed(7)
    pk.msgs.Time.set_now(0.0)
    kw = dict(motion="odometry", odom_alphas=ALPHAS) if motion == "odometry" else {}
    fs = pk.FastSLAM(feats, num_particles=P, device=0, weight_domain="log", rng="global", measurement_model="bearing",
                     proposal="measurement", record_ids=True, **kw)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = V, W
    fs.last_control = tw
    o = ProposalOracle(P, world, covs)
    rs, prn, noise = np.random.RandomState(11), random.Random(7), np.random.RandomState(8)
    pose = (0.0, 0.0, 0.0)
    if motion == "odometry":
        fs.odom_motion_update(_make_state(*pose))
    for s in range(steps):
        prev, pose = pose, truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world, pose, noise, SIGMA_B, SIGMA_C)
        pk.msgs.Time.set_now(DT * (s + 1))
        if motion == "odometry":
            fs.odom_motion_update(_make_state(*pose))
            control = pr.odom(odo.delta(prev, pose), ALPHAS)
        else:
            control = pr.twist(V, W, DT)
        z, u = rs.standard_normal((P, 3)), prn.random()
        want = _safe_ml_ids(o, control, blobs, (motion, s))
        o.propose(control, z, blobs, ids=want)
        _assert_conditioned(o, (motion, s))
        fs.cam_cb(_View(pk, blobs))
        assert np.array_equal(fs.last_ids, want), (motion, s)  # record_ids=True: the step's settled ids
        o.gather(low_variance_ancestors(np.exp(o.logw - np.max(o.logw)), u))
        assert np.allclose(fs.summary(), o.summary(), rtol=1e-12, atol=1e-14), (s, fs.summary(), o.summary())
    _compare_state(lib, fs._filter, o, "facade")
    fs.close()

"""GPU: ranges in the measurement-informed proposal (pk_proposal_ranges with pk_scan_ranges and pk_propose / pk_propose_odom;
DESIGN.md section 4, "Ranges in the proposal") against tests/range_proposal_reference.py.

Tolerances: those tests/test_gpu_proposal.py states for the same quantities, through its own helpers (_compare_step) -- xi, the
weight increments and the log-weights 1e-9 absolute, poses rtol 1e-12, means 1e-9 relative, covariances rtol 1e-9 / atol 1e-13,
ids and `used` exactly, cond_2(Lambda) <= 1e4 asserted from the reference first.  Where ids are associated the reference's own
margins are asserted before anything is compared, with the bounds of tests/test_range_bearing_host.py (assert_margins of
tests/test_gpu_range_bearing.py): no gate within 1e-9 rad / 1e-6 of turning over, the best probability of a contested blob at least
1e-6 (relative) above the second best.  tests/test_range_proposal_host.py runs that check on every scene here without a GPU.

Shapes, the smallest that take each path of k_propose_range and k_observe_proposed_range: B = 1; B = 12 (one partial wave); B = 300
on L = 600 (a lane of the 256 holds two blobs, all four waves contribute to the sums); L = 3 and 65; P = 16; and 16 400 x 3, where
the grid of 16 384 workgroups takes a second turn."""
import math
import random

import numpy as np
import pytest

from oracle.fastslam_oracle import low_variance_ancestors, synthetic_world, truth_step

import odom_reference as odo
import proposal_reference as pr
import test_gpu_proposal as tp
from bearing_model_reference import wrapped_scan
from range_bearing_reference import range_scan
from range_proposal_reference import RangedProposalOracle
from test_gpu_range_bearing import assert_margins

pytestmark = pytest.mark.gpu

V, W, DT, H0 = tp.V, tp.W, tp.DT, tp.H0
SIGMA_B, SIGMA_C, SIGMA_R = tp.SIGMA_B, tp.SIGMA_C, (0.05, 0.01)
ALPHAS, DELTA = tp.ALPHAS, tp.DELTA
LOG_LOW = tp.LOG_LOW
SHAPES = [(3, 1, 16), (65, 12, 16), (600, 300, 16)]
KINDS = ("all", "mixed")  # every blob ranged; every third blob has none


# ---------------------------------------------------------------------------------------------------------------- scenes
def oracle(P, means, covs, xyh, immutable=None):
    o = RangedProposalOracle(P, means, covs, immutable=immutable)
    o.x, o.y, o.h = xyh[:, 0].copy(), xyh[:, 1].copy(), xyh[:, 2].copy()
    return o


def shape_scene(L, B, P, kind, steps):
    """synthetic_world(L) seen from the turning drive's poses, blob b showing landmark b (L // B): (world, covs, the particles'
    poses, the landmarks seen, per step (blobs, ranges, variances, normals))."""
    world, covs = synthetic_world(L, seed=5)
    sees = (np.arange(B) * (L // B)) % L
    xyh = tp._poses(P, 3)
    rs, rr = np.random.RandomState(100 * L + P), np.random.RandomState(7 * L + B)
    pose = (0.0, 0.0, H0)
    rows = []
    for s in range(steps):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world[sees], pose, rs, SIGMA_B, SIGMA_C)
        rho, var = range_scan(world[sees], pose, rr, SIGMA_R[0], SIGMA_R[1], 3 if kind == "mixed" else None)
        rows.append((blobs, rho, var, rs.standard_normal((P, 3))))
    return world, covs, xyh, sees, rows


def shape_steps(L):
    return 2 if L < 600 else 1


def supplied_ids(sees, B):
    ids = (sees + 1).astype(np.int32)
    if B > 3:
        ids[1] = 0       # an unmatched blob
        ids[2] = ids[3]  # and a landmark seen twice: in a mixed scan by an unranged blob (2), then by a ranged one (3)
    return ids


def edge_scene():
    """Six landmarks, three particles, one hand-built scan: landmark 0 seen by a ranged blob and then by an unranged one, landmark 1
    by an unranged and then by a ranged one, landmark 2 -- a potential feature -- by a ranged blob, the immutable landmark 3 by a
    ranged blob, and landmark 4's sighting in another colour (unmatched, ranged)."""
    world, covs = synthetic_world(6, seed=5)
    xyh = tp._poses(3, 5)
    pose = truth_step((0.0, 0.0, H0), V, W, DT)
    rs, rr = np.random.RandomState(2), np.random.RandomState(3)
    sees = np.array([0, 0, 1, 1, 2, 3, 4])
    blobs = wrapped_scan(world[sees], pose, rs, SIGMA_B, SIGMA_C)
    blobs[6, 1:] += 60.0
    rho, var = range_scan(world[sees], pose, rr, SIGMA_R[0], SIGMA_R[1])
    rho[[1, 2]] = np.nan
    ids = np.array([1, 1, 2, 2, 3, 4, 0], dtype=np.int32)
    imm = np.zeros(6, dtype=np.uint8)
    imm[3] = 1
    return dict(world=world, covs=covs, xyh=xyh, blobs=blobs, rho=rho, var=var, ids=ids, immutable=imm, potential={2: 2})


def zero_sigma_scene():
    """rot1 = 0 under a2 = 0: the first sigma is 0 (tests/test_gpu_proposal.py's case), every blob ranged."""
    world, covs = synthetic_world(6, seed=5)
    rs, rr = np.random.RandomState(3), np.random.RandomState(4)
    pose = truth_step((0.0, 0.0, 0.0), V, W, DT)
    blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
    rho, var = range_scan(world, pose, rr, SIGMA_R[0], SIGMA_R[1])
    delta, alphas = (0.0, 0.5, 0.0875), (0.5, 0.0, 0.05, 0.05)
    return dict(world=world, covs=covs, xyh=tp._poses(3, 7, heading=0.0), blobs=blobs, rho=rho, var=var,
                ids=np.arange(1, 7, dtype=np.int32), control=pr.odom(delta, alphas))


def ml_scenes():
    """Every scene of this file whose ids are associated, as (name, the oracle before the first step, control, per step (blobs,
    ranges, variances, normals)): what tests/test_range_proposal_host.py checks the margins of."""
    for L, B, P in SHAPES:
        for kind in KINDS:
            for name, control in sorted(tp._controls().items()):
                world, covs, xyh, sees, rows = shape_scene(L, B, P, kind, shape_steps(L))
                yield ("shape", L, B, kind, name), oracle(P, world, covs, xyh), control, rows
    z3 = np.random.RandomState(17).standard_normal((3, 3))
    for name, control in sorted(tp._controls().items()):
        e = edge_scene()
        o = oracle(3, e["world"], e["covs"], e["xyh"], e["immutable"])
        o.potential[:, 2], o.count[:, 2] = True, 2
        yield ("edge", name), o, control, [(e["blobs"], e["rho"], e["var"], z3)]
    zs = zero_sigma_scene()
    yield ("zero sigma",), oracle(3, zs["world"], zs["covs"], zs["xyh"]), zs["control"], [(zs["blobs"], zs["rho"], zs["var"], z3)]


# ---------------------------------------------------------------------------------------------------------------- helpers
def _device(lib, P, world, covs, xyh, immutable=None, on=True, **kw):
    f = tp._device(lib, P, world, covs, xyh, immutable, **kw)
    if on:
        f.proposal_ranges(True)
    return f


def _propose(f, control, blobs, rho, var, **kw):
    if rho is not None:
        f.scan_ranges(rho, var)
    return tp._propose(f, control, blobs, **kw)


def _everything(f):
    return (f.download_poses(), f.download_log_weights()) + tuple(f.download_landmarks()) + tuple(f.proposal_download())


# ---------------------------------------------------------------------------------------------------------------- the shapes
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,B,P", SHAPES)
def test_ranged_proposal_against_the_reference(lib, L, B, P, kind):
    """Both motion models; supplied normals; maximum-likelihood ids through both association kernels, and supplied ids; two steps on
    the small shapes (the second with carried weights: fresh off), so that the second gathers from maps that differ between
    particles.  And the pose invariant: the sampled pose is the plain motion call's for the downloaded xi, bit for bit."""
    steps = shape_steps(L)
    for name, control in sorted(tp._controls().items()):
        world, covs, xyh, sees, rows = shape_scene(L, B, P, kind, steps)
        fs = {"grid": _device(lib, P, world, covs, xyh), "brute": _device(lib, P, world, covs, xyh, opts={"assoc_kernel": 1}),
              "ids": _device(lib, P, world, covs, xyh)}
        twin = tp._device(lib, P, world, covs, xyh)
        o_ml, o_ids = oracle(P, world, covs, xyh), oracle(P, world, covs, xyh)
        for s, (blobs, rho, var, z) in enumerate(rows):
            what, fresh = (name, L, B, P, kind, s), s == 0
            want = o_ml.propose(control, z, blobs, rho, var, fresh=fresh)
            assert_margins(o_ml, what)
            if kind == "all":
                assert np.array_equal(o_ml.n_rho, o_ml.used), what
            for k in ("grid", "brute"):
                twin.upload_poses(fs[k].download_poses())
                got = _propose(fs[k], control, blobs, rho, var, z=z, return_ids=True, fresh=fresh)
                assert np.array_equal(got, want), (what, k, int((got != want).sum()))
                assert fs[k].observe_route() == "ml_general" and fs[k].scan_ranges_state() == (0, 0)
                tp._compare_step(lib, fs[k], o_ml, what + (k,), twin, control)
            supplied = supplied_ids(sees, B)
            o_ids.propose(control, z, blobs, rho, var, ids=supplied, fresh=fresh)
            twin.upload_poses(fs["ids"].download_poses())
            got = _propose(fs["ids"], control, blobs, rho, var, z=z, ids=supplied, return_ids=True, fresh=fresh)
            assert np.array_equal(got, np.broadcast_to(supplied, (P, B)))
            assert fs["ids"].observe_route() == "known_ids"
            tp._compare_step(lib, fs["ids"], o_ids, what + ("ids",), twin, control)
        assert (o_ml.used > 0).all() and (o_ml.n_rho > 0).all()
        for g in list(fs.values()) + [twin]:
            g.close()


def test_k_propose_range_walks_more_particles_than_its_grid(lib):
    """16 400 particles on 3 landmarks: the last sixteen workgroups of the capped grid take a second particle."""
    P, L = 16400, 3
    world, covs = synthetic_world(L, seed=5)
    xyh = tp._poses(P, 13)
    rs, rr = np.random.RandomState(14), np.random.RandomState(15)
    control = tp._controls()["odom"]
    pose = truth_step((0.0, 0.0, H0), V, W, DT)
    blobs = wrapped_scan(world[:2], pose, rs, SIGMA_B, SIGMA_C)
    rho, var = range_scan(world[:2], pose, rr, SIGMA_R[0], SIGMA_R[1])
    z = rs.standard_normal((P, 3))
    f, twin, o = _device(lib, P, world, covs, xyh), tp._device(lib, P, world, covs, xyh), oracle(P, world, covs, xyh)
    want = o.propose(control, z, blobs, rho, var)
    assert_margins(o, "grid stride")
    got = _propose(f, control, blobs, rho, var, z=z, return_ids=True, fresh=True)
    assert np.array_equal(got, want) and (o.used == 2).all() and (o.n_rho == 2).all()
    tp._compare_step(lib, f, o, "grid stride", twin, control)
    f.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------- the edges
def _edge(lib, control, sc, what, ml):
    """One hand-built step, supplied ids (ml: the association must find the same), against the oracle."""
    world, covs, xyh = sc["world"], sc["covs"], sc["xyh"]
    P, L = len(xyh), len(world)
    imm = sc.get("immutable")
    f, twin, o = _device(lib, P, world, covs, xyh, imm), tp._device(lib, P, world, covs, xyh, imm), oracle(P, world, covs, xyh, imm)
    for l, count in (sc.get("potential") or {}).items():
        o.potential[:, l], o.count[:, l] = True, count
        k = np.zeros((P, L), dtype=np.int32)
        k[:, l] = count | lib.PK_LANDMARK_POTENTIAL
        for g in (f, twin):
            g.upload_landmarks(0, P, counts=k)
    z = np.random.RandomState(17).standard_normal((P, 3))
    blobs, rho, var, ids = sc["blobs"], sc["rho"], sc["var"], sc["ids"]
    if ml:
        want = o.propose(control, z, blobs, rho, var)
        assert_margins(o, what)
        assert np.array_equal(want, np.broadcast_to(ids, want.shape)), (what, want[0], ids)
        got = _propose(f, control, blobs, rho, var, z=z, return_ids=True, fresh=True)
        assert np.array_equal(got, want), what
    else:
        o.propose(control, z, blobs, rho, var, ids=ids)
        _propose(f, control, blobs, rho, var, z=z, ids=ids, fresh=True)
    tp._compare_step(lib, f, o, what, twin, control)
    f.close()
    twin.close()
    return o


@pytest.mark.parametrize("name", ["twist", "odom"])
def test_hand_built_edges(lib, name):
    control = tp._controls()[name]
    sc = edge_scene()
    for ml in (False, True):
        o = _edge(lib, control, sc, (name, "edges", ml), ml)
        # five matches weigh (the potential feature's and the unmatched blob do not); three of them carried a range
        assert (o.used == 5).all() and (o.n_rho == 3).all()
        assert (o.count[:, 0] == 4).all() and (o.count[:, 1] == 4).all() and (o.count[:, 2] == 4).all() and (o.count[:, 3] == 0).all()
    # the potential feature alone, matched by a ranged blob: log 0.1, nothing in the sums -- xi = z
    one = dict(sc, blobs=sc["blobs"][4:5], rho=sc["rho"][4:5], var=sc["var"][4:5], ids=sc["ids"][4:5])
    o = _edge(lib, control, one, (name, "potential"), False)
    assert not o.used.any() and np.array_equal(o.dlogw, np.full(3, LOG_LOW))
    assert np.array_equal(o.xi, np.random.RandomState(17).standard_normal((3, 3)))


def test_one_zero_sigma_and_a_landmark_at_the_predicted_pose(lib):
    zs = zero_sigma_scene()
    s = odo.sigmas(zs["control"][1], zs["control"][2])
    assert (s == 0).sum() == 1
    o = _edge(lib, zs["control"], zs, "one zero sigma", True)
    assert np.array_equal(o.Lambda[:, s == 0][:, :, s == 0], np.ones((3, 1, 1))) and (o.n_rho == 6).all()
    # q = 0: every particle at the origin looking along x, moved 0.5 m with no rotation -- the predicted pose is (0.5, 0, 0) exactly,
    # on the host and on the device -- and landmark 0 put there, seen by a ranged blob: both rows of h_x and h_m vanish, nu = (beta, rho)
    world, covs = synthetic_world(6, seed=5)
    at = world.copy()
    at[0, :2] = 0.5, 0.0
    rs = np.random.RandomState(3)
    blobs = wrapped_scan(at, (0.5, 0.0, 0.0), rs, SIGMA_B, SIGMA_C)
    blobs[0, 0] = 0.3
    rho, var = range_scan(at, (0.5, 0.0, 0.0), rs, SIGMA_R[0], SIGMA_R[1])
    rho[0], var[0] = 0.2, 0.052 ** 2
    sc = dict(world=at, covs=covs, xyh=np.zeros((3, 3)), blobs=blobs, rho=rho, var=var, ids=np.arange(1, 7, dtype=np.int32))
    o = _edge(lib, pr.odom((0.0, 0.5, 0.0), ALPHAS), sc, "q = 0", False)
    assert np.array_equal(o.xhat, np.broadcast_to([0.5, 0.0, 0.0], (3, 3))) and (o.used == 6).all()


# ---------------------------------------------------------------------------------------------------------------- draws, bits
@pytest.mark.parametrize("name", ["twist", "odom"])
def test_philox_draws_and_the_same_bits_every_run(lib, name):
    """Without supplied normals the step draws the motion kernel's own Philox normals: a scan that tells nothing leaves them as xi
    (tests/test_gpu_proposal.py), so they are read off a twin first and handed to the reference.  The sampled pose is the plain
    motion call's for the downloaded xi, bit for bit; and two identical runs leave identical bits everywhere."""
    control = tp._controls()[name]
    L, B, P = 65, 12, 16
    world, covs, xyh, sees, rows = shape_scene(L, B, P, "mixed", 1)
    blobs, rho, var, _ = rows[0]
    kw = dict(seed=12345, draw=7)
    blind = tp._device(lib, P, world, covs, xyh)
    off = blobs.copy()
    off[:, 1:] += 60.0
    tp._propose(blind, control, off, fresh=True, **kw)
    z = blind.proposal_download()[0]
    blind.close()
    o = oracle(P, world, covs, xyh)
    want = o.propose(control, z, blobs, rho, var)
    assert_margins(o, (name, "philox"))
    f, g, twin = _device(lib, P, world, covs, xyh), _device(lib, P, world, covs, xyh), tp._device(lib, P, world, covs, xyh)
    got = _propose(f, control, blobs, rho, var, return_ids=True, fresh=True, **kw)
    assert np.array_equal(got, want)
    tp._compare_step(lib, f, o, (name, "philox"), twin, control)
    _propose(g, control, blobs, rho, var, fresh=True, **kw)
    for a, b in zip(_everything(f), _everything(g)):
        assert np.array_equal(a, b)
    for h in (f, g, twin):
        h.close()


# ---------------------------------------------------------------------------------------------------------------- lifecycle
def test_an_armed_scan_without_a_finite_range_is_the_unarmed_call(lib):
    """Mode on with an armed all-NaN scan, mode on with nothing armed, mode off: array for array the same, with pk_device_bytes and
    pk_observe_route; maximum-likelihood and supplied ids.  And the state getter."""
    L, B, P = 65, 12, 16
    world, covs, xyh, sees, rows = shape_scene(L, B, P, "all", 1)
    blobs, rho, var, z = rows[0]
    nan = np.full(B, np.nan)
    for ids in (None, supplied_ids(sees, B)):
        out = []
        for on, arm in ((True, True), (True, False), (False, False)):
            f = _device(lib, P, world, covs, xyh, on=on)
            assert f.proposal_ranges_state() is on
            _propose(f, tp._controls()["twist"], blobs, nan if arm else None, None, z=z, ids=ids, fresh=True)
            assert f.scan_ranges_state() == (0, 0)
            out.append(_everything(f) + (np.array(f.device_bytes()), np.array(f.observe_route())))
            f.close()
        for other in out[1:]:
            for a, b in zip(out[0], other):
                assert np.array_equal(a, b)
    f = _device(lib, P, world, covs, xyh)
    f.proposal_ranges(False)
    assert f.proposal_ranges_state() is False
    f.close()


def test_the_first_ranged_scan_grows_the_scan_block_through_the_owner_of_device_memory(lib):
    """A ranged proposal step holds what a ranged pk_observe of the same scan holds plus the proposal's 84 P bytes."""
    L, B, P = 600, 300, 16
    world, covs, xyh, sees, rows = shape_scene(L, B, P, "all", 1)
    blobs, rho, var, z = rows[0]
    g = tp._device(lib, P, world, covs, xyh)
    g.scan_ranges(rho, var)
    g.observe(blobs, fresh=True)
    held = g.device_bytes()
    g.close()
    f = _device(lib, P, world, covs, xyh)
    _propose(f, tp._controls()["twist"], blobs, rho, var, z=z, fresh=True)
    assert f.device_bytes() == held + 84 * P
    _propose(f, tp._controls()["odom"], blobs, rho, var, z=z, fresh=True)
    assert f.device_bytes() == held + 84 * P
    f.close()


def test_refusals_carry_their_status_and_text_and_change_nothing(lib):
    world, covs = synthetic_world(12, seed=5)
    P, B = 16, 12
    xyh = tp._poses(P, 4)
    pose = truth_step((0.0, 0.0, H0), V, W, DT)
    blobs = wrapped_scan(world, pose)
    rho, var = range_scan(world, pose, None, SIGMA_R[0], SIGMA_R[1])

    def refused(f, status, text, n=B):
        before = tp._snapshot(f) + (f.download_log_weights(),)
        for call in (lambda: f.propose(V, W, DT, blobs, seed=1), lambda: f.propose_odom(DELTA, ALPHAS, blobs, seed=1)):
            f.scan_ranges(rho[:n], var[:n])
            assert f.scan_ranges_state() == (n, 0)
            with pytest.raises(lib.PkError) as e:
                call()
            assert e.value.status == status and text in str(e.value), str(e.value)
            assert f.scan_ranges_state() == (0, 0)  # refused, and the ranges are gone
        for a, b in zip(before, tp._snapshot(f) + (f.download_log_weights(),)):
            assert np.array_equal(a, b)

    f = _device(lib, P, world, covs, xyh, on=False)  # the mode is off: the proposal's refusal of ranges as it was
    refused(f, lib.PK_ERR_UNSUPPORTED, "not part of the measurement-informed proposal")
    f.proposal_ranges(True)
    refused(f, lib.PK_ERR_INVALID, "named the ranges of a scan of 5 blobs", n=5)  # the range scans' refusals, in their order ...
    f.close()
    f = _device(lib, P, world, covs, xyh, model=None)
    refused(f, lib.PK_ERR_UNSUPPORTED, "per-blob ranges (pk_scan_ranges) are an option of the bearing model")
    refused(f, lib.PK_ERR_INVALID, "named the ranges", n=5)  # (the number of blobs answers before the model)
    f.close()
    f = _device(lib, P, world, covs, xyh)
    Qt = 0.1 * np.identity(4)
    Qt[0, 1] = Qt[1, 0] = 0.01
    f.set_measurement_noise(Qt)
    refused(f, lib.PK_ERR_UNSUPPORTED, "dense layout")
    f.close()
    f = _device(lib, P, world, covs, xyh)
    f.grow_enable(10, 16, 30.0)
    refused(f, lib.PK_ERR_UNSUPPORTED, "per-blob ranges (pk_scan_ranges) have no kernel for growing maps")
    f.close()
    f = _device(lib, P, world, covs, xyh)  # ... then the proposal's own
    f.set_shard(64)
    refused(f, lib.PK_ERR_UNSUPPORTED, "one whole filter")
    f.close()
    f = _device(lib, P, world, covs, xyh)
    f.stage_scan(blobs)
    refused(f, lib.PK_ERR_STATE, "staged scan")
    f.observe_staged(fresh=True)
    _propose(f, tp._controls()["twist"], blobs, rho, var, seed=1)  # ... and once it is taken the call goes through
    f.close()


# ---------------------------------------------------------------------------------------------------------------- the facade
class _View(object):
    def __init__(self, pk, blobs, rho, as_array):
        class Scan(object):
            pass

        self.last_sensor_reading = Scan()
        if as_array:
            self.last_sensor_reading.observes = np.concatenate([blobs, rho[:, None]], axis=1)
            return
        obs = []
        for b, r in zip(blobs, rho):
            o = pk.msgs.Blob()
            o.bearing = float(b[0])
            o.color.r, o.color.g, o.color.b = float(b[1]), float(b[2]), float(b[3])
            if r == r:
                o.range = float(r)
            obs.append(o)
        self.last_sensor_reading.observes = obs


@pytest.mark.parametrize("as_array", [False, True])
@pytest.mark.parametrize("motion", ["twist", "odometry"])
def test_facade_against_the_reference(lib, motion, as_array):
    """cam_cb with proposal_ranges=True, scans as message objects with a ``range`` attribute (every third blob without) and as
    (B, 5) arrays: the variances are formed as the plain path forms them, the one call consumes them."""
    import parakeet_slam_amd as pk
    from parakeet_slam_amd.core import _make_state

    P, L, steps = 64, 12, 4
    world, covs = synthetic_world(L, seed=5)
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L)]
    np.random.seed(11)
    random.seed(7)
    pk.msgs.Time.set_now(0.0)
    kw = dict(motion="odometry", odom_alphas=ALPHAS) if motion == "odometry" else {}
    fs = pk.FastSLAM(feats, num_particles=P, device=0, weight_domain="log", rng="global", measurement_model="bearing",
                     proposal="measurement", range_noise=SIGMA_R, proposal_ranges=True, record_ids=True, **kw)
    assert fs._filter.proposal_ranges_state() is True
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = V, W
    fs.last_control = tw
    o = RangedProposalOracle(P, world, covs)
    rs, prn, noise, rr = np.random.RandomState(11), random.Random(7), np.random.RandomState(8), np.random.RandomState(9)
    pose = (0.0, 0.0, 0.0)
    if motion == "odometry":
        fs.odom_motion_update(_make_state(*pose))
    for s in range(steps):
        prev, pose = pose, truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world, pose, noise, SIGMA_B, SIGMA_C)
        rho, _ = range_scan(world, pose, rr, SIGMA_R[0], SIGMA_R[1], 3)
        sig = SIGMA_R[0] + SIGMA_R[1] * rho
        pk.msgs.Time.set_now(DT * (s + 1))
        if motion == "odometry":
            fs.odom_motion_update(_make_state(*pose))
            control = pr.odom(odo.delta(prev, pose), ALPHAS)
        else:
            control = pr.twist(V, W, DT)
        z, u = rs.standard_normal((P, 3)), prn.random()
        want = o.propose(control, z, blobs, rho, sig * sig)
        assert_margins(o, (motion, s))
        tp._assert_conditioned(o, (motion, s))
        assert (o.n_rho == 8).all()
        fs.cam_cb(_View(pk, blobs, rho, as_array))
        assert np.array_equal(fs.last_ids, want), (motion, s)
        o.gather(low_variance_ancestors(np.exp(o.logw - np.max(o.logw)), u))
        assert np.allclose(fs.summary(), o.summary(), rtol=1e-12, atol=1e-14), (s, fs.summary(), o.summary())
    tp._compare_state(lib, fs._filter, o, "facade")
    fs.close()

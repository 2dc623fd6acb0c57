"""Host: the reference of ranges in the measurement-informed proposal (tests/range_proposal_reference.py) against itself, against
ProposalOracle and against RangeBearingOracle -- the 3 x 3 weight formula with its closed-form 2 x 2 blocks against the dense
density, ProposalOracle bit for bit where no blob has a range, RangeBearingOracle's plain step at zero sigmas, the pose Jacobian of
the range row against central differences, what ranges in the proposal buy on the turning drive, and the margins of every scene of
tests/test_gpu_range_proposal.py.  One test needs the built library: the mode's entry points exist and the default is off.

The drive (64 particles, synthetic_world(12, seed=5), v = 1.0, w = 0.35, dt = 0.5, 40 steps, sigma_bearing 0.01, odometry alphas
(2, 0.2, 0.2, 0.2), range noise 0.05 + 0.01 rho, resampling every step), as test_ranges_in_the_proposal_... prints it; the map
starts 0.5 m off (test_range_bearing_host._pushed_map):

    seed   mean n_eff / P before resampling      mean pose error, m                 map error, m (map started 0.5 m off)
           1.0 ranged   proposal ranged          1.0 ranged   proposal ranged       1.0 ranged   proposal ranged
    1      0.111        0.859                    0.146        0.104                 0.374        0.327
    2      0.108        0.849                    0.218        0.089                 0.310        0.233
    3      0.105        0.803                    0.141        0.112                 0.262        0.242

(FastSLAM 1.0 and the proposal on bearings alone: 0.330 / 0.339 / 0.324 and 0.995 / 0.993 / 0.994.)  Only the n_eff figures are
asserted; the errors are printed for DESIGN.md section 4, "Ranges in the proposal".
"""
import math

import numpy as np
import pytest

import odom_reference as odo
import proposal_reference as pr
import range_bearing_reference as rref
import range_proposal_reference as rpr
import test_gpu_range_proposal as gpu_tests
import test_range_bearing_host as rbh
from bearing_model_reference import wrapped_scan
from oracle.fastslam_oracle import low_variance_ancestors, synthetic_world, truth_step
from proposal_reference import ProposalOracle
from range_bearing_reference import RangeBearingOracle, range_scan
from range_proposal_reference import RangedProposalOracle
from test_gpu_range_bearing import assert_margins

V, W, DT, STEPS, P = 1.0, 0.35, 0.5, 40, 64
SIGMA_B, SIGMA_C, SIGMA_R = 0.01, 0.3, (0.05, 0.01)
ALPHAS = (2.0, 0.2, 0.2, 0.2)  # tests/test_proposal_reference_host.py's: they starve the 1.0 filter
STATE = ("x", "y", "h", "logw", "mean", "cov", "count", "potential", "n_unmatched")


def test_the_library_has_the_mode_and_it_is_off_by_default(lib):
    """No GPU: the entry points are there, and the handle-free halves answer (a NULL handle is refused with its status)."""
    so = lib.load()
    assert so.pk_proposal_ranges(None, 1) == lib.PK_ERR_INVALID
    assert so.pk_proposal_ranges_state(None, None) == lib.PK_ERR_INVALID
    assert "proposal_ranges" in dir(lib.DeviceFilter) and "proposal_ranges_state" in dir(lib.DeviceFilter)


def test_the_facade_refuses_what_it_cannot_combine_before_any_device_work():
    """(No GPU here: every one of these is raised before a filter is created.)"""
    import parakeet_slam_amd as pk

    world, covs = synthetic_world(4, seed=5)
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(4)]
    pk.msgs.Time.set_now(0.0)
    kw = dict(num_particles=8, measurement_model="bearing")
    with pytest.raises(ValueError, match="proposal='measurement'"):  # without the keyword: the refusal as it was
        pk.FastSLAM(feats, proposal="measurement", range_noise=SIGMA_R, **kw)
    with pytest.raises(ValueError, match="proposal_ranges=True"):
        pk.FastSLAM(feats, proposal="measurement", proposal_ranges=True, **kw)
    with pytest.raises(ValueError, match="proposal_ranges=True"):
        pk.FastSLAM(feats, proposal="motion", range_noise=SIGMA_R, proposal_ranges=True, **kw)
    with pytest.raises(ValueError, match="new_landmarks"):
        pk.FastSLAM(feats, proposal="measurement", range_noise=SIGMA_R, proposal_ranges=True, new_landmarks=True, spare_landmarks=2, **kw)
    with pytest.raises(ValueError, match="one GPU"):
        pk.FastSLAM(feats, devices=[0, 0], proposal="measurement", range_noise=SIGMA_R, proposal_ranges=True, **kw)


@pytest.mark.parametrize("n", [0, 1, 2, 40])
def test_the_3x3_formula_is_the_dense_density(n):
    """n matches, a random mix of 1 x 1 (unranged) and 2 x 2 (ranged, correlated) blocks."""
    rs = np.random.RandomState(20 + n)
    for trial in range(20):
        two = rs.uniform(size=n) < 0.5
        if n and trial == 0:
            two[:] = True
        if n and trial == 1:
            two[:] = False
        blocks = []
        for t in two:
            if t:
                a = rs.standard_normal((2, 2)) * rs.uniform(0.1, 1.0)
                blocks.append(a @ a.T + np.diag(rs.uniform(0.01, 0.5, 2)))
            else:
                blocks.append(np.array([[rs.uniform(0.05, 2.0)]]))
        rows = int(sum(len(b) for b in blocks))
        A = rs.standard_normal((rows, 3)) * rs.uniform(0.1, 3.0, 3)
        nu = rs.standard_normal(rows) * 0.3
        kap = rs.uniform(-2.0, 9.0, n)
        low = int(rs.randint(0, 4))
        want = rpr.delta_dense_blocks(A, blocks, nu, kap, low)
        got, Lam, eta = rpr.delta_formula_blocks(A, blocks, nu, kap, low)
        assert abs(got - want) <= 1e-10, (n, trial, got, want)
        if n == 0:
            assert np.array_equal(Lam, np.identity(3)) and not eta.any() and got == low * math.log(0.1)
        if not two.any():  # 1 x 1 blocks alone: proposal_reference's own two functions
            D = np.array([b[0][0] for b in blocks])
            assert abs(got - pr.delta_formula(A, D, nu, kap, low)[0]) <= 1e-10
            assert abs(want - pr.delta_dense(A, D, nu, kap, low)) <= 1e-10


def test_with_no_finite_range_the_oracle_is_the_proposal_oracle_bit_for_bit():
    world, covs = synthetic_world(12, seed=5)
    a, b = RangedProposalOracle(P, world, covs), ProposalOracle(P, world, covs)
    rs = np.random.RandomState(1)
    pose = (0.0, 0.0, 0.0)
    for s in range(8):
        prev, pose = pose, truth_step(pose, V, W, DT)
        control = pr.odom(odo.delta(prev, pose), ALPHAS) if s % 2 else pr.twist(V, W, DT)
        blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        nan = np.full(len(blobs), np.nan)
        ids_a = a.propose(control, z, blobs, nan, nan) if s % 3 else a.propose(control, z, blobs)
        ids_b = b.propose(control, z, blobs)
        assert np.array_equal(ids_a, ids_b), s
        for name in STATE[:-1] + ("xi", "dlogw", "used", "Lambda", "xhat"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), (s, name)
        anc = low_variance_ancestors(np.exp(b.logw - np.max(b.logw)), u)
        a.gather(anc)
        b.gather(anc)
    assert (ids_b > 0).any() and not a.n_rho.any()


@pytest.mark.parametrize("every", [None, 3])
def test_zero_sigmas_give_the_plain_range_bearing_step(every):
    world, covs = synthetic_world(12, seed=5)
    o, b = RangedProposalOracle(P, world, covs), RangeBearingOracle(P, world, covs)
    rs, rr = np.random.RandomState(6), np.random.RandomState(7)
    pose = (0.0, 0.0, 0.0)
    for s in range(6):
        prev, pose = pose, truth_step(pose, V, W, DT)
        d = odo.delta(prev, pose)
        blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
        rho, var = range_scan(world, pose, rr, SIGMA_R[0], SIGMA_R[1], every)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        b.reset_weights()
        b.x, b.y, b.h = odo.sample(b.x, b.y, b.h, d, np.zeros(4), z)
        want = b.observe(blobs, None, rho, var)
        got = o.propose(pr.odom(d, np.zeros(4)), z, blobs, rho, var)
        assert np.array_equal(got, want) and (got == np.arange(1, 13)).all()
        assert np.array_equal(o.x, b.x) and np.array_equal(o.y, b.y) and np.array_equal(o.h, b.h)
        assert np.array_equal(o.mean, b.mean) and np.array_equal(o.cov, b.cov) and np.array_equal(o.count, b.count)
        assert np.allclose(o.logw, b.logw, rtol=0, atol=1e-12), np.abs(o.logw - b.logw).max()
        anc = low_variance_ancestors(np.exp(b.logw - np.max(b.logw)), u)
        o.gather(anc)
        b.gather(anc)


def test_the_pose_jacobian_is_the_predicted_measurements_derivative():
    """Both rows of h_x -- the range row is the new one -- against central differences of range_bearing_reference's
    predicted_measurement in the pose (x, y, h)."""
    rs = np.random.RandomState(8)
    n = 50
    sx, sy, sh = rs.uniform(-10, 10, n), rs.uniform(-10, 10, n), rs.uniform(-2.5, 2.5, n)
    phi, dist = rs.uniform(-math.pi, math.pi, n), rs.uniform(2.0, 30.0, n)
    mean = np.stack([sx + dist * np.cos(phi), sy + dist * np.sin(phi), np.zeros(n), np.zeros(n), np.zeros(n)], axis=-1)
    H = rpr.pose_jacobian(sx, sy, mean)
    eps = 1e-6
    # central differences with step eps: truncation eps^2 |f'''| / 6 -- the third derivatives of atan2 and of the distance are at
    # most 2 / r^3 <= 0.25 for r >= 2 -- <= 5e-14; rounding 2 ulp(|f|) / (2 eps) <= 2.2e-16 * 64 / 1e-6 = 1.5e-8 for a range below
    # 32 m (ulp(32) = 7.1e-15: 7.1e-9) and a bearing below 8 rad: 2e-8 bounds their sum
    for k in range(3):
        hi, lo = [sx.copy(), sy.copy(), sh.copy()], [sx.copy(), sy.copy(), sh.copy()]
        hi[k] += eps
        lo[k] -= eps
        d = rref.predicted_measurement(hi[0], hi[1], hi[2], mean) - rref.predicted_measurement(lo[0], lo[1], lo[2], mean)
        fd = d[:, :2] / (2 * eps)
        for i in range(2):
            assert np.abs(fd[:, i] - H[:, i, k]).max() < 2e-8, (i, k, np.abs(fd[:, i] - H[:, i, k]).max())
    # ... and it is minus the landmark's own Jacobian in x, y (the update's H): what h_m is
    up = rref.ekf_update_dense(sx, sy, sh, mean, np.broadcast_to(np.identity(5), (n, 5, 5)), np.zeros(4), 1.0, 1.0, np.identity(4))[3]["H"]
    assert np.array_equal(-H[:, :, :2], up[:, :2, :2])
    # q = 0: every entry is zero
    assert not rpr.pose_jacobian(1.0, 2.0, np.array([1.0, 2.0, 0.0, 0.0, 0.0])).any()


def _drive(seed, proposal, ranged, start_map=None):
    """The turning drive under the odometry model, resampled every step: (mean n_eff / P before resampling, mean pose error, the
    oracle at the end)."""
    world, covs = synthetic_world(12, seed=5)
    rs, rr = np.random.RandomState(seed), np.random.RandomState(1000 + seed)
    f = RangedProposalOracle(P, world if start_map is None else start_map, covs)
    pose = (0.0, 0.0, 0.0)
    ne, err = [], []
    for s in range(STEPS):
        prev, pose = pose, truth_step(pose, V, W, DT)
        d = odo.delta(prev, pose)
        blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
        rho, var = range_scan(world, pose, rr, SIGMA_R[0], SIGMA_R[1])
        if not ranged:
            rho = var = None
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        if proposal:
            f.propose(pr.odom(d, ALPHAS), z, blobs, rho, var)
        else:
            f.reset_weights()
            f.x, f.y, f.h = odo.sample(f.x, f.y, f.h, d, ALPHAS, z)
            f.observe(blobs, None, rho, var)
        ne.append(pr.n_eff(f.logw) / P)
        f.gather(low_variance_ancestors(np.exp(f.logw - np.max(f.logw)), u))
        x, y, _ = f.summary()
        err.append(math.hypot(x - pose[0], y - pose[1]))
    return float(np.mean(ne)), float(np.mean(err)), f


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ranges_in_the_proposal_keep_the_particles_ranges_starve_on_the_turning_drive(seed):
    world, start, _ = rbh._pushed_map(seed)
    rows = {}
    for name, proposal, ranged in (("1.0 bearings", False, False), ("1.0 ranges", False, True), ("proposal bearings", True, False),
                                   ("proposal ranges", True, True)):
        ne, err, _ = _drive(seed, proposal, ranged)
        _, _, f = _drive(seed, proposal, ranged, start_map=start)
        rows[name] = (ne, err, rbh._map_error(f, world))
        # (printed for DESIGN.md section 4; the pose and map errors are for the record, not asserted)
        print("seed %d, %-17s: mean n_eff / P %.3f, mean pose error %.3f m | map started 0.5 m off: map error %.3f m" % ((seed, name) + rows[name]))
    assert rows["1.0 ranges"][0] < 0.5, "ranges do not starve the 1.0 filter: %.3f" % rows["1.0 ranges"][0]
    assert rows["proposal ranges"][0] > rows["1.0 ranges"][0], (seed, rows)


def test_the_scenes_of_the_gpu_tests_keep_their_margins():
    """The reference's half of tests/test_gpu_range_proposal.py: at every association (made at the predicted poses) no gate within
    rounding of turning over and no contested blob whose best probability is less than 1e-6 (relative) above the second best --
    the bounds those tests assert before they compare ids exactly -- and cond_2(Lambda) <= 1e4."""
    for what, o, control, rows in gpu_tests.ml_scenes():
        for blobs, rho, var, z in rows:
            ids = o.propose(control, z, blobs, rho, var)
            assert (ids > 0).any(), what
            assert np.linalg.cond(o.Lambda).max() <= 1e4, (what, np.linalg.cond(o.Lambda).max())
        assert_margins(o, what)
        print("%s: gate margins %.3g rad %.3g, smallest best-to-second gap %.3g, cond(Lambda) <= %.3g"
              % (what, o.min_gate_margins[0], o.min_gate_margins[1], o.min_rel_gap, np.linalg.cond(o.Lambda).max()))

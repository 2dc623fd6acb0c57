"""Host: the measurement-informed proposal's reference (tests/proposal_reference.py) against itself and against BearingOracle -- the
3 x 3 weight formula against the dense density, xi = z where nothing matches, the plain bearing step at zero sigmas, the noise
Jacobian against finite differences, and what the proposal buys on the turning drive.

The benefit, measured (64 particles, synthetic_world(12, seed=5), v = 1.0, w = 0.35, dt = 0.5, 40 steps, sigma_bearing 0.01,
odometry alphas (2, 0.2, 0.2, 0.2), resampling every step; mean n_eff / P before resampling | final summary() error):

    seed   FastSLAM 1.0 (BearingOracle)      proposal (ProposalOracle)
    1      0.330 | 0.761 m                   0.995 | 0.197 m
    2      0.339 | 0.349 m                   0.993 | 0.103 m
    3      0.324 | 0.335 m                   0.994 | 0.079 m
"""
import math

import numpy as np
import pytest

import odom_reference as odo
import proposal_reference as pr
from bearing_model_reference import BearingOracle, wrap, wrapped_scan
from oracle.fastslam_oracle import low_variance_ancestors, synthetic_world, truth_step
from proposal_reference import ProposalOracle

V, W, DT, STEPS, P = 1.0, 0.35, 0.5, 40, 64
SIGMA_B, SIGMA_C = 0.01, 0.3
# The drive under the odometry model: per move rot1 = rot2 = 0.0875 rad, trans = 0.5 m.  The filter's own bearing variance is
# Q00 + h' P h ~ 0.1 (sigma 0.32 rad; twelve blobs together: 0.09 rad), so the alphas are chosen for sigma_rot =
# sqrt(2 0.0875^2 + 0.2 0.25) = 0.26 rad and sigma_trans = sqrt(0.2 0.25 + 0.2 0.0153) = 0.23 m per move -- well above what a scan
# resolves, which leaves the 1.0 filter a third of its particles before every resampling
ALPHAS = (2.0, 0.2, 0.2, 0.2)


@pytest.mark.parametrize("n", [0, 1, 2, 40])
def test_the_3x3_formula_is_the_dense_density(n):
    rs = np.random.RandomState(10 + n)
    for _ in range(20):
        A = rs.standard_normal((n, 3)) * rs.uniform(0.1, 3.0, 3)
        D = rs.uniform(0.05, 2.0, n)
        nu = rs.standard_normal(n) * 0.3
        kap = rs.uniform(-2.0, 9.0, n)
        low = int(rs.randint(0, 4))
        want = pr.delta_dense(A, D, nu, kap, low)
        got, Lam, eta = pr.delta_formula(A, D, nu, kap, low)
        assert abs(got - want) <= 1e-10, (n, got, want)
        if n == 0:
            assert np.array_equal(Lam, np.identity(3)) and not eta.any() and got == low * math.log(0.1)


def _scene(seed=5, L=12):
    world, covs = synthetic_world(L, seed=seed)
    return world, covs


def test_xi_is_z_exactly_when_nothing_matches():
    world, covs = _scene()
    o = ProposalOracle(P, world, covs)
    rs = np.random.RandomState(4)
    z = rs.standard_normal((P, 3))
    blobs = wrapped_scan(world, (0.5, 0.0, 0.0875))
    blobs[:, 1:] += 40.0  # every colour gate fails
    plain = BearingOracle(P, world, covs)
    plain.motion(V, W, DT, z)
    ids = o.propose(pr.twist(V, W, DT), z, blobs)
    assert not ids.any() and not o.used.any()
    assert np.array_equal(o.xi, z)
    assert np.array_equal(o.x, plain.x) and np.array_equal(o.y, plain.y) and np.array_equal(o.h, plain.h)
    assert np.array_equal(o.logw, np.full(P, len(blobs) * math.log(0.1)))
    # ... and with every id supplied as 0, and with no blob at all
    o.propose(pr.odom((0.1, 0.5, 0.05), ALPHAS), z, blobs, ids=np.zeros(len(blobs), dtype=np.int32))
    assert np.array_equal(o.xi, z)
    o.propose(pr.twist(V, W, DT), z, np.zeros((0, 4)))
    assert np.array_equal(o.xi, z) and not o.logw.any()


def test_zero_sigmas_give_the_plain_bearing_step():
    world, covs = _scene()
    o, b = ProposalOracle(P, world, covs), BearingOracle(P, world, covs)
    rs = np.random.RandomState(6)
    pose = (0.0, 0.0, 0.0)
    for s in range(6):
        prev, pose = pose, truth_step(pose, V, W, DT)
        d = odo.delta(prev, pose)
        blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)  # single sightings: blob j sees landmark j
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        b.reset_weights()
        b.x, b.y, b.h = odo.sample(b.x, b.y, b.h, d, np.zeros(4), z)
        want = b.observe(blobs)
        got = o.propose(pr.odom(d, np.zeros(4)), z, blobs)
        assert np.array_equal(got, want) and (got == np.arange(1, 13)).all()
        assert np.array_equal(o.x, b.x) and np.array_equal(o.y, b.y) and np.array_equal(o.h, b.h)
        assert np.array_equal(o.mean, b.mean) and np.array_equal(o.cov, b.cov) and np.array_equal(o.count, b.count)
        assert np.allclose(o.logw, b.logw, rtol=0, atol=1e-12), np.abs(o.logw - b.logw).max()
        anc = low_variance_ancestors(np.exp(b.logw - np.max(b.logw)), u)
        o.gather(anc)
        b.gather(anc)


@pytest.mark.parametrize("kind", ["twist", "odom"])
def test_the_noise_jacobian_is_the_motion_functions_derivative(kind):
    rs = np.random.RandomState(8)
    n = 50
    x, y, h = rs.uniform(-10, 10, n), rs.uniform(-10, 10, n), rs.uniform(-2.5, 2.5, n)
    control = pr.twist(1.3, -0.4, 0.5) if kind == "twist" else pr.odom((0.3, 0.8, -0.2), ALPHAS)
    xh = pr.move(x, y, h, control, np.zeros((n, 3)))
    G = pr.noise_jacobian(control, xh[2])
    eps = 1e-6
    # central differences with step eps: truncation eps^2 |g'''| / 6 <= 1e-12 (third derivatives are at most ds <= 1), rounding
    # 2 ulp(|pose|) / (2 eps) <= 2.2e-16 * 16 / 1e-6 = 3.6e-9 for |pose| <= 13: 1e-8 bounds their sum
    for k in range(3):
        e = np.zeros((n, 3))
        e[:, k] = eps
        hi, lo = pr.move(x, y, h, control, e), pr.move(x, y, h, control, -e)
        for i in range(3):
            fd = (hi[i] - lo[i]) / (2 * eps)
            assert np.abs(fd - G[:, i, k]).max() < 1e-8, (kind, i, k, np.abs(fd - G[:, i, k]).max())


def _drive(seed, proposal):
    """The turning drive under the odometry model, resampled every step: (mean n_eff / P before resampling, final summary error)."""
    world, covs = _scene()
    rs = np.random.RandomState(seed)
    f = (ProposalOracle if proposal else BearingOracle)(P, world, covs)
    pose = (0.0, 0.0, 0.0)
    ne = []
    for s in range(STEPS):
        prev, pose = pose, truth_step(pose, V, W, DT)
        d = odo.delta(prev, pose)
        blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        if proposal:
            f.propose(pr.odom(d, ALPHAS), z, blobs)
        else:
            f.reset_weights()
            f.x, f.y, f.h = odo.sample(f.x, f.y, f.h, d, ALPHAS, z)
            f.observe(blobs)
        ne.append(pr.n_eff(f.logw) / P)
        f.gather(low_variance_ancestors(np.exp(f.logw - np.max(f.logw)), u))
    x, y, _ = f.summary()
    return float(np.mean(ne)), math.hypot(x - pose[0], y - pose[1])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_proposal_keeps_more_particles_alive_on_the_turning_drive(seed):
    ne1, err1 = _drive(seed, False)
    ne2, err2 = _drive(seed, True)
    print("seed %d: FastSLAM 1.0 n_eff/P %.3f, error %.3f m; proposal n_eff/P %.3f, error %.3f m" % (seed, ne1, err1, ne2, err2))
    assert ne1 < 0.5, "the alphas do not starve the 1.0 filter: %.3f" % ne1
    assert ne2 > ne1, (seed, ne1, ne2)

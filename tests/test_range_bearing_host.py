"""CPU: the yardstick of range-bearing scans (tests/range_bearing_reference.py) -- that it IS the bearing model's where no blob has a
range, that its update and weight are the textbook's, and what ranges buy on the turning drive of tests/test_bearing_model_host.py
(64 particles, synthetic_world(12, seed=5), 40 steps, sigma 0.01 rad and 0.3 per colour channel) with range noise 0.05 + 0.01 rho.
No GPU, no library: this file passes with or without the feature."""
import math

import numpy as np
import pytest

from oracle.fastslam_oracle import low_variance_ancestors, synthetic_world, truth_step

import range_bearing_reference as rref
import test_gpu_range_bearing as gpu_tests
from bearing_model_reference import BearingOracle, wrap, wrapped_scan
from range_bearing_reference import RangeBearingOracle, range_scan

V, W, DT, STEPS, P = 1.0, 0.35, 0.5, 40, 64
SIGMA_B, SIGMA_C = 0.01, 0.3
SIGMA_R = (0.05, 0.01)
STATE = ("x", "y", "h", "logw", "mean", "cov", "count", "potential", "n_unmatched")


def _pushed_map(seed):
    """The map's starting positions 0.5 m (one sigma of their covariance) off the truth."""
    world, covs = synthetic_world(12, seed=5)
    start = world.copy()
    start[:, :2] += 0.5 * np.random.RandomState(100 + seed).standard_normal((12, 2))
    return world, start, covs


def _drive(seed, ranged, every=None, start_map=None, P=P, steps=STEPS):
    """The turning drive: per step the share of (particle, blob) pairs matched to the blob's own landmark and the pose error; at
    the end the oracle.  ranged: the scans carry ranges (every = k: each k-th blob has none)."""
    world, covs = synthetic_world(12, seed=5)
    rs, rr = np.random.RandomState(seed), np.random.RandomState(1000 + seed)
    f = RangeBearingOracle(P, world if start_map is None else start_map, covs)
    pose = (0.0, 0.0, 0.0)
    own, err = [], []
    for s in range(steps):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
        rho, var = range_scan(world, pose, rr, SIGMA_R[0], SIGMA_R[1], every)
        z = rs.standard_normal((P, 3))
        u = float(rs.uniform())
        f.reset_weights()
        f.motion(V, W, DT, z)
        ids = f.observe(blobs, None, rho, var) if ranged else f.observe(blobs)
        own.append(float(np.mean(ids == np.arange(1, 13)[None, :])))
        f.gather(low_variance_ancestors(np.exp(f.logw - np.max(f.logw)), u))
        x, y, h = f.summary()
        err.append((math.hypot(x - pose[0], y - pose[1]), abs(float(wrap(h - pose[2])))))
    return np.array(own), np.array(err), f


def _map_error(f, world):
    """Mean over the landmarks of the distance between the particles' mean estimate and the truth."""
    est = f.mean[:, :, :2].mean(axis=0)
    return float(np.mean(np.hypot(est[:, 0] - world[:, 0], est[:, 1] - world[:, 1])))


def test_with_no_finite_range_the_oracle_is_the_bearing_oracle_bit_for_bit():
    world, covs = synthetic_world(12, seed=5)
    a, b = RangeBearingOracle(P, world, covs), BearingOracle(P, world, covs)
    rs = np.random.RandomState(1)
    pose = (0.0, 0.0, 0.0)
    for s in range(12):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world, pose, rs, SIGMA_B, SIGMA_C)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        for f in (a, b):
            f.reset_weights()
            f.motion(V, W, DT, z)
        nan = np.full(len(blobs), np.nan)
        ids_a = a.observe(blobs, None, nan, nan) if s % 2 else a.observe(blobs)
        ids_b = b.observe(blobs)
        assert np.array_equal(ids_a, ids_b), s
        for name in STATE:
            assert np.array_equal(getattr(a, name), getattr(b, name)), (s, name)
        anc = low_variance_ancestors(np.exp(b.logw - np.max(b.logw)), u)
        a.gather(anc)
        b.gather(anc)
    assert (ids_b > 0).any()


def _random_case(rs):
    sx, sy, sh = rs.uniform(-3, 3), rs.uniform(-3, 3), rs.uniform(-3, 3)
    phi, dist = rs.uniform(-math.pi, math.pi), rs.uniform(2.0, 30.0)
    mean = np.array([sx + dist * math.cos(phi), sy + dist * math.sin(phi), *rs.uniform(0, 255, 3)])
    a, c = rs.standard_normal((2, 2)), rs.standard_normal((3, 3))
    cov = np.zeros((5, 5))
    cov[:2, :2] = 0.3 * (a @ a.T) + 0.05 * np.identity(2)
    cov[2:, 2:] = c @ c.T + 0.5 * np.identity(3)
    blob = np.array([float(wrap(phi - sh + rs.uniform(-0.3, 0.3))), *(mean[2:] + rs.uniform(-6, 6, 3))])
    rho = dist + rs.uniform(-0.5, 0.5)
    return sx, sy, sh, mean, cov, blob, rho, rs.uniform(0.01, 0.5) ** 2


def test_the_update_is_the_textbook_ekf_and_the_weight_the_gaussian_density():
    rs = np.random.RandomState(4)
    Qt = np.diag([0.02, 0.1, 0.2, 0.3])
    for i in range(200):
        sx, sy, sh, mean, cov, blob, rho, q_rho = _random_case(rs)
        nm, nc, lw, aux = rref.ekf_update_dense(sx, sy, sh, mean, cov, blob, rho, q_rho, Qt)
        # H against a central-difference Jacobian of (bearing, range, r, g, b) in the landmark's five coordinates
        J = np.empty((5, 5))
        for k in range(5):
            step = 1e-5 * max(1.0, abs(mean[k]))
            hi, lo = mean.copy(), mean.copy()
            hi[k] += step
            lo[k] -= step
            d = rref.predicted_measurement(sx, sy, sh, hi) - rref.predicted_measurement(sx, sy, sh, lo)
            d[0] = float(wrap(d[0]))
            J[:, k] = d / (2 * step)
        assert np.allclose(aux["H"], J, rtol=1e-7, atol=1e-8), (i, np.abs(aux["H"] - J).max())
        # the weight: the 5-D Gaussian density of the innovation, written out term by term with no matrix library
        S, d = aux["S"], aux["delz"]
        assert np.array_equal(S[:2, 2:], np.zeros((2, 3)))  # position and colour do not couple on the compact layout
        a, b, c = S[0, 0], S[0, 1], S[1, 1]
        det2 = a * c - b * b
        maha2 = (c * d[0] ** 2 - 2 * b * d[0] * d[1] + a * d[1] ** 2) / det2
        C = S[2:, 2:]
        det3 = (C[0, 0] * (C[1, 1] * C[2, 2] - C[1, 2] * C[2, 1]) - C[0, 1] * (C[1, 0] * C[2, 2] - C[1, 2] * C[2, 0])
                + C[0, 2] * (C[1, 0] * C[2, 1] - C[1, 1] * C[2, 0]))
        maha3 = float(d[2:] @ np.linalg.solve(C, d[2:]))
        want = -0.5 * (5 * math.log(2 * math.pi) + math.log(det2 * det3) + maha2 + maha3)
        assert abs(lw - want) < 1e-10 * max(1.0, abs(want)), (i, lw, want)
        # ... and the posterior is the information-form one: Sigma'^-1 = Sigma^-1 + H' R^-1 H
        R = rref.measurement_noise(Qt, q_rho)
        info = np.linalg.inv(cov) + aux["H"].T @ np.linalg.inv(R) @ aux["H"]
        assert np.allclose(np.linalg.inv(nc), info, rtol=1e-7, atol=1e-9), i
    # q = 0: both position rows of H vanish, the position stays, the innovation's range is the whole range
    mean = np.array([1.0, -2.0, 10.0, 20.0, 30.0])
    nm, nc, lw, aux = rref.ekf_update_dense(1.0, -2.0, 0.4, mean, 0.25 * np.identity(5), np.array([0.1, 11.0, 19.0, 31.0]), 3.0, 0.04, Qt)
    assert not aux["H"][:2].any() and np.array_equal(nm[:2], mean[:2]) and aux["delz"][1] == 3.0
    assert np.array_equal(nc[:2, :2], 0.25 * np.identity(2))


def test_the_depth_pair_is_told_apart_by_the_range_and_by_nothing_else():
    """Two landmarks of one colour on one ray: at (8, 0) and (14, 0), seen from the origin, a blob at bearing 0."""
    means = np.array([[8.0, 0.0, 120.0, 60.0, 200.0], [14.0, 0.0, 120.0, 60.0, 200.0]])
    covs = np.broadcast_to(0.25 * np.identity(5), (2, 5, 5)).copy()
    blob = np.array([[0.0, 120.0, 60.0, 200.0]])
    for rho, want in ((8.0, 1), (14.0, 2), (np.nan, 1)):
        f = RangeBearingOracle(4, means, covs)
        ids = f.associate(blob, [rho], [(0.05 + 0.01 * rho) ** 2])
        assert np.array_equal(ids, np.full((4, 1), want)), (rho, ids)
        if rho == rho:
            assert f.min_rel_gap > 1 - 1e-12  # the other landmark is thirty sigma off
    assert np.array_equal(BearingOracle(4, means, covs).associate(blob), np.ones((4, 1)))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ranges_pull_a_pushed_map_back_on_the_turning_drive(seed):
    world, start, _ = _pushed_map(seed)
    own_r, err_r, fr = _drive(seed, True, start_map=start)
    own_b, err_b, fb = _drive(seed, False, start_map=start)
    assert np.all(own_r == 1.0), "with ranges a blob was not matched to its own landmark at steps %s" % (np.nonzero(own_r < 1.0)[0],)
    e_r, e_b = _map_error(fr, world), _map_error(fb, world)
    # (printed for DESIGN.md section 4; the pose errors are for the record, not asserted: the pose does not gain on this drive)
    print("seed %d: landmarks' mean distance from the truth %.3f m bearing-only, %.3f m with ranges; pose error mean / max "
          "%.3f / %.3f m bearing-only, %.3f / %.3f m with ranges; smallest best-to-second gap %.3g, gate margins %.3g rad %.3g"
          % (seed, e_b, e_r, err_b[:, 0].mean(), err_b[:, 0].max(), err_r[:, 0].mean(), err_r[:, 0].max(), fr.min_rel_gap,
             fr.min_gate_margins[0], fr.min_gate_margins[1]))
    assert e_r < e_b, (e_r, e_b)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mixed_scans_keep_every_blob_on_its_own_landmark(seed):
    own, _, f = _drive(seed, True, every=3)
    assert np.all(own == 1.0), np.nonzero(own < 1.0)[0]
    own, _, f = _drive(seed, True, every=3, start_map=_pushed_map(seed)[1])
    assert np.all(own == 1.0), np.nonzero(own < 1.0)[0]


@pytest.mark.parametrize("kind", ["all", "mixed"])
@pytest.mark.parametrize("L,B,P", gpu_tests.SHAPES)
def test_the_scenes_of_the_gpu_tests_keep_their_margins(L, B, P, kind):
    """The reference's half of tests/test_gpu_range_bearing.py's drives: no gate within rounding of turning over, no contested blob
    whose best probability is less than 1e-6 (relative) above the second best -- the bounds those tests assert before they compare."""
    _, _, rows, o = gpu_tests.oracle_drive(L, B, P, kind)
    gpu_tests.assert_margins(o, (L, kind))
    print("L %d %s: gate margins %.3g rad %.3g, smallest best-to-second gap %.3g" % (L, kind, o.min_gate_margins[0], o.min_gate_margins[1], o.min_rel_gap))
    assert all((r["ids"] > 0).any() for r in rows)

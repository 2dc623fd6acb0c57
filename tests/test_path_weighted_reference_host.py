"""CPU: the weighted path estimate's reference (path_weighted_reference.py) on cases worked by hand, and the host class
``path.WeightedPathSummary``."""
import math

import numpy as np

import path_reference as pr
import path_weighted_reference as pw


def two_by_two():
    """Two particles, one recorded row and the current one; the particles kept their order."""
    poses = np.array([[(0, 0, 0), (4, 8, math.pi / 2)]], dtype=np.float64)
    ancestors = np.array([[0, 1]])
    current = np.array([(1, 1, 0), (5, 3, 0)], dtype=np.float64)
    return poses, ancestors, current


def test_two_particles_two_rows_weights_three_to_one():
    poses, ancestors, current = two_by_two()
    for logw, is_log in (([math.log(3.0), 0.0], False), ([math.log(3.0), 0.0], True), ([5.0 + math.log(3.0), 5.0], True)):
        mean, spread, n_eff = pw.summary(poses, ancestors, current, np.array(logw), is_log)
        # row 0: x = 0, 4 and y = 0, 8 by 3 : 1 -- mean (1, 2); var x = (3 1 + 1 9) / 4, cov = (3 2 + 1 18) / 4, var y = (3 4 + 1 36) / 4;
        # headings 0 and a quarter turn: sum w sin = 1, sum w cos = 3
        assert np.allclose(mean[0], [1.0, 2.0, math.atan2(1.0, 3.0)], rtol=1e-14, atol=0)
        assert np.allclose(spread[0], [3.0, 6.0, 12.0, math.sqrt(10.0) / 4.0], rtol=1e-14, atol=0)
        # row 1, the current generation: x = 1, 5 and y = 1, 3 -- mean (2, 1.5); var x = (3 1 + 9) / 4, cov = (3 .5 + 3 1.5) / 4, var y = (3 .25 + 2.25) / 4
        assert np.allclose(mean[1], [2.0, 1.5, 0.0], rtol=1e-14, atol=0)
        assert np.allclose(spread[1], [3.0, 1.5, 0.75, 1.0], rtol=1e-14, atol=0)
        assert abs(n_eff - 1.6) <= 1e-14  # (3 + 1)^2 / (9 + 1)


def test_a_zero_weight_contributes_nothing():
    rs = np.random.RandomState(3)
    P, T = 6, 3
    poses, current = rs.uniform(-5, 5, (T, P, 3)), rs.uniform(-5, 5, (P, 3))
    anc = np.tile(np.arange(P), (T, 1))  # identity maps: the rows are the particles' own
    logw = rs.uniform(-3, 0, P)
    logw[4] = -np.inf
    mean, spread, n_eff = pw.summary(poses, anc, current, logw, True)
    keep = np.arange(P) != 4
    mean5, spread5, n_eff5 = pw.summary(poses[:, keep], np.tile(np.arange(P - 1), (T, 1)), current[keep], logw[keep], True)
    assert np.allclose(mean, mean5, rtol=1e-13, atol=1e-13) and np.allclose(spread, spread5, rtol=1e-13, atol=0) and abs(n_eff - n_eff5) <= 1e-14 * n_eff
    # ... also when it is particle 0, whose lineage is the reference pose
    logw0 = logw.copy()
    logw0[4], logw0[0] = -1.0, -np.inf
    mean, spread, n_eff = pw.summary(poses, anc, current, logw0, False)
    keep = np.arange(P) != 0
    mean5, spread5, n_eff5 = pw.summary(poses[:, keep], np.tile(np.arange(P - 1), (T, 1)), current[keep], logw0[keep], False)
    assert np.allclose(mean, mean5, rtol=1e-13, atol=1e-13) and np.allclose(spread, spread5, rtol=1e-13, atol=0) and abs(n_eff - n_eff5) <= 1e-14 * n_eff
    # only one particle left with a weight: its own path, no spread
    only = np.full(P, -np.inf)
    only[2] = -7.0
    mean, spread, n_eff = pw.summary(poses, anc, current, only, True)
    # (about particle 0's lineage, as on the device: x0 + (x2 - x0), a rounding away from x2)
    assert np.allclose(mean[:T, :2], poses[:, 2, :2], rtol=0, atol=4e-15) and np.allclose(mean[T, :2], current[2, :2], rtol=0, atol=4e-15)
    assert np.all(spread[:, :3] == 0.0) and np.allclose(spread[:, 3], 1.0, rtol=1e-15) and n_eff == 1.0


def test_a_coalesced_row_is_its_pose_with_no_spread():
    rs = np.random.RandomState(4)
    P, T = 9, 3
    poses, current = rs.uniform(-5, 5, (T, P, 3)), rs.uniform(-5, 5, (P, 3))
    anc = rs.randint(0, P, (T, P))
    anc[1] = 7  # every particle of generation 2 descends from generation 1's particle 7 -- and so from generation 0's anc[0][7]
    logw = rs.uniform(-4, 0, P)
    mean, spread, _ = pw.summary(poses, anc, current, logw, True)
    for t, j in ((1, 7), (0, anc[0][7])):
        assert mean[t, 0] == poses[t, j, 0] and mean[t, 1] == poses[t, j, 1]
        assert pr.angle_diff(mean[t, 2], poses[t, j, 2]) < 1e-15
        assert spread[t, :3].tolist() == [0.0, 0.0, 0.0] and abs(spread[t, 3] - 1.0) < 1e-15
    assert np.all(spread[2:, [0, 2]] > 0.0)


def test_uniform_weights_are_the_plain_path_summary():
    rs = np.random.RandomState(5)
    P, T = 41, 4
    poses, current = rs.uniform(-5, 5, (T, P, 3)), rs.uniform(-5, 5, (P, 3))
    anc = rs.randint(0, P, (T, P))
    want_mean, want_spread, _ = pr.summary(poses, anc, current)
    for logw, is_log in ((np.zeros(P), False), (np.full(P, -3.25), True), (np.full(P, -3.25), False)):
        mean, spread, n_eff = pw.summary(poses, anc, current, logw, is_log)
        assert np.allclose(mean, want_mean, rtol=1e-14, atol=1e-15) and np.allclose(spread, want_spread, rtol=1e-13, atol=0)
        assert abs(n_eff - P) <= 1e-13 * P


def test_the_exact_products():
    rs = np.random.RandomState(6)
    a, b = rs.standard_normal(200) * 1e6, rs.standard_normal(200) * 1e-7
    p, e = pw.two_product(a, b)
    from fractions import Fraction

    for x, y, pp, ee in zip(a, b, p, e):
        assert Fraction(x) * Fraction(y) == Fraction(pp) + Fraction(ee)
    assert pw.dot(a, b) == float(sum(Fraction(x) * Fraction(y) for x, y in zip(a, b)))


def test_the_checker_holds_its_bounds():
    poses, ancestors, current = two_by_two()
    logw = np.array([math.log(3.0), 0.0])
    mean, spread, n_eff = pw.summary(poses, ancestors, current, logw, False)

    class Got(object):
        pass

    def got(dm=0.0, dv=0.0, dn=0.0):
        g = Got()
        g.mean, g.spread, g.n_eff = mean.copy(), spread.copy(), n_eff * (1.0 + dn)
        g.mean[0, 0] *= 1.0 + dm
        g.spread[1, 2] *= 1.0 + dv
        return g

    pw.check(got(), poses, ancestors, current, logw, False)
    pw.check(got(dm=5e-13, dv=5e-13, dn=5e-13), poses, ancestors, current, logw, False)
    for bad in (got(dm=1e-11), got(dv=3e-12), got(dn=3e-12)):
        try:
            pw.check(bad, poses, ancestors, current, logw, False)
        except AssertionError:
            continue
        raise AssertionError("a figure beyond its bound passed")
    # an exact zero must be met exactly
    anc = np.array([[1, 1]])
    mean, spread, n_eff = pw.summary(poses, anc, current, logw, False)
    assert spread[0, :3].tolist() == [0.0, 0.0, 0.0]
    g = got()
    g.spread[0, 0] = 1e-300
    try:
        pw.check(g, poses, anc, current, logw, False)
    except AssertionError:
        pass
    else:
        raise AssertionError("a variance that should be exactly zero passed")


def test_weighted_path_summary_class_and_as_poses():
    from parakeet_slam_amd import path as pkpath

    poses, ancestors, current = two_by_two()
    mean, spread, n_eff = pw.summary(poses, ancestors, current, np.array([math.log(3.0), 0.0]), False)
    s = pkpath.WeightedPathSummary(mean.ravel(), spread.ravel(), np.float64(n_eff), 5)
    assert s.mean.shape == (2, 3) and s.spread.shape == (2, 4) and s.held == 1 and s.first_step == 5
    assert isinstance(s.n_eff, float) and s.n_eff == n_eff
    assert s.steps().tolist() == [5, 6]
    assert "n_eff" in repr(s)
    track = pkpath.as_poses(s)
    assert track == [tuple(float(v) for v in row) for row in mean] and all(type(v) is float for row in track for v in row)
    plain = pkpath.PathSummary(mean, spread, [2, 2], 0)
    assert pkpath.as_poses(plain) == track == pkpath.as_poses(mean)

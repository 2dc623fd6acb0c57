"""CPU: the path estimate's reference (path_reference.py) on cases worked by hand."""
import math

import numpy as np

import path_reference as pr


def hand_case():
    poses = np.array([[(0, 0, 0), (1, 2, 0.1), (2, 4, 0.2), (3, 6, 0.3)],
                      [(10, 0, 0), (11, 1, 0), (12, 2, 0), (13, 3, 0)]], dtype=np.float64)
    ancestors = np.array([[1, 1, 3, 3],    # generation 1's particles 0, 1 descend from generation 0's particle 1; 2, 3 from 3
                          [0, 0, 0, 2]])   # the current particles 0, 1, 2 descend from generation 1's particle 0; 3 from 2
    current = np.array([(20, 0, 0), (21, 0, 0), (22, 0, 0), (23, 0, 0)], dtype=np.float64)
    return poses, ancestors, current


def test_four_particles_two_rows_by_hand():
    poses, ancestors, current = hand_case()
    J = pr.lineages(ancestors, 4)
    assert J.tolist() == [[1, 1, 1, 3], [0, 0, 0, 2], [0, 1, 2, 3]]
    X = pr.paths(poses, ancestors, current)
    assert X[0].tolist() == [[1, 2, 0.1], [10, 0, 0], [20, 0, 0]]
    assert X[2].tolist() == [[1, 2, 0.1], [10, 0, 0], [22, 0, 0]]
    assert X[3].tolist() == [[3, 6, 0.3], [12, 2, 0], [23, 0, 0]]
    mean, spread, surv = pr.summary(poses, ancestors, current)
    assert surv.tolist() == [2, 2, 4]
    assert pr.survivors(ancestors, 4).tolist() == [2, 2, 4]
    # row 1: x = 10 10 10 12, y = 0 0 0 2, headings 0
    assert mean[1].tolist() == [10.5, 0.5, 0.0] and spread[1].tolist() == [0.75, 0.75, 0.75, 1.0]
    # row 0: x = 1 1 1 3, y = 2 2 2 6, headings .1 .1 .1 .3
    s, c = 3 * math.sin(0.1) + math.sin(0.3), 3 * math.cos(0.1) + math.cos(0.3)
    assert mean[0, :2].tolist() == [1.5, 3.0] and abs(mean[0, 2] - math.atan2(s, c)) < 1e-15
    assert spread[0, :3].tolist() == [0.75, 1.5, 3.0] and abs(spread[0, 3] - math.hypot(s, c) / 4) < 1e-15
    # row 2, the current generation: x = 20 21 22 23
    assert mean[2].tolist() == [21.5, 0.0, 0.0] and spread[2].tolist() == [1.25, 0.0, 0.0, 1.0]


def random_ring(rs, P, T):
    return rs.uniform(-5, 5, (T, P, 3)), rs.uniform(-5, 5, (P, 3))


def test_identity_ancestors_every_particle_survives():
    rs = np.random.RandomState(1)
    P, T = 37, 4
    poses, current = random_ring(rs, P, T)
    anc = np.tile(np.arange(P), (T, 1))
    mean, spread, surv = pr.summary(poses, anc, current)
    assert surv.tolist() == [P] * (T + 1)
    X = pr.paths(poses, anc, current)
    assert np.array_equal(X[:, :T], poses.transpose(1, 0, 2)) and np.array_equal(X[:, T], current)
    assert np.allclose(mean[:T, :2], poses[:, :, :2].mean(axis=1), rtol=1e-13, atol=1e-14)
    assert np.allclose(spread[:T, 0], poses[:, :, 0].var(axis=1), rtol=1e-12)
    assert np.allclose(spread[:T, 1], [np.cov(p[:, 0], p[:, 1], bias=True)[0, 1] for p in poses], rtol=1e-11)


def test_constant_ancestors_one_survivor_its_pose_and_no_spread():
    rs = np.random.RandomState(2)
    P, T = 29, 3
    poses, current = random_ring(rs, P, T)
    anc = np.tile(np.arange(P), (T, 1))
    anc[1] = 11  # every particle of generation 2 descends from generation 1's particle 11
    mean, spread, surv = pr.summary(poses, anc, current)
    assert surv.tolist() == [1, 1, P, P]  # ... and so from ONE particle of generation 0 too: anc[0][11] = 11
    for t in (0, 1):
        assert mean[t, 0] == poses[t, 11, 0] and mean[t, 1] == poses[t, 11, 1]
        assert abs(pr.angle_diff(mean[t, 2], poses[t, 11, 2])) < 1e-15
        assert spread[t, :3].tolist() == [0.0, 0.0, 0.0] and abs(spread[t, 3] - 1.0) < 1e-15


def test_unsorted_maps_compose():
    P = 5
    anc = np.array([[4, 3, 2, 1, 0], [2, 2, 0, 4, 4]])
    assert pr.lineages(anc, P).tolist() == [[2, 2, 4, 0, 0], [2, 2, 0, 4, 4], [0, 1, 2, 3, 4]]
    assert pr.survivors(anc, P).tolist() == [3, 3, 5]


def test_the_tolerance_helpers():
    assert pr.close([1.0, 0.0], [1.0 + 5e-13, 0.0]) and not pr.close([1.0], [1.0 + 2e-12]) and not pr.close([1e-300], [0.0])
    assert pr.angle_diff(math.pi - 1e-13, -math.pi + 1e-13) < 1e-12

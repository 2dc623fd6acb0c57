"""CPU: the reference of the discovered-landmark tests (map_match_reference.py) on hand-made cases with known answers, and the
host side of the estimate (mapsum.MatchedMoments, finish_matched, DiscoveredMap.as_features) against it."""
import numpy as np
import pytest

from map_match_reference import COLOUR_RADIUS, RADIUS, check, match_table, moments_of, planted_state, reference
from mapsum_reference import POT

L0 = 2
R = np.array([[10.0, 20.0, 100.0, 50.0, 200.0]])  # one reference feature


def particle(*slots, spare=4, used=None):
    """(1, L0 + spare, 5) means of one particle holding `slots` in its spare slots, and its u_p."""
    m = np.zeros((1, L0 + spare, 5))
    m[0, :L0] = [[500.0, 500.0, 1.0, 2.0, 3.0], [600.0, 500.0, 3.0, 2.0, 1.0]]
    m[0, L0:] = R[0]  # (beyond u_p: exact copies of the reference feature, which nobody may read)
    for i, s in enumerate(slots):
        m[0, L0 + i] = s
    return m, np.array([len(slots) if used is None else used])


def one(m, u, radius=RADIUS, colour_radius=COLOUR_RADIUS, ref=R):
    t, passing, tie = match_table(m, u, L0, ref, radius, colour_radius)
    return int(t[0, 0]), int(passing[0, 0]), bool(tie[0, 0])


def test_a_colour_decoy_inside_the_position_gate_is_not_matched():
    m, u = particle(R[0] + [1.0, 0, 100.0, 0, 0])
    assert one(m, u) == (-1, 0, False)
    m, u = particle(R[0] + [1.0, 0, 100.0, 0, 0], R[0] + [2.0, 0, 1.0, 0, 0])  # ... and the true one behind it is
    assert one(m, u) == (1, 1, False)


def test_the_right_colour_just_outside_the_radius_is_not_matched():
    m, u = particle(R[0] + [RADIUS + 0.05, 0, 0, 0, 0])
    assert one(m, u) == (-1, 0, False)
    m, u = particle(R[0] + [RADIUS, 0, 0, 0, 0])  # on the radius: dpos2 == rho^2 passes (<=)
    assert one(m, u) == (0, 1, False)
    m, u = particle(R[0] + [0, 0, 0, COLOUR_RADIUS, 0])
    assert one(m, u) == (0, 1, False)
    m, u = particle(R[0] + [0, 0, 0, COLOUR_RADIUS + 0.5, 0])
    assert one(m, u) == (-1, 0, False)


def test_of_two_passing_candidates_the_nearer_wins():
    far, near = R[0] + [1.5, 0, 0, 0, 0], R[0] + [0.01, -0.02, 0.3, 0, 0]
    assert one(*particle(far, near)) == (1, 2, False)
    assert one(*particle(near, far)) == (0, 2, False)
    # position and colour weigh by their radii: 1.5 / 3 in position loses to 12 / 30 in colour
    assert one(*particle(R[0] + [1.5, 0, 0, 0, 0], R[0] + [0, 0, 12.0, 0, 0])) == (1, 2, False)


def test_an_exact_tie_goes_to_the_lower_slot():
    left, right = R[0] - [0.5, 0, 0, 0, 0], R[0] + [0.5, 0, 0, 0, 0]
    assert one(*particle(left, right)) == (0, 2, True)
    assert one(*particle(right, left)) == (0, 2, True)
    assert one(*particle(R[0] + [2.0, 0, 0, 0, 0], right, left)) == (1, 3, True)


def test_infinite_radii():
    anywhere = R[0] + [1e5, -1e5, 0, 0, 0]
    assert one(*particle(anywhere))[0] == -1
    assert one(*particle(anywhere), radius=np.inf) == (0, 1, False)  # position plays no part: score = the colour term
    assert one(*particle(anywhere, R[0] + [3e5, 0, 1.0, 0, 0]), radius=np.inf) == (0, 2, False)
    assert one(*particle(anywhere + [0, 0, 2.0, 0, 0], R[0] + [3e5, 0, 1.0, 0, 0]), radius=np.inf) == (1, 2, False)
    odd = R[0] + [1.0, 0, 200.0, 0, 0]
    assert one(*particle(odd))[0] == -1
    assert one(*particle(odd), colour_radius=np.inf) == (0, 1, False)


def test_both_radii_infinite_take_the_first_slot_in_use():
    """Both terms of the score vanish: every candidate scores 0 and the lowest slot in use wins."""
    m, u = particle(R[0] + [1e5, 0, 77.0, 0, 0], R[0])
    assert one(m, u, radius=np.inf, colour_radius=np.inf) == (0, 2, True)
    assert one(*particle(), radius=np.inf, colour_radius=np.inf) == (-1, 0, False)


def test_nan_means_fail_the_gates():
    bad = R[0].copy()
    bad[3] = np.nan
    assert one(*particle(bad, R[0] + [1.0, 0, 0, 0, 0])) == (1, 1, False)
    assert one(*particle(bad), radius=np.inf, colour_radius=np.inf)[0] == -1


def test_no_spare_slot_in_use_and_slots_beyond_the_count():
    m, u = particle()
    assert one(m, u) == (-1, 0, False)  # (the copies of the reference feature beyond u_p are not candidates)
    m, u = particle(R[0] + [9.0, 0, 0, 0, 0], R[0], used=1)
    assert one(m, u) == (-1, 0, False)
    m, u = particle(R[0] + [9.0, 0, 0, 0, 0], R[0], used=99)  # clamped to the spare slots there are
    assert one(m, u)[0] == 1


def hand_population():
    """Three particles about two features; the second feature is held by nobody."""
    ref = np.array([[0.0, 0.0, 10.0, 10.0, 10.0], [50.0, 0.0, 200.0, 10.0, 10.0]])
    means = np.zeros((3, L0 + 2, 5))
    means[:, :L0] = 900.0
    means[0, L0] = ref[0] + [1.0, 0, 0, 0, 0]
    means[1, L0 + 1] = ref[0] + [-1.0, 0, 0, 0, 0]
    means[1, L0] = [70.0, 70.0, 0, 0, 0]
    means[2, L0] = ref[0] + [0.0, 2.0, 0, 0, 0]
    used = np.array([1, 2, 1])
    covs = np.broadcast_to(np.identity(5), (3, L0 + 2, 5, 5)).copy()
    covs[1] *= 3.0
    counts = np.array([[0, 0, 4, 0], [0, 0, 0, 6 | POT], [0, 0, 8, 0]], dtype=np.int32)
    return ref, means, covs, counts, used


def test_an_unmatched_feature_is_nan_with_support_zero_and_known_moments():
    ref, means, covs, counts, used = hand_population()
    r = reference(means, covs, counts, used, L0, ref, RADIUS, COLOUR_RADIUS)
    assert r.matches.tolist() == [[0, -1], [1, -1], [0, -1]]
    assert r.support.tolist() == [1.0, 0.0] and np.isnan(r.mean[1]).all() and np.isnan(r.cov[1]).all() and np.isnan(r.n_eff[1])
    assert np.allclose(r.mean[0], [0.0, 2.0 / 3.0, 10.0, 10.0, 10.0], atol=1e-15)
    assert np.allclose(r.between[0, :2, :2], [[2.0 / 3.0, 0.0], [0.0, 8.0 / 9.0]])
    assert np.allclose(r.within[0], np.identity(5) * 5.0 / 3.0)
    assert r.count[0] == 6.0 and r.potential_fraction[0] == 1.0 / 3.0 and r.n_eff[0] == 3.0 and r.n_eff_all == 3.0


def test_a_particle_of_weight_zero_counts_for_nothing():
    ref, means, covs, counts, used = hand_population()
    r = reference(means, covs, counts, used, L0, ref, RADIUS, COLOUR_RADIUS, w=[1.0, 0.0, 3.0])
    assert r.matches.tolist() == [[0, -1], [1, -1], [0, -1]]  # (matched all the same)
    assert r.support[0] == 1.0 and r.potential_fraction[0] == 0.0 and r.count[0] == 7.0
    assert np.allclose(r.mean[0], [0.25, 1.5, 10.0, 10.0, 10.0]) and np.allclose(r.within[0], np.identity(5))
    assert r.n_eff[0] == 16.0 / 10.0
    alone = reference(means, covs, counts, used, L0, ref[:1], RADIUS, COLOUR_RADIUS, w=[0.0, 1.0, 0.0])
    assert np.array_equal(alone.mean[0], means[1, L0 + 1]) and np.array_equal(alone.between[0], np.zeros((5, 5)))
    nobody = reference(means[:1], covs[:1], counts[:1], used[:1], L0, ref[:1], RADIUS, COLOUR_RADIUS, w=[0.0])
    assert nobody.matches.tolist() == [[0]] and nobody.Wj[0] == 0.0 and np.isnan(nobody.mean[0]).all()


@pytest.mark.parametrize("weighted", [False, True])
def test_finish_matched_against_the_reference(weighted):
    from parakeet_slam_amd import mapsum

    st = planted_state(300, 3, 6, seed=4)
    w = np.exp(np.random.RandomState(1).normal(0.0, 1.0, size=300)) if weighted else None
    r = reference(st["means"], st["covs"], st["counts"], st["used"], 3, st["truth"], RADIUS, COLOUR_RADIUS, w)
    assert 0.1 < r.support.min() and r.support.max() < 0.9
    got = mapsum.finish_matched(moments_of(r), st["truth"])
    check(got, r, what="finish_matched")
    assert got.reference_particle is None and np.array_equal(got.ids, np.arange(1, 7)) and np.array_equal(got.reference_mean, st["truth"])
    with pytest.raises(ValueError):
        mapsum.finish_matched(moments_of(r), st["truth"][:5])
    # with a feature nobody holds
    ref = np.vstack([st["truth"], [[-300.0, -300.0, 5.0, 5.0, 5.0]]])
    r = reference(st["means"], st["covs"], st["counts"], st["used"], 3, ref, RADIUS, COLOUR_RADIUS, w)
    got = mapsum.finish_matched(moments_of(r), ref)
    check(got, r, what="finish_matched, a feature nobody holds")
    assert got.support[6] == 0.0 and np.isnan(got.cov[6]).all()


def test_as_features_filters_by_support_and_promotion():
    from parakeet_slam_amd import mapsum

    n = 5
    mean = np.arange(n * 5, dtype=np.float64).reshape(n, 5)
    mean[4] = np.nan
    eye = np.broadcast_to(np.identity(5), (n, 5, 5))
    d = mapsum.DiscoveredMap(mean, eye, 2 * eye, [3.4, 7.6, 9.0, 1.0, np.nan], support=[0.9, 0.6, 0.3, 0.5, 0.0],
                             potential_fraction=[0.1, 0.7, 0.0, 0.49, np.nan], n_eff=[9, 6, 3, 5, np.nan], n_eff_all=10.0,
                             reference_particle=7, ids=[41, 44, 42, 47, 43], slots=[40, 41, 42, 43, 44],
                             ref_counts=[3, 1 | POT, 9, 2, POT])
    assert d.potential.tolist() == [False, True, False, False, True] and d.ref_update_count.tolist() == [3, 1, 9, 2, 0]
    f = d.as_features()
    assert sorted(f) == [41, 47]  # support >= 0.5 and mostly promoted
    assert np.array_equal(f[41].mean, mean[0]) and np.array_equal(f[41].covar, 3 * np.identity(5)) and f[41].update_count == 3
    assert sorted(d.as_features(promoted_only=False)) == [41, 44, 47]
    assert sorted(d.as_features(min_support=0.0)) == [41, 42, 47]  # (the NaN row never)
    assert sorted(d.as_features(min_support=0.0, promoted_only=False)) == [41, 42, 44, 47]
    assert sorted(d.as_features(min_support=0.95)) == []


def test_the_generator_keeps_its_promises_at_every_shape_of_the_gpu_tests():
    for P, S in ((1, 1), (3, 6), (257, 64), (1000, 6), (257, 70)):
        st = planted_state(P, 5, S, seed=P + S)
        assert st["means"].shape == (P, 5 + S, 5) and (st["used"] <= S).all()

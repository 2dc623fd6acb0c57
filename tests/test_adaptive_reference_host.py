"""CPU: the reference of the adaptive-resampling tests (adaptive_reference.py) against closed forms -- before the GPU tests hold
the device to it."""
import math
from fractions import Fraction

import numpy as np
import pytest

import adaptive_reference as ar


@pytest.fixture(autouse=True)
def wide_longdouble():
    ar.need_longdouble()


def logw_of(w):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(w, dtype=np.float64))


@pytest.mark.parametrize("log_domain", [False, True])
@pytest.mark.parametrize("P,m", [(1, 1), (64, 1), (1024, 300), (4097, 4096)])
def test_ones_and_zeros_count_the_ones_exactly(P, m, log_domain):
    w = np.zeros(P)
    w[np.random.RandomState(P).permutation(P)[:m]] = 1.0
    s1, s2, n_eff = ar.sums(logw_of(w), log_domain)
    assert (s1, s2, n_eff) == (float(m), float(m), float(m))
    theta = m / float(P)
    assert ar.keeps(logw_of(w), log_domain, theta) and ar.margin(logw_of(w), log_domain, theta) == 0.0
    if m > 1:
        w[np.flatnonzero(w)[0]] = 0.0
        assert not ar.keeps(logw_of(w), log_domain, theta)


@pytest.mark.parametrize("log_domain", [False, True])
def test_equal_weights_are_all_effective(log_domain):
    for P, w in ((1, 3.0), (63, 1.0), (1000, 0.125), (4097, 7.0)):
        lw = np.full(P, math.log(w))
        s1, s2, n_eff = ar.sums(lw, log_domain)
        assert ar.rel(n_eff, P) <= 1e-15
        assert ar.keeps(lw, log_domain, 0.999) and not ar.keeps(lw, log_domain, 2.0)
        assert ar.shift_of(lw, log_domain) == (math.log(w) if log_domain else 0.0)


def test_ones_and_epsilons_in_a_known_ratio():
    eps = 2.0 ** -10  # log and exp of a power of two: the weights are what was meant to within an ulp
    for a, b in ((1, 1), (10, 1000), (300, 724), (1, 4096)):
        w = np.concatenate([np.ones(a), np.full(b, eps)])
        e = Fraction(eps)
        want = (a + b * e) ** 2 / (a + b * e * e)
        for log_domain in (False, True):
            s1, s2, n_eff = ar.sums(logw_of(w), log_domain)
            assert ar.rel(s1, float(a + b * e)) <= 1e-15 and ar.rel(s2, float(a + b * e * e)) <= 1e-15
            assert ar.rel(n_eff, float(want)) <= 1e-15, (a, b, n_eff, float(want))
    # the log domain divides every weight by the largest: n_eff does not move
    lw = logw_of(np.random.RandomState(1).uniform(0.1, 1.0, 500) ** 12) - 700.0
    assert ar.rel(ar.sums(lw, True)[2], ar.sums(lw + 700.0, False)[2]) <= 1e-13
    assert ar.sums(lw - 100.0, False)[0] == 0.0 and math.isnan(ar.sums(lw - 100.0, False)[2])  # underflown: every weight zero
    assert not ar.keeps(lw - 100.0, False, 0.0)  # NaN fails the comparison: resample


def test_all_zero_weights_resample_in_both_domains():
    lw = np.full(70, -np.inf)
    for log_domain in (False, True):
        s1, s2, n_eff = ar.sums(lw, log_domain)
        assert s1 == 0.0 and s2 == 0.0 and math.isnan(n_eff)
        assert not ar.keeps(lw, log_domain, 0.5)
        assert ar.shift_of(lw, log_domain) == 0.0


def test_weighted_pose_summary_closed_forms():
    # two particles, weights 3 : 1
    poses = np.array([[1.0, 2.0, 0.0], [5.0, 10.0, 0.0]])
    mean, spread, n_eff = ar.pose_summary(poses, logw_of([3.0, 1.0]), False)
    assert np.allclose(mean, [2.0, 4.0, 0.0], rtol=1e-15, atol=0)
    assert np.allclose(spread, [3.0, 6.0, 12.0, 1.0], rtol=1e-15)  # var = p (1 - p) d^2 = 3/16 * (16, 32, 64)
    assert ar.rel(n_eff, 16.0 / 10.0) <= 1e-15
    # equal poses: their pose, bit for bit, and exactly no spread
    poses = np.tile([[1e6 + 0.1, -3.3, 0.7]], (50, 1))
    mean, spread, _ = ar.pose_summary(poses, logw_of(np.random.RandomState(2).uniform(0.1, 1, 50)), True)
    assert mean[0] == poses[0, 0] and mean[1] == poses[0, 1] and abs(mean[2] - 0.7) <= 1e-15
    assert np.all(spread[:3] == 0.0) and abs(spread[3] - 1.0) <= 1e-15
    # equal weights: the plain moments
    rs = np.random.RandomState(3)
    poses = np.column_stack([rs.uniform(10, 20, 400), rs.uniform(-5, 5, 400), rs.uniform(-0.5, 0.5, 400)])
    mean, spread, n_eff = ar.pose_summary(poses, np.zeros(400), True)
    assert np.allclose(mean[:2], poses[:, :2].mean(axis=0), rtol=1e-13)
    assert np.allclose(spread[:3], [poses[:, 0].var(), np.cov(poses[:, 0], poses[:, 1], bias=True)[0, 1], poses[:, 1].var()], rtol=1e-12)
    assert ar.rel(n_eff, 400.0) <= 1e-15
    # headings opposite and equally heavy: no resultant
    mean, spread, _ = ar.pose_summary(np.array([[0.0, 0, 0.0], [1.0, 0, math.pi]]), np.zeros(2), False)
    assert spread[3] <= 1e-16

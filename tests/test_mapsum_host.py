"""CPU: parakeet_slam_amd/mapsum.py -- combine_moments (Chan's pairwise update over shard moments) and finish, on random shard
splits against the direct two-pass computation over all particles (mapsum_reference.py, where the tolerances are stated).

Half the landmarks sit 1e6 from the origin with a particle spread of 1e-3: raw second moments (sum w mu mu^T - W mean mean^T)
lose every digit of their between-particle covariance there (1e12 against 1e-6 in float64)."""
import numpy as np
import pytest

from mapsum_reference import POT, block_diagonal_covs, check, moments_of, two_pass

L, P = 12, 1000
FAR = np.arange(L) % 2 == 1  # the landmarks offset by 1e6


def population(seed, weighted):
    rs = np.random.RandomState(seed)
    centre = rs.uniform(-30.0, 30.0, size=(L, 5))
    centre[:, 2:] = rs.uniform(0.0, 255.0, size=(L, 3))
    spread = np.where(FAR, 1e-3, rs.uniform(0.01, 0.5, size=L))
    centre[FAR] += 1e6
    means = centre + spread[None, :, None] * rs.standard_normal((P, L, 5))
    covs = block_diagonal_covs(rs, P, L)
    counts = rs.randint(0, 40, size=(P, L)).astype(np.int32)
    counts[rs.uniform(size=(P, L)) < 0.1] |= POT
    w = np.exp(rs.normal(0.0, 2.0, size=P)) if weighted else None
    return means, covs, counts, w


def split(sizes):
    edges = np.concatenate([[0], np.cumsum(sizes)])
    assert edges[-1] == P
    return [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


SPLITS = {
    "two": [617, 383],
    "three": [1, 700, 299],  # one part is a single particle
    "eight": [5, 250, 1, 144, 300, 64, 200, 36],
}


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", sorted(SPLITS))
def test_combined_shard_moments_give_the_two_pass_estimate(name, weighted):
    from parakeet_slam_amd import mapsum

    means, covs, counts, w = population(3 + len(name), weighted)
    ref = two_pass(means, covs, counts, w)
    parts = [moments_of(means[s], covs[s], counts[s], None if w is None else w[s]) for s in split(SPLITS[name])]
    got = mapsum.finish(mapsum.combine_moments(parts))
    check(got, ref, what="%s parts%s" % (name, ", weighted" if weighted else ""))
    assert np.array_equal(got.ids, np.arange(1, L + 1))
    assert np.array_equal(got.cov, got.cov_within + got.cov_between)
    # Where the landmarks are far out the between-particle covariance (1e-6) is far below 1e-10 of the total (0.2 and more), so
    # the check above says nothing about it.  What Chan's update can give there: a part's mean is one double, off the part's
    # true mean by eps <= ulp(1e6) / 2 = 6e-11 (a few of those for a NumPy sum of hundreds of values near 1e6), which enters
    # delta delta^T Wa Wb / W in first order -- relative to W sigma^2 at most (delta / sigma)(eps / sigma) / 2 per join, with
    # delta / sigma <= 4 (a single particle against the rest) and eps / sigma <= 5e-7: 1e-6 a join, 1e-5 over eight parts.
    # Raw second moments are off by 1e2 and more.
    d = np.einsum("lii->li", got.cov_between)[FAR] / np.einsum("lii->li", ref.between)[FAR] - 1.0
    print("between diagonals of the far landmarks, worst relative error %.3g" % np.abs(d).max())
    assert np.abs(d).max() < 1e-5


def test_one_part_is_itself_and_the_flat_block_round_trips():
    from parakeet_slam_amd import mapsum

    means, covs, counts, w = population(1, True)
    m = moments_of(means, covs, counts, w)
    flat = m.flat()
    assert flat.shape == (2 + 30 * L,)
    back = mapsum.Moments.from_flat(flat)
    one = mapsum.combine_moments([back])
    for a in ("wsum", "mean", "m2", "within", "counts"):
        assert np.array_equal(getattr(one, a), getattr(m, a)), a
    check(mapsum.finish(one), two_pass(means, covs, counts, w), what="one part")
    with pytest.raises(ValueError):
        mapsum.Moments.from_flat(np.zeros(2 + 30 * L + 1))
    with pytest.raises(ValueError):
        mapsum.combine_moments([])


def test_rows_outside_the_estimate_stay_nan_and_leave_as_features():
    from parakeet_slam_amd import mapsum

    means, covs, counts, w = population(2, False)
    parts = []
    for s in split([400, 600]):
        m = moments_of(means[s], covs[s], counts[s])
        for a in (m.mean, m.m2, m.within, m.counts):
            a[L - 3:] = np.nan  # what pk_map_moments hands out for the spare slots of a growing filter
        parts.append(m)
    got = mapsum.finish(mapsum.combine_moments(parts))
    ref = two_pass(means, covs, counts)
    check(got, ref, rows=slice(0, L - 3), what="rows inside")
    for a in (got.mean, got.cov, got.cov_within, got.cov_between, got.update_count):
        assert np.isnan(a[L - 3:]).all() and not np.isnan(a[:L - 3]).any()
    feats = got.as_features()
    assert sorted(feats) == list(range(1, L - 2))
    assert np.array_equal(feats[2].mean, got.mean[1]) and np.array_equal(feats[2].covar, got.cov[1])


def test_weighting_names():
    from parakeet_slam_amd import mapsum

    assert mapsum.weighting_code("uniform") == 0 and mapsum.weighting_code("weights") == 1
    assert mapsum.weighting_code(0) == 0 and mapsum.weighting_code(1) == 1
    for bad in ("log", 2, None, -1):
        with pytest.raises(ValueError):
            mapsum.weighting_code(bad)

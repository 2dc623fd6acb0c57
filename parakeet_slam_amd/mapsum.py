"""The map estimate on the host side: what ``pk_map_moments`` hands out per shard, combined over shards and finished.

NumPy only.  A shard's *moments* of every landmark over its particles (weights ``w_p``, ``W = sum w_p``):

    wsum    (2,)      W, sum w_p^2
    mean    (L, 5)    sum w_p mu_p / W
    m2      (L, 15)   sum w_p (mu_p - mean)(mu_p - mean)^T about THIS shard's mean, upper triangle row-major
    within  (L, 9)    sum w_p Sigma_p, the compact fields pxx pxy pyy crr crg crb cgg cgb cbb
    counts  (L,)      sum w_p update_count_p

``combine_moments`` joins shards with Chan's pairwise update (no raw second moments: a landmark far from the origin keeps
its digits), ``finish`` divides by W.  Rows the estimate does not cover (the spare slots of a growing filter) are NaN
throughout and stay NaN.

Those spare slots have an estimate of their own, the discovered landmarks (second half of this file): ``MatchedMoments`` is what
``pk_map_match_moments`` hands out about a list of reference features, ``finish_matched`` divides every feature by ITS matched
weight, ``DiscoveredMap`` is the finished estimate with the share of the population behind every feature.
"""
from __future__ import annotations

import numpy as np

UNIFORM, WEIGHTED = 0, 1  # PK_MAP_UNIFORM, PK_MAP_WEIGHTED

_TRI = np.triu_indices(5)
# compact field -> (row, column) of the dense 5x5 (pk_layout.hpp: F_PXX ... F_CBB)
_WITHIN_IJ = ((0, 0), (0, 1), (1, 1), (2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (4, 4))


def weighting_code(weighting):
    """"uniform" / "weights" (or the ABI's 0 / 1) -> PK_MAP_UNIFORM / PK_MAP_WEIGHTED."""
    if isinstance(weighting, str):
        if weighting in ("uniform", "weights"):
            return UNIFORM if weighting == "uniform" else WEIGHTED
    elif weighting in (UNIFORM, WEIGHTED):
        return int(weighting)
    raise ValueError("weighting must be 'uniform' or 'weights', not %r" % (weighting,))


class Moments(object):
    """One shard's (or several combined shards') moments; ``flat()`` is the block the ranks exchange: 2 + 30 L doubles."""

    def __init__(self, wsum, mean, m2, within, counts):
        self.wsum = np.asarray(wsum, dtype=np.float64).reshape(2)
        self.mean = np.asarray(mean, dtype=np.float64).reshape(-1, 5)
        L = self.mean.shape[0]
        self.m2 = np.asarray(m2, dtype=np.float64).reshape(L, 15)
        self.within = np.asarray(within, dtype=np.float64).reshape(L, 9)
        self.counts = np.asarray(counts, dtype=np.float64).reshape(L)

    @property
    def L(self):
        return self.mean.shape[0]

    def flat(self):
        return np.concatenate([self.wsum, self.mean.ravel(), self.m2.ravel(), self.within.ravel(), self.counts])

    @classmethod
    def from_flat(cls, a):
        a = np.asarray(a, dtype=np.float64).ravel()
        L, rest = divmod(a.size - 2, 30)
        if a.size < 2 or rest:
            raise ValueError("a moments block holds 2 + 30 L doubles, not %d" % a.size)
        return cls(a[:2], a[2:2 + 5 * L], a[2 + 5 * L:2 + 20 * L], a[2 + 20 * L:2 + 29 * L], a[2 + 29 * L:])


def combine_moments(parts):
    """Chan's pairwise update over a list of shard moments, in list order:
    W = Wa + Wb, delta = mean_b - mean_a, mean = mean_a + delta Wb / W, M2 = M2a + M2b + delta delta^T Wa Wb / W;
    within, counts, sum w and sum w^2 add."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_moments: no parts")
    a = parts[0]
    wsum, mean, m2, within, counts = a.wsum.copy(), a.mean.copy(), a.m2.copy(), a.within.copy(), a.counts.copy()
    for b in parts[1:]:
        if b.L != a.L:
            raise ValueError("combine_moments: parts of %d and %d landmarks" % (a.L, b.L))
        Wa, Wb = wsum[0], b.wsum[0]
        W = Wa + Wb
        delta = b.mean - mean
        mean = mean + delta * (Wb / W)
        m2 = m2 + b.m2 + delta[:, _TRI[0]] * delta[:, _TRI[1]] * (Wa * Wb / W)
        within = within + b.within
        counts = counts + b.counts
        wsum = wsum + b.wsum
    return Moments(wsum, mean, m2, within, counts)


class MapSummary(object):
    """The finished estimate.  ids (L,) 1 ... L (the reference's feature ids, prkt_core_v2.py:294-299); mean (L, 5);
    cov_within (L, 5, 5) the EKFs' own uncertainty, averaged; cov_between (L, 5, 5) how much the particles disagree;
    cov = cov_within + cov_between, the moment-matched covariance of the mixture; update_count (L,) the average number of
    updates; n_eff = W^2 / sum w^2.  Rows the estimate does not cover are NaN."""

    def __init__(self, mean, cov_within, cov_between, update_count, n_eff):
        self.mean = np.asarray(mean, dtype=np.float64).reshape(-1, 5)
        L = self.mean.shape[0]
        self.ids = np.arange(1, L + 1)
        self.cov_within = np.asarray(cov_within, dtype=np.float64).reshape(L, 5, 5)
        self.cov_between = np.asarray(cov_between, dtype=np.float64).reshape(L, 5, 5)
        self.cov = self.cov_within + self.cov_between
        self.update_count = np.asarray(update_count, dtype=np.float64).reshape(L)
        self.n_eff = float(n_eff)

    def as_features(self):
        """{id: Feature(mean, covar)} with the total covariance; NaN rows are left out."""
        from .core import Feature

        out = {}
        for i, l in enumerate(self.ids):
            if np.isnan(self.mean[i, 0]):
                continue
            f = Feature(mean=self.mean[i].copy(), covar=self.cov[i].copy())
            f.update_count = int(round(self.update_count[i]))
            out[int(l)] = f
        return out


def finish(moments):
    """Moments -> MapSummary."""
    m = moments
    L, W = m.L, m.wsum[0]
    between = np.empty((L, 5, 5))
    between[:, _TRI[0], _TRI[1]] = m.m2 / W
    between[:, _TRI[1], _TRI[0]] = m.m2 / W
    within = np.zeros((L, 5, 5))
    within[np.isnan(m.within[:, 0])] = np.nan
    for k, (i, j) in enumerate(_WITHIN_IJ):
        within[:, i, j] = within[:, j, i] = m.within[:, k] / W
    return MapSummary(m.mean, within, between, m.counts / W, W * W / m.wsum[1])


# ---- the discovered landmarks: the spare slots of a growing filter, matched across the particles (pk_map_match_moments)
POTENTIAL = 0x40000000  # PK_LANDMARK_POTENTIAL


class MatchedMoments(object):
    """The unfinished moments of the spare slots matched to n reference features (what shards would combine):

        wsum     (2,)      W, sum w_p^2 over ALL particles
        support  (n, 3)    per feature W_j = sum w over its matches, sum w^2, sum w over the matches still potential
        mean     (n, 5)    r_j + sum w (mu - r_j) / W_j
        m2       (n, 15)   sum w (mu - mean)(mu - mean)^T, upper triangle row-major
        within   (n, 9)    sum w Sigma, compact fields
        counts   (n,)      sum w update_count
        matches  (P, n)    the spare slot of particle p matched to feature j, -1 = none (None: not asked for)

    A slot matches a feature inside both radii and the smallest normalised distance wins, per feature: NOT one-to-one."""

    def __init__(self, wsum, support, mean, m2, within, counts, matches=None):
        self.wsum = np.asarray(wsum, dtype=np.float64).reshape(2)
        self.mean = np.asarray(mean, dtype=np.float64).reshape(-1, 5)
        n = self.mean.shape[0]
        self.support = np.asarray(support, dtype=np.float64).reshape(n, 3)
        self.m2 = np.asarray(m2, dtype=np.float64).reshape(n, 15)
        self.within = np.asarray(within, dtype=np.float64).reshape(n, 9)
        self.counts = np.asarray(counts, dtype=np.float64).reshape(n)
        self.matches = None
        if matches is not None:
            t = np.asarray(matches, dtype=np.int32)
            self.matches = t.reshape(t.shape[0] if t.ndim == 2 else -1, n)  # ((P, 0) stays (P, 0))

    @property
    def n(self):
        return self.mean.shape[0]


class DiscoveredMap(object):
    """The estimate of the discovered landmarks, one row per reference feature: mean (n, 5); cov_within, cov_between, cov
    (n, 5, 5) as in ``MapSummary``; update_count (n,); support (n,) = W_j / W, the share of the population whose particles hold
    the feature; potential_fraction (n,), the share of those that still hold it as a potential feature; n_eff (n,) = W_j^2 /
    sum_j w^2 and n_eff_all of the whole population.  From ``map_discovered``: reference_particle, and that particle's own ids
    (its feature ids: ids are per particle), slots (landmark index of every feature in its map), potential and
    ref_update_count; from ``finish_matched``: reference_particle None, ids 1 .. n, reference_mean the reference features.  A
    feature nobody matched has support 0 and NaN elsewhere.  The matches behind it are per feature, NOT one-to-one."""

    def __init__(self, mean, cov_within, cov_between, update_count, support, potential_fraction, n_eff, n_eff_all,
                 reference_particle=None, ids=None, slots=None, ref_counts=None, reference_mean=None):
        self.mean = np.array(mean, dtype=np.float64).reshape(-1, 5)
        n = self.mean.shape[0]
        self.cov_within = np.array(cov_within, dtype=np.float64).reshape(n, 5, 5)
        self.cov_between = np.array(cov_between, dtype=np.float64).reshape(n, 5, 5)
        self.cov = self.cov_within + self.cov_between
        self.update_count = np.array(update_count, dtype=np.float64).reshape(n)
        self.support = np.array(support, dtype=np.float64).reshape(n)
        self.potential_fraction = np.array(potential_fraction, dtype=np.float64).reshape(n)
        self.n_eff = np.array(n_eff, dtype=np.float64).reshape(n)
        self.n_eff_all = float(n_eff_all)
        self.reference_particle = reference_particle
        self.ids = np.arange(1, n + 1) if ids is None else np.array(ids, dtype=np.int64).reshape(n)
        self.slots = None if slots is None else np.array(slots, dtype=np.int64).reshape(n)
        self.potential = self.ref_update_count = None
        if ref_counts is not None:
            c = np.array(ref_counts, dtype=np.int64).reshape(n)
            self.potential = (c & POTENTIAL) != 0
            self.ref_update_count = c & ~POTENTIAL
        self.reference_mean = None if reference_mean is None else np.array(reference_mean, dtype=np.float64).reshape(n, 5)

    def as_features(self, min_support=0.5, promoted_only=True):
        """{id: Feature(mean, covar)} with the total covariance, of the features at least ``min_support`` of the population
        holds; promoted_only: and that less than half of their holders still keep as a potential feature."""
        from .core import Feature

        out = {}
        for i, l in enumerate(self.ids):
            if not self.support[i] >= min_support or np.isnan(self.mean[i, 0]):
                continue
            if promoted_only and not self.potential_fraction[i] < 0.5:
                continue
            f = Feature(mean=self.mean[i].copy(), covar=self.cov[i].copy())
            f.update_count = int(round(self.update_count[i]))
            out[int(l)] = f
        return out


def finish_matched(moments, ref_means):
    """MatchedMoments (about the reference features ref_means (n, 5)) -> DiscoveredMap."""
    m = moments
    ref = np.asarray(ref_means, dtype=np.float64).reshape(-1, 5)
    if ref.shape[0] != m.n:
        raise ValueError("finish_matched: %d reference features for moments of %d" % (ref.shape[0], m.n))
    n, W = m.n, m.wsum[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        Wj = m.support[:, 0]
        between = np.empty((n, 5, 5))
        between[:, _TRI[0], _TRI[1]] = m.m2 / Wj[:, None]
        between[:, _TRI[1], _TRI[0]] = m.m2 / Wj[:, None]
        within = np.zeros((n, 5, 5))
        within[~(Wj > 0.0)] = np.nan
        for k, (i, j) in enumerate(_WITHIN_IJ):
            within[:, i, j] = within[:, j, i] = m.within[:, k] / Wj
        return DiscoveredMap(m.mean, within, between, m.counts / Wj, Wj / W, m.support[:, 2] / Wj, Wj * Wj / m.support[:, 1],
                             W * W / m.wsum[1], reference_mean=ref)

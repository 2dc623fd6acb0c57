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

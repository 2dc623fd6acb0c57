"""Adaptive resampling on the host side: what ``pk_resample_stats`` and ``pk_summary_weighted`` hand out.

NumPy only.  A filter that resamples adaptively (``FastSLAM(..., resample_threshold=theta)``) resamples only when the effective
sample size ``n_eff = (sum w)^2 / sum w^2`` of its weights falls below ``theta * P``; otherwise the weights carry over into the next
step, and the estimate is the WEIGHTED mean of the particles, not their plain mean.
"""
from __future__ import annotations

import numpy as np


class ResampleStats(object):
    """What the last gated call decided, and the counters since the filter was made.

    n_eff, s1, s2   of the weights the call looked at: w = exp(logw - shift), s1 = sum w, s2 = sum w^2, n_eff = s1 / s2 * s1
    shift           what the weight scan subtracted: the maximum log-weight in the log domain, 0 in the linear one
    resampled       True: the call resampled; False: it kept the particles and their (renormalised) weights
    calls           gated calls so far (one per step)
    resamples       how many of them resampled
    """

    def __init__(self, n_eff, s1, s2, shift, resampled, calls, resamples):
        self.n_eff, self.s1, self.s2, self.shift = float(n_eff), float(s1), float(s2), float(shift)
        self.resampled = bool(resampled)
        self.calls, self.resamples = int(calls), int(resamples)

    def __repr__(self):
        return "ResampleStats(n_eff=%.6g, resampled=%s, calls=%d, resamples=%d)" % (self.n_eff, self.resampled, self.calls, self.resamples)


class PoseSummary(object):
    """The pose estimate by the particles' weights.

    mean    (3,)  weighted mean x, mean y, circular mean heading
    spread  (4,)  var x, cov xy, var y, mean resultant length R of the headings (1: all agree) -- ``path.PathSummary``'s figures
    n_eff         the effective sample size of the weights
    """

    def __init__(self, mean, spread, n_eff):
        self.mean = np.asarray(mean, dtype=np.float64).reshape(3)
        self.spread = np.asarray(spread, dtype=np.float64).reshape(4)
        self.n_eff = float(n_eff)

    def pose(self):
        """(x, y, heading) as plain floats: what ``summary()`` returns."""
        return float(self.mean[0]), float(self.mean[1]), float(self.mean[2])

    def covariance(self):
        """The 2 x 2 position covariance."""
        return np.array([[self.spread[0], self.spread[1]], [self.spread[1], self.spread[2]]])

    def __repr__(self):
        return "PoseSummary(mean=%s, n_eff=%.6g)" % (self.mean.tolist(), self.n_eff)


def threshold_value(resample_threshold):
    """``resample_threshold`` as the float the device takes; ValueError unless it is a finite number >= 0."""
    try:
        theta = float(resample_threshold)
    except (TypeError, ValueError):
        raise ValueError("resample_threshold must be None (resample at every step) or a number >= 0, not %r" % (resample_threshold,))
    if not (np.isfinite(theta) and theta >= 0.0):
        raise ValueError("resample_threshold must be finite and >= 0 (a share of the particle count), not %r" % (resample_threshold,))
    return theta

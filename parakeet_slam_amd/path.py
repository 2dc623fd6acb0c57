"""The path estimate on the host side: what ``pk_path_summary`` and ``pk_path_summary_weighted`` hand out, and their way into a
``nav_msgs/Path``.

NumPy only.  Row convention, as everywhere in the path estimate: rows ``0 .. held - 1`` are the recorded steps, oldest first --
each the generation a resample worked on, at the pose the scan was applied --, row ``held`` is the current generation.
"""
from __future__ import annotations

import numpy as np


class PathSummary(object):
    """The smoothed path over the surviving lineages, every current particle counting once.

    mean       (held + 1, 3)  mean x, mean y, circular mean heading of the P lineages in that row
    spread     (held + 1, 4)  var x, cov xy, var y, mean resultant length R of the headings (1: all agree)
    survivors  (held + 1,)    distinct ancestors the population still has in that row: P in a fresh row, 1 once it has coalesced
    first_step                the global index of row 0: rows ever recorded - rows held
    """

    def __init__(self, mean, spread, survivors, first_step):
        self.mean = np.asarray(mean, dtype=np.float64).reshape(-1, 3)
        n = self.mean.shape[0]
        self.spread = np.asarray(spread, dtype=np.float64).reshape(n, 4)
        self.survivors = np.asarray(survivors, dtype=np.int64).reshape(n)
        self.first_step = int(first_step)

    @property
    def held(self):
        return self.mean.shape[0] - 1

    def steps(self):
        """The global step index of every row (the current generation's is the number of rows ever recorded)."""
        return self.first_step + np.arange(self.mean.shape[0])

    def __repr__(self):
        return "PathSummary(held=%d, first_step=%d, survivors=%s)" % (self.held, self.first_step, self.survivors.tolist())


class WeightedPathSummary(object):
    """The smoothed path by the weights of the current particles (``pk_path_summary_weighted``): the estimate between an observe
    and a resample, where the particles do not count alike.

    mean       (held + 1, 3)  weighted mean x, mean y, circular mean heading of the lineages in that row
    spread     (held + 1, 4)  var x, cov xy, var y over the sum of the weights, mean resultant length R of the headings
    n_eff                     the effective sample size of the current weights (one number: every row is weighted by them)
    first_step                the global index of row 0: rows ever recorded - rows held
    """

    def __init__(self, mean, spread, n_eff, first_step):
        self.mean = np.asarray(mean, dtype=np.float64).reshape(-1, 3)
        n = self.mean.shape[0]
        self.spread = np.asarray(spread, dtype=np.float64).reshape(n, 4)
        self.n_eff = float(n_eff)
        self.first_step = int(first_step)

    @property
    def held(self):
        return self.mean.shape[0] - 1

    def steps(self):
        """The global step index of every row (the current generation's is the number of rows ever recorded)."""
        return self.first_step + np.arange(self.mean.shape[0])

    def __repr__(self):
        return "WeightedPathSummary(held=%d, first_step=%d, n_eff=%.6g)" % (self.held, self.first_step, self.n_eff)


def as_poses(summary):
    """``summary.mean`` as the list of (x, y, heading) tuples of plain floats a ``nav_msgs/Path`` is filled from, oldest first."""
    mean = summary.mean if isinstance(summary, (PathSummary, WeightedPathSummary)) else np.asarray(summary, dtype=np.float64).reshape(-1, 3)
    return [(float(x), float(y), float(h)) for x, y, h in mean]

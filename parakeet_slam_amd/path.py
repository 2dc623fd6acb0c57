"""The path estimate on the host side: what ``pk_path_summary`` and ``pk_path_summary_weighted`` hand out, the whole run's path
(the trunk of settled rows in front of them), and their way into a ``nav_msgs/Path``.

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


TRUNK_RES = 13  # doubles of a trunk row (kPathTrunkRes)


class FullPath(object):
    """The path of the whole run: the trunk's settled rows, then the ring's, then the current generation.

    mean       (n, 3)  x, y, heading per step: of a final row the recorded pose of its one ancestor, bit for bit
    spread     (n, 4)  var x, cov xy, var y, mean resultant length R of the headings ((0, 0, 0, 1) for a final trunk row)
    final      (n,)    every current particle descends from ONE ancestor in that row: no later step can change it
    in_trunk   (n,)    the row has left the ring (its estimate was taken when it was settled, by the weights of that moment)
    ancestors  (n, 2)  the lowest and highest lineage index of a trunk row; -1 for the ring's rows
    first_step         the global index of row 0
    """

    def __init__(self, mean, spread, final, in_trunk, ancestors, first_step):
        self.mean = np.asarray(mean, dtype=np.float64).reshape(-1, 3)
        n = self.mean.shape[0]
        self.spread = np.asarray(spread, dtype=np.float64).reshape(n, 4)
        self.final = np.asarray(final, dtype=bool).reshape(n)
        self.in_trunk = np.asarray(in_trunk, dtype=bool).reshape(n)
        self.ancestors = np.asarray(ancestors, dtype=np.int64).reshape(n, 2)
        self.first_step = int(first_step)

    @classmethod
    def assemble(cls, trunk, summary, ring_final):
        """``trunk``: (mean, spread, ancestors, first_step) of the settled rows or None; ``summary``: the PathSummary /
        WeightedPathSummary of the ring, which follows it without a gap; ``ring_final`` (held + 1,): which of its rows are final."""
        m = summary.mean.shape[0]
        if trunk is None:
            t_mean, t_spread, t_anc, first = np.empty((0, 3)), np.empty((0, 4)), np.empty((0, 2), dtype=np.int64), summary.first_step
        else:
            t_mean, t_spread, t_anc, first = trunk
            t_mean, t_spread = np.asarray(t_mean, dtype=np.float64).reshape(-1, 3), np.asarray(t_spread, dtype=np.float64).reshape(-1, 4)
            t_anc = np.asarray(t_anc, dtype=np.int64).reshape(-1, 2)
            if int(first) + t_mean.shape[0] != summary.first_step:
                raise ValueError("FullPath: a trunk of steps [%d, %d) does not meet a ring that begins at step %d"
                                 % (first, int(first) + t_mean.shape[0], summary.first_step))
        n = t_mean.shape[0]
        return cls(np.concatenate([t_mean, summary.mean]), np.concatenate([t_spread, summary.spread]),
                   np.concatenate([t_anc[:, 0] == t_anc[:, 1], np.asarray(ring_final, dtype=bool).reshape(m)]),
                   np.concatenate([np.ones(n, dtype=bool), np.zeros(m, dtype=bool)]),
                   np.concatenate([t_anc, np.full((m, 2), -1, dtype=np.int64)]), first)

    def steps(self):
        """The global step index of every row (the current generation's is the number of rows ever recorded)."""
        return self.first_step + np.arange(self.mean.shape[0])

    def __repr__(self):
        return "FullPath(steps=[%d, %d], in_trunk=%d, final=%d)" % (self.first_step, self.first_step + self.mean.shape[0] - 1,
                                                                    int(self.in_trunk.sum()), int(self.final.sum()))


def as_poses(summary):
    """``summary.mean`` as the list of (x, y, heading) tuples of plain floats a ``nav_msgs/Path`` is filled from, oldest first."""
    mean = summary.mean if isinstance(summary, (PathSummary, WeightedPathSummary, FullPath)) else np.asarray(summary, dtype=np.float64).reshape(-1, 3)
    return [(float(x), float(y), float(h)) for x, y, h in mean]

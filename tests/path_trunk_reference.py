"""Reference for the trunk of the path estimate (pk_path_settle, pk_path_trunk_*), shared by the tests: a NumPy restatement of
the definitions in include/parakeet_slam.h, built on ``path_reference.lineages`` and ``path_weighted_reference.summary``.

A ring of T rows as in path_reference.py.  Settling its oldest E rows leaves one trunk row of 13 doubles per settled row t:

    0-7    mean x, mean y, sum w sin h, sum w cos h, var x, cov xy, var y, S1 of pose_t[j_t(k)] by the weights of the current
           particles k -- path_weighted_reference's moments, which are delegated to it with its tolerance TOL = 1e-12
    8, 9   lo_t = min_k j_t(k), hi_t = max_k j_t(k) over ALL current particles (exact); the row is FINAL iff they are equal
    10-12  pose_t[lo_t] (exact: a gather)

and the ring without those rows.  Weighting: 0 linear, 1 log (path_weighted_reference's domains), 2 uniform -- every particle once,
which is the log domain with every log-weight 0.
"""
import math

import numpy as np

import path_weighted_reference as pw
from path_reference import lineages

TOL = pw.TOL
RES = 13
LIN, LOG, UNIFORM = 0, 1, 2


def span(ancestors, P):
    """(lo (T + 1,), hi (T + 1,)): the lowest and highest lineage index of every row over all current particles."""
    J = lineages(ancestors, P)
    return J.min(axis=1), J.max(axis=1)


def final_rows(ancestors, P):
    lo, hi = span(ancestors, P)
    return lo == hi


def effective_logw(logw, weighting, P):
    """(log-weights, domain_is_log) path_weighted_reference takes for this weighting."""
    if weighting == UNIFORM:
        return np.zeros(P), True
    return np.asarray(logw, dtype=np.float64), weighting == LOG


class Settled(object):
    """What settling rows 0 .. E - 1 of a ring must leave: per settled row lo, hi, the ancestor's pose, the estimate (mean (E, 3),
    spread (E, 4)) and S1; and the rows of the ring that stay."""

    def __init__(self, poses, ancestors, current, logw, weighting, E):
        current = np.asarray(current, dtype=np.float64)
        P = current.shape[0]
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, P, 3)
        anc = np.asarray(ancestors, dtype=np.int64).reshape(-1, P)
        assert 0 <= E <= anc.shape[0]
        lo, hi = span(anc, P)
        self.E, self.P = E, P
        self._settled_poses, self._settled_anc = poses[:E], anc[:E].astype(np.int32)
        self.lo, self.hi = lo[:E], hi[:E]
        self.final = self.lo == self.hi
        self.pose = np.array([poses[t][lo[t]] for t in range(E)]).reshape(E, 3)
        lw, is_log = effective_logw(logw, weighting, P)
        mean, spread, _ = pw.summary(poses, anc, current, lw, is_log)
        self.mean, self.spread = mean[:E], spread[:E]
        self.s1 = math.fsum(pw.weights(lw, is_log))
        self.ring_poses, self.ring_anc = poses[E:], anc[E:].astype(np.int32)

    def first(self, E):
        """The same ring with only its first E <= self.E rows settled (a row's figures do not depend on how many are settled)."""
        assert 0 <= E <= self.E
        part = object.__new__(Settled)
        part.E, part.P, part.s1 = E, self.P, self.s1
        for name in ("lo", "hi", "final", "pose", "mean", "spread"):
            setattr(part, name, getattr(self, name)[:E])
        k = self.E - E
        part.ring_poses = np.concatenate([self._settled_poses[E:], self.ring_poses]) if k else self.ring_poses
        part.ring_anc = np.concatenate([self._settled_anc[E:], self.ring_anc]) if k else self.ring_anc
        return part


def row_estimate(rows):
    """(mean (n, 3), spread (n, 4)) of raw trunk rows by doubles 0-7 alone: what a row that is not final is summarised to."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, RES)
    mean = np.column_stack([rows[:, 0], rows[:, 1], np.arctan2(rows[:, 2], rows[:, 3])])
    with np.errstate(invalid="ignore", divide="ignore"):
        spread = np.column_stack([rows[:, 4], rows[:, 5], rows[:, 6], np.hypot(rows[:, 2], rows[:, 3]) / rows[:, 7]])
    return mean, spread


def summary_of(rows):
    """pk_path_trunk_summary's host arithmetic: (mean, spread, ancestors (n, 2) int64)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, RES)
    mean, spread = row_estimate(rows)
    fin = rows[:, 8] == rows[:, 9]
    mean[fin] = rows[fin, 10:13]
    spread[fin] = (0.0, 0.0, 0.0, 1.0)
    return mean, spread, rows[:, 8:10].astype(np.int64)


def check_rows(rows, ref, what=""):
    """Raw trunk rows against a ``Settled``: lo, hi and the pose exact, the moments within TOL of their scales
    (path_weighted_reference.errors), S1 within TOL relative; a final row's first eight doubles give its ancestor's pose and
    exactly no variance."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, RES)
    assert rows.shape[0] == ref.E, (what, rows.shape, ref.E)
    if ref.E == 0:
        return
    assert np.array_equal(rows[:, 8], ref.lo.astype(np.float64)) and np.array_equal(rows[:, 9], ref.hi.astype(np.float64)), \
        (what, rows[:, 8:10], ref.lo, ref.hi)
    assert np.array_equal(rows[:, 10:13].view(np.uint64), np.ascontiguousarray(ref.pose).view(np.uint64)), (what, "pose")
    mean, spread = row_estimate(rows)
    errs = pw.errors(mean, spread, ref.mean, ref.spread)
    e_s1 = float(np.max(np.abs(rows[:, 7] - ref.s1) / ref.s1))
    print("%s: mean xy %.2e, var %.2e, cov %.2e, R %.2e of their scales; heading %.2e rad; S1 %.2e; final %s"
          % ((what,) + errs + (e_s1, ref.final.tolist())))
    assert max(errs) <= TOL and e_s1 <= TOL, (what, errs, e_s1)
    for t in np.flatnonzero(ref.final):
        assert rows[t, 0] == ref.pose[t, 0] and rows[t, 1] == ref.pose[t, 1], (what, t)
        assert np.all(rows[t, 4:7] == 0.0), (what, t, rows[t, 4:7])


# ---- the scene of the automatic mode: every random number of a driven filter, drawn ahead of the run so that the CPU and the GPU
# tests see the same one.  Per step: the motion noise, the resample draw u, and on every second step three giant weights (as
# test_gpu_adaptive.giants: a thousand times heavier than the rest).  Three giants leave hundreds of lineages alive per step, so a
# row that leaves a ring of six is never final through them alone (a NumPy systematic resample: none of 19, 20, 24 settled rows
# for batches 1, 2, 6); on steps DOMINANT one further particle outweighs the whole population, and every row up to that step
# coalesces to it.
GIANT, DOMINANT_WEIGHT, DOMINANT = 1e3, 1e12, (9, 19)
AUTO_SEED = 4  # fixed where test_path_trunk_reference_host.py confirms final rows and others for every batch


class AutoScene(object):
    def __init__(self, P, steps, seed):
        rs = np.random.RandomState(seed)
        self.P, self.steps = P, steps
        self.start_weights = rs.uniform(0.1, 1.0, P) ** 4
        self.z = [rs.standard_normal((P, 3)) for _ in range(steps)]
        self.u = [float(rs.uniform(0.0, 1.0)) for _ in range(steps)]
        self.heavy = []  # per step: [(particle, weight)], applied in front of its resample
        for s in range(steps):
            h = []
            if s % 2 == 1:
                h = [(int(i), GIANT * float(rs.uniform(0.5, 1.0))) for i in rs.randint(0, P, size=min(P, 3))]
            if s in DOMINANT:
                h.append((int(rs.randint(0, P)), DOMINANT_WEIGHT))
            self.heavy.append(h)


def settled_kinds(ancestors, P, cap, batch):
    """Which rows the automatic mode settles from a run with these ancestors, and whether each is final: [(step, final)]."""
    out, held = [], 0
    for n in range(1, len(ancestors) + 1):
        held += 1
        if held == cap:
            lo, hi = span(np.array(ancestors[n - held:n]), P)
            out += [(n - held + t, bool(lo[t] == hi[t])) for t in range(batch)]
            held -= batch
    return out

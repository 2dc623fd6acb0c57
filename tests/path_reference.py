"""Reference for the path estimate (pk_path_trace / pk_path_summary), shared by the tests: a NumPy restatement of the definitions
in include/parakeet_slam.h.

A ring of T rows: ``poses[t]`` (P, 3) = x, y, heading of the generation resample t worked on, ``ancestors[t]`` (P,) = for every
particle of the NEXT generation the index of its parent in that one; ``current`` (P, 3) = the live generation, row T.

    lineage of current particle k:   j_T = k,   j_t = ancestors[t][j_{t+1}]
    its path:                        poses[t][j_t] for t < T, then current[k]

The summary counts every current particle once.  Per row: mean x, mean y and the circular mean heading of the P lineages; var x,
cov xy, var y and the mean resultant length of the headings; the number of distinct j_t.  The position moments are taken about the
pose of particle 0's lineage in that row (the device's reference pose: the differences are the same float64 numbers), every sum
with ``math.fsum`` -- exact -- and the second moments in two passes about the mean, so this side's own error is a few roundings of
the final arithmetic, 1e-15 relative.

Tolerances (``check_summary``): survivors and traces exact.  mean x, mean y and the four spread figures within RTOL = 1e-12 of
the reference, relative, the figure the project holds pk_summary to: the device merges (count, mean, centred moments) triples
pairwise, every merge a handful of roundings on terms of one sign, log2(P) + 17 + P / 65 536 levels deep -- 1e-14 at the sizes
tested.  A quantity that is exactly zero here (a row with one survivor) must be exactly zero there.  Heading within 1e-12 rad
modulo one turn.
"""
import math

import numpy as np

RTOL = 1e-12


def lineages(ancestors, P):
    """J (T + 1, P) int64: J[T] = arange(P), J[t] = ancestors[t][J[t + 1]]."""
    anc = np.asarray(ancestors, dtype=np.int64).reshape(-1, P)
    T = anc.shape[0]
    J = np.empty((T + 1, P), dtype=np.int64)
    J[T] = np.arange(P)
    for t in range(T - 1, -1, -1):
        J[t] = anc[t][J[t + 1]]
    return J


def paths(poses, ancestors, current):
    """(P, T + 1, 3): the path of every current particle, pure gathers."""
    current = np.asarray(current, dtype=np.float64)
    P = current.shape[0]
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, P, 3)
    J = lineages(ancestors, P)
    T = poses.shape[0]
    out = np.empty((P, T + 1, 3))
    for t in range(T):
        out[:, t] = poses[t][J[t]]
    out[:, T] = current
    return out


def survivors(ancestors, P):
    return np.array([np.unique(j).size for j in lineages(ancestors, P)], dtype=np.int64)


def summary(poses, ancestors, current):
    """(mean (T + 1, 3), spread (T + 1, 4), survivors (T + 1,))."""
    X = paths(poses, ancestors, current)
    P, rows = X.shape[0], X.shape[1]
    J = lineages(ancestors, P)
    mean, spread = np.empty((rows, 3)), np.empty((rows, 4))
    surv = np.empty(rows, dtype=np.int64)
    n = float(P)
    for t in range(rows):
        x, y, h = X[:, t, 0], X[:, t, 1], X[:, t, 2]
        dx, dy = x - x[0], y - y[0]
        mx, my = math.fsum(dx) / n, math.fsum(dy) / n
        ex, ey = dx - mx, dy - my
        s, c = math.fsum(np.sin(h)), math.fsum(np.cos(h))
        mean[t] = (x[0] + mx, y[0] + my, math.atan2(s, c))
        spread[t] = (math.fsum(ex * ex) / n, math.fsum(ex * ey) / n, math.fsum(ey * ey) / n, math.hypot(s, c) / n)
        surv[t] = np.unique(J[t]).size
    return mean, spread, surv


def angle_diff(a, b):
    d = (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64) + math.pi) % (2.0 * math.pi) - math.pi
    return np.abs(d)


def close(got, ref):
    """|got - ref| <= RTOL |ref| element by element (an exact zero must be met exactly)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(got - ref) <= RTOL * np.abs(ref)))


def check_summary(got, poses, ancestors, current, what=""):
    """``got`` (anything with mean, spread, survivors) against the reference; returns the reference's (mean, spread, survivors)."""
    mean, spread, surv = summary(poses, ancestors, current)
    assert np.array_equal(np.asarray(got.survivors), surv), (what, got.survivors, surv)
    err_m = np.max(np.abs(got.mean[:, :2] - mean[:, :2]) / np.abs(mean[:, :2]))
    with np.errstate(invalid="ignore", divide="ignore"):
        err_s = np.nanmax(np.where(spread == 0.0, np.where(got.spread == 0.0, 0.0, np.inf), np.abs(got.spread - spread) / np.abs(spread)))
    err_h = np.max(angle_diff(got.mean[:, 2], mean[:, 2]))
    print("%s: mean xy %.2e, spread %.2e relative; heading %.2e rad; survivors %s" % (what, err_m, err_s, err_h, surv.tolist()))
    assert close(got.mean[:, :2], mean[:, :2]), (what, err_m)
    assert close(got.spread, spread), (what, err_s)
    assert err_h <= 1e-12, (what, err_h)
    P = np.asarray(current).shape[0]
    X = paths(poses, ancestors, current)
    for t in np.flatnonzero(surv == 1):  # one survivor: its recorded pose bit for bit, exactly no spread
        assert got.mean[t, 0] == X[0, t, 0] and got.mean[t, 1] == X[0, t, 1], (what, t)
        assert np.all(got.spread[t, :3] == 0.0), (what, t, got.spread[t])
        assert abs(got.spread[t, 3] - 1.0) <= 1e-12, (what, t)
    assert np.all(surv[-1:] == P)
    return mean, spread, surv

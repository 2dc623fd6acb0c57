"""Reference for the path estimate by the weights (pk_path_summary_weighted), shared by the tests: a NumPy restatement of the
definition in include/parakeet_slam.h, built on ``path_reference.lineages`` and ``paths``.

    w_k = exp(logw_k - shift)        shift = max logw in the log domain (0 when no weight is finite), 0 in the linear one
    row t:  the moments of pose_t[j_t(k)] over the current particles k, each counted w_k times
    n_eff = S1^2 / S2 of the w_k     one number: every row is weighted by the current weights

The weights are ``np.exp(logw - shift)`` in float64 (half an ulp each; the device's exp is within an ulp of it).  Every sum is
exact: each product is split into its rounded value and its rounding error (Dekker's two-product, Veltkamp splitting) and both go
into ``math.fsum``.  The position moments are taken about the pose of particle 0's lineage in that row (the device's reference
pose: the differences are the same float64 numbers), the second moments in two passes about the weighted mean.  What is left is a
few roundings of the final arithmetic: this side's own error is about 1e-15 relative.

Tolerances (``check``), the project's figure for pk_summary and the path estimate, 1e-12:
    mean x, mean y      within 1e-12 max(|reference|, sqrt(var))
    var x, var y        within 1e-12 relative
    cov xy              within 1e-12 sqrt(var x var y)
    R, n_eff            within 1e-12 relative
    heading             within 1e-12 rad modulo one turn
and an exact zero here must be an exact zero there.
"""
import math

import numpy as np

from path_reference import angle_diff, lineages, paths

TOL = 1e-12


def shift_of(logw, domain_is_log):
    if not domain_is_log:
        return 0.0
    m = float(np.max(np.asarray(logw, dtype=np.float64)))
    return m if m > -np.inf else 0.0


def weights(logw, domain_is_log):
    with np.errstate(under="ignore"):
        return np.exp(np.asarray(logw, dtype=np.float64) - shift_of(logw, domain_is_log))


def _split(a):
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (no overflow or underflow at the magnitudes used here)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def dot(a, b):
    """sum a_i b_i, rounded once."""
    p, e = two_product(a, b)
    return math.fsum(np.concatenate([p, e]))


def dot3(w, a, b):
    """sum w_i a_i b_i: a b exactly as two terms, each times w as two more; only the error term's own product is rounded."""
    q, qe = two_product(a, b)
    p, e = two_product(w, q)
    return math.fsum(np.concatenate([p, e, w * qe]))


def weighted_mean(w, d, s1):
    live = d[w > 0.0]
    if live.size and np.all(live == live[0]):
        return float(live[0])  # lineages that all share a pose: that pose, exactly
    return dot(w, d) / s1


def summary(poses, ancestors, current, logw, domain_is_log):
    """(mean (T + 1, 3), spread (T + 1, 4), n_eff)."""
    X = paths(poses, ancestors, current)
    rows = X.shape[1]
    w = weights(logw, domain_is_log)
    s1, s2 = math.fsum(w), dot(w, w)
    mean, spread = np.empty((rows, 3)), np.empty((rows, 4))
    for t in range(rows):
        x, y, h = X[:, t, 0], X[:, t, 1], X[:, t, 2]
        dx, dy = x - x[0], y - y[0]
        mx, my = weighted_mean(w, dx, s1), weighted_mean(w, dy, s1)
        ex, ey = dx - mx, dy - my
        s, c = dot(w, np.sin(h)), dot(w, np.cos(h))
        mean[t] = (x[0] + mx, y[0] + my, math.atan2(s, c))
        spread[t] = (dot3(w, ex, ex) / s1, dot3(w, ex, ey) / s1, dot3(w, ey, ey) / s1, math.hypot(s, c) / s1)
    return mean, spread, s1 * s1 / s2


def errors(got_mean, got_spread, mean, spread):
    """The measured errors in units of their bounds' scales: mean xy, var, cov, R, heading (rad)."""
    sd = np.sqrt(spread[:, [0, 2]])
    with np.errstate(invalid="ignore", divide="ignore"):
        e_mean = np.abs(got_mean[:, :2] - mean[:, :2]) / np.maximum(np.abs(mean[:, :2]), sd)
        e_var = np.abs(got_spread[:, [0, 2]] - spread[:, [0, 2]]) / spread[:, [0, 2]]
        e_cov = np.abs(got_spread[:, 1] - spread[:, 1]) / (sd[:, 0] * sd[:, 1])
    e_var = np.where(spread[:, [0, 2]] == 0.0, np.where(got_spread[:, [0, 2]] == 0.0, 0.0, np.inf), e_var)
    e_cov = np.where(spread[:, 1] == 0.0, np.where(got_spread[:, 1] == 0.0, 0.0, np.inf), e_cov)
    e_mean = np.where(np.isnan(e_mean), np.where(got_mean[:, :2] == mean[:, :2], 0.0, np.inf), e_mean)  # (a mean of 0 with no spread)
    e_r = np.abs(got_spread[:, 3] - spread[:, 3]) / spread[:, 3]
    e_h = angle_diff(got_mean[:, 2], mean[:, 2])
    return float(np.max(e_mean)), float(np.max(e_var)), float(np.max(e_cov)), float(np.max(e_r)), float(np.max(e_h))


def check(got, poses, ancestors, current, logw, domain_is_log, what=""):
    """``got`` (anything with mean, spread, n_eff) against the reference; returns the reference's (mean, spread, n_eff)."""
    mean, spread, n_eff = summary(poses, ancestors, current, logw, domain_is_log)
    assert got.mean.shape == mean.shape and got.spread.shape == spread.shape, (what, got.mean.shape, mean.shape)
    e_mean, e_var, e_cov, e_r, e_h = errors(got.mean, got.spread, mean, spread)
    e_n = abs(got.n_eff - n_eff) / n_eff
    print("%s: mean xy %.2e, var %.2e, cov %.2e, R %.2e, n_eff %.2e of their scales; heading %.2e rad (n_eff / P = %.4f)"
          % (what, e_mean, e_var, e_cov, e_r, e_n, e_h, n_eff / len(logw)))
    assert e_mean <= TOL, (what, e_mean)
    assert e_var <= TOL, (what, e_var)
    assert e_cov <= TOL, (what, e_cov)
    assert e_r <= TOL, (what, e_r)
    assert e_h <= TOL, (what, e_h)
    assert e_n <= TOL, (what, e_n)
    return mean, spread, n_eff


__all__ = ["lineages", "paths", "summary", "check", "weights", "errors", "TOL"]

"""Reference for adaptive resampling (pk_resample_adaptive, pk_weight_sums, pk_summary_weighted), shared by the tests: a NumPy
restatement of the definitions in include/parakeet_slam.h, working from DOWNLOADED log-weights and poses.

    shift = max logw in the log domain (0 when no weight is finite), 0 in the linear one
    w_p = exp(logw_p - shift)          ``resample_reference.true_weights``, numpy.longdouble
    S1 = sum w,  S2 = sum w^2,  n_eff = S1^2 / S2,  keep iff n_eff >= theta P

The weights are rounded to float64 once (half an ulp each) and every sum is ``math.fsum`` -- exact --, the second moments in two
passes about the weighted mean: this side's own error is a few roundings of the final arithmetic, 1e-15 relative.

Tolerances.  S1, S2 and n_eff: 1e-12 relative, the bound ``mapsum_reference`` holds n_eff to -- the device adds P non-negative
terms, a lane's four, six butterfly or scan levels, three waves, then the blocks one by one: (13 + P / 1024) roundings of at most
eps / 2 of the running sum each, plus an ulp of its exp per term, 3e-14 at P = 262 145.  The weighted pose summary:
``path_reference``'s bounds -- means and the four spread figures within RTOL = 1e-12 relative, heading within 1e-12 rad -- for
the same reason as there (pairwise merges of terms of one sign).  A quantity that is exactly zero here must be exactly zero
there.  The verdict is discrete: the tests assert ``margin(...) >= 1e-6`` on their inputs first, six decades above any of the
above, so that rounding cannot flip it.
"""
import math

import numpy as np
import pytest

from path_reference import RTOL, angle_diff, close
from resample_reference import true_weights

SUMS_RTOL = 1e-12
MARGIN = 1e-6


def need_longdouble():
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("numpy.longdouble is no wider than float64 here: no exact weights to compare with")


def shift_of(logw, domain_is_log):
    """What the device's weight scan subtracts."""
    if not domain_is_log:
        return 0.0
    m = float(np.max(np.asarray(logw, dtype=np.float64)))
    return m if m > -np.inf else 0.0


def weights(logw, domain_is_log):
    """The weights the device means, rounded to float64 once."""
    return np.asarray(true_weights(logw, domain_is_log), dtype=np.float64)


def sums(logw, domain_is_log):
    """(S1, S2, n_eff); n_eff is NaN when every weight is zero."""
    w = weights(logw, domain_is_log)
    w2 = np.asarray(true_weights(logw, domain_is_log) ** 2, dtype=np.float64)
    s1, s2 = math.fsum(w), math.fsum(w2)
    return s1, s2, (s1 * s1 / s2 if s2 > 0.0 else float("nan"))


def keeps(logw, domain_is_log, theta):
    """The verdict: True = keep (no resample).  NaN fails the comparison: resample."""
    n_eff = sums(logw, domain_is_log)[2]
    return bool(n_eff >= theta * float(len(logw)))


def margin(logw, domain_is_log, theta):
    """|n_eff / P - theta|: how far the input is from the edge of the verdict."""
    return abs(sums(logw, domain_is_log)[2] / float(len(logw)) - theta)


def pose_summary(poses, logw, domain_is_log):
    """(mean (3,), spread (4,), n_eff): the weighted mean x, mean y and circular mean heading; var x, cov xy, var y over S1 and the
    mean resultant length.  Position moments about particle 0's pose, as on the device (the differences are the same float64 numbers)."""
    poses = np.asarray(poses, dtype=np.float64)
    w = weights(logw, domain_is_log)
    s1, _, n_eff = sums(logw, domain_is_log)
    x, y, h = poses[:, 0], poses[:, 1], poses[:, 2]
    dx, dy = x - x[0], y - y[0]
    mx, my = math.fsum(w * dx) / s1, math.fsum(w * dy) / s1
    ex, ey = dx - mx, dy - my
    s, c = math.fsum(w * np.sin(h)), math.fsum(w * np.cos(h))
    mean = np.array([x[0] + mx, y[0] + my, math.atan2(s, c)])
    spread = np.array([math.fsum(w * ex * ex) / s1, math.fsum(w * ex * ey) / s1, math.fsum(w * ey * ey) / s1, math.hypot(s, c) / s1])
    return mean, spread, n_eff


def rel(got, ref):
    return abs(float(got) - float(ref)) / abs(float(ref))


def check_sums(got_s1, got_s2, got_n_eff, logw, domain_is_log, what=""):
    s1, s2, n_eff = sums(logw, domain_is_log)
    errs = rel(got_s1, s1), rel(got_s2, s2), rel(got_n_eff, n_eff)
    print("%s: S1 %.2e, S2 %.2e, n_eff %.2e relative (n_eff / P = %.6f)" % ((what,) + errs + (n_eff / len(logw),)))
    assert max(errs) <= SUMS_RTOL, (what, errs)
    return s1, s2, n_eff


def check_pose_summary(got, poses, logw, domain_is_log, what=""):
    """``got`` (anything with mean, spread, n_eff) against the reference; returns the reference's (mean, spread, n_eff)."""
    mean, spread, n_eff = pose_summary(poses, logw, domain_is_log)
    err_m = np.max(np.abs(got.mean[:2] - mean[:2]) / np.abs(mean[:2]))
    with np.errstate(invalid="ignore", divide="ignore"):
        err_s = np.nanmax(np.where(spread == 0.0, np.where(got.spread == 0.0, 0.0, np.inf), np.abs(got.spread - spread) / np.abs(spread)))
    err_h = float(angle_diff(got.mean[2], mean[2]))
    print("%s: mean xy %.2e, spread %.2e relative; heading %.2e rad; n_eff %.2e" % (what, err_m, err_s, err_h, rel(got.n_eff, n_eff)))
    assert close(got.mean[:2], mean[:2]), (what, err_m)
    assert close(got.spread, spread), (what, err_s)
    assert err_h <= 1e-12, (what, err_h)
    assert rel(got.n_eff, n_eff) <= SUMS_RTOL, what
    return mean, spread, n_eff

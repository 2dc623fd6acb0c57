"""The odometry motion model's host side, shared by the facades (core.py, multi.py): the keywords' checks and the pose of an
odometry message.  The model itself -- delta, sigmas, sample -- is the library's (include/parakeet_slam.h, pk_odom_delta ...)."""
from __future__ import annotations

import math

# (a1, a2, a3, a4): VARIANCES per squared unit -- sigma_rot^2 = a1 rot^2 + a2 trans^2, sigma_trans^2 = a3 trans^2 + a4 (rot1^2 + rot2^2).
# The default is 5 % of a rotation and of a translation (the twist model's .05 v), and 0.01 rad per metre / 0.01 m per radian across.
DEFAULT_ALPHAS = (0.0025, 0.0001, 0.0025, 0.0001)
DEFAULT_MIN_TRANS = 0.01  # metres
MODES = ("twist", "odometry")


def check_keywords(motion, odom_alphas, odom_min_trans):
    """(motion, alphas as four floats, min_trans as a float), or ValueError: what FastSLAM(...) checks before it creates anything."""
    if motion not in MODES:
        raise ValueError("motion must be 'twist' or 'odometry', not %r" % (motion,))
    try:
        alphas = tuple(float(a) for a in odom_alphas)
    except TypeError:
        raise ValueError("odom_alphas must be four numbers (a1, a2, a3, a4), not %r" % (odom_alphas,))
    if len(alphas) != 4 or not all(math.isfinite(a) and a >= 0.0 for a in alphas):
        raise ValueError("odom_alphas must be four finite numbers >= 0 (a1, a2, a3, a4), not %r" % (odom_alphas,))
    try:
        min_trans = float(odom_min_trans)
    except TypeError:
        raise ValueError("odom_min_trans must be a number of metres >= 0, not %r" % (odom_min_trans,))
    if not (math.isfinite(min_trans) and min_trans >= 0.0):
        raise ValueError("odom_min_trans must be a finite number of metres >= 0, not %r" % (odom_min_trans,))
    return motion, alphas, min_trans


def check_pose(pose, what="odometry message"):
    """(x, y, heading) as three finite floats, or ValueError -- before the pose is stored or anything moves."""
    p = tuple(float(v) for v in pose)
    if len(p) != 3 or not all(math.isfinite(v) for v in p):
        raise ValueError("%s: the pose (x, y, heading) = %r is not three finite numbers" % (what, p))
    return p


def is_zero(delta):
    """A delta of exactly (0, 0, 0): the robot stood still -- nothing to launch, no draw consumed."""
    return float(delta[0]) == 0.0 and float(delta[1]) == 0.0 and float(delta[2]) == 0.0

"""The odometry motion model (Thrun, Burgard, Fox, Probabilistic Robotics, Table 5.6; include/parakeet_slam.h) restated for the
tests: the delta between two odometry poses, its sigmas and the per-particle sample, in float64 -- and the same in
numpy.longdouble for the tolerance cases.  Nothing here calls the library.

Angles are compared by their WRAPPED difference (angle_diff), so +pi and -pi are one value.

float64: the scalar functions use ``math`` (the C library's hypot / atan2 / remainder / sqrt on IEEE doubles, every product and sum
rounded by itself), the formulas of pk_odom_delta and pk_odom_sigmas one for one; the sample is NumPy over the particles."""
import math

import numpy as np

TWO_PI = 2.0 * math.pi
LD = np.longdouble
LD_PI = LD(4) * np.arctan(LD(1))
LD_TWO_PI = LD(2) * LD_PI


def wrap(a):
    """Into [-pi, pi]: IEEE remainder by 2 pi (exact; wrap(a) == a for |a| <= pi)."""
    return math.remainder(a, TWO_PI)


def angle_diff(a, b):
    """|a - b| on the circle, elementwise: 0 for +pi against -pi."""
    d = np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)
    return np.abs(d - LD_TWO_PI * np.rint(d / LD_TWO_PI)).astype(np.float64)


def delta(prev, now, min_trans=0.01):
    """(rot1, trans, rot2) between two poses (x, y, heading)."""
    dx, dy = float(now[0]) - float(prev[0]), float(now[1]) - float(prev[1])
    trans = math.hypot(dx, dy)
    dth = wrap(float(now[2]) - float(prev[2]))
    rot1 = 0.0 if trans < min_trans else wrap(math.atan2(dy, dx) - float(prev[2]))
    return np.array([rot1, trans, wrap(dth - rot1)])


def sigmas(d, alphas):
    """(sigma_rot1, sigma_trans, sigma_rot2): rotations folded, so that driving backwards is no large turn."""
    a1, a2, a3, a4 = (float(a) for a in alphas)
    r1n = min(abs(float(d[0])), math.pi - abs(float(d[0])))
    r2n = min(abs(float(d[2])), math.pi - abs(float(d[2])))
    r1q, r2q, tq = r1n * r1n, r2n * r2n, float(d[1]) * float(d[1])
    return np.array([math.sqrt(a1 * r1q + a2 * tq), math.sqrt(a3 * tq + a4 * (r1q + r2q)), math.sqrt(a1 * r2q + a2 * tq)])


def _sample(x, y, h, d, s, z, dtype):
    x, y, h = (np.asarray(v, dtype=dtype) for v in (x, y, h))
    z = np.asarray(z, dtype=dtype).reshape(-1, 3)
    d, s = np.asarray(d, dtype=dtype), np.asarray(s, dtype=dtype)
    r1 = d[0] - s[0] * z[:, 0]
    t = d[1] - s[1] * z[:, 1]
    r2 = d[2] - s[2] * z[:, 2]
    h1 = h + r1
    h2 = h1 + r2
    return x + t * np.cos(h1), y + t * np.sin(h1), np.arctan2(np.sin(h2), np.cos(h2))  # wrap_heading: to (-pi, pi]


def sample(x, y, h, d, alphas, z):
    """Every particle moved by the delta d with its three standard normals z[i]: float64 (x, y, h)."""
    return _sample(x, y, h, d, sigmas(d, alphas), z, np.float64)


def sample_ld(x, y, h, d, alphas, z):
    """The same in numpy.longdouble from the float64 inputs (delta and sigmas are the float64 ones: they are the kernel's
    arguments); returned as longdouble."""
    return _sample(x, y, h, d, sigmas(d, alphas), z, LD)


def compose(prev, d):
    """The delta put back onto prev with no noise: the pose it leads to (longdouble arithmetic, float64 out)."""
    x, y, h = _sample([prev[0]], [prev[1]], [prev[2]], d, np.zeros(3), np.zeros((1, 3)), LD)
    return np.array([x[0], y[0], h[0]], dtype=np.float64)


def poses_close(got_xyh, ref_x, ref_y, ref_h, rtol=1e-12, atol=1e-13):
    """(ok, worst figures) of poses (n, >=3) against a reference: x and y by |d| <= atol + rtol |ref|, the heading by its wrapped
    difference under the same bound."""
    got = np.asarray(got_xyh, dtype=np.float64)
    rx, ry, rh = (np.asarray(v, dtype=LD) for v in (ref_x, ref_y, ref_h))
    ex = np.abs(got[:, 0].astype(LD) - rx).astype(np.float64) - (atol + rtol * np.abs(rx).astype(np.float64))
    ey = np.abs(got[:, 1].astype(LD) - ry).astype(np.float64) - (atol + rtol * np.abs(ry).astype(np.float64))
    eh = angle_diff(got[:, 2], rh) - (atol + rtol * np.abs(rh).astype(np.float64))
    worst = (float(ex.max()), float(ey.max()), float(eh.max()))  # <= 0: inside the bound
    return max(worst) <= 0.0, worst

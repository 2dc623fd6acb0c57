"""The exact reference of one EKF update and of the match densities, and the input classes they are tested on.

What ekf_update, prob_position_match, prob_color_match and probability_of_match (pk_math.hpp) compute, in mpmath at 300 bits and
in the DENSE form the reference program states it in (prkt_core_v2.py:748-930: the 4x5 Jacobian, Q = H Sigma H' + Qt, its inverse,
K = Sigma H' Q^-1, Sigma' = (I - K H) Sigma; :457-544 for the densities) -- not the factored scalar-plus-3x3 form of the device
code, so that an error of the factoring is seen.  Every input double is taken exactly.  The expected bearing zhat0 and the blob's
unit ray (ux, uy) are INPUTS: pk_atan2 is held to 2.3 ulp by its own test, and its error would be amplified by 1 / |innovation| here.

Errors are counted in UNITS: |got - exact| / (2^-53 scale), scale being the sum of the absolute values of the terms of the exact
expression (an output that is a sum of terms cannot be asked for more than that):
  new covariance entry   (|Sigma| + |K| |H| |Sigma|)_ij
  new mean entry         |mu_i| + sum_j |K_ij| |d_j|
  log weight             1/2 |log(2 pi ||Q||_F)| + 1/2 d' Q^-1 d
  log density, k dims    1/2 (k log 2 pi + |log det| + Mahalanobis term)
  closest point          |s| + |u| |mag|
The bounds (set from CPU measurements of the float64 restatement of the reference, oracle.ekf_update_dense, and of a float64
restatement of the factored form; on the classes below the oracle's worst is 0.57 of a bound, tests/test_ekf_reference_host.py):
  update                                  units <= 32 + kappa^2 / 8,   kappa  = cond_2(C + Qc)
  log position density, closest point     units <= 32 + kappa2,        kappa2 = cond_2(P)
  log colour density, log probability     units <= 32 + kappa3^2 / 8 + kappa2,  kappa3 = cond_2(C)
A lost term, a wrong sign or a float32 intermediate costs 1e3 units or more at kappa <= 10."""
import functools
import math

import numpy as np

try:
    import mpmath
    from mpmath import mp, mpf
except ImportError:  # the tests that need the reference skip
    mpmath = None

MP_BITS = 300
UNIT = 2.0 ** -53
POTENTIAL = 0x40000000  # PK_LANDMARK_POTENTIAL
LOG_NO_MATCH = -2.3025850929940456840179914546844
DENSITY_FLOOR = 1e-300  # densities are compared where the exact value is at least this
N_POINTS = 192          # per class (at most 256: a class stays within a few seconds of mpmath)

# flags of PK_MATH_EKF_UPDATE
IMMUTABLE, ZHAT0_KNOWN, NO_COLOUR, FRO_PROD = 1, 2, 4, 8
# columns of its rows: in 31, out 17
E_SX, E_SY, E_F, E_COUNT, E_BLOB, E_QT, E_ZHAT0, E_FLAGS, E_PROD = 0, 1, 2, 16, 17, 21, 28, 29, 30
O_LOGW, O_F, O_COUNT, O_PROD = 0, 1, 15, 16
# PK_MATH_MATCH: in 23, out 5
M_SX, M_SY, M_H, M_F, M_BLOB, M_UX, M_UY = 0, 1, 2, 3, 17, 21, 22
FIELDS = ("mx", "my", "mr", "mg", "mb", "pxx", "pxy", "pyy", "crr", "crg", "crb", "cgg", "cgb", "cbb")
# where the 14 compact fields sit in the dense 5x5
COV_AT = ((0, 0), (0, 1), (1, 1), (2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (4, 4))

CLASSES = ("typical", "close_range", "far", "converged", "fresh", "general_qt", "kappa_1e3", "kappa_1e5", "q_zero")


def update_bound(kappa):
    return 32.0 + kappa * kappa / 8.0


def position_bound(kappa2):
    return 32.0 + kappa2


def colour_bound(kappa3, kappa2):
    return 32.0 + kappa3 * kappa3 / 8.0 + kappa2


def _ctx():
    mp.prec = MP_BITS
    return mp


def _mat(rows):
    return [[mpf(v) for v in r] for r in rows]


def _mul(a, b):
    return [[mp.fsum(a[i][k] * b[k][j] for k in range(len(b))) for j in range(len(b[0]))] for i in range(len(a))]


def _t(a):
    return [list(r) for r in zip(*a)]


def _abs(a):
    return [[abs(v) for v in r] for r in a]


def _inv(a):
    m = mp.inverse(mp.matrix(a))
    n = len(a)
    return [[m[i, j] for j in range(n)] for i in range(n)]


def dense_cov(f):
    """the 14 compact fields -> (mean 5, covariance 5x5), numpy float64"""
    f = np.asarray(f, dtype=np.float64)
    cov = np.zeros((5, 5))
    for v, (i, j) in zip(f[5:14], COV_AT):
        cov[i, j] = cov[j, i] = v
    return f[:5].copy(), cov


def dense_qt(q):
    """q00 rr rg rb gg gb bb -> Qt 4x4"""
    q00, rr, rg, rb, gg, gb, bb = [float(v) for v in q]
    return np.array([[q00, 0, 0, 0], [0, rr, rg, rb], [0, rg, gg, gb], [0, rb, gb, bb]])


def cond_sym(m):
    w = np.linalg.eigvalsh(np.asarray(m, dtype=np.float64))
    return float(w[-1] / w[0]) if w[0] > 0 else math.inf


def exact_update(row, cov=None, Qt=None):
    """One row of PK_MATH_EKF_UPDATE (the flags and prod are not read: this is the mutable, plain call) -> dict:
    fields (14 mpf, the state afterwards), field_scales (14 floats), logw (mpf), logw_scale, fro2 (mpf), kappa, q (float).

    With cov (a full 5x5) and / or Qt (a full 4x4) given, those stand for the row's compact blocks (which are then not read), and
    the pose, mean, blob and expected bearing of the row may be mpf as well as float (tests/scan_reference.py keeps a chain's state
    unrounded); the dict then also holds mean, cov, mean_scale, cov_scale (all 5 / 5x5: the dense state afterwards and its
    scales) and kappa_q, cond_2 of the whole 4x4 Q."""
    _ctx()
    full = cov is not None or Qt is not None
    if not full:
        row = [float(v) for v in row]
    sx, sy = mpf(row[E_SX]), mpf(row[E_SY])
    if cov is None:
        mean64, cov64 = dense_cov(row[E_F:E_F + 14])
        mu = [mpf(v) for v in mean64]
        S = _mat(cov64.tolist())
    else:
        mu = [mpf(v) for v in row[E_F:E_F + 5]]
        S = _mat(cov)
        cov64 = np.array([[float(v) for v in r] for r in S])
    Qt64 = dense_qt(row[E_QT:E_QT + 7]) if Qt is None else np.array([[float(v) for v in r] for r in Qt])
    Qt = _mat(Qt64.tolist()) if Qt is None else _mat(Qt)
    z = [mpf(v) for v in row[E_BLOB:E_BLOB + 4]]
    dx, dy = mu[0] - sx, mu[1] - sy
    q = dx * dx + dy * dy  # :785
    h0, h1 = (mpf(0), mpf(0)) if q == 0 else (dy / q, dx / q)  # :789, :795 and the ZeroDivisionError branches
    H = [[h0, h1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1]]
    H = _mat(H)
    Ht = _t(H)
    Q = _mul(_mul(H, S), Ht)  # :817
    Q = [[Q[i][j] + Qt[i][j] for j in range(4)] for i in range(4)]  # :818
    Qinv = _inv(Q)  # matrix.py:11
    K = _mul(_mul(S, Ht), Qinv)  # :833
    zhat = [mpf(row[E_ZHAT0]), mu[2], mu[3], mu[4]]
    d = [z[i] - zhat[i] for i in range(4)]  # :846 / :911, not wrapped
    new_mu = [mu[i] + mp.fsum(K[i][j] * d[j] for j in range(4)) for i in range(5)]  # :912-913
    KH = _mul(K, H)
    A = [[(1 if i == j else 0) - KH[i][j] for j in range(5)] for i in range(5)]  # :928
    new_S = _mul(A, S)  # :929
    fro2 = mp.fsum(Q[i][j] * Q[i][j] for i in range(4) for j in range(4))  # matrix.py:31-33
    maha = mp.fsum(d[i] * Qinv[i][j] * d[j] for i in range(4) for j in range(4))
    log_norm = mp.log(2 * mp.pi * mp.sqrt(fro2))
    logw = -log_norm / 2 - maha / 2  # :844-849
    mean_scale = [abs(mu[i]) + mp.fsum(abs(K[i][j]) * abs(d[j]) for j in range(4)) for i in range(5)]
    KHS = _mul(_mul(_abs(K), _abs(H)), _abs(S))
    cov_scale = [abs(S[i][j]) + KHS[i][j] for i, j in COV_AT]
    C64 = cov64[2:, 2:] + Qt64[1:, 1:]
    out = dict(fields=new_mu + [new_S[i][j] for i, j in COV_AT], field_scales=[float(v) for v in mean_scale + cov_scale],
               logw=logw, logw_scale=float(abs(log_norm) / 2 + maha / 2), fro2=fro2, kappa=cond_sym(C64), q=float(q),
               asymmetry=float(max(abs(new_S[i][j] - new_S[j][i]) for i in range(5) for j in range(5))))
    if full:
        Q64 = np.array([[float(v) for v in r] for r in Q])
        out.update(mean=new_mu, cov=new_S, mean_scale=[float(v) for v in mean_scale],
                   cov_scale=[[float(abs(S[i][j]) + KHS[i][j]) for j in range(5)] for i in range(5)],
                   kappa_q=cond_sym(0.5 * (Q64 + Q64.T)))
    return out


def exact_match(row):
    """One row of PK_MATH_MATCH -> dict: near (2 mpf), near_scale (2 floats), log_position / log_colour / log_match (mpf, None
    where the reference returns exactly 0), their scales, the gates that closed, kappa2, kappa3."""
    _ctx()
    row = [float(v) for v in row]
    sx, sy, heading = mpf(row[M_SX]), mpf(row[M_SY]), mpf(row[M_H])
    mean64, cov64 = dense_cov(row[M_F:M_F + 14])
    mu = [mpf(v) for v in mean64]
    bearing, r, g, b = [mpf(v) for v in row[M_BLOB:M_BLOB + 4]]
    ux, uy = mpf(row[M_UX]), mpf(row[M_UY])
    ox, oy = mu[0] - sx, mu[1] - sy
    mag = ox * ux + oy * uy  # :496-522
    behind = mag < 0
    near = [sx, sy] if behind else [sx + ux * mag, sy + uy * mag]
    near_scale = [float(abs(sx) + abs(ux) * abs(mag)), float(abs(sy) + abs(uy) * abs(mag))]
    log2pi = mp.log(2 * mp.pi)
    pse = mp.atan2(oy, ox) if (ox != 0 or oy != 0) else mpf(0)
    # position, :457-494
    P = _mat(cov64[:2, :2].tolist())
    Pinv = _inv(P)
    det2 = P[0][0] * P[1][1] - P[0][1] * P[1][0]
    e = [near[0] - mu[0], near[1] - mu[1]]
    maha2 = mp.fsum(e[i] * Pinv[i][j] * e[j] for i in range(2) for j in range(2))
    log_position = -(2 * log2pi + mp.log(det2) + maha2) / 2
    position_scale = float((2 * log2pi + abs(mp.log(det2)) + maha2) / 2)
    gate_side = abs(pse - bearing) > mp.pi / 2  # :473-475
    # colour, :524-544
    C = _mat(cov64[2:, 2:].tolist())
    Cinv = _inv(C)
    det3 = mp.det(mp.matrix(C))
    dc = [r - mu[2], g - mu[3], b - mu[4]]
    maha3 = mp.fsum(dc[i] * Cinv[i][j] * dc[j] for i in range(3) for j in range(3))
    log_colour = -(3 * log2pi + mp.log(det3) + maha3) / 2
    colour_scale = float((3 * log2pi + abs(mp.log(det3)) + maha3) / 2)
    # probability_of_match, :383-455
    delb = bearing - (pse - heading)
    cd = dc[0] * dc[0] + dc[1] * dc[1] + dc[2] * dc[2]
    gate_bearing, gate_colour = abs(delb) > mpf("0.5"), cd > 300
    closed = bool(gate_side or gate_bearing or gate_colour)
    return dict(near=near, near_scale=near_scale, behind=bool(behind),
                log_position=None if gate_side else log_position, position_scale=position_scale,
                log_colour=log_colour, colour_scale=colour_scale,
                log_match=None if closed else log_position + log_colour, match_scale=position_scale + colour_scale,
                gate_side=bool(gate_side), gate_bearing=bool(gate_bearing), gate_colour=bool(gate_colour),
                delb=float(delb), cd=float(cd), side=float(abs(pse - bearing)), maha2=float(maha2), maha3=float(maha3),
                kappa2=cond_sym(cov64[:2, :2]), kappa3=cond_sym(cov64[2:, 2:]))


def units(got, exact, scale):
    """|got - exact| in units of 2^-53 scale; NaN or infinity in got counts as infinitely many"""
    got = float(got)
    if not math.isfinite(got):
        return math.inf
    if scale == 0.0:
        return 0.0 if mpf(got) == exact else math.inf
    return float(abs(mpf(got) - exact) / (mpf(UNIT) * mpf(scale)))


def update_units(out_fields, out_logw, ex):
    """(worst units over the 5 means, over the 9 covariance entries, of the log weight) of one update against exact_update's"""
    _ctx()
    u = [units(g, x, s) for g, x, s in zip(out_fields, ex["fields"], ex["field_scales"])]
    return max(u[:5]), max(u[5:]), units(out_logw, ex["logw"], ex["logw_scale"])


def log_density_units(p, exact_log, scale):
    """units of log(p) for a density p returned as a number (the logarithm of the double p itself, taken exactly)"""
    _ctx()
    p = float(p)
    if not (p > 0.0) or not math.isfinite(p):
        return math.inf
    return float(abs(mp.log(mpf(p)) - exact_log) / (mpf(UNIT) * mpf(scale)))


# ------------------------------------------------------------------------------------------------------------ the input classes
def _log_uniform(rs, lo, hi, n):
    return 10.0 ** rs.uniform(math.log10(lo), math.log10(hi), n)


def _spd2(rs, scale, ratio):
    """rotated 2x2 blocks with eigenvalues scale, scale / ratio -> (pxx, pxy, pyy) columns"""
    th = rs.uniform(0, math.pi, scale.size)
    c, s = np.cos(th), np.sin(th)
    a, b = scale, scale / ratio
    return np.stack([a * c * c + b * s * s, (a - b) * c * s, a * s * s + b * c * c], axis=1)


def _spd3(rs, lam):
    """rotated 3x3 blocks with eigenvalues lam (n, 3) -> (rr, rg, rb, gg, gb, bb) columns"""
    n = lam.shape[0]
    q, _ = np.linalg.qr(rs.standard_normal((n, 3, 3)))
    spread = lam.max(axis=1) - lam.min(axis=1)
    for _ in range(64):  # no off-diagonal entry below 1 / 50 of the spread of the eigenvalues (see draw_class)
        C = np.einsum("nij,nj,nkj->nik", q, lam, q)
        C = 0.5 * (C + np.transpose(C, (0, 2, 1)))
        small = np.minimum(np.minimum(np.abs(C[:, 0, 1]), np.abs(C[:, 0, 2])), np.abs(C[:, 1, 2])) < 0.02 * spread
        if not small.any():
            break
        q[small], _ = np.linalg.qr(rs.standard_normal((int(small.sum()), 3, 3)))
    assert not small.any()
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], axis=1)


def _lam3(rs, scale, ratio):
    mid = ratio ** -rs.uniform(0, 1, scale.size)
    return scale[:, None] * np.stack([np.ones(scale.size), mid, 1.0 / ratio], axis=1)


def _kappa_blocks(rs, n, kmax, qc=0.1):
    """colour blocks whose C + qc I has a condition number log-uniform over 10 .. kmax"""
    target = _log_uniform(rs, 10.0, kmax, n)
    lo = 0.05
    hi = (lo + qc) * target - qc
    mid = lo * (hi / lo) ** rs.uniform(0, 1, n)
    return _spd3(rs, np.stack([hi, mid, np.full(n, lo)], axis=1))


SEEDS = {name: 9100 + i for i, name in enumerate(CLASSES)}


@functools.lru_cache(maxsize=None)
def draw_class(name, n=N_POINTS):
    """(ekf rows (n, 31), match rows (n, 23)) of one class, from its fixed seed.

    typical       range 1 .. 50, det P 1e-4 .. 1e2
    close_range   range 1e-6 .. 1e-1: h = d / q is huge, k0 a0 cancels against pxx
    far           range 50 .. 1e4
    converged     P down to 1e-16, C down to 1e-6
    fresh         P up to 1e12, C up to 1e6
    general_qt    Qt's colour block symmetric positive definite with off-diagonal terms: the long form of colour_block_update
    kappa_1e3/5   rotated colour blocks with cond(C + Qc) up to 1e3 / 1e5
    q_zero        the landmark exactly on the pose

    The match rows hold the same landmarks; their pose keeps the ray's closest point a comparable distance from the landmark and
    from the pose (bearing offsets 0.15 .. 0.45: the error e = near - mean is a difference of two rounded numbers, and its
    cancellation is no property of the density), and every second row rescales the range to the size of the position block, so
    that the position density is a number and not an underflow.

    Two conditions keep the float64 restatement of the reference itself inside the bounds (tests/test_ekf_reference_host.py
    asserts that it is; they are conditions on the inputs, not allowances for the device).  The scales are entry by entry, the
    error of a LAPACK inverse is norm by norm: an off-diagonal entry of a rotated colour block that happens to vanish has a scale
    of nothing and an error of the block's size, so the rotations are redrawn until no off-diagonal entry is below 1 / 50 of the
    spread of the eigenvalues.  And where C is far above Qc (fresh) the gain is the identity up to 1e-7, its off-diagonal entries are
    rounding errors of the product C Q^-1 in float64 and multiply the other channels' innovations: there the colour block is
    close to a multiple of the identity (eigenvalue ratio up to 3) and the innovation has components of one size.  A third one for
    the position mean: where K d is far above the mean itself (close_range: the mean is 1e-6; fresh: P is 1e12) a cancellation
    between pxx h0 and pxy h1 in P h, which the scale |K| |d| of the exact gain knows nothing of, is all of the result: there the
    position block's eigenvalue ratio stays below 2 (up to 100 everywhere else) and the block is turned until neither component of
    P h is below half the sum of its terms' absolute values."""
    rs = np.random.RandomState(SEEDS[name])
    rng = {"close_range": (1e-6, 1e-1), "far": (50.0, 1e4)}.get(name, (1.0, 50.0))
    dist = _log_uniform(rs, rng[0], rng[1], n)
    phi = rs.uniform(-math.pi, math.pi, n)
    pose = dist[:, None] * rs.uniform(-0.2, 0.2, (n, 2))
    if name == "q_zero":
        pose = rs.uniform(-20, 20, (n, 2))
        dist = np.zeros(n)
    f = np.zeros((n, 14))
    f[:, 0] = pose[:, 0] + dist * np.cos(phi)
    f[:, 1] = pose[:, 1] + dist * np.sin(phi)
    f[:, 2:5] = rs.uniform(0, 255, (n, 3))
    if name == "converged":
        p_scale, c_scale = _log_uniform(rs, 1e-16, 1e-2, n), _log_uniform(rs, 1e-6, 1.0, n)
    elif name == "fresh":
        p_scale, c_scale = _log_uniform(rs, 1.0, 1e12, n), _log_uniform(rs, 1.0, 1e6, n)
    else:
        p_scale, c_scale = None, _log_uniform(rs, 0.5, 50.0, n)
    p_ratio = _log_uniform(rs, 1.0, 2.0 if name in ("close_range", "fresh") else 100.0, n)
    if p_scale is None:  # det P = scale^2 / ratio log-uniform over 1e-4 .. 1e2
        p_scale = np.sqrt(_log_uniform(rs, 1e-4, 1e2, n) * p_ratio)
    f[:, 5:8] = _spd2(rs, p_scale, p_ratio)
    if name in ("close_range", "fresh"):  # no cancellation in P h (below): the block is turned until there is none
        dx, dy = f[:, 0] - pose[:, 0], f[:, 1] - pose[:, 1]
        for _ in range(64):
            t0, t1, t2, t3 = f[:, 5] * dy, f[:, 6] * dx, f[:, 6] * dy, f[:, 7] * dx
            bad = (np.abs(t0) + np.abs(t1) > 2.0 * np.abs(t0 + t1)) | (np.abs(t2) + np.abs(t3) > 2.0 * np.abs(t2 + t3))
            if not bad.any():
                break
            f[bad, 5:8] = _spd2(rs, p_scale[bad], p_ratio[bad])
        assert not bad.any()
    if name == "kappa_1e3":
        f[:, 8:14] = _kappa_blocks(rs, n, 1e3)
    elif name == "kappa_1e5":
        f[:, 8:14] = _kappa_blocks(rs, n, 1e5)
    else:
        f[:, 8:14] = _spd3(rs, _lam3(rs, c_scale, _log_uniform(rs, 1.2, 3.0 if name == "fresh" else 30.0, n)))
    qt = np.tile(np.array([0.1, 0.1, 0.0, 0.0, 0.1, 0.0, 0.1]), (n, 1))
    if name == "general_qt":
        qt[:, 0] = rs.uniform(0.02, 0.5, n)
        qt[:, 1:] = _spd3(rs, _lam3(rs, rs.uniform(0.05, 0.5, n), _log_uniform(rs, 1.0, 8.0, n)))
    ekf = np.zeros((n, 31))
    ekf[:, E_SX:E_SY + 1] = pose
    ekf[:, E_F:E_F + 14] = f
    ekf[:, E_COUNT] = 2.0 * rs.randint(0, 6, n)
    ekf[:, E_QT:E_QT + 7] = qt
    dx, dy = f[:, 0] - pose[:, 0], f[:, 1] - pose[:, 1]
    zhat0 = np.arctan2(dy, dx)
    ekf[:, E_ZHAT0] = zhat0
    # the blob: an innovation of 0.3 .. 3 standard deviations of Q in every component
    q = dx * dx + dy * dy
    with np.errstate(all="ignore"):
        h0, h1 = np.where(q == 0, 0.0, dy / q), np.where(q == 0, 0.0, dx / q)
    q00 = h0 * (f[:, 5] * h0 + f[:, 6] * h1) + h1 * (f[:, 6] * h0 + f[:, 7] * h1) + qt[:, 0]
    ekf[:, E_BLOB] = zhat0 + np.sqrt(q00) * rs.standard_normal(n) * rs.uniform(0.3, 3.0, n)
    for i in range(n):
        _, cov = dense_cov(f[i])
        lower = np.linalg.cholesky(cov[2:, 2:] + dense_qt(qt[i])[1:, 1:])
        ekf[i, E_BLOB + 1:E_BLOB + 4] = f[i, 2:5] + lower @ rs.standard_normal(3) * rs.uniform(0.3, 3.0)
        if name == "fresh":
            ekf[i, E_BLOB + 1:E_BLOB + 4] = f[i, 2:5] + math.sqrt(c_scale[i]) * rs.uniform(0.5, 2.0, 3) * rs.choice([-1.0, 1.0], 3)
    ekf[:, E_PROD] = 1.0

    match = np.zeros((n, 23))
    delta = rs.uniform(0.15, 0.45, n) * rs.choice([-1.0, 1.0], n)
    mdist = dist.copy()
    if name == "q_zero":
        mdist = _log_uniform(rs, 1.0, 50.0, n)  # (probability_of_match has no branch for q == 0: the typical geometry)
    sigma = np.sqrt(p_scale)
    rescaled = np.arange(n) % 2 == 1
    mdist[rescaled] = (sigma * rs.uniform(0.5, 6.0, n) / np.sin(np.abs(delta)))[rescaled]
    mpose = mdist[:, None] * rs.uniform(-0.2, 0.2, (n, 2))
    mf = f.copy()
    mf[:, 0] = mpose[:, 0] + mdist * np.cos(phi)
    mf[:, 1] = mpose[:, 1] + mdist * np.sin(phi)
    pse = np.arctan2(mf[:, 1] - mpose[:, 1], mf[:, 0] - mpose[:, 0])
    bearing = pse + delta  # the side gate |pse - bearing| <= pi / 2 open
    heading = rs.uniform(-0.04, 0.04, n)  # delb = delta + heading: 1e-2 clear of the 0.5 gate
    cb, sb = np.cos(bearing), np.sin(bearing)
    length = np.sqrt(cb * cb + sb * sb + 0.0)  # utils.py:68-76 as the oracle forms it
    match[:, M_SX:M_SY + 1] = mpose
    match[:, M_H] = heading
    match[:, M_F:M_F + 14] = mf
    match[:, M_BLOB] = bearing
    for i in range(n):
        _, cov = dense_cov(mf[i])
        lower = np.linalg.cholesky(cov[2:, 2:])
        match[i, M_BLOB + 1:M_BLOB + 4] = mf[i, 2:5] + lower @ rs.standard_normal(3) * rs.uniform(0.3, 3.0)
    match[:, M_UX], match[:, M_UY] = cb * (1.0 / length), sb * (1.0 / length)
    ekf.setflags(write=False)
    match.setflags(write=False)
    return ekf, match


@functools.lru_cache(maxsize=None)
def exact_class(name, n=N_POINTS):
    """(list of exact_update dicts, list of exact_match dicts) over draw_class(name): computed once, shared, never changed"""
    ekf, match = draw_class(name, n)
    return [exact_update(r) for r in ekf], [exact_match(r) for r in match]


# ------------------------------------------------------------------------------------ the oracle's float64 on the same rows
def oracle_update(row):
    """oracle.ekf_update_dense on one row -> (14 fields afterwards, log weight)"""
    from oracle import fastslam_oracle as O

    mean, cov = dense_cov(row[E_F:E_F + 14])
    with np.errstate(all="ignore"):
        nm, nc, _, aux = O.ekf_update_dense(row[E_SX], row[E_SY], mean, cov, row[E_BLOB:E_BLOB + 4], dense_qt(row[E_QT:E_QT + 7]))
    return np.concatenate([nm, [nc[i, j] for i, j in COV_AT]]), float(aux["logweight"])


def oracle_match(row):
    """the oracle's mvn_pdf_2 / mvn_pdf_3 and the closest point with the row's own unit ray -> (probability as :439-455 forms it
    from the two, gates left out; position; colour; near x; near y)"""
    from oracle import fastslam_oracle as O

    sx, sy = row[M_SX], row[M_SY]
    f = row[M_F:M_F + 14]
    mag = (f[0] - sx) * row[M_UX] + (f[1] - sy) * row[M_UY]
    nx, ny = (sx, sy) if mag < 0 else (sx + row[M_UX] * mag, sy + row[M_UY] * mag)
    with np.errstate(all="ignore"):
        p2 = float(O.mvn_pdf_2(nx - f[0], ny - f[1], f[5], f[6], f[7]))
        p3 = float(O.mvn_pdf_3(row[M_BLOB + 1] - f[2], row[M_BLOB + 2] - f[3], row[M_BLOB + 3] - f[4], *f[8:14]))
        pm = (500.0 * p2) * (500.0 * p3) / 250000.0
    return pm, p2, p3, nx, ny


def class_figures(name, update_outputs, match_outputs):
    """Worst units and worst ratio to the bound, per output, of one class: update_outputs = [(14 fields, logw)] and match_outputs =
    [(probability or None, position, colour, near x, near y)] in the order of draw_class.  -> {output: dict(worst_units, worst_ratio,
    points)}"""
    ex_u, ex_m = exact_class(name)
    fig = {k: dict(worst_units=0.0, worst_ratio=0.0, points=0) for k in
           ("mean", "covariance", "log_weight", "closest_point", "log_position", "log_colour", "log_match")}

    def note(key, u, bound):
        d = fig[key]
        d["worst_units"], d["worst_ratio"], d["points"] = max(d["worst_units"], u), max(d["worst_ratio"], u / bound), d["points"] + 1

    for (fields, logw), ex in zip(update_outputs, ex_u):
        um, uc, uw = update_units(fields, logw, ex)
        b = update_bound(ex["kappa"])
        note("mean", um, b)
        note("covariance", uc, b)
        note("log_weight", uw, b)
    for (pm, p2, p3, nx, ny), ex in zip(match_outputs, ex_m):
        b2, b3 = position_bound(ex["kappa2"]), colour_bound(ex["kappa3"], ex["kappa2"])
        note("closest_point", max(units(nx, ex["near"][0], ex["near_scale"][0]), units(ny, ex["near"][1], ex["near_scale"][1])), b2)
        if ex["log_position"] is not None and ex["log_position"] >= math.log(DENSITY_FLOOR):
            note("log_position", log_density_units(p2, ex["log_position"], ex["position_scale"]), b2)
        if ex["log_colour"] >= math.log(DENSITY_FLOOR):
            note("log_colour", log_density_units(p3, ex["log_colour"], ex["colour_scale"]), b3)
        if pm is not None and ex["log_match"] is not None and ex["log_match"] >= math.log(DENSITY_FLOOR):
            note("log_match", log_density_units(pm, ex["log_match"], ex["match_scale"]), b3)
    return fig

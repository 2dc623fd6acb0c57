"""GPU: the hand-written float64 primitives the observe kernels build their verdicts on -- pk_math.hpp, pk_pub_math.hpp,
pk_device.hpp -- each swept over its domain through pk_probe_math and held to an exact reference computed on the CPU.

Every route calls the same functions, so a wrong last digit in one of them fails no route-agreement test, and no oracle test
at rtol 1e-9 either: it shows as one blob matched to the wrong landmark in 1e8 pairs, or as a look-alike pruned that had
probability 5e-324.  Here each documented claim is a test: accuracy claims in ulp (ulp = numpy.spacing of the reference rounded
to float64), safety claims (round-down, the far bound, the key order, the zero beyond kPubFarKey, NaN in / NaN out) exactly.

References: mpmath at 200 bits where it imports (sweeps of about 2e4 points), numpy.longdouble (64-bit mantissa) for the bulk.
Run with -s to see the measured figures (recorded in profiles/r10/device_math_errors.json)."""
import math

import numpy as np
import pytest

from figures_record import record

try:
    import mpmath
except ImportError:  # the longdouble references stand alone then
    mpmath = None

gpu = pytest.mark.gpu  # (every test but the last needs the card)

LD = np.longdouble
LD_OK = np.finfo(np.longdouble).nmant >= 63
MP_BITS = 200
MP_SWEEP = 20000
SQRT_HALF = 0.70710678118654752440  # the mantissa switch of log_few_ulp / pub_log
TAN_PI_8 = 0.41421356237309503      # the 'upper' switch of pk_atan2
LOG_2PI = 1.8378770664093454835606594728112
FAR_KEY = 1492.0                    # kPubFarKey

# Measured on an MI355X (profiles/r10/device_math_errors.json); the bound asserted is 1.5 x the figure -- room for a compiler
# that schedules the Newton steps or a polynomial differently, none for a lost Newton step (1e4 ulp) or a lost term.
RECIP_MEASURED_ULP = 0.5000      # pub_recip: no number existed; the bound is rounded up to a whole ulp: 1
PR_MEASURED_RELERR = 1.145e-13   # pr_from_parts: no number existed; exp near -700 alone is 700 x 2^-53 = 8e-14
ATAN2_MEASURED_ULP = 2.2974      # pk_atan2: documented as 2 ulp, which it misses just above its tan(pi / 8) switch (pk_math.hpp now
#                                  says 2.3); 3.4 ulp of an angle is 1.5e-15 rad, six orders below the 1e-9 of the parity tests


def need_reference():
    if mpmath is None and not LD_OK:
        pytest.skip("no exact reference here: mpmath does not import and numpy.longdouble has a %d-bit mantissa"
                    % (np.finfo(np.longdouble).nmant + 1))


def mp_ctx():
    mpmath.mp.prec = MP_BITS
    return mpmath.mp


def ulp_of(ref64):
    return np.spacing(np.abs(np.asarray(ref64, dtype=np.float64)))


def errors_ld(got, ref_ld):
    """|got - ref| in ulp of the reference rounded to float64; ref in longdouble."""
    ref64 = ref_ld.astype(np.float64)
    return (np.abs(got.astype(LD) - ref_ld) / ulp_of(ref64).astype(LD)).astype(np.float64)


def errors_mp(got, ref_mp):
    """The same against a list of mpmath values, in mpmath throughout."""
    mp = mp_ctx()
    out = np.empty(len(ref_mp))
    for i, (g, r) in enumerate(zip(got.tolist(), ref_mp)):
        out[i] = float(abs(mp.mpf(g) - r) / mp.mpf(float(np.spacing(abs(float(r))))))
    return out


def subsample(n, m, rs):
    return np.arange(n) if n <= m else np.sort(rs.choice(n, m, replace=False))


def worst_ulp(got, xs, f_ld, f_mp, rs, always_mp=None, sweep=MP_SWEEP):
    """Worst error in ulp of got = f(xs rows): longdouble over everything (where it is wide enough), mpmath over a sweep of
    MP_SWEEP rows plus the rows `always_mp`.  Returns (worst, index of the worst, points checked)."""
    need_reference()
    n = got.shape[0]
    err = np.zeros(n)
    checked = 0
    if LD_OK:
        err = errors_ld(got, f_ld(xs))
        checked = n
    if mpmath is not None:
        idx = subsample(n, sweep, rs)
        if always_mp is not None:
            idx = np.union1d(idx, always_mp)
        e = errors_mp(got[idx], [f_mp(row) for row in xs[idx].tolist()])
        err[idx] = np.maximum(err[idx], e) if LD_OK else e
        checked = max(checked, idx.size)
    k = int(np.argmax(err))
    return float(err[k]), k, checked


def log_uniform(rs, lo, hi, n):
    return 10.0 ** rs.uniform(math.log10(lo), math.log10(hi), n)


def switch_points(rs, centre, n_each):
    """centre 2^k (1 + delta), |delta| <= 2^-40, k = -3 .. 3, and the neighbours of the rounded centre itself."""
    out = []
    for k in range(-3, 4):
        c = centre * 2.0 ** k
        out.append(c * (1.0 + rs.uniform(-1.0, 1.0, n_each) * 2.0 ** -40))
        out.append(np.array([np.nextafter(c, 0.0), c, np.nextafter(c, np.inf)]))
    return np.concatenate(out)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------- 1. log_few_ulp
@gpu
def test_log_few_ulp_within_two_ulp(lib):
    rs = np.random.RandomState(101)
    near_switch = switch_points(rs, SQRT_HALF, 10000)
    powers = 2.0 ** np.arange(-1022, 1024)
    xs = np.concatenate([log_uniform(rs, 1e-304, 1e304, 400000), rs.uniform(0.5, 2.0, 200000),
                         1.0 + rs.uniform(-1e-6, 1e-6, 100000), np.array([np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)]),
                         near_switch, powers,
                         # the edges of the fast path (2.3e-308, 1.7e308) and the library's side of them
                         np.array([2.2250738585072014e-308, 2.29e-308, 2.3e-308, 2.31e-308, 1.69e308, 1.7e308, 1.71e308,
                                   np.finfo(np.float64).max])])
    got = lib.probe_math(lib.PK_MATH_LOG_FEW_ULP, xs)
    mp = mp_ctx() if mpmath is not None else None
    worst, k, n = worst_ulp(got, xs[:, None], lambda a: np.log(a[:, 0].astype(LD)), lambda r: mp.log(mp.mpf(r[0])), rs)
    print("log_few_ulp: worst %.4f ulp at x = %r over %d points" % (worst, xs[k], n))
    record("ops", "log_few_ulp", worst_ulp=worst, at=float(xs[k]), points=n, documented=2.0)
    assert np.all(got[xs == 1.0] == 0.0)
    assert worst <= 2.0, (worst, xs[k])


@gpu
def test_log_few_ulp_library_fallback(lib):
    rs = np.random.RandomState(102)
    sub = np.concatenate([np.array([5e-324, 1e-323, 2.2250738585072009e-308]), log_uniform(rs, 1e-323, 2.2e-308, 2000)])
    got = lib.probe_math(lib.PK_MATH_LOG_FEW_ULP, sub)
    mp = mp_ctx() if mpmath is not None else None
    worst, k, n = worst_ulp(got, sub[:, None], lambda a: np.log(a[:, 0].astype(LD)), lambda r: mp.log(mp.mpf(r[0])), rs)
    print("log_few_ulp on subnormals (library path): worst %.4f ulp at x = %r over %d points" % (worst, sub[k], n))
    record("ops", "log_few_ulp_library_path_subnormals", worst_ulp=worst, points=n)
    assert worst <= 2.0, (worst, sub[k])
    special = np.array([0.0, -0.0, -1.0, -1e-320, -np.inf, np.inf, np.nan])
    out = lib.probe_math(lib.PK_MATH_LOG_FEW_ULP, special)
    assert out[0] == -np.inf and out[1] == -np.inf
    assert np.isnan(out[2:5]).all()
    assert out[5] == np.inf
    assert np.isnan(out[6])


# ---------------------------------------------------------------------------------------------- 2. pub_log
@gpu
def test_pub_log_absolute_error_below_1e_12(lib):
    need_reference()
    rs = np.random.RandomState(201)
    xs = np.concatenate([log_uniform(rs, 1e-40, 1e120, 400000), switch_points(rs, SQRT_HALF, 10000), np.array([1e-40, 1.0, 1e120])])
    got = lib.probe_math(lib.PK_MATH_PUB_LOG, xs)
    err = np.zeros(xs.size)
    if LD_OK:
        err = np.abs(got.astype(LD) - np.log(xs.astype(LD))).astype(np.float64)
    if mpmath is not None:
        mp = mp_ctx()
        idx = subsample(xs.size, MP_SWEEP, rs)
        e = np.array([float(abs(mp.mpf(g) - mp.log(mp.mpf(x)))) for g, x in zip(got[idx].tolist(), xs[idx].tolist())])
        err[idx] = np.maximum(err[idx], e)
    k = int(np.argmax(err))
    print("pub_log: worst absolute error %.3e at x = %r over %d points" % (err[k], xs[k], xs.size))
    record("ops", "pub_log", worst_abs=float(err[k]), at=float(xs[k]), points=int(xs.size), documented=1e-12)
    assert err[k] < 1e-12, (err[k], xs[k])


@gpu
def test_pub_log_equal_inputs_give_equal_bits_in_every_lane(lib):
    """'A tie stays a tie': 64 copies each of 1 000 values, a stride of 1 000 elements apart (1 000 = 40 mod 64: the copies of one
    value sit in many different lanes and workgroups)."""
    rs = np.random.RandomState(202)
    vals = log_uniform(rs, 1e-40, 1e120, 1000)
    got = lib.probe_math(lib.PK_MATH_PUB_LOG, np.tile(vals, 64)).reshape(64, 1000)
    assert np.array_equal(bits(got), np.tile(bits(got[0]), (64, 1)))


# ---------------------------------------------------------------------------------------------- 3. pub_recip
@gpu
def test_pub_recip_error_in_ulp(lib):
    rs = np.random.RandomState(301)
    k = np.arange(-996, 997)
    around = [2.0 ** k]
    for sign in (0.0, np.inf):
        p = 2.0 ** k
        for _ in range(4):
            p = np.nextafter(p, sign)
            around.append(p)
    pos = np.concatenate([log_uniform(rs, 1e-300, 1e300, 500000), rs.uniform(1.0, 2.0, 200000)] + around)
    xs = np.concatenate([pos, -pos[::7]])
    got = lib.probe_math(lib.PK_MATH_PUB_RECIP, xs)
    mp = mp_ctx() if mpmath is not None else None
    worst, kk, n = worst_ulp(got, xs[:, None], lambda a: LD(1.0) / a[:, 0].astype(LD), lambda r: 1 / mp.mpf(r[0]), rs)
    print("pub_recip: worst %.4f ulp at x = %r over %d points" % (worst, xs[kk], n))
    record("ops", "pub_recip", worst_ulp=worst, at=float(xs[kk]), points=n, asserted_bound_ulp=math.ceil(1.5 * RECIP_MEASURED_ULP))
    assert worst <= math.ceil(1.5 * RECIP_MEASURED_ULP), (worst, xs[kk])


# ---------------------------------------------------------------------------------------------- 4. pk_atan2
def atan2_points():
    rs = np.random.RandomState(401)

    def variants(mn, mx):
        """all four sign combinations, both orders: rows (y, x)"""
        rows = []
        for a, b in ((mn, mx), (mx, mn)):
            for sy in (1.0, -1.0):
                for sx in (1.0, -1.0):
                    rows.append(np.stack([sy * a, sx * b], axis=1))
        return np.concatenate(rows)

    mx = log_uniform(rs, 1e-300, 1e300, 100000)
    mn = mx * log_uniform(rs, 1e-30, 1.0, 100000)
    general = variants(mn, mx)
    mx2 = np.concatenate([log_uniform(rs, 1e-300, 1e300, 15000), rs.uniform(0.1, 10.0, 5000)])
    upper = variants(TAN_PI_8 * mx2 * (1.0 + rs.uniform(-1.0, 1.0, mx2.size) * 2.0 ** -40), mx2)
    octant = variants(mx2 * (1.0 + rs.uniform(-1.0, 0.0, mx2.size) * 2.0 ** -40), mx2)
    equal = variants(mx2[:2000], mx2[:2000])
    return np.concatenate([general, upper, octant, equal]), general.shape[0]


@gpu
def test_pk_atan2_error_in_ulp_and_odd_symmetry(lib):
    pts, n_general = atan2_points()
    got = lib.probe_math(lib.PK_MATH_ATAN2, pts)
    rs = np.random.RandomState(402)
    mp = mp_ctx() if mpmath is not None else None
    edge = n_general + subsample(pts.shape[0] - n_general, MP_SWEEP // 2, rs)  # the two switches: mpmath's share of them
    worst, k, n = worst_ulp(got, pts, lambda a: np.arctan2(a[:, 0].astype(LD), a[:, 1].astype(LD)),
                            lambda r: math.copysign(1.0, r[0]) * mp.atan2(mp.mpf(abs(r[0])), mp.mpf(r[1])), rs, always_mp=edge,
                            sweep=MP_SWEEP // 2)  # (odd in y: mpmath has no -0.0, atan2(-0.0, x < 0) is -pi)
    print("pk_atan2: worst %.4f ulp at (y, x) = %r over %d points" % (worst, pts[k].tolist(), n))
    record("ops", "pk_atan2", worst_ulp=worst, at_y_x=pts[k].tolist(), points=n, documented=2.0, asserted_bound_ulp=1.5 * ATAN2_MEASURED_ULP)
    assert worst <= 1.5 * ATAN2_MEASURED_ULP, (worst, pts[k].tolist())
    # odd in y, bit for bit
    neg = lib.probe_math(lib.PK_MATH_ATAN2, pts * np.array([-1.0, 1.0]))
    assert np.array_equal(bits(neg), bits(-got))


@gpu
def test_pk_atan2_axes_zeros_and_nan(lib):
    pts = np.array([[0.0, 0.0], [-0.0, 2.5], [0.0, 2.5], [0.0, -2.5], [3.0, 0.0], [-3.0, 0.0], [1e-300, 0.0], [0.0, 1e300],
                    [np.nan, 1.0], [1.0, np.nan], [np.nan, np.nan], [np.nan, 0.0], [0.0, np.nan], [-0.0, 1e-300]])
    got = lib.probe_math(lib.PK_MATH_ATAN2, pts)
    assert got[0] == 0.0 and not np.signbit(got[0])
    assert got[1] == 0.0 and np.signbit(got[1])
    assert got[2] == 0.0 and not np.signbit(got[2])
    assert got[13] == 0.0 and np.signbit(got[13])
    want = np.array([math.pi, math.pi / 2, -math.pi / 2, math.pi / 2, 0.0])
    assert np.all(np.abs(got[3:8] - want) <= 2.0 * np.spacing(np.abs(want))), got[3:8]
    assert np.isnan(got[8:13]).all()


# ---------------------------------------------------------------------------------------------- 5. pub_round_down_to_float
@gpu
def test_round_down_to_float_never_rounds_up(lib):
    rs = np.random.RandomState(501)
    mag = log_uniform(rs, 1e-50, 1e40, 400000)
    p2 = 2.0 ** np.arange(-149, 128)  # every float32 power of two, subnormal ones included
    fmax = float(np.finfo(np.float32).max)
    edges = np.concatenate([p2, np.nextafter(p2, 0.0), np.nextafter(p2, np.inf),
                            np.array([fmax, np.nextafter(fmax, 0.0), np.nextafter(fmax, np.inf), fmax + 2.0 ** 102, fmax + 2.0 ** 103, 2.0 ** 128,
                                      np.nextafter(2.0 ** 128, 0.0), 1e39, 1e-50, 1e-46, 7e-46, 1.4e-45, 1.5e-45])])
    floats = np.concatenate([rs.standard_normal(50000).astype(np.float32).astype(np.float64) * 10.0 ** rs.randint(-38, 38, 50000),
                             rs.randint(1, 1 << 23, 20000).astype(np.uint32).view(np.float32).astype(np.float64)])  # (subnormals)
    floats = floats.astype(np.float32).astype(np.float64)
    floats = floats[np.isfinite(floats)]
    xs = np.concatenate([mag, -mag, edges, -edges, floats, -floats, np.array([0.0, -0.0])])
    got = lib.probe_math(lib.PK_MATH_ROUND_DOWN_F32, xs)
    with np.errstate(over="ignore"):
        as_float = got.astype(np.float32)
        above = np.nextafter(as_float, np.float32(np.inf)).astype(np.float64)
        exact = xs.astype(np.float32).astype(np.float64) == xs
    assert np.array_equal(bits(as_float.astype(np.float64)), bits(got)), "a result that is no float32 value"
    assert np.all(got <= xs), xs[~(got <= xs)][:5]
    assert np.all(above > xs), xs[~(above > xs)][:5]  # the LARGEST float not above x
    assert exact.sum() > 2 * floats.size
    assert np.array_equal(bits(got[exact]), bits(xs[exact]))  # (-0.0 stays -0.0)
    tiny = lib.probe_math(lib.PK_MATH_ROUND_DOWN_F32, np.array([1e-50, -1e-50]))
    assert tiny[0] == 0.0 and not np.signbit(tiny[0])
    assert tiny[1] == -float(np.uint32(1).view(np.float32))  # the smallest negative subnormal
    print("pub_round_down_to_float: %d arguments, none rounded up" % xs.size)
    record("ops", "pub_round_down_to_float", rounded_up=0, points=int(xs.size))


# ---------------------------------------------------------------------------------------------- 6. keys
@gpu
def test_weight_keys_preserve_order_and_round_trip(lib):
    rs = np.random.RandomState(601)
    raw = rs.randint(0, 1 << 63, 100000, dtype=np.int64).astype(np.uint64)  # random bit patterns: every exponent, subnormals
    raw = np.concatenate([raw, rs.randint(1, 1 << 52, 5000, dtype=np.int64).astype(np.uint64)])
    pos = raw.view(np.float64)
    pos = np.unique(pos[np.isfinite(pos) & (pos > 0)])
    neg = -np.unique(rs.permutation(pos)[:pos.size // 2])[::-1]
    special_pos = np.array([5e-324, 1e-320, 2.2250738585072009e-308, 2.2e-308, 1.0, 1e308, np.finfo(np.float64).max])
    pos = np.unique(np.concatenate([pos, special_pos]))
    neg = np.unique(np.concatenate([neg, -special_pos, np.array([-2.2e-308, -1.0, -1e308])]))
    xs = np.concatenate([np.array([-np.inf]), neg, np.array([-0.0, 0.0]), pos, np.array([np.inf])])
    assert np.all(np.diff(xs[np.isfinite(xs)]) >= 0) and xs.size > 100000
    keys, back = lib.probe_math(lib.PK_MATH_KEY, xs)
    assert keys.dtype == np.uint64
    assert np.all(keys[1:] > keys[:-1]), "the keys are not strictly increasing"  # -0.0 below +0.0 included
    assert np.array_equal(bits(back), bits(xs))
    b = bits(xs)
    restated = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    assert np.array_equal(keys, restated)
    print("keys: %d doubles in order" % xs.size)
    record("ops", "keys", out_of_order=0, round_trip_mismatches=0, points=int(xs.size))


# ---------------------------------------------------------------------------------------------- 7. pub_far_bound
def random_rotations3(rs, n):
    q, _ = np.linalg.qr(rs.standard_normal((n, 3, 3)))
    return q


def far_bound_landmarks():
    """2e4 rows in the compact order (mean x y r g b, pxx pxy pyy, crr crg crb cgg cgb cbb) and what they were drawn as:
    kind 0 colour block c I, 1 random SPD (condition number up to 1e6), 2 indefinite, 3 semidefinite (exactly: small integers),
    4 semidefinite up to rounding, 5 a determinant outside (1e-20, 1e60), 6 a NaN entry."""
    rs = np.random.RandomState(701)
    n = 20000
    kind = rs.choice([0, 1, 2, 3, 4], n, p=[0.25, 0.5, 0.1, 0.05, 0.1])
    kind[-60:-30] = 5
    kind[-30:] = 6
    rows = np.zeros((n, 14))
    rows[:, 0:5] = rs.uniform(-50, 50, (n, 5))
    # position block: SPD, determinant log-uniform over 1e-18 .. 1e58, axes ratio up to 1e6
    det2 = log_uniform(rs, 1e-18, 1e58, n)
    ratio = log_uniform(rs, 1.0, 1e6, n)  # (beyond 500 or so the position block is too ill-conditioned for a bound: kFarCond)
    a, b = np.sqrt(det2 * ratio), np.sqrt(det2 / ratio)
    th = rs.uniform(0, math.pi, n)
    c, s = np.cos(th), np.sin(th)
    rows[:, 5] = a * c * c + b * s * s
    rows[:, 6] = (a - b) * c * s
    rows[:, 7] = a * s * s + b * c * c
    # colour block
    det3 = log_uniform(rs, 1e-18, 1e58, n)
    cond = log_uniform(rs, 1.0, 1e6, n)
    mid = cond ** -rs.uniform(0, 1, n)
    lam = np.stack([np.ones(n), mid, 1.0 / cond], axis=1)  # eigenvalues up to scale
    lam[kind == 0] = 1.0
    lam[kind == 2, 2] *= -1.0
    two = (kind == 2) & (rs.uniform(0, 1, n) < 0.5)  # two negative eigenvalues: indefinite with a POSITIVE determinant
    lam[two, 1] *= -1.0
    lam[kind == 4, 2] = 0.0
    unit = np.where(np.isin(kind, (2, 4)), np.abs(lam[:, 0] * lam[:, 1]) * np.maximum(np.abs(lam[:, 2]), 1e-3), np.prod(lam, axis=1))
    lam *= ((det3 / unit) ** (1.0 / 3.0))[:, None]
    q = random_rotations3(rs, n)
    q[kind == 0] = np.identity(3)
    C = np.einsum("nij,nj,nkj->nik", q, lam, q)
    C = 0.5 * (C + np.transpose(C, (0, 2, 1)))
    for i in np.flatnonzero(kind == 3):  # v1 v1' + v2 v2' in small integers: rank two, determinant exactly 0 in float64 too
        v = rs.randint(-9, 10, (2, 3)).astype(np.float64)
        C[i] = np.outer(v[0], v[0]) + np.outer(v[1], v[1])
    rows[:, 8], rows[:, 9], rows[:, 10] = C[:, 0, 0], C[:, 0, 1], C[:, 0, 2]
    rows[:, 11], rows[:, 12], rows[:, 13] = C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]
    out = np.flatnonzero(kind == 5)
    scale = np.where(rs.uniform(0, 1, out.size) < 0.5, 1e-23, 1e63)
    which = rs.uniform(0, 1, out.size) < 0.5  # the position block's determinant, or the colour block's
    rows[out, 5:8] = np.where(which, np.sqrt(scale), 1.0)[:, None] * np.array([1.0, 0.25, 1.0])
    cs = np.where(which, 1.0, scale ** (1.0 / 3.0))
    rows[out, 8:14] = cs[:, None] * np.array([1.0, 0.1, -0.2, 1.0, 0.3, 1.0])
    for i in np.flatnonzero(kind == 6):
        rows[i, 5:14] = [2.0, 0.5, 1.0, 1.0, 0.1, -0.2, 1.0, 0.3, 1.0]
        rows[i, rs.randint(5, 14)] = np.nan
    return rows, kind


def exact_blocks(row):
    """mpmath: (det2, det3, adjugate of P (3 numbers), adjugate of C (6), colour block positive definite by Sylvester, both
    determinants exact: 600 bits hold every product of three doubles of one block and their sums."""
    mp = mpmath.mp
    with mp.workprec(600):
        pxx, pxy, pyy, a, b, c, d, e, f = [mp.mpf(v) for v in row[5:14]]
        det2 = pxx * pyy - pxy * pxy
        c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
        c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
        det3 = a * c00 + b * c01 + c * c02
        pd3 = bool(a > 0 and c22 > 0 and det3 > 0)
        pd2 = bool(pxx > 0 and det2 > 0)
        return det2, det3, (pyy, -pxy, pxx), (c00, c01, c02, c11, c12, c22), pd3, pd2


def exact_sylvester_fractions(row):
    """The same verdicts as exact_blocks in fractions.Fraction: both blocks positive definite, both determinants in the window."""
    from fractions import Fraction

    pxx, pxy, pyy, a, b, c, d, e, f = [Fraction(float(v)) for v in row[5:14]]
    det2 = pxx * pyy - pxy * pxy
    det3 = a * (d * f - e * e) + b * (c * e - b * f) + c * (b * e - c * d)
    lo, hi = Fraction(1, 10 ** 20), Fraction(10 ** 60)
    return pxx > 0 and a > 0 and a * d - b * b > 0 and lo < det2 < hi and lo < det3 < hi


@gpu
def test_far_bound_is_a_bound_and_claims_it_only_for_positive_definite_blocks(lib):
    rows, kind = far_bound_landmarks()
    out = lib.probe_math(lib.PK_MATH_FAR_BOUND, rows)
    fk, fi = out[:, 0], out[:, 1]
    assert np.all(fi >= 0.0) and not np.isnan(fi).any()
    # (a)
    assert np.all(fi[np.isin(kind, (2, 3, 5, 6))] == 0.0), "a bound claimed for an indefinite, singular, out-of-window or NaN block"
    assert (fi[kind == 0] > 0).sum() > 1000 and (fi[kind == 1] > 0).sum() > 1000  # (the test is about blocks the bound IS claimed for)
    blocks = {}
    claimed = np.flatnonzero(fi > 0)
    if mpmath is None:  # doubles are exact rationals: Sylvester without mpmath; the exact keys of (b) need its logarithm
        for i in claimed:
            assert exact_sylvester_fractions(rows[i]), "landmark %d (kind %d): fi = %g for blocks not positive definite and inside the window" % (i, kind[i], fi[i])
        pytest.skip("(a) held in exact rational arithmetic; the exact keys of (b) need mpmath")
    mp = mp_ctx()
    lo, hi = mp.mpf("1e-20"), mp.mpf("1e60")
    for i in claimed:  # (a block that is semidefinite only up to rounding, kind 4, may be claimed -- if it IS positive definite)
        blocks[i] = exact_blocks(rows[i])
        det2, det3, _, _, pd3, pd2 = blocks[i]
        assert pd3 and pd2, "landmark %d (kind %d): fi = %g for a block that is not positive definite: %r" % (i, kind[i], fi[i], rows[i, 5:14].tolist())
        assert lo < det2 < hi and lo < det3 < hi, "landmark %d: fi = %g with determinants %s, %s" % (i, fi[i], mp.nstr(det2, 8), mp.nstr(det3, 8))
    print("pub_far_bound (a): %d of %d landmarks claim a bound, every one positive definite and inside the window" % (claimed.size, rows.shape[0]))
    # (b) on an mpmath sweep of the claimed ones: 8 colour differences x 8 position errors each... one key per pair (d_i, e_i)
    rs = np.random.RandomState(702)
    sweep = claimed[subsample(claimed.size, MP_SWEEP // 8, rs)]
    worst = -np.inf
    for i in sweep:
        det2, det3, adj2, adj3, _, _ = blocks[i]
        base = 5 * mp.mpf(LOG_2PI) + mp.log(det2 * det3)
        dirs = rs.standard_normal((8, 3))
        ds = dirs / np.linalg.norm(dirs, axis=1)[:, None] * rs.uniform(0, 20, 8)[:, None]
        ds[0] = 0.0
        sd = math.sqrt(max(rows[i, 5], rows[i, 7]))
        es = rs.standard_normal((8, 2)) * sd * rs.uniform(0, 5, 8)[:, None]
        es[1] = 0.0
        for d, e in zip(ds.tolist(), es.tolist()):
            d0, d1, d2 = [mp.mpf(v) for v in d]
            e0, e1 = [mp.mpf(v) for v in e]
            q3 = (adj3[0] * d0 * d0 + adj3[3] * d1 * d1 + adj3[5] * d2 * d2 + 2 * (adj3[1] * d0 * d1 + adj3[2] * d0 * d2 + adj3[4] * d1 * d2)) / det3
            q2 = (adj2[0] * e0 * e0 + 2 * adj2[1] * e0 * e1 + adj2[2] * e1 * e1) / det2
            key = base + q2 + q3
            bound = mp.mpf(float(fk[i])) + mp.mpf(float(fi[i])) * (d0 * d0 + d1 * d1 + d2 * d2)
            # the slack: fk carries pub_log's 1e-12, fi lies a few ulp above 1 / rowmax at worst; the callers' own margins
            # (kFarKeySlack = 8, kFarVarFactor = 2, + 0.5) are twelve orders of magnitude wider
            excess = float((bound - key) / (1 + abs(key)))
            worst = max(worst, excess)
            assert excess <= 1e-12, "landmark %d (kind %d): key %s below its bound %s (d = %r)" % (i, kind[i], mp.nstr(key, 20), mp.nstr(bound, 20), d)
    print("pub_far_bound (b): %d landmarks x 8 pairs, largest (bound - key) / (1 + |key|) = %.3e" % (sweep.size, worst))
    record("ops", "pub_far_bound", landmarks=int(rows.shape[0]), claimed=int(claimed.size), claimed_not_positive_definite=0,
           worst_bound_minus_key_over_1_plus_abs_key=worst, pairs=int(8 * sweep.size), allowed=1e-12)


# ---------------------------------------------------------------------------------------------- 8. pr_from_parts
def pr_inputs():
    """rows (det2, det3, num2, num3) whose key 5 log 2 pi + log(det2 det3) + num2 / det2 + num3 / det3 sweeps 0 .. 1 500.  The
    split of the Mahalanobis term between the two factors is drawn so that, for keys up to 1 480, neither factor's exponent
    falls below -700: bp and cp stay normal numbers there (one of them underflowing by itself gives 0 in the reference too)."""
    rs = np.random.RandomState(801)
    n = 200000
    det2, det3 = log_uniform(rs, 1e-18, 1e58, n), log_uniform(rs, 1e-18, 1e58, n)
    target = np.concatenate([rs.uniform(0, 1500, n - 60000), rs.uniform(1470, 1500, 60000)])
    a2max, a3max = -0.5 * (2 * LOG_2PI + np.log(det2)), -0.5 * (3 * LOG_2PI + np.log(det3))  # exponents at Mahalanobis term 0
    t = np.minimum(-0.5 * target, a2max + a3max)  # (the key cannot go below its constant term)
    lo, hi = t - a3max, a2max
    small = -2.0 * t <= 1485.0
    lo = np.where(small, np.maximum(lo, -700.0), lo)
    hi = np.where(small, np.minimum(hi, t + 700.0), hi)
    assert np.all(lo <= hi + 1e-9)
    a2 = lo + rs.uniform(0, 1, n) * (hi - lo)
    a3 = t - a2
    maha2, maha3 = np.maximum(2.0 * (a2max - a2), 0.0), np.maximum(2.0 * (a3max - a3), 0.0)
    return np.stack([det2, det3, maha2 * det2, maha3 * det3], axis=1)


@gpu
def test_pr_from_parts_and_the_underflow_edge(lib):
    need_reference()
    rows = pr_inputs()
    got = lib.probe_math(lib.PK_MATH_PR_FROM_PARTS, rows)
    det2, det3, num2, num3 = [rows[:, i] for i in range(4)]
    # the exact key of every row (longdouble: 1e-19 relative, the classes below keep 1e-9 clear of their edges)
    if LD_OK:
        key = (5 * LD(LOG_2PI) + np.log(det2.astype(LD)) + np.log(det3.astype(LD)) + num2.astype(LD) / det2.astype(LD)
               + num3.astype(LD) / det3.astype(LD))
    else:
        mp = mp_ctx()
        key = np.array([float(5 * mp.mpf(LOG_2PI) + mp.log(mp.mpf(r[0])) + mp.log(mp.mpf(r[1])) + mp.mpf(r[2]) / mp.mpf(r[0])
                              + mp.mpf(r[3]) / mp.mpf(r[1])) for r in rows.tolist()])
    key64 = key.astype(np.float64)
    assert key64.min() < 1.0 and key64.max() > 1499.0
    # beyond kPubFarKey: exactly 0 -- on the device, and in the reference's own expression (prkt_core_v2.py:439-455) in float64
    far = key64 >= FAR_KEY + 1e-9
    assert far.sum() > 10000
    with np.errstate(under="ignore"):
        bp = 500.0 * np.exp(-0.5 * (2.0 * LOG_2PI + np.log(det2[far]) + num2[far] / det2[far]))
        cp = 500.0 * np.exp(-0.5 * (3.0 * LOG_2PI + np.log(det3[far]) + num3[far] / det3[far]))
        assert np.all(bp * cp / 250000.0 == 0.0), "kPubFarKey is not beyond the reference's own underflow edge"
    assert np.all(got[far] == 0.0), "a probability above 0 beyond kPubFarKey: keys %r" % key64[far][got[far] != 0.0][:5].tolist()
    near = key64 <= 1480.0
    assert np.all(got[near] > 0.0), "probability 0 at keys %r" % key64[near][~(got[near] > 0.0)][:5].tolist()
    # the value, where it is a normal number with room to spare
    big = np.flatnonzero(key64 <= -2.0 * math.log(1e-300))
    assert big.size > 50000
    rs = np.random.RandomState(802)
    rel = np.zeros(big.size)
    if LD_OK:
        ref = np.exp(-0.5 * key[big])
        rel = (np.abs(got[big].astype(LD) - ref) / ref).astype(np.float64)
    if mpmath is not None:
        mp = mp_ctx()
        sub = subsample(big.size, MP_SWEEP, rs)
        for j in sub:
            r = rows[big[j]].tolist()
            k = 5 * mp.mpf(LOG_2PI) + mp.log(mp.mpf(r[0]) * mp.mpf(r[1])) + mp.mpf(r[2]) / mp.mpf(r[0]) + mp.mpf(r[3]) / mp.mpf(r[1])
            ref_j = mp.exp(-k / 2)
            rel[j] = max(rel[j], float(abs(mp.mpf(float(got[big[j]])) - ref_j) / ref_j))
    j = int(np.argmax(rel))
    print("pr_from_parts: worst relative error %.3e at key %.3f over %d values >= 1e-300; %d keys beyond %g all exactly 0; %d keys "
          "<= 1480 all above 0" % (rel[j], key64[big[j]], big.size, far.sum(), FAR_KEY, near.sum()))
    record("ops", "pr_from_parts", worst_relative_error=float(rel[j]), at_key=float(key64[big[j]]), points=int(big.size),
           asserted_bound=1.5 * PR_MEASURED_RELERR, keys_beyond_1492=int(far.sum()), nonzero_beyond_1492=0,
           keys_up_to_1480=int(near.sum()), zero_up_to_1480=0)
    assert rel[j] <= 1.5 * PR_MEASURED_RELERR, (rel[j], key64[big[j]])


# ---------------------------------------------------------------------------------------------- 9. refusals
@gpu
def test_probe_math_refusals(lib):
    import ctypes as C

    so = lib.load()
    x = np.array([1.0, 2.0, 4.0])
    out = np.zeros(3)
    xp, op = lib.dptr(x), lib.dptr(out)
    ndev = so.pk_device_count()

    def good():
        assert np.array_equal(lib.probe_math(lib.PK_MATH_PUB_RECIP, x), [1.0, 0.5, 0.25])

    good()
    bad = [
        ((0, lib.PK_MATH_PUB_RECIP, 3, None, op), lib.PK_ERR_INVALID, "NULL"),
        ((0, lib.PK_MATH_PUB_RECIP, 3, xp, None), lib.PK_ERR_INVALID, "NULL"),
        ((0, 8, 3, xp, op), lib.PK_ERR_INVALID, "unknown op"),
        ((0, 11, 3, xp, op), lib.PK_ERR_INVALID, "unknown op"),  # PK_MATH_COUNT: the first op beyond the last
        ((0, -1, 3, xp, op), lib.PK_ERR_INVALID, "unknown op"),
        ((0, lib.PK_MATH_PUB_RECIP, -1, xp, op), lib.PK_ERR_INVALID, "n = -1"),
        ((-1, lib.PK_MATH_PUB_RECIP, 3, xp, op), lib.PK_ERR_INVALID, "device -1"),
        ((ndev, lib.PK_MATH_PUB_RECIP, 3, xp, op), lib.PK_ERR_INVALID, "device %d" % ndev),
    ]
    for args, status, text in bad:
        out[:] = 7.0
        assert so.pk_probe_math(*args) == status, args
        msg = so.pk_last_error().decode()
        assert msg.startswith("pk_probe_math:") and text in msg, msg
        assert np.all(out == 7.0)
        good()
    # n == 0: PK_OK, nothing launched, nothing written
    out[:] = 7.0
    assert so.pk_probe_math(0, lib.PK_MATH_PUB_RECIP, 0, xp, op) == lib.PK_OK
    assert np.all(out == 7.0)
    assert lib.probe_math(lib.PK_MATH_KEY, np.zeros(0))[0].shape == (0,)
    assert lib.probe_math(lib.PK_MATH_FAR_BOUND, np.zeros((0, 14))).shape == (0, 2)
    assert sorted(lib.PK_MATH_SHAPES) == [0, 1, 2, 3, 4, 5, 6, 7, 9, 10]  # (8 is refused for good, 11 is the first beyond the last)
    assert lib.probe_math(lib.PK_MATH_EKF_UPDATE, np.zeros((0, 31))).shape == (0, 17)
    assert lib.probe_math(lib.PK_MATH_MATCH, np.zeros((0, 23))).shape == (0, 5)
    with pytest.raises(lib.PkError) as ei:
        lib.probe_math(lib.PK_MATH_ATAN2, np.zeros((2, 2)), device=ndev)
    assert ei.value.status == lib.PK_ERR_INVALID
    good()


def test_probe_math_refuses_without_a_device(lib):
    """CPU: no HIP device, no answer (the HIP path has no CPU fallback) -- and a bad argument is refused before the device is asked
    for, as in pk_probe."""
    so = lib.load()
    if so.pk_device_count() != 0:
        pytest.skip("a HIP device is visible")
    with pytest.raises(lib.PkError) as ei:
        lib.probe_math(lib.PK_MATH_PUB_LOG, np.ones(4))
    assert ei.value.status == lib.PK_ERR_HIP and "pk_probe_math: no HIP device" in str(ei.value)
    x = np.ones(4)
    assert so.pk_probe_math(0, 99, 4, lib.dptr(x), lib.dptr(x)) == lib.PK_ERR_INVALID
    assert "unknown op 99" in so.pk_last_error().decode()

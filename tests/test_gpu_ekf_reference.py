"""GPU: ekf_update in every variant, prob_position_match, prob_color_match and probability_of_match (pk_math.hpp) -- the algebra
every observe route ends in -- through the PK_MATH_EKF_UPDATE / PK_MATH_MATCH ops of pk_probe_math, against the exact dense
reference of tests/ekf_reference.py (mpmath, 300 bits) on its input classes, every point:

  update (new mean, new covariance blocks, log weight)   units <= 32 + kappa^2 / 8        kappa = cond(C + Qc)
  log position density, closest point                     units <= 32 + kappa2             kappa2 = cond(P)
  log colour density, log probability_of_match            units <= 32 + kappa3^2 / 8 + kappa2,  kappa3 = cond(C)

(units, scales and where the constants come from: ekf_reference.py; tests/test_ekf_reference_host.py holds the float64
restatement of the reference to the same bounds on the same points, without a GPU).  Route agreement cannot see a wrong digit
here -- every route calls these functions -- and the oracle tests at 1e-9 draw well-conditioned landmarks at ranges of metres.
Then the variants no test isolated, bit for bit: the expected bearing supplied, COLOUR = false, immutable, the one-logarithm
form, the potential bit and its promotion, q == 0, the two forms of the colour block, NaN in / NaN out, the gates' exact zeros.

With PK_FIGURES_JSON=profiles/r10/ekf_errors.json the measured figures, the device's beside the oracle's on the same points, are
written there (run with -s to see them)."""
import math

import numpy as np
import pytest

import ekf_reference as er
from figures_record import record

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(er.mpmath is None, reason="mpmath does not import: no exact reference here")]

WHAT = ("worst errors of ekf_update and the match densities (pk_math.hpp, through PK_MATH_EKF_UPDATE / PK_MATH_MATCH) against the "
        "exact dense reference of tests/ekf_reference.py, per input class and output, in units of 2^-53 x the sum of the absolute "
        "terms, and the worst ratio to the asserted bound; the float64 oracle's figures on the same points beside them; written "
        "by the tests: PK_FIGURES_JSON=<this file> pytest -m gpu tests/test_gpu_ekf_reference.py")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def ekf(lib, rows, flags=None, **cols):
    """PK_MATH_EKF_UPDATE on a copy of rows with the flags (and other columns) set"""
    r = np.array(rows, dtype=np.float64)
    if flags is not None:
        r[:, er.E_FLAGS] = flags
    for k, v in cols.items():
        r[:, getattr(er, "E_" + k.upper())] = v
    return lib.probe_math(lib.PK_MATH_EKF_UPDATE, r)


def typical(n=64):
    return np.array(er.draw_class("typical")[0][:n])


def device_atan2(lib, rows):
    return lib.probe_math(lib.PK_MATH_ATAN2, np.stack([rows[:, er.E_F + 1] - rows[:, er.E_SY], rows[:, er.E_F] - rows[:, er.E_SX]], axis=1))


# ------------------------------------------------------------------------------------------------- the classes, every point
@pytest.mark.parametrize("name", er.CLASSES)
def test_device_against_the_exact_reference(lib, name):
    rows, mrows = er.draw_class(name)
    out = ekf(lib, rows, flags=er.ZHAT0_KNOWN)  # (the expected bearing is an input of the reference too)
    mout = lib.probe_math(lib.PK_MATH_MATCH, mrows)
    assert out.shape == (er.N_POINTS, 17) and mout.shape == (er.N_POINTS, 5)
    dev = er.class_figures(name, [(o[er.O_F:er.O_F + 14], o[er.O_LOGW]) for o in out], [tuple(m) for m in mout])
    ora = er.class_figures(name, [er.oracle_update(r) for r in rows], [er.oracle_match(r) for r in mrows])
    for key in sorted(dev):
        d, o = dev[key], ora[key]
        print("%s %-13s device %.4g units, %.3f of the bound (%d points); oracle %.4g units, %.3f" % (
            name, key, d["worst_units"], d["worst_ratio"], d["points"], o["worst_units"], o["worst_ratio"]))
        record("ekf", "%s.%s" % (name, key), _what=WHAT, device_worst_units=d["worst_units"], device_worst_ratio_to_bound=d["worst_ratio"],
               oracle_worst_units=o["worst_units"], oracle_worst_ratio_to_bound=o["worst_ratio"], points=d["points"])
    assert np.array_equal(out[:, er.O_COUNT], rows[:, er.E_COUNT] + 2.0)
    assert same_bits(out[:, er.O_PROD], rows[:, er.E_PROD])  # (not the one-logarithm form: untouched)
    ex_u, ex_m = er.exact_class(name)
    floor = math.log(er.DENSITY_FLOOR)
    for m, e in zip(mout, ex_m):  # what is not compared as a number: an exact zero where a gate is closed, a tiny one below the floor
        if e["log_match"] is None:
            assert m[0] == 0.0
        elif e["log_match"] < floor - 1.0:
            assert 0.0 <= m[0] < 10.0 * er.DENSITY_FLOOR
        if e["log_position"] is None:
            assert m[1] == 0.0
        elif e["log_position"] < floor - 1.0:
            assert 0.0 <= m[1] < 10.0 * er.DENSITY_FLOOR
    if name == "q_zero":  # h = 0: the position mean and block are not touched, bit for bit
        assert same_bits(out[:, er.O_F:er.O_F + 2], rows[:, er.E_F:er.E_F + 2])
        assert same_bits(out[:, er.O_F + 5:er.O_F + 8], rows[:, er.E_F + 5:er.E_F + 8])
    for key in ("mean", "covariance", "log_weight", "closest_point"):
        assert dev[key]["points"] == er.N_POINTS
    assert dev["log_position"]["points"] == ora["log_position"]["points"] >= er.N_POINTS // 2
    assert dev["log_colour"]["points"] == ora["log_colour"]["points"] >= er.N_POINTS // 2
    assert dev["log_match"]["points"] >= er.N_POINTS // 4
    for key, d in dev.items():
        assert d["worst_ratio"] <= 1.0, (name, key, d)


# ------------------------------------------------------------------------------------------------- the variants, bit for bit
def test_a_supplied_expected_bearing_gives_the_bits_of_the_call_without_it(lib):
    rows = np.concatenate([typical(), np.array(er.draw_class("close_range")[0][:32]), np.array(er.draw_class("q_zero")[0][:8])])
    plain = ekf(lib, rows, flags=0, zhat0=123.0)  # (not read)
    known = ekf(lib, rows, flags=er.ZHAT0_KNOWN, zhat0=device_atan2(lib, rows))
    assert same_bits(plain, known)
    other = ekf(lib, rows, flags=er.ZHAT0_KNOWN, zhat0=device_atan2(lib, rows) + 1e-3)  # ... and it IS read
    assert np.all(other[:, er.O_LOGW] != plain[:, er.O_LOGW])


def test_colour_false_leaves_the_colour_block_and_changes_nothing_else(lib):
    rows = np.concatenate([typical(), np.array(er.draw_class("general_qt")[0][:32])])
    for base in (0, er.FRO_PROD, er.ZHAT0_KNOWN):
        full = ekf(lib, rows, flags=base, prod=3.0)
        table = ekf(lib, rows, flags=base | er.NO_COLOUR, prod=3.0)
        block = slice(er.O_F + 8, er.O_F + 14)
        assert same_bits(table[:, block], rows[:, er.E_F + 8:er.E_F + 14])
        assert not np.any(full[:, block] == rows[:, er.E_F + 8:er.E_F + 14])
        keep = np.ones(17, dtype=bool)
        keep[block] = False
        assert same_bits(table[:, keep], full[:, keep])


def test_immutable_touches_no_field_and_weighs_like_the_mutable_call(lib):
    rows = typical()
    rows[::3, er.E_COUNT] += er.POTENTIAL
    for base in (0, er.FRO_PROD, er.NO_COLOUR):
        mutable = ekf(lib, rows, flags=base, prod=0.5)
        frozen = ekf(lib, rows, flags=base | er.IMMUTABLE, prod=0.5)
        assert same_bits(frozen[:, er.O_F:er.O_F + 14], rows[:, er.E_F:er.E_F + 14])
        assert same_bits(frozen[:, er.O_COUNT], rows[:, er.E_COUNT])
        assert same_bits(frozen[:, er.O_LOGW], mutable[:, er.O_LOGW]) and same_bits(frozen[:, er.O_PROD], mutable[:, er.O_PROD])
        assert not np.any(mutable[:, er.O_F + 2:er.O_F + 5] == rows[:, er.E_F + 2:er.E_F + 5])


def test_the_one_logarithm_form(lib):
    """fro_prod: the squared Frobenius norm is multiplied into the caller's product, exactly; the returned value lacks exactly the
    -1/4 log(fro2) of the plain form (within 4 units of the log weight's scale: the two roundings of either side); a potential
    landmark returns log(0.1) and leaves the product alone."""
    rows = np.concatenate([typical(), np.array(er.draw_class("fresh")[0][:32]), np.array(er.draw_class("converged")[0][:32])])
    plain = ekf(lib, rows, flags=0)
    one = ekf(lib, rows, flags=er.FRO_PROD, prod=1.0)
    fro2 = one[:, er.O_PROD]  # 1.0 * fro2
    assert np.all(fro2 > 0) and np.all(np.isfinite(fro2))
    for p in (0.75, 3.0, 1.2345678901234567e-40, 7.0e35):
        got = ekf(lib, rows, flags=er.FRO_PROD, prod=p)
        assert same_bits(got[:, er.O_PROD], p * fro2)
        assert same_bits(got[:, er.O_LOGW], one[:, er.O_LOGW])
    assert same_bits(one[:, er.O_F:er.O_COUNT + 1], plain[:, er.O_F:er.O_COUNT + 1])
    mp = er._ctx()
    worst = 0.0
    for i, r in enumerate(rows):
        e = er.exact_update(r)
        whole = mp.mpf(float(one[i, er.O_LOGW])) - mp.log(mp.mpf(float(fro2[i]))) / 4
        u = float(abs(whole - mp.mpf(float(plain[i, er.O_LOGW]))) / (mp.mpf(er.UNIT) * mp.mpf(e["logw_scale"])))
        worst = max(worst, u)
        assert u <= 4.0, (i, u)
    print("one-logarithm form against the plain form: worst %.3f units of the log weight's scale" % worst)
    record("ekf", "fro_prod_against_plain", _what=WHAT, worst_units=worst, asserted=4.0, points=int(rows.shape[0]))
    pot = ekf(lib, rows, flags=er.FRO_PROD, prod=0.75, count=rows[:, er.E_COUNT] + er.POTENTIAL)
    assert np.all(pot[:, er.O_LOGW] == er.LOG_NO_MATCH)
    assert np.all(pot[:, er.O_PROD] == 0.75)


def test_the_product_of_norms_never_leaves_the_normal_numbers(lib):
    """fro_prod with a caller's product at either end of the doubles: p fro2 would be infinite, zero or subnormal (eight factors of
    3e40, Qt = 1e20 I, were).  The product returned is a positive normal number, and together with the returned value it still
    says what the plain form says: logw_one - 1/4 log(prod_out) = logw_plain - 1/4 log(p), within 4 units of the scale
    logw_scale + 1/4 |log p| + 1/4 |log prod_out|.  The 4 is a count, not a measurement: both log-weights are doubles (half a
    unit of their own size each), the term e ln 2 / 4 is rounded once with the sum it is added to (half a unit) and its constant
    ln 2 / 4 is a rounded double (half a unit of e ln 2 / 4, which |log p| / 4 + |log prod_out| / 4 bounds): 2 units, doubled for
    the sum that the one-logarithm form orders differently -- the same allowance test_the_one_logarithm_form makes.  Where the
    product stays normal it is p fro2, bit for bit, as test_the_one_logarithm_form holds."""
    ignored = typical()  # Qt's colour block 1e20 I, what a caller sets to make the filter ignore colour: fro2 = 3e40
    ignored[:, [er.E_QT + 1, er.E_QT + 4, er.E_QT + 6]] = 1e20
    rows = np.concatenate([typical(), np.array(er.draw_class("fresh")[0][:32]), np.array(er.draw_class("converged")[0][:32]), ignored])
    plain = ekf(lib, rows, flags=0)
    one = ekf(lib, rows, flags=er.FRO_PROD, prod=1.0)
    fro2 = one[:, er.O_PROD]
    assert np.all(fro2[-64:] > 2.9e40) and np.all(fro2[-64:] < 3.1e40)
    mp = er._ctx()
    tiny = float(np.finfo(np.float64).tiny)
    worst, split = 0.0, 0
    for p in (1.7e308, 3e40 ** 7, tiny, 1e3 * tiny):  # (3e40^7: the eighth factor of a landmark pair)
        got = ekf(lib, rows, flags=er.FRO_PROD, prod=p)
        out = got[:, er.O_PROD]
        assert np.all(np.isfinite(out)) and np.all(out >= tiny), p
        with np.errstate(over="ignore", under="ignore"):
            whole = p * fro2
        stays = np.isfinite(whole) & (whole >= tiny)
        assert same_bits(out[stays], whole[stays]) and same_bits(got[stays, er.O_LOGW], one[stays, er.O_LOGW])
        split += int((~stays).sum())
        assert not stays[-64:].any() or p < 1.0  # (every one of the 3e40 takes the split path at the top)
        assert (~stays)[96:128].sum() >= 16 or p != tiny  # (and the converged landmarks, fro2 about 0.04, at the very bottom)
        for i in np.flatnonzero(~stays):
            e = er.exact_update(rows[i])
            lhs = mp.mpf(float(got[i, er.O_LOGW])) - mp.log(mp.mpf(float(out[i]))) / 4
            rhs = mp.mpf(float(plain[i, er.O_LOGW])) - mp.log(mp.mpf(p)) / 4
            scale = e["logw_scale"] + float(abs(mp.log(mp.mpf(p)))) / 4 + float(abs(mp.log(mp.mpf(float(out[i]))))) / 4
            u = float(abs(lhs - rhs) / (mp.mpf(er.UNIT) * mp.mpf(scale)))
            worst = max(worst, u)
            assert u <= 4.0, (p, i, u)
    assert split >= 128
    print("split product against the plain form: worst %.3f units over %d points" % (worst, split))
    record("ekf", "fro_prod_split_against_plain", _what=WHAT, worst_units=worst, asserted=4.0)
    pot = ekf(lib, rows, flags=er.FRO_PROD, prod=1e300, count=rows[:, er.E_COUNT] + er.POTENTIAL)  # a potential landmark: left alone
    assert np.all(pot[:, er.O_PROD] == 1e300) and np.all(pot[:, er.O_LOGW] == er.LOG_NO_MATCH)


def test_the_count_and_the_potential_bit(lib):
    """+2 per update (:914, :930); a potential landmark weighs log(0.1) (:111-112), is updated like any other, and loses the bit
    exactly when its count passes 5 (:113-117)."""
    rows = typical(9 * 7)
    counts = np.tile(np.arange(9.0), 7)
    full = ekf(lib, rows, flags=0, count=counts)
    pot = ekf(lib, rows, flags=0, count=counts + er.POTENTIAL)
    assert np.array_equal(full[:, er.O_COUNT], counts + 2.0)
    promoted = counts + 2.0 > 5.0
    assert promoted.sum() == 5 * 7 and (~promoted).sum() == 4 * 7
    assert np.array_equal(pot[:, er.O_COUNT], np.where(promoted, counts + 2.0, counts + 2.0 + er.POTENTIAL))
    assert same_bits(pot[:, er.O_F:er.O_F + 14], full[:, er.O_F:er.O_F + 14])
    assert np.all(pot[:, er.O_LOGW] == er.LOG_NO_MATCH) and not np.any(full[:, er.O_LOGW] == er.LOG_NO_MATCH)
    frozen = ekf(lib, rows, flags=er.IMMUTABLE, count=counts + er.POTENTIAL)  # an immutable one is never promoted
    assert np.array_equal(frozen[:, er.O_COUNT], counts + er.POTENTIAL)


def test_both_forms_of_the_colour_block_are_one_matrix(lib):
    """Qt with rg = 1e-300 takes the general form C - C M of colour_block_update, rg = 0 the short one Qc M: two expressions, one
    matrix -- both within the bound of the same exact value (1e-300 is below every digit of it)."""
    rows = np.array(er.draw_class("typical")[0])
    ex = er.exact_class("typical")[0]
    short = ekf(lib, rows, flags=er.ZHAT0_KNOWN)
    rows[:, er.E_QT + 2] = 1e-300
    general = ekf(lib, rows, flags=er.ZHAT0_KNOWN)
    block = slice(er.O_F + 8, er.O_F + 14)
    assert not same_bits(short[:, block], general[:, block])  # (two different expressions did run)
    keep = np.ones(17, dtype=bool)
    keep[block] = False
    assert same_bits(short[:, keep], general[:, keep])
    worst = {}
    for form, out in (("short", short), ("general", general)):
        ratios = [er.update_units(o[er.O_F:er.O_F + 14], o[er.O_LOGW], e)[1] / er.update_bound(e["kappa"]) for o, e in zip(out, ex)]
        worst[form] = max(ratios)
        assert worst[form] <= 1.0, (form, worst[form])
    print("colour block, worst ratio to the bound: short form %.3f, general form %.3f" % (worst["short"], worst["general"]))
    record("ekf", "colour_block_forms", _what=WHAT, short_form_worst_ratio=worst["short"], general_form_worst_ratio=worst["general"],
           points=int(rows.shape[0]))


def test_the_position_block_is_treated_symmetrically(lib):
    """The compact layout holds pxy once: nxy = pxy - (k0 a1 + k1 a0) / 2, the mean of the two products of (I - K H) Sigma.  With x
    and y exchanged in every input (h = (dy, dx) / q exchanges with them) the outputs come back exchanged, within the bound of the
    same exact values."""
    rows = np.array(er.draw_class("typical")[0])
    ex = er.exact_class("typical")[0]
    mirrored = rows.copy()
    for a, b in ((er.E_SX, er.E_SY), (er.E_F, er.E_F + 1), (er.E_F + 5, er.E_F + 7)):
        mirrored[:, [a, b]] = rows[:, [b, a]]
    out = ekf(lib, mirrored, flags=er.ZHAT0_KNOWN)
    back = out.copy()
    for a, b in ((er.O_F, er.O_F + 1), (er.O_F + 5, er.O_F + 7)):
        back[:, [a, b]] = out[:, [b, a]]
    for o, e in zip(back, ex):
        um, uc, uw = er.update_units(o[er.O_F:er.O_F + 14], o[er.O_LOGW], e)
        assert max(um, uc, uw) <= er.update_bound(e["kappa"])


def test_nan_in_any_input_is_nan_out(lib):
    """A NaN state fails every comparison downstream only if it stays a NaN: never a finite log weight from a NaN input."""
    base = typical(1)[0]
    cols = [c for c in range(31) if c not in (er.E_COUNT, er.E_FLAGS, er.E_PROD)]
    for flags in (0, er.ZHAT0_KNOWN, er.FRO_PROD | er.ZHAT0_KNOWN, er.NO_COLOUR, er.IMMUTABLE):
        use = [c for c in cols if c != er.E_ZHAT0 or flags & er.ZHAT0_KNOWN]
        rows = np.tile(base, (len(use), 1))
        rows[np.arange(len(use)), use] = np.nan
        out = ekf(lib, rows, flags=flags)
        assert np.isnan(out[:, er.O_LOGW]).all(), (flags, [use[i] for i in np.flatnonzero(~np.isnan(out[:, er.O_LOGW]))])
    m = np.array(er.draw_class("typical")[1][0])
    assert er.exact_class("typical")[1][0]["log_match"] is not None
    # the match probability: every field but the heading and the bearing, which enter the gates alone (abs(nan) > 0.5 is False in
    # the reference program too, :433; a NaN bearing comes with a NaN unit ray)
    use = [c for c in range(23) if c not in (er.M_H, er.M_BLOB)]
    mrows = np.tile(m, (len(use), 1))
    mrows[np.arange(len(use)), use] = np.nan
    mout = lib.probe_math(lib.PK_MATH_MATCH, mrows)
    assert np.isnan(mout[:, 0]).all(), [use[i] for i in np.flatnonzero(~np.isnan(mout[:, 0]))]


def test_the_gates_return_exact_zeros(lib):
    """probability_of_match: |delb| > 0.5 (:433), colour distance^2 > 300 (:441); prob_position_match: |pse - bearing| > pi / 2
    (:473-475); closest_point behind the ray: the pose itself (:515-516).  Every input 1e-6 clear of its gate (the edges themselves:
    test_gate_boundaries)."""
    mrows, ex = er.draw_class("typical")[1], er.exact_class("typical")[1]
    pick = [i for i, e in enumerate(ex) if e["log_match"] is not None and e["log_match"] > -600.0][:32]
    assert len(pick) == 32
    base = np.array(mrows[pick])
    open_ = lib.probe_math(lib.PK_MATH_MATCH, base)
    assert np.all(open_[:, :3] > 0.0)
    delta = np.array([ex[i]["delb"] for i in pick]) - base[:, er.M_H]  # bearing - pse
    for delb in (0.6, -0.6, 0.5 + 2e-6, -0.5 - 2e-6):
        rows = base.copy()
        rows[:, er.M_H] = delb - delta
        out = lib.probe_math(lib.PK_MATH_MATCH, rows)
        assert np.all(out[:, 0] == 0.0) and same_bits(out[:, 1:], open_[:, 1:])  # the heading enters nothing else
    rows = base.copy()
    rows[:, er.M_BLOB + 1] = base[:, er.M_F + 2] + math.sqrt(301.0)
    rows[:, er.M_BLOB + 2:er.M_BLOB + 4] = base[:, er.M_F + 3:er.M_F + 5]
    out = lib.probe_math(lib.PK_MATH_MATCH, rows)
    assert np.all(out[:, 0] == 0.0) and np.all(out[:, 1] == open_[:, 1])
    for turn in (math.pi / 2 + 1e-3, 2.0, math.pi - 0.3, -2.5):  # the ray points away: behind it from pi / 2 on
        rows = base.copy()
        bearing = base[:, er.M_BLOB] - delta + turn
        rows[:, er.M_BLOB] = bearing
        rows[:, er.M_UX], rows[:, er.M_UY] = np.cos(bearing), np.sin(bearing)
        out = lib.probe_math(lib.PK_MATH_MATCH, rows)
        assert np.all(out[:, 0] == 0.0) and np.all(out[:, 1] == 0.0) and np.all(out[:, 2] == open_[:, 2])
        assert same_bits(out[:, 3:5], rows[:, er.M_SX:er.M_SY + 1])  # the pose itself

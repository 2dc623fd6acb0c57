"""CPU: the odometry motion model's host side.  The formulas themselves (tests/odom_reference.py) close -- the delta between two
poses, put back onto the first with no noise, gives the second -- the library's pk_odom_delta / pk_odom_sigmas (host only: the
library loads without a GPU) are those formulas, they refuse what the header says they refuse, and the kernel's code object uses
no scratch."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import odom_reference as ref


@pytest.fixture(scope="module")
def lib():
    from parakeet_slam_amd import _lib, build

    build.build(verbose=False)
    _lib.load()
    return _lib


def random_pairs(n, seed, min_step=0.0, max_step=1.5):
    rs = np.random.RandomState(seed)
    prev = np.stack([rs.uniform(-50, 50, n), rs.uniform(-50, 50, n), rs.uniform(-math.pi, math.pi, n)], 1)
    step, direction = rs.uniform(min_step, max_step, n), rs.uniform(-math.pi, math.pi, n)
    now = np.stack([prev[:, 0] + step * np.cos(direction), prev[:, 1] + step * np.sin(direction), rs.uniform(-math.pi, math.pi, n)], 1)
    return prev, now


def closure_error(prev, now, min_trans=0.01, delta=None):
    """(position error, heading error) of the delta put back onto prev; delta: ref.delta, or the library's pk_odom_delta."""
    got = ref.compose(prev, (delta or ref.delta)(prev, now, min_trans))
    return math.hypot(got[0] - now[0], got[1] - now[1]), float(ref.angle_diff(got[2], now[2]))


def both_deltas(lib):
    """The restatement and the product: every closure case runs through both."""
    return (("tests/odom_reference.py", ref.delta), ("pk_odom_delta", lib.odom_delta))


# |x|, |y| <= 50, steps <= 1.5: the worst error of the formulas over 200 000 random pairs was 1.8e-15
CLOSURE = 1e-12


def test_the_delta_composed_onto_prev_gives_now_forward_backward_and_across_the_seam(lib):
    cases = {
        "forward": ((1.0, 2.0, 0.5), (1.0 + 0.8 * math.cos(0.5), 2.0 + 0.8 * math.sin(0.5), 0.5)),
        "forward and turning": ((-30.0, 12.0, 2.0), (-30.4, 12.9, 2.6)),
        "backward": ((1.0, 2.0, 0.0), (0.2, 2.0, 0.0)),
        "backward, oblique": ((5.0, -7.0, 1.0), (5.0 - 0.6 * math.cos(1.0), -7.0 - 0.6 * math.sin(1.0), 1.0)),
        "heading just below +pi to just above -pi": ((10.0, 10.0, math.pi - 0.05), (9.3, 10.02, -math.pi + 0.07)),
        "heading just above -pi to just below +pi": ((-49.0, 50.0, -math.pi + 0.01), (-49.9, 49.97, math.pi - 0.02)),
        "heading exactly +pi, now exactly -pi": ((0.0, 0.0, math.pi), (-1.0, 0.0, -math.pi)),
    }
    for who, delta in both_deltas(lib):
        for name, (prev, now) in cases.items():
            ep, eh = closure_error(prev, now, delta=delta)
            print("%-24s %-45s position %.3g heading %.3g" % (who, name, ep, eh))
            assert ep <= CLOSURE and eh <= CLOSURE, (who, name)
        # backward: rot1 = -+pi, rot2 = +-pi, and the folded magnitudes are 0: the noise is that of a straight drive
        d = delta((1.0, 2.0, 0.0), (0.2, 2.0, 0.0), 0.01)
        assert abs(abs(d[0]) - math.pi) < 1e-15 and abs(abs(d[2]) - math.pi) < 1e-15 and d[0] * d[2] < 0 and abs(d[1] - 0.8) < 1e-15
    for sig in (ref.sigmas, lib.odom_sigmas):
        s_back, s_fwd = sig(d, (0.3, 0.02, 0.1, 0.05)), sig((0.0, d[1], 0.0), (0.3, 0.02, 0.1, 0.05))
        assert np.allclose(s_back, s_fwd, rtol=0, atol=1e-15)


def test_the_delta_closes_over_random_pairs(lib):
    prev, now = random_pairs(4000, 7, min_step=0.01)
    for who, delta in both_deltas(lib):
        worst_p = worst_h = 0.0
        for a, b in zip(prev, now):
            ep, eh = closure_error(a, b, delta=delta)
            worst_p, worst_h = max(worst_p, ep), max(worst_h, eh)
        print("%s: worst closure error over 4000 pairs: position %.3g heading %.3g" % (who, worst_p, worst_h))
        assert worst_p <= CLOSURE and worst_h <= CLOSURE, who


def test_a_turn_in_place_keeps_the_heading_exact_and_costs_a_bounded_position_error(lib):
    """trans < min_trans: rot1 = 0, rot2 = the heading change, and the translation goes along the current heading.  The position is
    then off by trans |u(heading) - u(direction)| = 2 trans sin(phi / 2), phi the angle between the heading and the dropped
    direction: at most min_trans while phi <= 60 degrees (a creep forward), and never more than 2 trans < 2 min_trans (a creep
    backwards, applied forwards)."""
    min_trans = 0.01
    cases = (((3.0, 4.0, 1.0), (3.0, 4.0, -2.5)),                                              # no translation at all
             ((3.0, 4.0, 1.0), (3.0 + 0.009 * math.cos(1.5), 4.0 + 0.009 * math.sin(1.5), 2.0)),   # a creep 0.5 rad off the heading
             ((0.0, 0.0, 0.0), (0.0, -0.0099, 0.3)),                                             # sideways
             ((3.0, 4.0, 3.0), (3.004, 3.993, -3.0)),                                            # nearly backwards, across the seam
             ((1.0, 1.0, 0.0), (1.0 - 0.0099, 1.0, 0.0)))                                        # straight backwards: the worst case
    for who, delta in both_deltas(lib):
        for prev, now in cases:
            d = delta(prev, now, min_trans)
            assert d[0] == 0.0 and ref.angle_diff(d[2], now[2] - prev[2]) <= 1e-15  # rot1 = 0, rot2 = the heading change
            ep, eh = closure_error(prev, now, min_trans, delta=delta)
            phi = float(ref.angle_diff(math.atan2(now[1] - prev[1], now[0] - prev[0]), prev[2])) if d[1] > 0 else 0.0
            print("%s, turn in place: trans %.4g, phi %.3g rad: position off by %.4g, heading by %.3g" % (who, d[1], phi, ep, eh))
            assert eh <= CLOSURE
            assert abs(ep - 2.0 * d[1] * math.sin(phi / 2.0)) <= CLOSURE and ep <= 2.0 * d[1] < 2.0 * min_trans, (who, prev, now, ep)
            if phi <= math.pi / 3:
                assert ep <= min_trans, (who, prev, now, ep)
        # at the threshold and beyond it the translation's direction counts again
        assert delta((0.0, 0.0, 0.0), (0.0, 0.01, 0.0), min_trans)[0] == pytest.approx(math.pi / 2, abs=1e-15)
        # min_trans = 0: no guard
        assert delta((0.0, 0.0, 0.0), (0.0, 1e-9, 0.0), 0.0)[0] == pytest.approx(math.pi / 2, abs=1e-15)


def rel_close(got, want, tol=1e-15):
    return abs(got - want) <= tol * abs(want)


def angle_rel_close(got, want, tol=1e-15):
    """An angle against its reference: the wrapped difference (so +pi and -pi are one value) within tol of the reference's own
    magnitude -- exactly 0 where the reference is 0."""
    return float(ref.angle_diff(got, want)) <= tol * abs(want)


def test_pk_odom_delta_and_sigmas_are_the_reference_formulas(lib):
    prev, now = random_pairs(2000, 11)
    prev[:50, 2] = math.pi - np.linspace(0, 1e-3, 50)  # headings either side of the seam
    now[:50, 2] = -math.pi + np.linspace(0, 1e-3, 50)
    now[50:80, :2] = prev[50:80, :2] + 1e-3  # turns in place
    now[80:100] = prev[80:100]  # a robot that stood still
    alphas = (0.3, 0.02, 0.1, 0.05)
    worst = [0.0, 0.0]
    for a, b in zip(prev, now):
        d, dr = lib.odom_delta(a, b, 0.01), ref.delta(a, b, 0.01)
        assert rel_close(d[1], dr[1]), (a, b, d, dr)
        for k in (0, 2):  # rot1, rot2: 1e-15 relative as well, by the wrapped difference
            assert angle_rel_close(d[k], dr[k]), (a, b, d, dr)
            worst[0] = max(worst[0], float(ref.angle_diff(d[k], dr[k])) / abs(dr[k]) if dr[k] else 0.0)
        s, sr = lib.odom_sigmas(d, alphas), ref.sigmas(d, alphas)
        for k in range(3):
            assert rel_close(s[k], sr[k]), (d, s, sr)
            worst[1] = max(worst[1], abs(s[k] - sr[k]) / sr[k] if sr[k] else 0.0)
    print("worst relative angle error %.3g, worst relative sigma error %.3g" % tuple(worst))
    assert np.array_equal(lib.odom_delta(prev[90], now[90]), np.zeros(3))
    assert np.array_equal(lib.odom_sigmas(np.zeros(3), alphas), np.zeros(3))
    assert np.array_equal(lib.odom_sigmas((0.4, 0.9, -0.2), np.zeros(4)), np.zeros(3))


def test_pk_odom_delta_and_sigmas_refuse_what_the_header_says(lib):
    so = lib.load()
    dp = C.POINTER(C.c_double)
    good3, out = (C.c_double * 3)(0.1, 0.5, -0.2), (C.c_double * 3)(7.0, 7.0, 7.0)
    alpha = (C.c_double * 4)(0.1, 0.1, 0.1, 0.1)
    null = C.cast(None, dp)
    nan, inf, inf_ = float("nan"), float("inf"), float("inf")

    def refused(rc):
        assert rc == lib.PK_ERR_INVALID and list(out) == [7.0, 7.0, 7.0]  # nothing written

    refused(so.pk_odom_delta(null, good3, 0.01, out))
    refused(so.pk_odom_delta(good3, null, 0.01, out))
    assert so.pk_odom_delta(good3, good3, 0.01, null) == lib.PK_ERR_INVALID
    for bad in (nan, inf, -inf_):
        refused(so.pk_odom_delta((C.c_double * 3)(0.0, bad, 0.0), good3, 0.01, out))
        refused(so.pk_odom_delta(good3, (C.c_double * 3)(0.0, 0.0, bad), 0.01, out))
    for bad in (nan, inf, -1e-3):
        refused(so.pk_odom_delta(good3, good3, bad, out))
    refused(so.pk_odom_sigmas(null, alpha, out))
    refused(so.pk_odom_sigmas(good3, null, out))
    assert so.pk_odom_sigmas(good3, alpha, null) == lib.PK_ERR_INVALID
    for k in range(3):
        for bad in (nan, inf):
            d = [0.1, 0.5, -0.2]
            d[k] = bad
            refused(so.pk_odom_sigmas((C.c_double * 3)(*d), alpha, out))
    refused(so.pk_odom_sigmas((C.c_double * 3)(0.1, -0.5, 0.2), alpha, out))  # trans < 0
    for k in range(4):
        for bad in (nan, inf, -1e-9):
            a = [0.1] * 4
            a[k] = bad
            refused(so.pk_odom_sigmas(good3, (C.c_double * 4)(*a), out))
    with pytest.raises(lib.PkError):
        lib.odom_sigmas((0.0, -1.0, 0.0), (0, 0, 0, 0))
    # the filter calls check their handle and arguments before they touch a device
    assert so.pk_motion_odom(None, good3, alpha, null, 0, 0) == lib.PK_ERR_INVALID
    assert so.pk_motion_odom_range(None, good3, alpha, 0, 0, 0, 0) == lib.PK_ERR_INVALID
    assert so.pk_step_odom(None, good3, alpha, null, 0, 0, null, 0, None, 0.5, 0, nan) == lib.PK_ERR_INVALID


def test_k_motion_odom_uses_no_scratch_and_spills_nothing(lib):
    """The library holds the kernel (parakeet_slam_amd.codeobj), and its code-object metadata, read as test_kernel_resources.py reads
    it, says: no scratch, nothing spilled, block_sum's four words of LDS and no more."""
    from parakeet_slam_amd import codeobj
    from test_kernel_resources import READELF, code_object_kernels

    syms = [s for s in codeobj.kernel_hashes() if "k_motion_odom" in s]
    assert len(syms) == 1, syms
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    recs = [k for k in code_object_kernels(codeobj.LIB) if k["symbol"].replace(".kd", "") == syms[0]]
    assert len(recs) == 1, recs
    k = recs[0]
    assert int(k["private_segment_fixed_size"]) == 0 and int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
    assert int(k["group_segment_fixed_size"]) == 32, k

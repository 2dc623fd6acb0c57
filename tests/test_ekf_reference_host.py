"""CPU: the exact reference of the EKF update and the match densities (tests/ekf_reference.py) and its input classes.

(a) the reference module agrees with the float64 restatement of the reference program (oracle.ekf_update_dense, mvn_pdf_2 / 3) and
    with what the unmodified reference program itself returned (the block-diagonal rows of tests/golden/ka_triples), within the
    bounds the GPU test holds the device to;
(b) on every input class the oracle stays within those bounds: this is the condition on the INPUTS -- a class on which the
    reference's own float64 arithmetic breaks a bound tests the class, not the device (ekf_reference.draw_class says which
    conditions that took);
(c) every class reaches the range it is named for.
Run with -s to see the oracle's figures per class."""
import math

import numpy as np
import pytest

import ekf_reference as er
from conftest import load_golden

pytestmark = pytest.mark.skipif(er.mpmath is None, reason="mpmath does not import: no exact reference here")


def oracle_figures(name):
    ekf, match = er.draw_class(name)
    return er.class_figures(name, [er.oracle_update(r) for r in ekf], [er.oracle_match(r) for r in match])


@pytest.mark.parametrize("name", er.CLASSES)
def test_the_oracle_stays_within_the_bounds_on_the_class(name):
    fig = oracle_figures(name)
    print("\n%s: " % name + "  ".join("%s %.3g units (%.2f of its bound, %d points)" % (k, d["worst_units"], d["worst_ratio"], d["points"])
                                       for k, d in sorted(fig.items()) if d["points"]))
    for key in ("mean", "covariance", "log_weight", "closest_point"):
        assert fig[key]["points"] == er.N_POINTS
    assert fig["log_position"]["points"] >= er.N_POINTS // 2 and fig["log_colour"]["points"] >= er.N_POINTS // 2
    for key, d in fig.items():
        assert d["worst_ratio"] <= 1.0, (name, key, d)


@pytest.mark.parametrize("name", er.CLASSES)
def test_the_class_reaches_its_range(name):
    ekf, match = er.draw_class(name)
    assert ekf.shape == (er.N_POINTS, 31) and match.shape == (er.N_POINTS, 23) and er.N_POINTS <= 256
    ex_u, ex_m = er.exact_class(name)
    kappa = np.array([e["kappa"] for e in ex_u])
    q = np.array([e["q"] for e in ex_u])
    kappa2 = np.array([e["kappa2"] for e in ex_m])
    kappa3 = np.array([e["kappa3"] for e in ex_m])
    p_det = ekf[:, er.E_F + 5] * ekf[:, er.E_F + 7] - ekf[:, er.E_F + 6] ** 2
    c_max = np.maximum(np.maximum(ekf[:, er.E_F + 8], ekf[:, er.E_F + 11]), ekf[:, er.E_F + 13])
    assert np.all(p_det > 0) and np.all(kappa >= 1.0) and np.all(np.isfinite(kappa))
    rng = {"close_range": (1e-6, 1e-1), "far": (50.0, 1e4), "q_zero": (0.0, 0.0)}.get(name, (1.0, 50.0))
    dist = np.sqrt(q)
    if name == "q_zero":
        assert np.all(q == 0.0)
        assert np.all(ekf[:, er.E_F] == ekf[:, er.E_SX]) and np.all(ekf[:, er.E_F + 1] == ekf[:, er.E_SY])
    else:
        assert rng[0] * 0.999 <= dist.min() <= rng[0] * 3 and rng[1] / 3 <= dist.max() <= rng[1] * 1.001, (dist.min(), dist.max())
    if name == "typical":
        assert p_det.min() < 1e-3 and p_det.max() > 10.0 and 1e-4 <= p_det.min() and p_det.max() <= 1e2
    if name == "converged":
        assert ekf[:, er.E_F + 5:er.E_F + 8:2].min() < 1e-14 and c_max.min() < 1e-5
    if name == "fresh":
        assert ekf[:, er.E_F + 5:er.E_F + 8:2].max() > 1e11 and c_max.max() > 1e5
    if name == "general_qt":
        off = np.abs(ekf[:, [er.E_QT + 2, er.E_QT + 3, er.E_QT + 5]])
        assert np.all(off.max(axis=1) > 0) and np.median(off.max(axis=1)) > 1e-3  # the long form of colour_block_update
        for r in ekf:
            assert np.linalg.eigvalsh(er.dense_qt(r[er.E_QT:er.E_QT + 7])[1:, 1:]).min() > 0
    else:
        assert np.all(ekf[:, [er.E_QT + 2, er.E_QT + 3, er.E_QT + 5]] == 0.0)  # the short form
    if name == "kappa_1e3":
        assert kappa.min() < 20 and 500 < kappa.max() <= 1e3
    elif name == "kappa_1e5":
        assert kappa.min() < 20 and 5e4 < kappa.max() <= 1e5 and (kappa > 2.7e3).sum() > er.N_POINTS // 5
    else:
        assert kappa.max() < 32  # (the kappa^2 / 8 of the bound stays below 128 units: the other classes test the algebra)
    if name not in ("close_range", "fresh"):
        assert kappa2.max() > 50
    assert kappa2.max() <= 100.0 * 1.001 and (kappa3.max() > 20 or name == "fresh")
    # the match rows: every gate 1e-6 clear, no row behind the ray, half of them with a position density that is a number
    for e in ex_m:
        assert abs(abs(e["delb"]) - 0.5) > 1e-6 and abs(e["cd"] - 300.0) > 1e-6 and abs(e["side"] - math.pi / 2) > 1e-6
        assert not e["behind"] and not e["gate_side"] and not e["gate_bearing"]
    assert sum(e["log_match"] is not None for e in ex_m) >= (er.N_POINTS // 4 if name in ("fresh", "kappa_1e5") else er.N_POINTS // 2)


def test_the_exact_update_is_symmetric_and_reproduces_a_hand_computed_case():
    """Sigma' = (I - K H) Sigma is symmetric in exact arithmetic; and SURVEY.md's known answer to the digits quoted there."""
    for name in ("typical", "general_qt", "q_zero"):
        for e in er.exact_class(name)[0][:32]:
            assert e["asymmetry"] <= 1e-60 * max(e["field_scales"][5:])
    row = np.zeros(31)
    row[er.E_SX:er.E_SY + 1] = (0.5, -0.25)
    row[er.E_F:er.E_F + 14] = [3, 4, 100, 150, 200, 0.25, 0, 0.25, 0.25, 0, 0, 0.25, 0, 0.25]
    row[er.E_BLOB:er.E_BLOB + 4] = (0.9, 101, 149, 202)
    row[er.E_QT:er.E_QT + 7] = [0.1, 0.1, 0, 0, 0.1, 0, 0.1]
    row[er.E_ZHAT0] = math.atan2(4.25, 2.5)
    e = er.exact_update(row)
    assert abs(float(er.mp.exp(e["logw"])) - 8.819701295333626e-05) < 1e-18
    assert np.allclose([float(v) for v in e["fields"][:5]], [2.944889780603, 3.967582223884, 100.714285714286, 149.285714285714,
                                                              201.428571428571], rtol=1e-12)
    assert np.allclose([float(e["fields"][i]) for i in (8, 11, 13)], 0.25 * 0.1 / 0.35, rtol=1e-15)
    assert e["kappa"] == 1.0 and abs(e["q"] - (2.5 ** 2 + 4.25 ** 2)) < 1e-12
    m = np.zeros(23)
    m[er.M_SX:er.M_H + 1] = (0.5, -0.25, 0.3)
    m[er.M_F:er.M_F + 14] = row[er.E_F:er.E_F + 14]
    m[er.M_BLOB:er.M_BLOB + 4] = row[er.E_BLOB:er.E_BLOB + 4]
    m[er.M_UX], m[er.M_UY] = math.cos(0.9), math.sin(0.9)
    x = er.exact_match(m)
    assert abs(float(er.mp.exp(x["log_match"])) - 7.804697433262233e-07) < 1e-19
    assert abs(float(er.mp.exp(x["log_position"])) - 0.2500746500315802) < 1e-13
    assert abs(float(er.mp.exp(x["log_colour"])) - 3.120947058119098e-06) < 1e-18


def test_the_reference_agrees_with_the_reference_programs_own_answers():
    """tests/golden/ka_triples: what the unmodified reference program returned (LAPACK's inverse, scipy's densities), on its
    block-diagonal rows (the compact layout holds no others), within the same bounds."""
    g = load_golden("ka_triples")
    worst = dict(mean=0.0, covariance=0.0, log_weight=0.0, closest_point=0.0, log_position=0.0, log_colour=0.0, log_match=0.0)
    rows = gates = 0
    for i in range(len(g["pom"])):
        cov, mean, pose, blob = g["cov"][i], g["mean"][i], g["pose"][i], g["blob"][i]
        if np.any(cov[:2, 2:] != 0) or np.any(cov[2:, :2] != 0):
            continue
        rows += 1
        fields = np.concatenate([mean, [cov[a, b] for a, b in er.COV_AT]])
        row = np.zeros(31)
        row[er.E_SX:er.E_SY + 1] = pose[:2]
        row[er.E_F:er.E_F + 14] = fields
        row[er.E_BLOB:er.E_BLOB + 4] = blob
        row[er.E_QT:er.E_QT + 7] = [g["Qt"][0, 0], g["Qt"][1, 1], g["Qt"][1, 2], g["Qt"][1, 3], g["Qt"][2, 2], g["Qt"][2, 3], g["Qt"][3, 3]]
        row[er.E_ZHAT0] = g["zhat"][i][0]
        e = er.exact_update(row)
        got = np.concatenate([g["new_mean"][i], [g["new_cov"][i][a, b] for a, b in er.COV_AT]])
        um, uc, _ = er.update_units(got, 0.0, e)
        floor = math.log(er.DENSITY_FLOOR)
        uw = er.log_density_units(g["weight"][i], e["logw"], e["logw_scale"]) if e["logw"] >= floor else 0.0  # (a weight, not its logarithm)
        b = er.update_bound(e["kappa"])
        for key, u in (("mean", um), ("covariance", uc), ("log_weight", uw)):
            worst[key] = max(worst[key], u / b)
        m = np.zeros(23)
        m[er.M_SX:er.M_H + 1] = pose
        m[er.M_F:er.M_F + 14] = fields
        m[er.M_BLOB:er.M_BLOB + 4] = blob
        m[er.M_UX], m[er.M_UY] = math.cos(blob[0]), math.sin(blob[0])  # (unit() of it divides by a length of 1 +- 1 ulp)
        x = er.exact_match(m)
        b2, b3 = er.position_bound(x["kappa2"]), er.colour_bound(x["kappa3"], x["kappa2"])
        # the golden closest point was formed with the program's own unit vector: 4 more units for its two roundings
        un = max(er.units(g["closest"][i][k], x["near"][k], x["near_scale"][k]) for k in range(2))
        worst["closest_point"] = max(worst["closest_point"], un / (b2 + 4.0))
        if x["gate_side"]:
            assert g["ppm"][i] == 0.0
        elif x["log_position"] >= floor and not x["behind"]:
            worst["log_position"] = max(worst["log_position"], er.log_density_units(g["ppm"][i], x["log_position"], x["position_scale"]) / b2)
        if x["log_colour"] >= floor and x["maha3"] <= 100.0:
            worst["log_colour"] = max(worst["log_colour"], er.log_density_units(g["pcm"][i], x["log_colour"], x["colour_scale"]) / b3)
        elif x["log_colour"] >= floor:
            # scipy takes the Mahalanobis term through an eigendecomposition, whose error is in units of |d|^2 |C^-1|, not of the
            # term: ten standard deviations out (one row, 108 units against a bound of 47) it is held to the 1e-11 the suite holds
            # the oracle to on these rows (tests/test_oracle_vs_golden.py)
            assert abs(g["pcm"][i] - float(er.mp.exp(x["log_colour"]))) <= 1e-11 * g["pcm"][i]
        if x["log_match"] is None:
            gates += 1
            assert g["pom"][i] == 0.0
        elif x["log_match"] >= floor and not x["behind"]:
            worst["log_match"] = max(worst["log_match"], er.log_density_units(g["pom"][i], x["log_match"], x["match_scale"]) / b3)
    print("\nka_triples, %d block-diagonal rows (%d with a closed gate): worst ratio to the bound " % (rows, gates)
          + "  ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    assert rows >= 60 and gates >= 5
    for key, ratio in worst.items():
        assert ratio <= 1.0, (key, ratio)

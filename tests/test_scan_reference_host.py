"""CPU: the exact scan (tests/scan_reference.py), its scenes, and the float64 oracle against it.

(a) on every scene the GPU test uses, the float64 oracle (OracleFilter.observe on the scene's ids) stays within 0.6 of the bounds
    the device is held to, fields and log-weight -- this is where C_CHAIN comes from, and the condition on the SCENES: one on which
    the reference's own float64 arithmetic breaks a bound tests the scene, not the device;
(b) exact_scan reproduces a two-update chain computed by hand, and the unmodified reference program's own answers on the step
    fixtures under tests/golden (chained updates, an unmatched blob, an immutable landmark, potential ones), within the bounds;
(c) every scene meets its conditions: safe ids, the stated sightings inside every landmark's gates, a finite exact log-weight
    on the overflow and underflow scenes.
Run with -s to see the oracle's figures."""
import math
from fractions import Fraction

import numpy as np
import pytest

import ekf_reference as er
import scan_reference as sr
from conftest import load_golden
from test_gpu_assoc import max_passers

pytestmark = pytest.mark.skipif(er.mpmath is None, reason="mpmath does not import: no exact reference here")


def host_exact(s):
    """the scene's exact scan with numpy's atan2 for the expected bearings, and the oracle's answer -> (ex, oracle tuple)"""
    o = sr.oracle_scan(s)
    with np.errstate(invalid="ignore"):
        zhat0 = np.arctan2(o[4][..., 0], o[4][..., 1])
    return sr.exact_scene(s, zhat0), o


SCENES = [(name, L, 0) for name in sr.CLASSES for L in sr.SIZES] + [("chains", 513, 6), ("chains", 3000, 7), ("chains", 40, 10), ("chains", 1030, 11)]


def oracle_figures(name, L, longest, c=None):
    """the oracle's figures on a scene, against the bounds with the constant of the scene's class (or with c)"""
    s = sr.scene(name, L, longest)
    ex, o = host_exact(s)
    return s, ex, sr.scan_figures(ex, *o[:4], c=sr.chain_constant(name) if c is None else c)


@pytest.mark.parametrize("name,L,longest", SCENES)
def test_the_oracle_stays_within_the_bounds_on_the_scene(name, L, longest):
    s, ex, fig = oracle_figures(name, L, longest)
    print("\n%s L=%d: oracle fields %.3g units, %.3f of the bound; W %.3g units, %.3f of the bound (%d blobs, longest chain %d)" % (
        name, L, fig["field_units"], fig["field_ratio"], fig["w_units"], fig["w_ratio"], len(s["blobs"]), s["most"]))
    assert fig["counts_equal"]
    assert fig["field_ratio"] <= 0.6 and fig["w_ratio"] <= 0.6, fig  # the margin the class's constant was chosen for
    # the scene's conditions
    assert len(s["blobs"]) <= 48 and sum(sum(st["n"] for st in e["landmarks"].values()) for e in ex) <= 200
    assert s["most"] == max_passers(s["means"], s["blobs"], s["pose"])  # (test_gpu_assoc's count of the blobs inside the gates)
    assert s["most"] == (longest or (4 if s["pair"] is not None else s["most"])) and s["most"] <= max(4, longest)
    if s["pair"] is not None:
        a, b = s["pair"]
        assert a % 2 == 0 and b == a + 1 and all(e["landmarks"][a]["n"] == 4 and e["landmarks"][b]["n"] == 4 for e in ex)
        assert sorted(st["n"] for st in ex[0]["landmarks"].values())[-5:-2] == [2, 3, 4] or longest
    if name in sr.SINGLES or name == "map_scale_huge":
        assert all(st["n"] == 1 for e in ex for st in e["landmarks"].values())
    for e in ex:
        assert math.isfinite(float(e["W"]))
    if name in ("norm_overflow", "norm_underflow"):
        per_update = [float(e["W"] - e["n_unmatched"] * er.mp.log(er.mpf(0.1))) / sum(st["n"] for st in e["landmarks"].values()) for e in ex]
        assert all(-25.0 < w < -23.0 for w in per_update) if name == "norm_overflow" else all(20.5 < w < 22.0 for w in per_update), per_update
        pr = [sr.O.probability_of_match(s["pose"][0, 0], s["pose"][0, 1], s["pose"][0, 2], z, s["means"], s["covs"]).max() for z in s["blobs"][s["ids"][0] > 0]]
        assert all(p > 0.0 and math.isfinite(p) for p in pr)
    if name == "flags":  # potential landmarks promoted in mid-chain, immutable ones left alone
        k0, k1 = s["counts"], np.array([[e["landmarks"][l]["count"] if l in e["landmarks"] else s["counts"][l] for l in range(L)] for e in ex])
        pot0, pot1 = (k0 & sr.POTENTIAL) != 0, (k1 & sr.POTENTIAL) != 0
        assert (pot0 & ~pot1[0]).sum() >= 3 and (pot0 & pot1[0]).sum() >= 2 and s["immutable"].sum() == 3
        assert np.array_equal(k1[:, s["immutable"]], np.broadcast_to(k0[s["immutable"]], (k1.shape[0], 3)))


def test_c_chain_is_the_smallest_that_leaves_the_margin():
    """C_CHAIN is the smallest of 1, 2, 4, 8 that keeps the oracle at or below 0.6 of the bounds on every scene of the classes the
    routes are to be held on, and the figures in scan_reference.py are the ones measured here (the scenes and their exact scans are
    cached: computed once a process).  C_EXTRA, the constant of scan_reference.EXTRA_CLASSES alone, is chosen and asserted the same way on those classes' scenes."""
    assert set(sr.EXTRA_CLASSES) < set(sr.CLASSES) and sr.chain_constant("typical") == sr.C_CHAIN and sr.chain_constant(sr.EXTRA_CLASSES[0]) == sr.C_EXTRA
    for what, const, scenes, want in (("C_CHAIN", sr.C_CHAIN, [c for c in SCENES if c[0] not in sr.EXTRA_CLASSES], (sr.ORACLE_WORST_FIELD_RATIO, sr.ORACLE_WORST_W_RATIO)),
                                      ("C_EXTRA", sr.C_EXTRA, [c for c in SCENES if c[0] in sr.EXTRA_CLASSES], (sr.ORACLE_WORST_EXTRA_FIELD_RATIO, sr.ORACLE_WORST_EXTRA_W_RATIO))):
        assert len(scenes) >= len(sr.SIZES)
        figs = [oracle_figures(*c, c=const)[2] for c in scenes]
        field, w = max(f["field_ratio"] for f in figs), max(f["w_ratio"] for f in figs)
        print("\noracle, worst over %d scenes: fields %.3f of the bound, W %.3f of the bound, %s = %g" % (len(figs), field, w, what, const))
        assert const in (1.0, 2.0, 4.0, 8.0) and max(field, w) <= 0.6
        if const > 1.0:  # (the bound of W is (T - 1) + the field bound: halving the constant does not quite double its ratio)
            half = [oracle_figures(*c, c=const / 2.0)[2] for c in scenes]
            assert max(max(f["field_ratio"] for f in half), max(f["w_ratio"] for f in half)) > 0.6, "half the constant would do"
        assert abs(field - want[0]) <= 0.02 and abs(w - want[1]) <= 0.02, "the figures in scan_reference.py are stale"


DENSE = [(name, L) for name in sr.DENSE_CLASSES for L in sr.DENSE_SIZES]


def dense_figures(name, L):
    s = sr.dense_scene(name, L)
    o = sr.oracle_scan(s)
    with np.errstate(invalid="ignore"):
        ex = sr.exact_dense(s, np.arctan2(o[4][..., 0], o[4][..., 1]))
    return s, ex, sr.scan_figures(ex, *o[:4], dense=True)


@pytest.mark.parametrize("name,L", DENSE)
def test_the_oracle_stays_within_the_dense_bounds_on_the_scene(name, L):
    s, ex, fig = dense_figures(name, L)
    kq = [st["kappa_q"] for e in ex for st in e["landmarks"].values()]
    print("\ndense %s L=%d: oracle fields %.3g units, %.3f of the bound; W %.3g units, %.3f of the bound; cond(Q) %.3g .. %.3g (%d blobs)" % (
        name, L, fig["field_units"], fig["field_ratio"], fig["w_units"], fig["w_ratio"], min(kq), max(kq), len(s["blobs"])))
    assert fig["counts_equal"] and fig["field_ratio"] <= 0.6 and fig["w_ratio"] <= 0.6, fig
    assert np.abs(s["covs"][:, :2, 2:]).max() > 1e-3 and abs(s["Qt"][0, 1:]).max() > 0  # coupled: the dense layout
    assert len(s["blobs"]) <= 48 and s["most"] <= 4 and all(math.isfinite(float(e["W"])) for e in ex)
    if name == "chains":
        assert sorted(st["n"] for st in ex[0]["landmarks"].values())[-5:] == [2, 3, 4, 4, 4]
    if name == "flags":
        assert any(st["count"] & sr.POTENTIAL for st in ex[0]["landmarks"].values()) and s["immutable"].sum() == 2
        assert sum(1 for l, st in ex[0]["landmarks"].items() if s["counts"][l] & sr.POTENTIAL and not st["count"] & sr.POTENTIAL) >= 2
    if name == "cond_q":  # log-uniform up to 1e5
        assert min(kq) < 1e3 and 1e4 < max(kq) < 3e5 and sum(k > 1e3 for k in kq) >= len(kq) // 4
    else:
        assert max(kq) < 100


def test_c_dense_is_the_smallest_that_leaves_the_margin():
    figs = [dense_figures(*c)[2] for c in DENSE]
    field, w = max(f["field_ratio"] for f in figs), max(f["w_ratio"] for f in figs)
    print("\ndense oracle, worst over %d scenes: fields %.3f of the bound, W %.3f, C_DENSE = %g" % (len(figs), field, w, sr.C_DENSE))
    assert sr.C_DENSE == 1.0 and max(field, w) <= 0.6  # (1 is the smallest of 1, 2, 4, 8)
    assert abs(field - sr.ORACLE_WORST_DENSE_FIELD_RATIO) <= 0.02 and abs(w - sr.ORACLE_WORST_DENSE_W_RATIO) <= 0.02, "the figures in scan_reference.py are stale"


def test_a_two_update_chain_computed_by_hand():
    """SURVEY.md's landmark (P = C = 0.25 I, Qt = 0.1 I) sighted twice.  The colour channels are scalar filters: the gain is 5/7 and
    then (1/14) / (1/14 + 1/10) = 5/12, the variance 1/14 and then 1/24; in rationals, red: 100 + 5/7 = 705/7, then
    705/7 + 5/12 (102 - 705/7) = 2835/28 = 101.25; green 4165/28 = 148.75; blue 5635/28 = 201.25."""
    pose = np.array([[0.5, -0.25, 0.0]])
    means = np.array([[3.0, 4.0, 100.0, 150.0, 200.0]])
    covs = 0.25 * np.identity(5)[None]
    blobs = np.array([[0.9, 101.0, 149.0, 202.0], [5.0, 0.0, 0.0, 0.0], [1.0, 102.0, 148.0, 201.0]])
    ids = np.array([[1, 0, 1]])
    ex = sr.exact_scan(pose, means, covs, np.zeros(1, dtype=np.int64), None, 0.1 * np.identity(4), blobs, ids, None, np.array([-3.5]))[0]
    st = ex["landmarks"][0]
    assert st["n"] == 2 and st["count"] == 4 and ex["n_unmatched"] == 1 and ex["T"] == 4
    for i, want in ((2, Fraction(2835, 28)), (3, Fraction(4165, 28)), (4, Fraction(5635, 28))):
        assert abs(float(st["mean"][i]) - float(want)) <= 1e-13
        assert abs(float(st["cov"][i][i]) - 1.0 / 24.0) <= 1e-16  # (0.25 and 0.1 are doubles, not the rationals: 1e-17 apart)
    # the log-weight: the carried one, log 0.1, and the two updates as ekf_reference.exact_update gives them one by one
    row = np.zeros(31)
    row[er.E_SX:er.E_SY + 1] = pose[0, :2]
    row[er.E_F:er.E_F + 14] = [3, 4, 100, 150, 200, 0.25, 0, 0.25, 0.25, 0, 0, 0.25, 0, 0.25]
    row[er.E_BLOB:er.E_BLOB + 4] = blobs[0]
    row[er.E_QT:er.E_QT + 7] = [0.1, 0.1, 0, 0, 0.1, 0, 0.1]
    row[er.E_ZHAT0] = math.atan2(4.25, 2.5)
    one = er.exact_update(row)
    assert abs(float(er.mp.exp(one["logw"])) - 8.819701295333626e-05) < 1e-18  # (SURVEY.md's known answer)
    row[er.E_F:er.E_F + 14] = [float(v) for v in one["fields"]]
    row[er.E_BLOB:er.E_BLOB + 4] = blobs[2]
    row[er.E_ZHAT0] = math.atan2(row[er.E_F + 1] + 0.25, row[er.E_F] - 0.5)
    two = er.exact_update(row)
    want = -3.5 + math.log(0.1) + float(one["logw"]) + float(two["logw"])
    assert abs(float(ex["W"]) - want) <= 1e-12 * abs(want)
    assert abs(ex["S"] - (3.5 + math.log(10.0) + one["logw_scale"] + two["logw_scale"])) <= 1e-9
    assert np.allclose([float(v) for v in st["mean"][:2]], [float(v) for v in two["fields"][:2]], rtol=1e-13)


def _golden_step(means, covs, counts, immutable, Qt, pose, blobs, ids, got_mean, got_cov, got_count, weights, ancestors):
    """one cam_cb of the reference program against exact_scan: worst ratio to the bound of the fields and of the weight"""
    s = dict(means=means, covs=covs, counts=counts, immutable=immutable, Qt=Qt, pose=pose, blobs=blobs, ids=ids, carried=None, fresh=True)
    o = sr.oracle_scan(s)
    with np.errstate(invalid="ignore"):
        zhat0 = np.arctan2(o[4][..., 0], o[4][..., 1])
    ex = sr.exact_scan(pose, means, covs, counts, immutable, Qt, blobs, ids, zhat0, None)
    worst_f = worst_w = 0.0
    for j, a in enumerate(ancestors):  # the fixture holds the maps behind the resample: particle j is a copy of particle a
        e = ex[a]
        for l, st in e["landmarks"].items():
            worst_f = max(worst_f, sr.compact_units(got_mean[j, l], got_cov[j, l], st) / sr.chain_bound(st["n"], st["kappa"]))
            assert int(got_count[j, l]) == st["count"] & ~sr.POTENTIAL
    for p, e in enumerate(ex):
        worst_w = max(worst_w, er.log_density_units(weights[p], e["W"], e["S"]) / sr.w_bound(e))  # (a weight, not its logarithm)
    return worst_f, worst_w, ex


def test_the_exact_scan_agrees_with_the_reference_programs_own_answers():
    """tests/golden/step_small (the unmodified reference program: a doubly matched landmark, an unmatched blob, an immutable
    landmark), its first two steps -- the second from per-particle maps -- and the first step of step_potential (potential
    features weigh 0.1 and are updated), within the bounds of a chain."""
    g = load_golden("step_small")
    imm = g["immutable"].astype(bool)
    f0, w0, ex = _golden_step(g["means0"], g["covs0"], np.zeros(int(g["L"]), dtype=np.int64), imm, g["Qt"], g["post_motion"][0], g["blobs"][0], g["ids"][0],
                              g["mean"][0], g["cov"][0], g["count"][0], g["weights"][0], g["ancestors"][0])
    assert max(st["n"] for st in ex[0]["landmarks"].values()) == 2 and ex[0]["n_unmatched"] >= 1
    f1, w1, _ = _golden_step(g["mean"][0], g["cov"][0], g["count"][0], imm, g["Qt"], g["post_motion"][1], g["blobs"][1], g["ids"][1],
                             g["mean"][1], g["cov"][1], g["count"][1], g["weights"][1], g["ancestors"][1])
    from test_oracle_vs_golden import potential_filter

    gp = load_golden("step_potential")
    f = potential_filter(gp)
    counts = f.count | np.where(f.potential, sr.POTENTIAL, 0)
    fp, wp, exp_ = _golden_step(f.mean, f.cov, counts, f.immutable, gp["Qt"], gp["post_motion"][0], gp["blobs"][0], np.abs(gp["ids"][0]),
                                gp["mean"][0], gp["cov"][0], gp["count"][0], gp["weights"][0], gp["ancestors"][0])
    assert any(st["count"] & sr.POTENTIAL or f.potential[0, l] for l, st in exp_[0]["landmarks"].items())
    print("\nstep_small: fields %.2f / %.2f of the bound, weights %.2f / %.2f; step_potential: %.2f, %.2f" % (f0, f1, w0, w1, fp, wp))
    assert max(f0, f1, fp, w0, w1, wp) <= 1.0

"""GPU: what every observe route makes of a WHOLE SCAN -- updates chained on a landmark in scan order, the particle's log-weight
summed over lanes, waves and landmarks, the log 0.1 of every unmatched blob, the carried weight -- against the exact scan of
tests/scan_reference.py (mpmath, 300 bits), per scene class and map size, every route of that size on the same scene:

  counts                                  equal
  a field behind a chain of n updates     units <= C_CHAIN n (32 + kappa_max^2 / 8)   (C_CHAIN = 1; the three classes added
                                          beside the ones asked for, scan_reference.EXTRA_CLASSES, have their own C_EXTRA = 4)
  the log-weight W, T terms              units <= (T - 1) + the largest field bound of the particle's chains
  two routes' log-weights                 within twice that bound of each other
  a landmark no blob is assigned to       the bits that were uploaded

(units, scales, the scenes and where C_CHAIN comes from: scan_reference.py; tests/test_scan_reference_host.py holds the float64
oracle to the same bounds on the same scenes without a GPU.)  The route tests compare the kernels with each other and with the
float64 oracle at rtol 1e-9 and Qt = 0.1 I; here Qt runs from 1e-13 to 1e20 and the covariances from 1e-20 to 2 500
(chains of updates on one landmark from Qt = 1e-4 and up to covariances of 250: scan_reference.scene says why).
norm_overflow is the scene on which the product of the squared Frobenius norms of a lane's updates, looked at once per landmark
pair as a double, went to infinity (eight factors of 3e40): k_step_pub<256>, k_step_pub and k_step_pub_big gave a log-weight of
-inf where the kernels that take a logarithm per update give -24 an update.  norm_underflow (+21 an update) never reaches those
kernels' arithmetic: they hand particles with determinants below 1e-20 to the fall-back kernels (asserted below).  So NO whole
scan here takes a publishing kernel's product towards the subnormals; that direction of the fix is held by the probe of ekf_update
alone (tests/test_gpu_ekf_reference.py::test_the_product_of_norms_never_leaves_the_normal_numbers).  A scan that did would need
Qt and covariances just inside pub_keys' limit, fro2 about 1e-12, and more than 25 updates in one lane of k_step_pub_big for
the product to reach 1e-308: with four slots a landmark and two landmarks a pair a lane holds eight, sixteen with two pairs
(and two sighted pairs do not share a lane at 48 blobs: scan_reference.scene, norm_overflow), so it cannot be built.

Per case the route actually taken is asserted (observe_route, observe_published, the instance of observe_pub_stats, nobody flagged):
a particle handed to the fall-back kernels would test those instead.

With PK_FIGURES_JSON=profiles/r11/scan_errors.json the measured figures, the float64 oracle's beside them, are written there."""
import numpy as np
import pytest

import ekf_reference as er
import scan_reference as sr
from figures_record import record

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(er.mpmath is None, reason="mpmath does not import: no exact reference here")]

WHAT = ("worst errors of a whole scan (chained updates, log-weight) of every observe route against the exact scan of "
        "tests/scan_reference.py, per scene class, map size and route, in units of 2^-53 x the scale and as a ratio to the asserted "
        "bound; the float64 oracle's figures on the same scene beside them; written by the tests: PK_FIGURES_JSON=<this file> "
        "pytest -m gpu tests/test_gpu_scan_reference.py")
LOG = 1  # PK_WEIGHTS_LOG


def device_zhat0(lib, args):
    """the device's atan2 of the (dy, dx) every update meets (NaN where a blob is unmatched)"""
    flat = args.reshape(-1, 2)
    use = ~np.isnan(flat[:, 0])
    out = np.full(flat.shape[0], np.nan)
    if use.any():
        out[use] = np.asarray(lib.probe_math(lib.PK_MATH_ATAN2, np.ascontiguousarray(flat[use]))).reshape(-1)
    return out.reshape(args.shape[:2])


def run_route(lib, s, opts, maps=None):
    """one filter, one observe of the scene -> dict(logw, means, covs, counts, route, published, instance, flagged, table, lean)"""
    P, L = s["pose"].shape[0], s["L"]
    f = lib.DeviceFilter(P, L)
    try:
        for k, v in opts.items():
            f.set_option(k, v)
        f.set_measurement_noise(s["Qt"])
        f.upload_map(s["means"], s["covs"].reshape(L, 25), s["immutable"])
        f.upload_poses(s["pose"])
        if s["counts"].any():
            f.upload_landmarks(0, P, counts=np.broadcast_to(s["counts"], (P, L)))
        if s["carried"] is not None:
            f.upload_log_weights(s["carried"])
        f.observe(s["blobs"], fresh=s["fresh"])
        m, c, k = f.download_landmarks()
        return dict(logw=f.download_log_weights(), means=m, covs=c, counts=k, route=f.observe_route(), published=int(f.observe_published()),
                    instance=f.observe_pub_stats()["instance"], flagged=f.observe_flagged(), table=f.colour_table_stats()["engaged"],
                    lean=f.observe_lean_stats())
    finally:
        f.close()


def check_scene(lib, s, routes):
    """every route of `routes` on the scene s against the exact scan and against each other"""
    o_logw, o_means, o_covs, o_counts, args = sr.oracle_scan(s)
    ex = sr.exact_scene(s, device_zhat0(lib, args))
    c = sr.chain_constant(s["name"])  # C_CHAIN, but for scan_reference.EXTRA_CLASSES
    ora = sr.scan_figures(ex, o_logw, o_means, o_covs, o_counts, c=c)
    touched = np.zeros((s["pose"].shape[0], s["L"]), dtype=bool)
    for p, e in enumerate(ex):
        touched[p, list(e["landmarks"])] = True
    got, bad = {}, []
    for name, (opts, route, published) in routes.items():
        g = got[name] = run_route(lib, s, opts)
        # nobody flagged -- but norm_underflow on the publishing kernels: pub_keys (pk_pub_math.hpp) takes no landmark whose det P or
        # det C is below 1e-20 and hands every particle to the fall-back kernels, as measured on the parent commit too.  (Inside
        # those limits fro2 is at least 1.4e-13, so the product of a lane's factors cannot reach the subnormals there; the
        # direction is held at ekf_update itself: tests/test_gpu_ekf_reference.py::test_the_product_of_norms_never_leaves_the_normal_numbers.)
        flagged = (s["pose"].shape[0], 0) if s["name"] == "norm_underflow" and name in sr.PUBLISHING else (0, 0)
        assert (g["route"], g["published"], g["flagged"]) == (route, published, flagged), (s["name"], s["L"], name, g["route"], g["published"], g["flagged"])
        assert (g["instance"] == 1) == bool(published), (name, g["instance"])
        fig = sr.scan_figures(ex, g["logw"], g["means"], g["covs"], g["counts"], c=c)
        print("%s L=%d %-12s fields %.4g units, %.3f of the bound; W %.4g units, %.3f of the bound (oracle %.3f, %.3f); table %d lean %s" % (
            s["name"], s["L"], name, fig["field_units"], fig["field_ratio"], fig["w_units"], fig["w_ratio"], ora["field_ratio"], ora["w_ratio"],
            g["table"], g["lean"]["marked"]))
        record("scan", "%s.L%d.%s" % (s["name"], s["L"], name), _what=WHAT, device_field_units=fig["field_units"], device_field_ratio_to_bound=fig["field_ratio"],
               device_w_units=fig["w_units"], device_w_ratio_to_bound=fig["w_ratio"], oracle_field_ratio_to_bound=ora["field_ratio"],
               oracle_w_ratio_to_bound=ora["w_ratio"], colour_table_engaged=int(g["table"]), lean_groups=int(g["lean"]["marked"]))
        # a landmark no blob is assigned to keeps its bits; the compact routes keep the blocks apart
        same = ~touched
        assert np.array_equal(g["means"][same], np.broadcast_to(s["means"], g["means"].shape)[same]), name
        assert np.array_equal(g["covs"][same], np.broadcast_to(s["covs"], g["covs"].shape)[same]), name
        assert np.array_equal(g["counts"][same], np.broadcast_to(s["counts"], g["counts"].shape)[same]), name
        assert not g["covs"][:, :, :2, 2:].any() and not g["covs"][:, :, 2:, :2].any(), name
        if not (fig["counts_equal"] and fig["field_ratio"] <= 1.0 and fig["w_ratio"] <= 1.0):
            bad.append((name, fig))
    assert not bad, (s["name"], s["L"], bad)
    names = list(got)
    for p, e in enumerate(ex):  # the routes against each other: particles of one filter are weighed by whichever kernel took them
        for a in names:
            for b in names[names.index(a) + 1:]:
                u = abs(float(got[a]["logw"][p]) - float(got[b]["logw"][p])) / (er.UNIT * e["S"])
                assert u <= 2.0 * sr.w_bound(e, c), (s["name"], s["L"], a, b, p, u, sr.w_bound(e, c))
    return got


@pytest.mark.parametrize("L", sr.SIZES)
@pytest.mark.parametrize("name", sr.CLASSES)
def test_every_route_against_the_exact_scan(lib, name, L):
    got = check_scene(lib, sr.scene(name, L), sr.ROUTES[L])
    if name == "typical" and L == 1030:  # the table mode and the lean groups were in play, and were not where they are switched off
        assert got["pub"]["table"] == 1 and got["pub_no_table"]["table"] == 0
        assert got["pub"]["lean"]["marked"] > 0  # ("pub_lean" = 0 still counts the groups the scan marked; it takes the usual body for them)
    if name == "norm_overflow" and L in (513, 1030):  # the overflow scene met the table mode and the plain one ...
        assert got["pub"]["table"] == 1 and got["pub_no_table"]["table"] == 0
    if name == "norm_overflow" and L == 1030:  # ... and both bodies of the two-pair instance: lean groups and usual ones
        lean = got["pub"]["lean"]
        assert 0 < lean["marked"] < lean["in_use"], lean


@pytest.mark.parametrize("L", sr.DENSE_SIZES)
@pytest.mark.parametrize("name", sr.DENSE_CLASSES)
def test_the_dense_route_against_the_exact_scan(lib, name, L):
    """k_observe_dense (coupled 5x5 covariances, a coupled Qt: the 30-row layout): its inverse of Q by cofactors and its unsymmetrised
    Sigma', all 30 stored fields against the exact scan -- the exact Sigma' is symmetric, so the stored one's asymmetry is held to
    the units of its entries -- in kappa_q = cond_2 of the whole Q, up to 1e5 in cond_q."""
    s = sr.dense_scene(name, L)
    o_logw, o_means, o_covs, o_counts, args = sr.oracle_scan(s)
    ex = sr.exact_dense(s, device_zhat0(lib, args))
    ora = sr.scan_figures(ex, o_logw, o_means, o_covs, o_counts, dense=True)
    g = run_route(lib, s, {})
    assert (g["route"], g["published"], g["flagged"]) == ("dense", 0, (0, 0)), (g["route"], g["published"], g["flagged"])
    fig = sr.scan_figures(ex, g["logw"], g["means"], g["covs"], g["counts"], dense=True)
    asym = max(abs(float(g["covs"][p, l, i, j]) - float(g["covs"][p, l, j, i])) / (er.UNIT * st["cov_scale"][i][j])
               for p, e in enumerate(ex) for l, st in e["landmarks"].items() for i in range(5) for j in range(i))
    print("dense %s L=%d: fields %.4g units, %.3f of the bound; W %.4g units, %.3f of the bound (oracle %.3f, %.3f); asymmetry %.3g units" % (
        name, L, fig["field_units"], fig["field_ratio"], fig["w_units"], fig["w_ratio"], ora["field_ratio"], ora["w_ratio"], asym))
    record("scan", "dense.%s.L%d" % (name, L), _what=WHAT, device_field_units=fig["field_units"], device_field_ratio_to_bound=fig["field_ratio"],
           device_w_units=fig["w_units"], device_w_ratio_to_bound=fig["w_ratio"], oracle_field_ratio_to_bound=ora["field_ratio"],
           oracle_w_ratio_to_bound=ora["w_ratio"], asymmetry_units=asym)
    touched = np.zeros((s["pose"].shape[0], L), dtype=bool)
    for p, e in enumerate(ex):
        touched[p, list(e["landmarks"])] = True
    assert np.array_equal(g["means"][~touched], np.broadcast_to(s["means"], g["means"].shape)[~touched])
    assert np.array_equal(g["covs"][~touched], np.broadcast_to(s["covs"], g["covs"].shape)[~touched])
    assert fig["counts_equal"] and fig["field_ratio"] <= 1.0 and fig["w_ratio"] <= 1.0, fig


@pytest.mark.parametrize("L,route,longest", [(513, "sweep8", 6), (3000, "sweep8", 7), (40, "general", 10), (1030, "general", 11)])
def test_long_chains_on_the_routes_that_keep_them(lib, L, route, longest):
    """one landmark with 5 .. 8 sightings (eight hand-off slots, fast_observe = 3) and with 9 .. 12 (the general kernels)"""
    s = sr.scene("chains", L, longest)
    assert s["most"] == longest
    check_scene(lib, s, {route: sr.ROUTES[L][route]})


def test_the_table_mode_on_a_second_scan_after_a_resample(lib):
    """k_step_pub with the colour table engaged: the second scan of a filter, behind a resample, its landmarks' colour blocks read
    from the table.  The state the second scan meets is the device's own (downloaded, every double taken exactly)."""
    s = dict(sr.scene("typical", 1030))
    P, L = s["pose"].shape[0], s["L"]
    f = lib.DeviceFilter(P, L)
    try:
        f.set_measurement_noise(s["Qt"])
        f.upload_map(s["means"], s["covs"].reshape(L, 25))
        f.upload_poses(s["pose"])
        f.observe(s["blobs"], fresh=True)
        f.resample(0.37, domain=LOG)
        pose = f.download_poses()
        m, c, k = f.download_landmarks()
        ids = np.concatenate([sr.safe_ids(pose[p:p + 1], m[p], c[p], s["blobs"], what=("second scan", p))[0] for p in range(P)])
        s.update(pose=pose, means=m, covs=c, counts=k.astype(np.int64), ids=ids)
        o_logw, o_means, o_covs, o_counts, args = sr.oracle_scan(s)
        ex = sr.exact_scan(pose, m, c, s["counts"], None, s["Qt"], s["blobs"], ids, device_zhat0(lib, args), None)
        f.observe(s["blobs"], fresh=True)
        assert (f.observe_route(), int(f.observe_published()), f.observe_flagged()) == ("ml_regs", 1, (0, 0))
        assert f.colour_table_stats()["engaged"] == 1 and f.colour_table_stats()["scans"] == 2
        m2, c2, k2 = f.download_landmarks()
        fig = sr.scan_figures(ex, f.download_log_weights(), m2, c2, k2)
        ora = sr.scan_figures(ex, o_logw, o_means, o_covs, o_counts)
    finally:
        f.close()
    print("second scan in table mode: fields %.3f of the bound, W %.3f (oracle %.3f, %.3f)" % (fig["field_ratio"], fig["w_ratio"], ora["field_ratio"], ora["w_ratio"]))
    record("scan", "typical.L1030.table_mode_second_scan", _what=WHAT, device_field_ratio_to_bound=fig["field_ratio"], device_w_ratio_to_bound=fig["w_ratio"],
           oracle_field_ratio_to_bound=ora["field_ratio"], oracle_w_ratio_to_bound=ora["w_ratio"])
    assert fig["counts_equal"] and fig["field_ratio"] <= 1.0 and fig["w_ratio"] <= 1.0, fig

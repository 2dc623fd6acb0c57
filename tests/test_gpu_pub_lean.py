"""GPU: the LEAN body of k_step_pub's two-pair instance (pk_k_step_pub.hip: pub_lean_pair; DESIGN.md section 4, "lean groups").
k_cand_entries marks the (wave, pair) groups of 128 landmarks all of which have at most one candidate blob that nobody else lists;
those groups skip the publish / subscribe machinery and decide their blob from bounds on its key, and fall back to the usual body
for the pair wherever a bound does not decide.  The lean body only decides: every state below must be the SAME BITS with the
switch on ("pub_lean" = 1, the default) and off, step by step -- log-weights, flagged particles, poses, landmark means, covariances
and counts, the growing maps' bookkeeping -- and is also held to the same run on the register route without publish / subscribe
("pub_step" = 0) the way tests/test_gpu_pub.py holds k_step_pub to it: maps and counts bit for bit, log-weights to the rounding
of another order of summation (rtol 1e-12: that kernel adds the lanes' shares up in another order; the figure is printed).

pk_observe_lean_stats says how many groups were marked and how many pairs fell back, so that no case can pass on the usual body
alone.  Maps of 1 025 .. 2 048 padded landmarks take the two-pair instance; L = 520 (the smallest map of the ONE-pair 512-lane
instance, which has no groups: all three figures are 0) rides along to show that the switch leaves it alone."""
import math

import numpy as np
import pytest

from oracle.fastslam_oracle import EMPTY_COLOUR, synthetic_scan, synthetic_world
from test_gpu_colour_table import truth

pytestmark = pytest.mark.gpu

LOG = 1  # PK_WEIGHTS_LOG
P = 64
SPACING = 36.0  # an 8 x 8 x 8 lattice: neighbours 36 apart, the colour gate (:441) is sqrt(300) = 17.3 wide, the lists' margin 1.5 a channel


def lattice_world(L, seed=123):
    """synthetic_world's ring with colours on a lattice: the ring is cut into n = ceil(L / 512) arcs of M = ceil(L / n) places and
    landmark l takes lattice point l mod M, so landmarks of one colour are a whole arc -- at least 1.5 rad of bearing, round the ring's
    end too -- apart, beyond the bearing gate (:433, 0.5) and the lists' margin (0.2) together: no blob is inside two landmarks' gates."""
    means, covs = synthetic_world(L, seed=seed)
    n = -(-L // 512)
    k = np.arange(L) % -(-L // n)
    means[:, 2:] = np.stack([k % 8, (k // 8) % 8, k // 64], axis=1) * SPACING
    return means, covs


def drive(lib, means, covs, scans, opts=None, poses=None, immutable=None, Qt=None, counts=None, grow=None, switch=None, particles=P, motion=(0.2, 0.05, 0.1)):
    """One filter through the scans: motion, a fresh observe, resample.  What it left, scan by scan and at the end."""
    L = means.shape[0]
    f = lib.DeviceFilter(particles, L)
    for k, v in (opts or {}).items():
        f.set_option(k, v)
    if Qt is not None:
        f.set_measurement_noise(Qt)
    f.upload_map(means, covs.reshape(L, 25), immutable)
    if poses is None:
        poses = np.zeros((particles, 4))
        poses[:, 3] = 1.0
    f.upload_poses(poses)
    if counts is not None:
        f.upload_landmarks(0, particles, counts=counts)
    if grow is not None:
        f.grow_enable(*grow)
    rs = np.random.RandomState(77)
    out = dict(logw=[], flags=[], lean=[], route=[], published=[])
    for s, blobs in enumerate(scans):
        if switch and s in switch:
            f.set_option("pub_lean", switch[s])
        f.motion(*motion, z=0.05 * rs.standard_normal((particles, 3)))
        f.observe(blobs, fresh=True)
        out["logw"].append(f.download_log_weights())
        out["flags"].append(f.observe_flags())
        out["lean"].append(f.observe_lean_stats())
        out["route"].append(f.observe_route())
        out["published"].append(f.observe_published())
        f.resample(float(rs.uniform()), domain=LOG)
    out["poses"] = f.download_poses()
    out["maps"] = f.download_landmarks()
    out["grow"] = f.grow_download() if grow is not None else None
    f.close()
    return out


def same_bits(a, b):
    for x, y in zip(a["logw"], b["logw"]):
        assert np.array_equal(x, y)
    for x, y in zip(a["flags"], b["flags"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["poses"], b["poses"])
    for x, y in zip(a["maps"], b["maps"]):
        assert np.array_equal(x, y)
    if a["grow"] is not None:
        (ca, ra, sa), (cb, rb, sb) = a["grow"], b["grow"]
        assert np.array_equal(ca, cb)
        for i in range(len(ca)):  # (beyond the stored readings and the slots in use: never written)
            assert np.array_equal(ra[i, :ca[i, 0]], rb[i, :cb[i, 0]]) and np.array_equal(sa[i, :ca[i, 1]], sb[i, :cb[i, 1]])


def same_as_the_register_route(a, r):
    """tests/test_gpu_pub.py's same_state, scan by scan: the maps bit for bit, the log-weights to the order of summation."""
    worst = max(float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300))) for x, y in zip(a["logw"], r["logw"]))
    print("log-weights against pub_step = 0: largest relative difference %.3g, identical %s" % (
        worst, all(np.array_equal(x, y) for x, y in zip(a["logw"], r["logw"]))))
    for x, y in zip(a["logw"], r["logw"]):
        assert np.allclose(x, y, rtol=1e-12, atol=1e-9)
    assert np.array_equal(a["poses"][:, :3], r["poses"][:, :3])
    for x, y in zip(a["maps"], r["maps"]):
        assert np.array_equal(x, y)
    if a["grow"] is not None:
        assert np.array_equal(a["grow"][0], r["grow"][0])


def three_ways(lib, means, covs, scans, opts=None, **kw):
    """The run with the lean body, without it, and on the register route without publish / subscribe; the first, checked."""
    on = drive(lib, means, covs, scans, dict(opts or {}), **kw)
    off = drive(lib, means, covs, scans, dict(opts or {}, pub_lean=0), **kw)
    regs = drive(lib, means, covs, scans, dict(opts or {}, pub_step=0), **kw)
    print("lean groups per scan:", on["lean"])
    assert all(r == "ml_regs" for r in on["route"] + off["route"])
    assert all(on["published"]) and all(off["published"]) and not any(regs["published"])
    assert all(st["fallbacks"] == 0 for st in off["lean"])  # (switched off, nothing is lean: nothing falls back)
    assert [(st["marked"], st["in_use"]) for st in on["lean"]] == [(st["marked"], st["in_use"]) for st in off["lean"]]
    same_bits(on, off)
    same_as_the_register_route(on, regs)
    return on


def scans_along(means, n, seen=None):
    return [synthetic_scan(means if seen is None else means[seen], pose) for pose in truth(n)]


@pytest.mark.parametrize("L", [520, 1025, 2000, 2048])
def test_every_group_lean(lib, L):
    means, covs = lattice_world(L)
    # (2 048 landmarks: no place beyond the map; the scan sees 2 000 of them -- the register route's scan tables hold no more blobs)
    seen = np.arange(L) if L < 2048 else np.flatnonzero(np.arange(L) % 43 != 0)
    on = three_ways(lib, means, covs, scans_along(means, 3, seen))
    for st in on["lean"]:
        assert st["marked"] == st["in_use"] and st["fallbacks"] == 0
        assert st["in_use"] == (0 if L <= 1024 else (L + 127) // 128)  # (no groups in the one-pair instance)
    assert all((fl == 0).all() for fl in on["flags"])
    assert (on["maps"][2][:, seen] == 6).mean() > 0.99  # three scans, an update each (the odd landmark across the bearings' branch cut misses one, :408-423)


def test_lean_and_usual_groups_side_by_side(lib):
    """Half the landmarks on the lattice; the other half in look-alike pairs, colours 5 and bearings 0.05 rad apart: both blobs of a
    pair are inside both landmarks' gates.  Landmarks 1 000 .. 1 999 -- octets 62 .. 124 -- are not simple: eight of the sixteen
    groups take the usual body.  A fresh map and three scans."""
    L = 2000
    means, covs = lattice_world(L)
    a = np.arange(1000, L, 2)
    phi = np.arctan2(means[a, 1], means[a, 0]) + 0.05
    rho = np.hypot(means[a, 0], means[a, 1])
    means[a + 1, 0], means[a + 1, 1] = rho * np.cos(phi), rho * np.sin(phi)
    means[a + 1, 2:] = means[a, 2:] + np.array([3.0, 4.0, 0.0])
    on = three_ways(lib, means, covs, scans_along(means, 3))
    for st in on["lean"]:
        assert 0 < st["marked"] < st["in_use"] == 16
        assert st["marked"] >= 7 and st["in_use"] - st["marked"] >= 7


def test_the_bench_scene(lib):
    # bench.py's world (synthetic_world, seed 123: random colours) and noise-free scans, steps 0-2
    means, covs = synthetic_world(2000)
    on = three_ways(lib, means, covs, scans_along(means, 3))
    assert all(st["in_use"] == 16 for st in on["lean"])


def test_the_underflow_edge_inside_a_lean_group(lib):
    """Second scan (colour blocks at level 1: 1 / 14): blob i stands off its landmark's colour by a distance swept from 9.5 to 12.5
    over the landmarks -- keys of about 1 330 to 2 190, across the strip 1 489 .. 1 491.5 in which the usual body evaluates the
    probability exactly (:369: a probability of 0 matches nobody, and the blob costs the particle log 0.1)."""
    L = 2000
    means, covs = lattice_world(L)
    scans = scans_along(means, 2)
    d = np.linspace(9.5, 12.5, L)
    scans[1][:, 1:] += d[:, None] * np.array([0.6, 0.64, 0.48])  # (a unit vector)
    on = three_ways(lib, means, covs, scans)
    assert on["lean"][0]["fallbacks"] == 0 and on["lean"][1]["fallbacks"] > 0
    assert on["lean"][1]["marked"] == on["lean"][1]["in_use"] == 16
    k = on["maps"][2]
    assert (k[:, :50] == 4).all() and (k[:, -50:] == 2).all()  # matched at 9.5, unmatched at 12.5
    assert all((fl == 0).all() for fl in on["flags"])


def test_particles_outside_the_candidate_margins_are_flagged_either_way(lib):
    means, covs = lattice_world(2000)
    poses = np.zeros((P, 4))
    poses[:, 3] = 1.0
    off_margin = [5, 17, 40]
    poses[off_margin, 2] = 0.3  # more than kCandBearing = 0.2 off the reference particle's heading
    on = three_ways(lib, means, covs, scans_along(means, 1), poses=poses)
    assert sorted(np.flatnonzero(on["flags"][0])) == off_margin
    assert on["lean"][0]["marked"] == 16 and on["lean"][0]["fallbacks"] > 0


def test_immutable_landmarks_and_potential_counts_in_lean_groups(lib):
    L = 2000
    means, covs = lattice_world(L)
    rs = np.random.RandomState(4)
    imm = (rs.uniform(size=L) < 0.1).astype(np.uint8)
    counts = np.zeros((P, L), dtype=np.int32)
    counts[:, rs.uniform(size=L) < 0.1] = lib.PK_LANDMARK_POTENTIAL | 4
    on = three_ways(lib, means, covs, scans_along(means, 3), immutable=imm, counts=counts)
    assert all(st["marked"] == st["in_use"] == 16 for st in on["lean"])
    assert (on["maps"][0][:, imm != 0] == means[imm != 0]).all()  # (:909, :926: an immutable landmark keeps its mean)


def test_a_measurement_noise_with_off_diagonal_terms(lib):
    means, covs = lattice_world(2000)
    Qt = np.diag([0.1, 0.1, 0.12, 0.08])
    Qt[1, 2] = Qt[2, 1] = 0.03
    Qt[1, 3] = Qt[3, 1] = -0.02
    Qt[2, 3] = Qt[3, 2] = 0.01
    on = three_ways(lib, means, covs, scans_along(means, 3), Qt=Qt)
    assert all(st["marked"] == st["in_use"] == 16 and st["fallbacks"] == 0 for st in on["lean"])


def test_the_plain_instance(lib):
    # "colour_table" = 0: the instance that reads and writes the slots' colour rows
    means, covs = lattice_world(2000)
    on = three_ways(lib, means, covs, scans_along(means, 3), {"colour_table": 0})
    assert all(st["marked"] == st["in_use"] == 16 and st["fallbacks"] == 0 for st in on["lean"])


def test_growing_maps(lib):
    """A growing map on the one-pass route (the plain instance): 1 500 known landmarks, three unknown ones in sight, four spare
    slots.  The kernel's rows of unmatched blobs feed the bookkeeping: stored readings, slots in use and ids are equal."""
    L0, U, spare = 1500, 3, 4
    world, _ = lattice_world(L0 + U)
    means = np.zeros((L0 + spare, 5))
    means[:L0] = world[:L0]
    means[L0:, 2:] = EMPTY_COLOUR
    covs = np.tile(np.identity(5), (L0 + spare, 1, 1))
    covs[:L0] = 0.25 * np.identity(5)
    scans = [synthetic_scan(world, pose) for pose in truth(5, v=0.8, w=0.35, dt=0.5)]
    on = three_ways(lib, means, covs, scans, grow=(L0, 128, 30.0), particles=32, motion=(0.8, 0.35, 0.5))
    # (a landmark a particle has added can be a second candidate of some blob: a group or two may stop being lean as the maps grow)
    assert on["lean"][0]["marked"] == 12 and all(st["in_use"] == 12 and st["marked"] >= 8 for st in on["lean"])
    assert on["grow"][0][:, 0].max() > 0  # readings were stored: blobs nobody matched


def test_the_switch_thrown_in_mid_run(lib):
    means, covs = lattice_world(2000)
    scans = scans_along(means, 4)
    d = np.linspace(9.5, 12.5, 2000)
    scans[1][:, 1:] += d[:, None] * np.array([0.6, 0.64, 0.48])  # (the underflow edge at colour level 1, as above)
    through = drive(lib, means, covs, scans)
    thrown = drive(lib, means, covs, scans, switch={0: 0, 1: 1, 2: 0, 3: 1})
    same_bits(through, thrown)
    assert [st["marked"] for st in thrown["lean"]] == [16, 16, 16, 16]
    assert [st["fallbacks"] > 0 for st in thrown["lean"]] == [False, True, False, False]

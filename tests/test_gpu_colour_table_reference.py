"""GPU: the colour table against references outside the project ("The colour table").

tests/test_gpu_colour_table.py holds the table mode to the run without it, bit for bit -- both sides through the same
colour_block_step.  This file keeps that twin comparison (`colour_table` = 0 beside the default, np.array_equal) and adds what it
cannot see:

  * deep levels against the closed form C_k = (C_0^-1 + k Qc^-1)^-1 in exact rational arithmetic (tests/colour_reference.py),
    within BOUND(k) = 4 e_ref(k) + 64 * 2^-52, e_ref(k) being what the oracle's own float64 update loses at that level in that
    world (tests/test_colour_recurrence_reference.py prints it): levels 1 .. 300 from the table, and levels 8 .. 40 from the
    recurrence the kernels run themselves beyond a table of eight;
  * whole steps in table mode against the oracle, six in a row, at L = 520, 1 030 and 2 000;
  * the transitions of pk_api.hip and pk_api_observe.hip nobody made: a second pk_upload_map, a Qt change between scans, pk_associate, supplied ids, the
    option switched in mid-run, the staged path, a ranged observe, and the edges of the map sizes the mode takes.

Every test asserts through colour_table_stats / observe_route / observe_published that the mode took the scans it claims.

Measured on an MI355X, worst rel_err / BOUND over all checkpoints (printed by the deep-level tests, run with -s):
               levels from the table (1 .. 300)      levels beyond a table of eight (8 .. 40)
               L = 520      L = 1 030                L = 520      L = 1 030
    W1         0.131        0.131                    0.032        0.032
    W2         0.063        0.066                    0.025        0.023
    W3         0.432        0.323                    0.430        0.322
    W4         0.162        0.140                    0.076        0.101
(W1: one block, Qt = 0.1 I; W2: a block per landmark, a full Qc; W3: W2 with blocks x 1200, Qc x 0.1; W4: W2's blocks, Qc = diag(0.1,
0.02, 3) -- the short form Qc M with unequal row factors.)  Nothing came near the bound; W3 (C - C M with |C| / |Qc| about 3e4) loses what the reference's own form loses there, no more.
"""
import numpy as np
import pytest

import colour_reference as cr
import test_gpu_colour_table as tct
from oracle.fastslam_oracle import OracleFilter
from test_gpu_colour_table import FULL_QT, LOG, SEEN, close, same_maps, same_poses, scan_of, truth, us_of
from test_gpu_random_worlds import random_case

pytestmark = pytest.mark.gpu

B = 64


def twins(lib, L, P, means, covs, immutable=None, Qt=None, opts=None, poses=None):
    """(`colour_table` = 0, the default): tct.pair at any map size."""
    out = []
    for table in (0, None):
        f = lib.DeviceFilter(P, L)
        if table is not None:
            f.set_option("colour_table", table)
        for k, v in (opts or {}).items():
            f.set_option(k, v)
        if Qt is not None:
            f.set_measurement_noise(np.asarray(Qt).reshape(16))
        f.upload_map(means, covs.reshape(L, 25), immutable)
        f.upload_poses(fresh_poses(P) if poses is None else poses)
        out.append(f)
    return out


def fresh_poses(P):
    poses = np.zeros((P, 4))
    poses[:, 3] = 1.0
    return poses


def took_the_table_kernel(fs):
    assert fs[1].observe_route() == "ml_regs" and fs[1].observe_published()
    assert fs[0].observe_route() == "ml_regs" and fs[0].observe_published()


def against_exact(c, k, covs0, Qt, seen, worst, exact=None, immutable=None):
    """Every downloaded colour block of the landmarks `seen` (c (n, L, 5, 5), k (n, L)) against the exact level its count names:
    rel_err <= BOUND(level).  Returns the worst rel_err / BOUND."""
    Qc = np.asarray(Qt).reshape(4, 4)[1:, 1:]
    ratio = 0.0
    for l in seen:
        if immutable is not None and immutable[l]:
            continue
        blocks = {}
        for p in range(c.shape[0]):
            blocks[(int(k[p, l]), c[p, l, 2:, 2:].tobytes())] = c[p, l, 2:, 2:]
        for (count, _), blk in blocks.items():
            assert count % 2 == 0
            lev = count // 2
            F = exact[(int(l), lev)] if exact is not None and (int(l), lev) in exact else cr.exact_level(covs0[l, 2:, 2:], Qc, lev)[0]
            e = cr.rel_err(blk, F)
            bnd = cr.bound(worst[lev] if lev > 0 else 0.0)
            assert e <= bnd, "landmark %d level %d: rel_err %.3g > bound %.3g (%.1f ulp against %.1f)" % (l, lev, e, bnd, e / cr.ULP, bnd / cr.ULP)
            ratio = max(ratio, e / bnd)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------------
# 3a. deep levels against the exact value
POSES4 = np.array([[0.0, 0.0, 0.0, 1.0], [0.03, -0.02, 0.004, 1.0], [-0.04, 0.01, -0.003, 1.0], [0.02, 0.04, 0.002, 1.0]])


def run_deep(lib, name, L, scans, checkpoints, opts, depth):
    means, covs, Qt, imm, seen = cr.deep_world(name, L)
    worst, _, exact = cr.deep_e_ref(name, L)
    fs = twins(lib, L, 4, means, covs, imm, Qt, opts, POSES4)
    blobs = scan_of(means, (0.0, 0.0, 0.0), seen)  # the same exact blobs in every scan
    mutable = np.array([l for l in seen if not imm[l]])
    frozen = np.array([l for l in seen if imm[l]])
    untouched = np.setdiff1d(np.arange(L), mutable)
    assert len(frozen) == 2
    ratio = 0.0
    for s in range(1, scans + 1):
        for f in fs:
            f.reset_weights()
            f.observe(blobs)
        took_the_table_kernel(fs)
        if s not in checkpoints:
            continue
        same_poses(fs)
        same_maps(fs)
        m, c, k = fs[1].download_landmarks()
        want = np.zeros(L, dtype=np.int32)
        want[mutable] = 2 * s
        assert np.array_equal(k, np.broadcast_to(want, (4, L))), "scan %d: counts" % s
        assert np.array_equal(c[:, untouched], np.broadcast_to(covs[untouched], (4, len(untouched), 5, 5)))  # the immutable two among them
        assert (np.linalg.eigvalsh(c[:, :, 2:, 2:]) > 0).all(), "scan %d: a colour block is not positive definite" % s
        ratio = max(ratio, against_exact(c, k, covs, Qt, mutable, worst, exact))
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == scans and st["depth"] == depth and st["materialisations"] == len(checkpoints)
    assert fs[0].colour_table_stats()["scans"] == 0
    close(fs)
    return ratio


@pytest.mark.parametrize("L", cr.DEEP_SIZES)
@pytest.mark.parametrize("name", cr.DEEP_WORLDS)
def test_levels_of_the_table_against_the_exact_value(lib, name, L):
    """300 scans of the same 64 exact blobs, no motion, no resample: levels 1, 2, 3, 8, 9, 64 and 300 of the table.
    Measured worst rel_err / BOUND: see the module docstring."""
    ratio = run_deep(lib, name, L, 300, cr.DEEP_LEVELS, None, 1024)
    print("\ncolour table, levels from the table: %s L=%d worst rel_err / bound = %.3f" % (name, L, ratio))


@pytest.mark.parametrize("L", cr.DEEP_SIZES)
@pytest.mark.parametrize("name", cr.DEEP_WORLDS)
def test_levels_beyond_a_table_of_eight_against_the_exact_value(lib, name, L):
    """`colour_table_depth` = 8, `colour_table_margin` = 0, 40 scans: from level 8 on the blocks come from the recurrence inside
    k_step_pub, from colour_block_at in k_colour_rows and from the reference particle in k_candidates."""
    ratio = run_deep(lib, name, L, 40, cr.SHALLOW_LEVELS, {"colour_table_depth": 8, "colour_table_margin": 0}, 8)
    print("\ncolour table, levels beyond the table: %s L=%d worst rel_err / bound = %.3f" % (name, L, ratio))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3b. whole steps in table mode against the oracle
def random_scan(rs, means, pose, pool):
    """A scan as test_gpu_random_worlds.random_case makes them: noisy sightings (of four fifths of `pool`), a tenth of them twice,
    four strays, shuffled."""
    seen = pool[rs.uniform(size=len(pool)) < 0.8]
    again = seen[rs.uniform(size=len(seen)) < 0.1]
    src = np.concatenate([seen, again])
    blobs = np.empty((len(src), 4))
    blobs[:, 0] = np.arctan2(means[src, 1] - pose[1], means[src, 0] - pose[0]) - pose[2] + rs.normal(0, 0.01, len(src))
    blobs[:, 1:] = means[src, 2:] + rs.normal(0, 1.0, (len(src), 3))
    strays = np.column_stack([rs.uniform(-3, 3, 4), rs.uniform(0, 255, (4, 3))])
    blobs = np.vstack([blobs, strays])
    return blobs[rs.permutation(len(blobs))]


@pytest.mark.parametrize("seed,L", [(5100, 520), (5101, 1030), (5102, 2000)])
def test_whole_steps_in_table_mode_against_the_oracle(lib, seed, L):
    """test_random_world_several_steps at the map sizes the table mode takes (NP = 1, NP = 2, the headline's), six steps, the route
    asserted: motion with host-supplied normals, observe, log-domain resample; immutables, a full Qt, landmarks sighted twice,
    strays.  The scans see a pool of 20 landmarks again and again: their levels climb, and some twenty blobs a scan keep the oracle's
    association (P x L probabilities per blob) within a few seconds."""
    P = 48
    rs = np.random.RandomState(seed)
    _, _, means, covs, immutable, _, _, qt = random_case(seed, L=L, P=P)
    o = OracleFilter(P, means, covs, immutable)
    o.Qt = qt.copy()
    filters = []
    for opts in ({}, {"fast_observe": 0}):
        f = lib.DeviceFilter(P, L)
        for k, v in opts.items():
            f.set_option(k, v)
        f.set_measurement_noise(qt)
        f.upload_map(means, covs.reshape(L, 25), immutable)
        filters.append(f)
    pose = np.zeros(3)
    pool = np.sort(rs.choice(L, 20, replace=False))
    for s in range(6):
        v, w, dt = 0.2 + 0.1 * rs.uniform(), 0.1 * rs.normal(), 0.1
        h1 = pose[2] + w * dt / 2
        pose = np.array([pose[0] + v * dt * np.cos(h1), pose[1] + v * dt * np.sin(h1), h1 + w * dt / 2])
        blobs = random_scan(rs, means, pose, pool)
        z = rs.standard_normal((P, 3))
        u = rs.uniform()
        o.reset_weights()
        o.motion(v, w, dt, z)
        o.observe(blobs)
        logw = o.logw.copy()
        anc = o.resample(u, domain="log")
        for f in filters:
            f.motion(v, w, dt, z=z)
            f.observe(blobs, fresh=True)
            assert np.allclose(f.download_log_weights(), logw, rtol=1e-10, atol=1e-9), "log-weights at step %d" % s
            got = f.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
            assert np.array_equal(got, anc), "ancestors differ from the oracle at step %d" % s
            ps = f.download_poses()
            assert np.allclose(ps[:, 0], o.x, rtol=1e-10, atol=1e-13) and np.allclose(ps[:, 1], o.y, rtol=1e-10, atol=1e-13)
            assert np.allclose(ps[:, 2], o.h, rtol=1e-10, atol=1e-13)
        assert filters[0].observe_route() == "ml_regs" and filters[0].observe_published()
        assert filters[1].observe_route() == "ml_general"
    st = filters[0].colour_table_stats()
    assert st["scans"] == 6 and st["engaged"] == 1
    assert o.count.max() >= 8  # (four updates of one landmark at least: the table was read well above level 0)
    for f in filters:
        m, c, k = f.download_landmarks()
        assert np.allclose(m, o.mean, rtol=1e-9, atol=1e-11)
        assert np.allclose(c, o.cov, rtol=1e-8, atol=1e-13)
        assert np.array_equal(k, o.count)
        f.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3c. transitions.  L = 520, P = 96 (tct.pair), six steps, the event between the third and the fourth.
def levels_within_bound(f, key, means, covs, Qt, seen, top):
    """The seen landmarks' blocks of every particle against the exact levels their counts name; `top`: the level they must reach."""
    Qt4 = (0.1 * np.identity(4)) if Qt is None else np.asarray(Qt).reshape(4, 4)
    worst, _, exact = cr.e_ref(key, means, covs, Qt4, seen, list(range(1, top + 1)))
    m, c, k = f.download_landmarks()
    assert k[:, seen].max() == 2 * top and (k % 2 == 0).all()
    assert (np.linalg.eigvalsh(c[:, :, 2:, 2:]) > 0).all()
    return against_exact(c, k, covs, Qt4, seen, worst, exact)


@pytest.mark.parametrize("change_qt", [True, False])
def test_a_second_upload_map_on_an_engaged_filter(lib, change_qt):
    """A stale table, a stale base or a stale depth would show: the second map has other colour blocks (and, change_qt, another Qt),
    and the filter must end where a filter created for the second map ends, bit for bit."""
    means, covs = tct.world(seed=21)
    fs = tct.pair(lib, means, covs)
    us, tr = us_of(6), truth(6)
    for s in range(3):
        tct.step(fs, s, scan_of(means, tr[s], SEEN), us)
        same_poses(fs)
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == 3 and st["depth"] == 1024
    means2, covs2 = tct.world(seed=22, one_block=False)
    Qt2 = FULL_QT if change_qt else None
    for f in fs:
        f.set_option("colour_table_depth", 64)
        if change_qt:
            f.set_measurement_noise(Qt2.reshape(16))
        f.upload_map(means2, covs2.reshape(tct.L, 25))
        f.upload_poses(fresh_poses(tct.P))
    assert fs[1].colour_table_stats()["engaged"] == 0
    fresh = tct.pair(lib, means2, covs2, Qt=None if Qt2 is None else Qt2.reshape(16), opts={"colour_table_depth": 64})
    for s in range(3, 6):
        tct.step(fs + fresh, s, scan_of(means2, tr[s - 3], SEEN), us)
        same_poses(fs)
        same_poses(fresh)
        same_poses([fs[1], fresh[1]])
        took_the_table_kernel(fs)
    st = fs[1].colour_table_stats()
    assert st["depth"] == 64 and st["engaged"] == 1 and st["scans"] == 6
    st = fresh[1].colour_table_stats()
    assert st["depth"] == 64 and st["engaged"] == 1 and st["scans"] == 3
    same_maps(fs)
    same_maps(fresh)
    same_maps([fs[1], fresh[1]])
    levels_within_bound(fs[1], ("second map", change_qt), means2, covs2, Qt2, SEEN, 3)
    close(fs + fresh)


def test_qt_changed_before_any_update(lib):
    """The first scan matches nothing (every blob's colour is 400 away from every landmark's): the maps are at level 0 still, a new
    Qt builds the table afresh and the mode goes on."""
    means, covs = tct.world(seed=23, one_block=False)
    fs = tct.pair(lib, means, covs)
    us, tr = us_of(6), truth(6)
    blobs = scan_of(means, tr[0], SEEN)
    blobs[:, 1:] = -400.0
    tct.step(fs, 0, blobs, us)
    same_poses(fs)
    assert fs[1].colour_table_stats()["scans"] == 1
    for f in fs:
        assert (f.download_landmarks()[2] == 0).all()
        f.set_measurement_noise(FULL_QT.reshape(16))
    for s in range(1, 6):
        tct.step(fs, s, scan_of(means, tr[s], SEEN), us)
        same_poses(fs)
        took_the_table_kernel(fs)
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == 6
    same_maps(fs)
    levels_within_bound(fs[1], "qt before any update", means, covs, FULL_QT, SEEN, 5)
    close(fs)


def test_associate_in_mid_run_and_the_mode_goes_on(lib):
    means, covs = tct.world(seed=24, one_block=False)
    fs = tct.pair(lib, means, covs)
    us, tr = us_of(6), truth(6)
    for s in range(6):
        blobs = scan_of(means, tr[s], SEEN)
        if s == 3:
            before = fs[1].colour_table_stats()
            assert before["engaged"] == 1 and before["scans"] == 3
            ids = [f.associate(blobs) for f in fs]
            assert np.array_equal(ids[0], ids[1]) and (ids[1] > 0).any()
            st = fs[1].colour_table_stats()
            assert st["materialisations"] == before["materialisations"] + 1 and st["engaged"] == 1 and st["scans"] == 3
        tct.step(fs, s, blobs, us)
        same_poses(fs)
        took_the_table_kernel(fs)
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == 6
    same_maps(fs)
    levels_within_bound(fs[1], "associate", means, covs, None, SEEN, 6)
    close(fs)


def test_an_observe_with_ids_supplied_ends_the_mode(lib):
    means, covs = tct.world(seed=25, one_block=False)
    fs = tct.pair(lib, means, covs)
    us, tr = us_of(6), truth(6)
    for s in range(6):
        blobs = scan_of(means, tr[s], SEEN)
        if s == 3:  # the ids pk_associate just returned (the first particle's: pk_observe takes one row for everybody)
            ids = [f.associate(blobs) for f in fs]
            assert np.array_equal(ids[0], ids[1])
            assert np.array_equal(ids[1][0], SEEN + 1)
            for f in fs:
                f.step(0.2, 0.05, 0.1, blobs, us[s], seed=5, draw=s, ids=ids[1][0], domain=LOG)
            assert fs[1].observe_route() == "known_ids"
            assert fs[1].colour_table_stats()["engaged"] == 0
        else:
            tct.step(fs, s, blobs, us)
        same_poses(fs)
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 0 and st["scans"] == 3  # off until the next pk_upload_map
    same_maps(fs)
    levels_within_bound(fs[1], "ids supplied", means, covs, None, SEEN, 6)
    close(fs)


def test_the_option_switched_off_in_mid_run_and_on_again(lib):
    means, covs = tct.world(seed=26, one_block=False)
    fs = tct.pair(lib, means, covs)
    us, tr = us_of(6), truth(6)
    for s in range(6):
        if s == 3:
            assert fs[1].colour_table_stats()["engaged"] == 1
            fs[1].set_option("colour_table", 0)
            assert fs[1].colour_table_stats()["engaged"] == 0
        if s == 4:
            fs[1].set_option("colour_table", -1)  # too late: off until the next pk_upload_map
        tct.step(fs, s, scan_of(means, tr[s], SEEN), us)
        same_poses(fs)
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 0 and st["scans"] == 3
    same_maps(fs)
    levels_within_bound(fs[1], "option off", means, covs, None, SEEN, 6)
    # ... and the next pk_upload_map brings it back
    fs[1].upload_map(means, covs.reshape(tct.L, 25))
    fs[0].upload_map(means, covs.reshape(tct.L, 25))
    for f in fs:
        f.upload_poses(fresh_poses(tct.P))
    tct.step(fs, 0, scan_of(means, tr[0], SEEN), us)
    same_poses(fs)
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == 4
    same_maps(fs)
    close(fs)


@pytest.mark.parametrize("ranged", [False, True])
def test_the_staged_path(lib, ranged):
    """pk_stage_scan + pk_observe_staged, the way the benchmark steps the filter: the mode takes every scan.  ranged: the fourth
    observe is one pk_observe_staged_range over all particles -- another route, the mode ends."""
    means, covs = tct.world(seed=27, one_block=False)
    fs = tct.pair(lib, means, covs)
    us, tr = us_of(6), truth(6)
    for s in range(6):
        blobs = scan_of(means, tr[s], SEEN)
        for f in fs:
            f.stage_scan(blobs)
            f.motion(0.2, 0.05, 0.1, seed=5, draw=s)
            if ranged and s == 3:
                assert f.staged_takes_regs()
                f.observe_staged_range(True, 0, tct.P, True, True)
            else:
                f.observe_staged(fresh=True)
            f.resample(us[s], domain=LOG)
        same_poses(fs)
        assert fs[1].observe_route() == "ml_regs"
        st = fs[1].colour_table_stats()
        if ranged and s >= 3:
            assert st["engaged"] == 0 and st["scans"] == 3
        else:
            assert st["engaged"] == 1 and st["scans"] == s + 1 and fs[1].observe_published()
    assert fs[0].colour_table_stats()["scans"] == 0
    same_maps(fs)
    levels_within_bound(fs[1], "staged", means, covs, None, SEEN, 6)
    close(fs)


# Lp = L rounded up to a multiple of 16 (pk_layout.hpp), and the mode wants 512 < Lp, L <= 2048 (plan_scan / ct_state_ok, pk_upload_map):
# L = 513 has Lp = 528 > 512 -- the smallest map on the table's side (L = 512: Lp = 512, k_step_fused);
# 1024 is the last map of the NP = 1 instance, 1025 (Lp = 1040) and 1026 the first of NP = 2; 2047 and 2048 (Lp = 2048) the last.
@pytest.mark.parametrize("L", [513, 1024, 1025, 1026, 2047, 2048])
def test_edges_of_the_map_size(lib, L):
    """Landmarks 0 and L - 1 are seen (the rows' ends; behind L - 1 come the padded lanes), three steps with resampling, then a scan
    in which L - 1 is sighted three times: its block goes through the register-carried path from a table level."""
    P = 8
    Lp = (L + 15) & ~15
    assert 512 < Lp and L <= 2048
    means, covs = cr.world_at(L, seed=30 + L % 7, one_block=False)
    seen = np.concatenate([[0], np.arange(3, L, 8)[:B - 2], [L - 1]])
    fs = twins(lib, L, P, means, covs, Qt=FULL_QT)
    worst, _, exact = cr.e_ref(("edge", L), means, covs, FULL_QT, seen, [1, 2, 3, 4, 5, 6])
    us, tr = us_of(4), truth(4)
    ends = np.array([0, L - 1])
    for s in range(4):
        blobs = scan_of(means, tr[s], seen)
        if s == 3:  # two more sightings of L - 1 in place of two other landmarks'
            extra = np.repeat(scan_of(means, tr[s], np.array([L - 1])), 2, axis=0)
            extra[:, 0] += (1e-3, -1e-3)
            extra[:, 1:] += ((0.05, -0.05, 0.02), (-0.04, 0.03, 0.05))
            blobs = np.vstack([blobs[:1], extra, blobs[3:]])
        for f in fs:
            f.step(0.2, 0.05, 0.1, blobs, us[s], seed=5, draw=s, domain=LOG)
        same_poses(fs)
        took_the_table_kernel(fs)
        assert fs[1].observe_flagged()[0] == 0
        same_maps(fs)
        m, c, k = fs[1].download_landmarks()
        want = 2 * (s + 1) if s < 3 else np.array([8, 12])
        assert np.array_equal(k[:, ends], np.broadcast_to(want, (P, 2))), "step %d" % s
        assert (np.linalg.eigvalsh(c[:, :, 2:, 2:]) > 0).all()
        against_exact(c, k, covs, FULL_QT, ends, worst, exact)
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == 4
    m, c, k = fs[1].download_landmarks()
    against_exact(c, k, covs, FULL_QT, seen, worst, exact)
    unseen = np.setdiff1d(np.arange(L), seen)
    assert (k[:, unseen] == 0).all() and np.array_equal(c[:, unseen], np.broadcast_to(covs[unseen], (P, len(unseen), 5, 5)))
    close(fs)

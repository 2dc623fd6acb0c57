"""GPU: the map estimate (pk_map_moments / pk_map_summary, pk_k_mapsum.hip) -- per-landmark moments of the
particles' landmark EKFs, reduced over the particles on the device, read through src[] where the particles are.

The reference in every case is the two-pass NumPy computation in float64 over download_landmarks of ALL particles
(mapsum_reference.py, where the tolerances are stated).  The estimate is taken BEFORE the download: the download materialises."""
import math
import random

import numpy as np
import pytest

from mapsum_reference import POT, block_diagonal_covs, check, two_pass
from oracle.fastslam_oracle import EMPTY_COLOUR, synthetic_scan, synthetic_world, truth_step

pytestmark = pytest.mark.gpu

LOG = 1  # PK_WEIGHTS_LOG
UNIFORM, WEIGHTED = 0, 1


def distinct_filter(lib, P, L, seed, offset=0.0, spread=0.3, weights=None):
    """A filter whose particles hold different maps (pk_upload_landmarks): means spread about a ring world (+ offset), a different
    block-diagonal covariance and update count in every particle and landmark, a tenth of the counts with the potential bit."""
    rs = np.random.RandomState(seed)
    base, bcov = synthetic_world(L, seed=seed + 1)
    base = base + offset
    f = lib.DeviceFilter(P, L)
    f.upload_map(base, bcov.reshape(L, 25))
    poses = np.zeros((P, 4))
    poses[:, :3] = rs.uniform(-1.0, 1.0, size=(P, 3))
    poses[:, 3] = 1.0 if weights is None else weights
    f.upload_poses(poses)
    means = base[None] + spread * rs.standard_normal((P, L, 5))
    counts = rs.randint(0, 40, size=(P, L)).astype(np.int32)
    counts[rs.uniform(size=(P, L)) < 0.1] |= POT
    f.upload_landmarks(0, P, means, block_diagonal_covs(rs, P, L).reshape(P, L, 25), counts)
    return f


def reference(f, w=None):
    m, c, k = f.download_landmarks()
    return two_pass(m, c, k, w)


def same_bits(a, b):
    return all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True) for n in ("mean", "cov_within", "cov_between", "update_count")) \
        and a.n_eff == b.n_eff


# ---- (a) shapes: maps below, at and beyond one tile of 256 landmarks and the padding of the rows; one particle, fewer particles than
# a group takes, several groups with a ragged last one; forced group counts at P = 1000
@pytest.mark.parametrize("P", [1, 3, 257, 1000])
@pytest.mark.parametrize("L", [5, 500, 513, 1030])
def test_shapes_uniform_weighting(lib, L, P):
    f = distinct_filter(lib, P, L, seed=L + P)
    got = []
    for groups in {1000: (0, 1, 3, 7), 3: (0, 7)}.get(P, (0,)):  # (7 groups of 3 particles: four of them are empty)
        f.set_option("map_sum_groups", groups)
        got.append((groups, f.map_summary()))
    ref = reference(f)
    for groups, g in got:
        check(g, ref, what="L %d P %d groups %d" % (L, P, groups))
        assert abs(g.n_eff - P) <= 1e-12 * P
        assert np.array_equal(g.ids, np.arange(1, L + 1))
    f.close()


# ---- (b) behind a resample: long runs of equal src that cross group boundaries; nothing of the filter changes
def test_behind_a_resample_with_a_few_heavy_particles(lib):
    P, L, G = 1000, 40, 7
    w = np.full(P, 1e-7)
    w[[100, 400, 401, 900]] = 1.0, 0.7, 1.3, 0.9
    f = distinct_filter(lib, P, L, seed=3, weights=w)
    f.set_option("map_sum_groups", G)
    f.resample(0.37)
    src = f.download_sources()
    chunk = -(-P // G)
    crossing = [b for b in range(chunk, P, chunk) if src[b - 1] == src[b]]
    assert len(np.unique(src)) <= 6 and len(crossing) >= 3, "runs of one slot must cross the groups' boundaries"
    poses, logw, route = f.download_poses(), f.download_log_weights(), f.observe_route()
    first = f.map_summary()
    second = f.map_summary()
    assert np.array_equal(f.download_sources(), src)
    assert np.array_equal(f.download_poses(), poses) and np.array_equal(f.download_log_weights(), logw) and f.observe_route() == route
    assert same_bits(first, second), "the same filter state must give the same bits twice"
    ref = reference(f)  # (materialises: every particle in its own slot from here on)
    assert np.array_equal(f.download_sources(), np.arange(P))
    check(first, ref, what="behind a resample")
    check(f.map_summary(), ref, what="behind the materialisation")
    f.close()


# ---- (c) by the weights, between an observe and a resample
def observed_filter(lib, P, L, B):
    means, covs = synthetic_world(L, seed=21)
    f = lib.DeviceFilter(P, L)
    f.upload_map(means, covs.reshape(L, 25))
    poses = np.zeros((P, 4))
    poses[:, 3] = 1.0
    f.upload_poses(poses)
    seen = np.arange(1, L, max(1, L // B))[:B]
    pose = truth_step((0.0, 0.0, 0.0), 0.2, 0.05, 0.1)
    f.motion(0.2, 0.05, 0.1, seed=5, draw=0)
    return f, synthetic_scan(means[seen], pose)


def test_weighted_between_an_observe_and_a_resample(lib):
    f, blobs = observed_filter(lib, 300, 48, 16)
    f.observe(blobs, fresh=True)
    logw = f.download_log_weights()
    assert np.isfinite(logw).all() and np.ptp(logw) > 0.0, "the particles must weigh differently"
    got = f.map_summary(WEIGHTED)
    w = np.exp(logw - logw.max())
    check(got, reference(f, w), what="weighted")
    assert 1.0 < got.n_eff < 300.0
    f.close()


def test_weighted_where_the_linear_weights_underflow(lib):
    """Log-weights near -2 000: every linear weight is 0 (pk_download_poses hands out exp(log w)), the estimate by the weights
    lives in the log domain.  pk_upload_pose takes a LINEAR weight, so no log-weight of -2 000 can be uploaded through it: the
    log-weights get there by observes that do not restart the weights (blob colours off by +-2.5, alternating, so that every
    scan costs likelihood), and pk_upload_pose -- which leaves the other particles' log-weights bit for bit -- then takes ONE
    particle out (weight 0)."""
    P = 300
    f, blobs = observed_filter(lib, P, 48, 16)
    f.observe(blobs, fresh=True)
    scans = 0
    while f.download_log_weights().max() > -2000.0 and scans < 400:
        off = blobs.copy()
        off[:, 1:] += 2.5 if scans % 2 else -2.5
        f.observe(off)
        scans += 1
    logw = f.download_log_weights()
    print("log-weights after %d scans: %.1f .. %.1f" % (scans, logw.min(), logw.max()))
    assert logw.max() < -2000.0 and np.isfinite(logw).all()
    assert (f.download_poses()[:, 3] == 0.0).all()
    out = int(np.argmax(logw))  # the heaviest particle leaves: the maximum is another one's
    pose = f.download_poses()[out]
    f.upload_pose(out, [pose[0], pose[1], pose[2], 0.0])
    after = f.download_log_weights()
    assert after[out] == -np.inf and np.array_equal(np.delete(after, out), np.delete(logw, out))
    got = f.map_summary(WEIGHTED)
    w = np.exp(after - after.max())
    assert w[out] == 0.0 and w.max() == 1.0
    check(got, reference(f, w), what="weighted, log-weights below -2000")
    f.close()


# ---- (d) conditioning: landmarks 1e6 from the origin, particles 1e-3 apart
def test_landmarks_far_from_the_origin_keep_their_between_covariance(lib):
    """Shifted sums (mu - the first particle's mean) give the between-particle covariance to about 1e-12 here; raw second moments
    (sum mu mu^T - W mean mean^T: 1e12 against 1e-6) are off by 1e2."""
    P, L = 257, 40
    f = distinct_filter(lib, P, L, seed=9, offset=1e6, spread=1e-3)
    got = f.map_summary()
    ref = reference(f)
    check(got, ref, what="offset 1e6")
    d = np.einsum("lii->li", got.cov_between) / np.einsum("lii->li", ref.between) - 1.0
    print("between diagonals at offset 1e6, spread 1e-3: worst relative error %.3g" % np.abs(d).max())
    assert np.abs(d).max() < 1e-8
    f.close()


# ---- (e) the colour table: the estimate reads the colour rows the table stands in for, and the mode goes on
def test_colour_table_mode_goes_on_behind_the_estimate(lib):
    L, P, B = 513, 64, 64  # the smallest map that engages the table (Lp > 512); the scene of test_gpu_colour_table.py
    rs = np.random.RandomState(11)
    phi = -math.pi + 2 * math.pi * np.arange(L) / float(L) + 0.01
    rho = rs.uniform(8.0, 30.0, size=L)
    means = np.empty((L, 5))
    means[:, 0], means[:, 1] = rho * np.cos(phi), rho * np.sin(phi)
    means[:, 2:] = rs.uniform(0.0, 255.0, size=(L, 3))
    covs = np.broadcast_to(0.25 * np.identity(5), (L, 5, 5)).copy()
    seen = np.arange(3, L, 8)[:B]
    f = lib.DeviceFilter(P, L)
    f.upload_map(means, covs.reshape(L, 25))
    poses = np.zeros((P, 4))
    poses[:, 3] = 1.0
    f.upload_poses(poses)
    us = np.random.RandomState(99).uniform(size=5)
    (x, y, h), tr = (0.0, 0.0, 0.0), []
    for _ in range(5):
        h1 = h + 0.05 * 0.1 / 2
        x, y, h = x + 0.2 * 0.1 * math.cos(h1), y + 0.2 * 0.1 * math.sin(h1), h1 + 0.05 * 0.1 / 2
        tr.append((x, y, h))

    def step(s):
        blobs = np.empty((B, 4))
        blobs[:, 0] = np.arctan2(means[seen, 1] - tr[s][1], means[seen, 0] - tr[s][0]) - tr[s][2]
        blobs[:, 1:] = means[seen, 2:]
        f.step(0.2, 0.05, 0.1, blobs, us[s], seed=5, draw=s, domain=LOG)

    for s in range(4):
        step(s)
    st = f.colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == 4
    got = f.map_summary()
    assert f.colour_table_stats()["engaged"] == 1
    ref = reference(f)  # (a download leaves the mode on as well)
    check(got, ref, what="colour table mode")
    assert not np.array_equal(got.cov_within[seen, 2:, 2:], np.broadcast_to(covs[0, 2:, 2:], (B, 3, 3))), "the seen landmarks' colour blocks have moved"
    step(4)
    st2 = f.colour_table_stats()
    assert st2["engaged"] == 1 and st2["scans"] == st["scans"] + 1
    f.close()


# ---- (f) a growing filter: the preset landmarks only
def test_growing_filter_covers_its_preset_landmarks(lib):
    P, L0, U, spare = 64, 40, 3, 6
    world, wcov = synthetic_world(L0 + U, seed=123)
    f = lib.DeviceFilter(P, L0 + spare)
    means = np.zeros((L0 + spare, 5))
    means[:L0] = world[:L0]
    means[L0:, 2:] = EMPTY_COLOUR
    covs = np.tile(np.identity(5).reshape(25), (L0 + spare, 1))
    covs[:L0] = wcov[:L0].reshape(L0, 25)
    f.upload_map(means, covs)
    f.grow_enable(L0, 64, 30.0)
    rs = np.random.RandomState(5)
    pose = (0.0, 0.0, 0.0)
    for s in range(6):
        pose = truth_step(pose, 0.8, 0.35, 0.5)
        f.motion(0.8, 0.35, 0.5, z=rs.standard_normal((P, 3)))
        f.observe(synthetic_scan(world, pose), fresh=True)
        f.resample(float(rs.uniform()), domain=LOG)
    got = f.map_summary()
    m, c, k = f.download_landmarks()
    print("spare slots in use: %d of %d" % (int((k[:, L0:] != 0).sum()), P * spare))
    check(got, two_pass(m[:, :L0], c[:, :L0], k[:, :L0]), rows=slice(0, L0), what="growing filter, preset rows")
    for a in (got.mean, got.cov, got.cov_within, got.cov_between, got.update_count):
        assert np.isnan(a[L0:]).all() and not np.isnan(a[:L0]).any()
    assert sorted(got.as_features()) == list(range(1, L0 + 1))
    f.close()


# ---- (g) refusals: status and message
def test_refusals(lib):
    def refused(call, status, words):
        with pytest.raises(lib.PkError) as ei:
            call()
        assert ei.value.status == status and words in str(ei.value), str(ei.value)

    L = 4
    means, covs = synthetic_world(L)
    f = lib.DeviceFilter(8, L)
    for who in ("map_summary", "map_moments"):  # no map yet
        refused(getattr(f, who), lib.PK_ERR_STATE, "pk_%s: no map uploaded" % who)
    f.upload_map(means, covs.reshape(L, 25))
    for who in ("map_summary", "map_moments"):
        for bad in (2, -1):
            refused(lambda: getattr(f, who)(bad), lib.PK_ERR_INVALID, "pk_%s: weighting %d" % (who, bad))
    poses = np.zeros((8, 4))  # every weight 0: every log-weight -inf
    f.upload_poses(poses)
    for who in ("map_summary", "map_moments"):
        refused(lambda: getattr(f, who)(WEIGHTED), lib.PK_ERR_STATE, "pk_%s: no finite maximum log-weight" % who)
    refused(lambda: f.map_moments(WEIGHTED, gmax=float("inf")), lib.PK_ERR_STATE, "no finite maximum log-weight")
    assert f.map_summary(UNIFORM).n_eff == 8.0  # (the weights play no part)
    f.close()
    coupled = covs.copy()
    coupled[1, 0, 3] = coupled[1, 3, 0] = 0.05  # position-colour coupling: the dense 30-row layout
    d = lib.DeviceFilter(8, L)
    d.upload_map(means, coupled.reshape(L, 25))
    for who in ("map_summary", "map_moments"):
        refused(getattr(d, who), lib.PK_ERR_UNSUPPORTED, "pk_%s: the map estimate reads the compact layout" % who)
    d.close()
    abi = lib.load()
    assert abi.pk_map_summary(None, 0, None, None, None, None, None) == lib.PK_ERR_INVALID
    assert b"pk_map_summary: NULL handle" in abi.pk_last_error()
    assert abi.pk_map_moments(None, 0, 0.0, None, None, None, None, None) == lib.PK_ERR_INVALID
    assert b"pk_map_moments: NULL handle" in abi.pk_last_error()


# ---- (h) two handles holding parts of one population; the facade
@pytest.mark.parametrize("weighting", [UNIFORM, WEIGHTED])
def test_two_filters_moments_combine_to_the_whole_filters_summary(lib, weighting):
    from parakeet_slam_amd import mapsum

    P, L, cut = 1000, 37, 600
    rs = np.random.RandomState(17)
    w = np.exp(rs.normal(0.0, 1.5, size=P)) if weighting == WEIGHTED else np.ones(P)
    whole = distinct_filter(lib, P, L, seed=8, weights=w)
    m, c, k = whole.download_landmarks()
    poses = whole.download_poses()
    parts = []
    for a, b in ((0, cut), (cut, P)):
        f = lib.DeviceFilter(b - a, L)
        base, bcov = synthetic_world(L, seed=9)
        f.upload_map(base, bcov.reshape(L, 25))
        f.upload_poses(poses[a:b])
        f.upload_landmarks(0, b - a, m[a:b], c[a:b].reshape(b - a, L, 25), k[a:b])
        parts.append(f)
    gmax = max(f.shard_max_logw() for f in parts) if weighting == WEIGHTED else None
    combined = mapsum.finish(mapsum.combine_moments([f.map_moments(weighting, gmax) for f in parts]))
    one = whole.map_summary(weighting)
    logw = whole.download_log_weights()
    ref = two_pass(m, c, k, np.exp(logw - logw.max()) if weighting == WEIGHTED else None)
    check(one, ref, what="one filter of 1000")
    check(combined, ref, what="600 + 400 combined")
    # own maximum (gmax = None) of a part: the same moments up to the common factor exp(gmax - own), which the finish divides out
    if weighting == WEIGHTED:
        own = mapsum.finish(parts[1].map_moments(WEIGHTED))
        lw = parts[1].download_log_weights()
        check(own, two_pass(m[cut:], c[cut:], k[cut:], np.exp(lw - lw.max())), what="a part by its own maximum")
    for f in parts + [whole]:
        f.close()


def test_facade_map_summary_agrees_with_the_particle_views():
    import parakeet_slam_amd as pk
    from conftest import load_golden
    from test_gpu_facade import View

    g = load_golden("step_small")
    P, L = int(g["P"]), int(g["L"])
    np.random.seed(int(g["seed"]))
    random.seed(int(g["seed"]))
    pk.msgs.Time.set_now(0.0)
    fs = pk.FastSLAM([pk.Feature(mean=g["means0"][l], covar=g["covs0"][l]) for l in range(L)], num_particles=P)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = float(g["v"]), float(g["w"])
    fs.last_control = tw
    t = 0.0
    for s in range(3):
        t += float(g["dts"][s])
        pk.msgs.Time.set_now(t)
        fs.cam_cb(View(pk, g["blobs"][s]))
    got = fs.map_summary()
    also = fs.map_summary("weights")  # (behind the resample the particles carry their ancestors' weights)
    sets = [fs.particles[i].feature_set for i in range(P)]
    means = np.array([[fsi[l + 1].mean for l in range(L)] for fsi in sets], dtype=np.float64)
    covs = np.array([[fsi[l + 1].covar for l in range(L)] for fsi in sets], dtype=np.float64)
    counts = np.array([[fsi[l + 1].update_count for l in range(L)] for fsi in sets])
    ref = two_pass(means, covs, counts)
    check(got, ref, what="facade")
    check(also, two_pass(means, covs, counts, np.array([fs.particles[i].weight for i in range(P)])), what="facade, by the weights")
    feats = got.as_features()
    assert sorted(feats) == list(range(1, L + 1)) and np.array_equal(feats[1].covar, got.cov[0])
    with pytest.raises(ValueError):
        fs.map_summary("linear")
    fs.close()


# ---- (i) memory: nothing until the first call
def test_device_memory_grows_at_the_first_estimate_only(lib):
    def stepped():
        f, blobs = observed_filter(lib, 128, 48, 16)
        for s in range(3):
            f.step(0.2, 0.05, 0.1, blobs, 0.3 + 0.1 * s, seed=5, draw=1 + s, domain=LOG)
        f.synchronize()
        return f

    a, b = stepped(), stepped()
    held = b.device_bytes()
    assert a.device_bytes() == held, "two filters with the same history hold the same bytes"
    a.map_summary()
    first = a.device_bytes()
    assert first > held
    a.map_summary()
    a.map_summary(WEIGHTED)
    a.map_moments()
    assert a.device_bytes() == first
    assert b.device_bytes() == held  # (the one that never asked)
    a.close()
    b.close()

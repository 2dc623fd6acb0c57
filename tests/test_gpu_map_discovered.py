"""GPU: the estimate of the discovered landmarks (pk_map_match_moments / pk_map_discovered, pk_k_mapmatch.hip)
-- the spare slots of a growing filter matched across the particles against a list of reference features, and per feature the
moments of the matched slots.

The reference in every case is map_match_reference.py over download_landmarks / grow_download of ALL particles: the matching rule
in NumPy with the device's operation order (the match table must agree EXACTLY), then a two-pass computation per feature (the
tolerances are stated there).  The estimate is taken BEFORE the download: the download materialises."""
import random

import numpy as np
import pytest

from map_match_reference import COLOUR_RADIUS, RADIUS, check, planted_state, reference, upload_state
from mapsum_reference import POT, check as check_map, two_pass
from oracle.fastslam_oracle import EMPTY_COLOUR, synthetic_scan, synthetic_world, truth_step

pytestmark = pytest.mark.gpu

LOG = 1  # PK_WEIGHTS_LOG
UNIFORM, WEIGHTED = 0, 1
L0 = 5  # preset landmarks of the planted states: the spare slots start off the 16-landmark padding of the rows

FIELDS = ("mean", "cov_within", "cov_between", "update_count", "support", "potential_fraction", "n_eff")


def same_bits(a, b):
    return all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True) for n in FIELDS) and a.n_eff_all == b.n_eff_all \
        and a.reference_particle == b.reference_particle and np.array_equal(a.ids, b.ids)


def check_reference_particle(got, r, means, counts, counters, slot_ids):
    """What the estimate says of its reference particle r, against the downloads."""
    u = int(counters[r, 1])
    assert got.reference_particle == r and got.mean.shape == (u, 5)
    assert np.array_equal(got.ids, slot_ids[r, :u]) and np.array_equal(got.slots, L0 + np.arange(u))
    assert np.array_equal(got.potential, (counts[r, L0:L0 + u] & POT) != 0)
    assert np.array_equal(got.ref_update_count, counts[r, L0:L0 + u] & ~POT)
    return means[r, L0:L0 + u]


# ---- (1) shapes: one feature, a typical handful, a full wave of reference features, beyond a wave; one particle, fewer particles
# than groups, several groups with a ragged last one; forced group counts
@pytest.mark.parametrize("P", [1, 3, 257, 1000])
@pytest.mark.parametrize("S", [1, 6, 64, 70])
def test_shapes_uniform_weighting(lib, S, P):
    from parakeet_slam_amd import mapsum

    st = planted_state(P, L0, S, seed=100 * S + P)
    f = upload_state(lib, st)
    r = 2 if P >= 3 else 0  # (particle 2 holds all S features)
    got = []
    for groups in {1000: (0, 1, 3, 7), 3: (0, 7)}.get(P, (0,)):  # (7 groups of 3 particles: four of them are empty)
        f.set_option("map_match_groups", groups)
        got.append((groups, f.map_match_moments(st["truth"], RADIUS, COLOUR_RADIUS, matches=True), f.map_discovered(RADIUS, COLOUR_RADIUS, reference=r)))
    m, c, k = f.download_landmarks()
    counters, _, sids = f.grow_download(readings=False)
    assert np.array_equal(m, st["means"]) and np.array_equal(counters[:, 1], st["used"])
    ref = reference(m, c, k, counters[:, 1], L0, st["truth"], RADIUS, COLOUR_RADIUS)
    for groups, mm, dm in got:
        what = "S %d P %d groups %d" % (S, P, groups)
        assert mm.matches.shape == (P, S) and np.array_equal(mm.matches, ref.matches), what + ": the match table"
        check(mapsum.finish_matched(mm, st["truth"]), ref, what=what + ", explicit references")
        assert mm.wsum[0] == P and mm.wsum[1] == P
        own = check_reference_particle(dm, r, m, k, counters, sids)
        check(dm, reference(m, c, k, counters[:, 1], L0, own, RADIUS, COLOUR_RADIUS), what=what + ", particle %d's features" % r)
        assert abs(dm.n_eff_all - P) <= 1e-12 * P
    f.close()


def test_no_reference_feature_and_a_reference_particle_without_features(lib):
    st = planted_state(3, L0, 6, seed=2)
    f = upload_state(lib, st)
    mm = f.map_match_moments(np.zeros((0, 5)), RADIUS, COLOUR_RADIUS, matches=True)
    assert mm.n == 0 and mm.matches.shape == (3, 0) and mm.wsum.tolist() == [3.0, 3.0]
    dm = f.map_discovered(RADIUS, COLOUR_RADIUS, reference=1)  # (particle 1 holds nothing)
    assert dm.reference_particle == 1 and dm.mean.shape == (0, 5) and dm.ids.size == 0 and dm.n_eff_all == 3.0 and dm.as_features() == {}
    f.close()


# ---- (2) behind a resample: long runs of equal src that cross group boundaries; nothing of the filter changes
def test_behind_a_resample_with_a_few_heavy_particles(lib):
    P, S, G = 1000, 6, 7
    w = np.full(P, 1e-7)
    w[[100, 400, 401, 900]] = 1.0, 0.7, 1.3, 0.9
    st = planted_state(P, L0, S, seed=3)
    f = upload_state(lib, st, weights=w)
    f.set_option("map_match_groups", G)
    f.resample(0.37)
    src = f.download_sources()
    chunk = -(-P // G)
    crossing = [b for b in range(chunk, P, chunk) if src[b - 1] == src[b]]
    assert len(np.unique(src)) <= 6 and len(crossing) >= 3, "runs of one slot must cross the groups' boundaries"
    poses, logw, route, grow = f.download_poses(), f.download_log_weights(), f.observe_route(), f.grow_download()
    first = f.map_discovered(RADIUS, COLOUR_RADIUS)
    second = f.map_discovered(RADIUS, COLOUR_RADIUS)
    ma = f.map_match_moments(st["truth"], RADIUS, COLOUR_RADIUS, matches=True)
    mb = f.map_match_moments(st["truth"], RADIUS, COLOUR_RADIUS, matches=True)
    assert np.array_equal(f.download_sources(), src)
    assert np.array_equal(f.download_poses(), poses) and np.array_equal(f.download_log_weights(), logw) and f.observe_route() == route
    assert all(np.array_equal(a, b) for a, b in zip(f.grow_download(), grow))
    assert same_bits(first, second), "the same filter state must give the same bits twice"
    assert all(np.array_equal(getattr(ma, n), getattr(mb, n), equal_nan=True) for n in ("wsum", "support", "mean", "m2", "within", "counts", "matches"))
    m, c, k = f.download_landmarks()  # (materialises: every particle in its own slot from here on)
    assert np.array_equal(f.download_sources(), np.arange(P))
    counters, _, sids = f.grow_download(readings=False)
    best = f.best_particle()[0]
    own = check_reference_particle(first, best, m, k, counters, sids)
    check(first, reference(m, c, k, counters[:, 1], L0, own, RADIUS, COLOUR_RADIUS), what="behind a resample")
    check(f.map_discovered(RADIUS, COLOUR_RADIUS), reference(m, c, k, counters[:, 1], L0, own, RADIUS, COLOUR_RADIUS), what="behind the materialisation")
    assert np.array_equal(ma.matches, reference(m, c, k, counters[:, 1], L0, st["truth"], RADIUS, COLOUR_RADIUS).matches)
    f.close()


# ---- (3) by the weights
def test_weighted(lib):
    P, S = 257, 6
    rs = np.random.RandomState(8)
    w = np.exp(rs.normal(0.0, 1.5, size=P))
    w[[0, 5]] = 0.0  # particle 0, and one that alone holds a feature of its own
    st = planted_state(P, L0, S, seed=31)
    st["means"][5, L0] = [-300.0, -300.0, 5.0, 5.0, 5.0]
    st["used"][5] = max(st["used"][5], 1)
    f = upload_state(lib, st, weights=w)
    logw = f.download_log_weights()
    assert logw[0] == -np.inf and logw[5] == -np.inf and np.ptp(logw[np.isfinite(logw)]) > 1.0
    best = f.best_particle()[0]
    assert best == int(np.argmax(logw)) and best not in (0, 5)
    by_best = f.map_discovered(RADIUS, COLOUR_RADIUS, WEIGHTED)
    by_zero = f.map_discovered(RADIUS, COLOUR_RADIUS, WEIGHTED, reference=0)
    by_lone = f.map_discovered(RADIUS, COLOUR_RADIUS, WEIGHTED, reference=5)
    mm = f.map_match_moments(st["truth"], RADIUS, COLOUR_RADIUS, WEIGHTED, matches=True)
    half = f.map_match_moments(st["truth"], RADIUS, COLOUR_RADIUS, WEIGHTED, gmax=float(logw.max()) + np.log(2.0))
    m, c, k = f.download_landmarks()
    counters, _, sids = f.grow_download(readings=False)
    wr = np.exp(logw - logw.max())
    assert wr[0] == 0.0 and wr.max() == 1.0
    for got, r, what in ((by_best, best, "the most likely particle"), (by_zero, 0, "a reference particle of weight 0"), (by_lone, 5, "a lone feature")):
        own = check_reference_particle(got, r, m, k, counters, sids)
        check(got, reference(m, c, k, counters[:, 1], L0, own, RADIUS, COLOUR_RADIUS, wr), what="weighted, " + what)
        assert 1.0 < got.n_eff_all < P
    assert by_lone.support[0] == 0.0 and np.isnan(by_lone.mean[0]).all(), "a feature only a particle of weight 0 holds"
    assert np.isfinite(by_zero.mean).any(), "the others hold what the particle of weight 0 holds"
    from parakeet_slam_amd import mapsum

    ref = reference(m, c, k, counters[:, 1], L0, st["truth"], RADIUS, COLOUR_RADIUS, wr)
    assert np.array_equal(mm.matches, ref.matches)
    check(mapsum.finish_matched(mm, st["truth"]), ref, what="weighted, explicit references")
    check(mapsum.finish_matched(half, st["truth"]), ref, what="weighted, a maximum from outside")  # (the common factor 1/2 divides out)
    assert abs(half.wsum[0] / mm.wsum[0] - 0.5) < 1e-12
    f.close()


# ---- (4) conditioning: features 1e6 from the origin, particles 1e-3 apart
def test_features_far_from_the_origin_keep_their_between_covariance(lib):
    """The sums are shifted by the reference feature, which the radius bounds: d = mu - r is exact to the spacing of the doubles at
    1e6, and the two-pass reference loses nothing to first order either (sum w d = 0 about its mean), so the between-particle
    variances agree far inside the tolerance -- raw second moments (1e12 against 1e-6) would be off by 1e2."""
    P, S = 257, 6
    st = planted_state(P, L0, S, seed=9, offset=1e6, noise=1e-3)
    f = upload_state(lib, st)
    r = 2
    got = f.map_discovered(RADIUS, COLOUR_RADIUS, reference=r)
    m, c, k = f.download_landmarks()
    counters, _, sids = f.grow_download(readings=False)
    own = check_reference_particle(got, r, m, k, counters, sids)
    ref = reference(m, c, k, counters[:, 1], L0, own, RADIUS, COLOUR_RADIUS)
    check(got, ref, what="offset 1e6")
    assert (ref.holders > 2).all()
    d = np.einsum("lii->li", got.cov_between) / np.einsum("lii->li", ref.between) - 1.0
    print("between diagonals at offset 1e6, spread 1e-3: worst relative error %.3g" % np.abs(d).max())
    assert np.abs(d).max() < 1e-8
    f.close()


# ---- (5) end to end: the scene of test_gpu_mapsum.py::test_growing_filter_covers_its_preset_landmarks
def test_grown_filter_end_to_end(lib):
    P, L0_, U, spare = 64, 40, 3, 6
    world, wcov = synthetic_world(L0_ + U, seed=123)
    f = lib.DeviceFilter(P, L0_ + spare)
    means = np.zeros((L0_ + spare, 5))
    means[:L0_] = world[:L0_]
    means[L0_:, 2:] = EMPTY_COLOUR
    covs = np.tile(np.identity(5).reshape(25), (L0_ + spare, 1))
    covs[:L0_] = wcov[:L0_].reshape(L0_, 25)
    f.upload_map(means, covs)
    f.grow_enable(L0_, 64, 30.0)
    rs = np.random.RandomState(5)
    pose = (0.0, 0.0, 0.0)
    for s in range(6):
        pose = truth_step(pose, 0.8, 0.35, 0.5)
        f.motion(0.8, 0.35, 0.5, z=rs.standard_normal((P, 3)))
        f.observe(synthetic_scan(world, pose), fresh=True)
        f.resample(float(rs.uniform()), domain=LOG)
    got = f.map_discovered(3.0, 30.0)
    summary = f.map_summary()
    best = f.best_particle()[0]
    m, c, k = f.download_landmarks()
    counters, _, sids = f.grow_download(readings=False)
    u = int(counters[best, 1])
    assert got.reference_particle == best and got.mean.shape[0] == u and u >= 1
    assert np.array_equal(got.ids, sids[best, :u]) and np.array_equal(got.slots, L0_ + np.arange(u))
    ref = reference(m, c, k, counters[:, 1], L0_, m[best, L0_:L0_ + u], 3.0, 30.0)
    check(got, ref, what="grown filter")
    print("spare slots in use: %d of %d; particles holding each of the best particle's features: %s" % (int(counters[:, 1].sum()), P * spare, ref.holders.tolist()))
    assert ((ref.holders > 1) & (ref.holders < P)).any(), "the match must be non-trivial: some feature held by several particles, not by all"
    near = np.sqrt(((got.mean[:, None, :2] - world[None, L0_:, :2]) ** 2).sum(axis=2)).min(axis=1)
    for i in range(u):
        print("feature id %d: support %.3f, potential %.2f, distance to the nearest true unknown landmark %.3f" % (got.ids[i], got.support[i], got.potential_fraction[i], near[i]))
    check_map(summary, two_pass(m[:, :L0_], c[:, :L0_], k[:, :L0_]), rows=slice(0, L0_), what="map_summary beside it, preset rows")
    for a in (summary.mean, summary.cov, summary.update_count):
        assert np.isnan(a[L0_:]).all() and not np.isnan(a[:L0_]).any(), "map_summary() is unchanged: NaN spare rows"
    f.close()


# ---- (6) through the facade
class _View(object):
    def __init__(self, pk, blobs):
        class Scan(object):
            pass

        self.last_sensor_reading = Scan()
        obs = []
        for b in blobs:
            z = pk.msgs.Blob()
            z.bearing = float(b[0])
            z.color.r, z.color.g, z.color.b = float(b[1]), float(b[2]), float(b[3])
            obs.append(z)
        self.last_sensor_reading.observes = obs


def test_facade_discovered_landmarks(lib):
    import parakeet_slam_amd as pk
    from parakeet_slam_amd import mapsum

    L0_, U, P, spare, steps = 10, 3, 12, 6, 8
    v, w, dt = 0.8, 0.35, 0.5
    world, covs = synthetic_world(L0_ + U)
    feats = [pk.Feature(mean=m.copy(), covar=c.copy()) for m, c in zip(world[:L0_], covs[:L0_])]
    np.random.seed(5)
    random.seed(5)
    pk.msgs.Time.set_now(0.0)
    fs = pk.FastSLAM(feats, num_particles=P, weight_domain="log", new_landmarks=True, spare_landmarks=spare)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = v, w
    fs.last_control = tw
    pose = (0.0, 0.0, 0.0)
    for s in range(steps):
        pose = truth_step(pose, v, w, dt)
        pk.msgs.Time.set_now(dt * (s + 1))
        fs.cam_cb(_View(pk, synthetic_scan(world, pose)))
    got = fs.discovered_landmarks()
    assert isinstance(got, mapsum.DiscoveredMap) and got.reference_particle == fs.best_particle()
    assert same_bits(got, fs.discovered_landmarks(radius=3.0, colour_radius=30.0, weighting="uniform")), "the defaults: 3.0, the pair threshold, uniform"
    other = fs.discovered_landmarks(reference=P - 1, weighting="weights")
    m, c, k = fs._filter.download_landmarks()
    counters, _, sids = fs._filter.grow_download(readings=False)
    for d, r, wts in ((got, got.reference_particle, None), (other, P - 1, np.array([p.weight for p in fs.particles]))):
        u = int(counters[r, 1])
        assert d.reference_particle == r and u >= 1 and np.array_equal(d.ids, sids[r, :u]) and np.array_equal(d.slots, L0_ + np.arange(u))
        assert np.array_equal(d.potential, (k[r, L0_:L0_ + u] & POT) != 0)
        check(d, reference(m, c, k, counters[:, 1], L0_, m[r, L0_:L0_ + u], 3.0, 30.0, wts), what="facade, particle %d" % r)
    feats_all = got.as_features(min_support=0.0, promoted_only=False)
    assert sorted(feats_all) == sorted(int(i) for i in got.ids[got.support > 0]) and all(i > L0_ for i in feats_all)
    i0 = int(got.ids[0])
    assert np.array_equal(feats_all[i0].mean, got.mean[0]) and np.array_equal(feats_all[i0].covar, got.cov[0])
    assert set(got.as_features()) <= set(feats_all)
    with pytest.raises(ValueError):
        fs.discovered_landmarks("linear")
    fs.close()
    plain = pk.FastSLAM(feats, num_particles=P)
    with pytest.raises(ValueError, match="new_landmarks=True"):
        plain.discovered_landmarks()
    plain.close()
    host = pk.FastSLAM(feats, num_particles=P, new_landmarks=True, spare_landmarks=2, bookkeeping="host", weight_domain="log")
    with pytest.raises(ValueError, match="bookkeeping='device'"):
        host.discovered_landmarks()
    host.close()


# ---- (7) refusals: status and message; memory
def test_refusals(lib):
    def refused(call, status, words):
        with pytest.raises(lib.PkError) as ei:
            call()
        assert ei.value.status == status and words in str(ei.value), str(ei.value)

    L = 8
    means, covs = synthetic_world(L)
    one = np.zeros((1, 5))
    calls = (("pk_map_match_moments", lambda f, **kw: f.map_match_moments(kw.pop("ref", one), kw.pop("radius", 3.0), kw.pop("colour_radius", 30.0), **kw)),
             ("pk_map_discovered", lambda f, **kw: f.map_discovered(kw.pop("radius", 3.0), kw.pop("colour_radius", 30.0), **kw)))
    f = lib.DeviceFilter(8, L)
    for who, call in calls:  # no map yet
        refused(lambda: call(f), lib.PK_ERR_STATE, "%s: no map uploaded" % who)
    f.upload_map(means, covs.reshape(L, 25))
    for who, call in calls:  # a filter that does not grow
        refused(lambda: call(f), lib.PK_ERR_STATE, "%s: pk_grow_enable was not called on this filter" % who)
    f.grow_enable(5, 4, 30.0)
    for who, call in calls:
        for bad in (2, -1):
            refused(lambda: call(f, weighting=bad), lib.PK_ERR_INVALID, "%s: weighting %d" % (who, bad))
        for bad in (float("nan"), 0.0, -1.0, -float("inf")):
            refused(lambda: call(f, radius=bad), lib.PK_ERR_INVALID, "%s: radius" % who)
            refused(lambda: call(f, colour_radius=bad), lib.PK_ERR_INVALID, "%s: colour_radius" % who)
        call(f, radius=float("inf"), colour_radius=float("inf"))
    refused(lambda: f.map_match_moments(np.zeros((4097, 5)), 3.0, 30.0), lib.PK_ERR_INVALID, "pk_map_match_moments: 4097 reference features")
    assert f.map_match_moments(np.zeros((4096, 5)), 3.0, 30.0).n == 4096
    for bad in (8, -2):
        refused(lambda: f.map_discovered(3.0, 30.0, reference=bad), lib.PK_ERR_INVALID, "pk_map_discovered: reference particle %d of 8" % bad)
    refused(lambda: f.map_match_moments(one, 3.0, 30.0, WEIGHTED, gmax=1e6), lib.PK_ERR_STATE, "pk_map_match_moments: the weights sum to 0")
    refused(lambda: f.map_match_moments(one, 3.0, 30.0, WEIGHTED, gmax=float("inf")), lib.PK_ERR_STATE, "no finite maximum log-weight")
    f.upload_poses(np.zeros((8, 4)))  # every weight 0: every log-weight -inf
    for who, call in calls:
        refused(lambda: call(f, weighting=WEIGHTED), lib.PK_ERR_STATE, "%s: no finite maximum log-weight" % who)
    assert f.map_discovered(3.0, 30.0).reference_particle == 0 and f.map_discovered(3.0, 30.0).n_eff_all == 8.0  # (uniform: the weights play no part; all at -inf: particle 0)
    assert f.map_discovered(3.0, 30.0, reference=3).reference_particle == 3
    f.close()
    coupled = covs.copy()
    coupled[1, 0, 3] = coupled[1, 3, 0] = 0.05  # position-colour coupling: the dense 30-row layout
    d = lib.DeviceFilter(8, L)
    d.upload_map(means, coupled.reshape(L, 25))
    for who, call in calls:
        refused(lambda: call(d), lib.PK_ERR_UNSUPPORTED, "%s: the map estimate reads the compact layout" % who)
    d.close()
    abi = lib.load()
    assert abi.pk_map_match_moments(None, 0, 0.0, None, 0, 3.0, 30.0, None, None, None, None, None, None, None) == lib.PK_ERR_INVALID
    assert b"pk_map_match_moments: NULL handle" in abi.pk_last_error()
    assert abi.pk_map_discovered(None, 0, -1, 3.0, 30.0, None, None, None, None, None, None, None, None, None, None, None, None) == lib.PK_ERR_INVALID
    assert b"pk_map_discovered: NULL handle" in abi.pk_last_error()


def test_every_output_may_be_null(lib):
    st = planted_state(3, L0, 6, seed=2)
    f = upload_state(lib, st)
    abi = lib.load()
    ref = np.ascontiguousarray(st["truth"])
    assert abi.pk_map_match_moments(f._h, 0, 0.0, lib.dptr(ref), 6, 3.0, 30.0, None, None, None, None, None, None, None) == lib.PK_OK
    assert abi.pk_map_discovered(f._h, 0, -1, 3.0, 30.0, None, None, None, None, None, None, None, None, None, None, None, None) == lib.PK_OK
    f.close()


def test_device_memory_grows_at_the_first_estimate_only(lib):
    def grown():
        return upload_state(lib, planted_state(128, L0, 6, seed=6))

    a, b = grown(), grown()
    held = b.device_bytes()
    assert a.device_bytes() == held, "two filters with the same history hold the same bytes"
    a.map_discovered(3.0, 30.0)
    first = a.device_bytes()
    assert first > held
    a.map_discovered(3.0, 30.0)
    a.map_discovered(3.0, 30.0, WEIGHTED, reference=4)
    a.map_match_moments(np.zeros((6, 5)), 3.0, 30.0)
    assert a.device_bytes() == first, "a second call allocates nothing more"
    a.map_match_moments(np.zeros((6, 5)), 3.0, 30.0, matches=True)  # (the match table, for the calls that ask for it)
    table = a.device_bytes()
    assert table > first
    a.map_match_moments(np.zeros((6, 5)), 3.0, 30.0, matches=True)
    assert a.device_bytes() == table
    assert b.device_bytes() == held  # (the one that never asked)
    a.close()
    b.close()
